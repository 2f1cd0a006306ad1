#pragma once
// ba_one_pose.h -- one free pose + free points: stage 1 of localBundleAdjust.  k_ba_one_pose.

// ---------------------------------------------------------------- one free pose + free points: stage 1 of localBundleAdjust (bundle_adjuster.cpp:251-252, :268, :322-333)
// ONE free keyframe, every other keyframe fixed, the map points free: the reduced camera system is 6 x 6 whatever the window's size.  The general kernel
// still walked it through its whole machinery (pass sets, LDS tile, windowed Cholesky of one block, ~7 team barriers per damped solve): 0.60 ms for the
// 8 iterations of a C4 window on 32 workgroups, 3.3 ms for 256 such windows with one workgroup each.  Here a point belongs to a GROUP of G = 1 .. 8
// neighbouring lanes (G chosen so that the launch's lanes cover the points): the group's lanes share the point's observations out, their sums meet over
// the DPP network.  With a lane group per point (ONE: a single window on a team) the point -- position, Hll, bl, W = sum of Jp^T w Jl over its observations
// in the free keyframe -- stays in the group's REGISTERS from the first linearisation to the last trial; a batch (one workgroup per window, several points
// per group) keeps these records in memory that only the owning workgroup touches.  Per iteration: linearise, and in the same pass every group forms its
// point's W (Hll + lambda I)^-1 W^T and W (Hll + lambda I)^-1 bl (3 x 3 Cholesky, as in schur_fused).  Only ~1 point in 4 is seen by the free keyframe, so
// these 27-value contributions are SPARSE: the contributing lanes write them side by side into the wave's LDS slab, the wave adds the entries up and issues
// one atomic per value (27 uniform-address atomics per observation cost a wave reduction each: 5 x the time of everything else).  ONE reduction over the
// team, the 6 x 6 Cholesky in every thread (as in k_ba_pose_only), then each group back-substitutes its point, moves it, and evaluates the robust chi2 of
// its observations at the trial state; a second reduction (chi2, gain denominator) decides.  Trial points are separate from the accepted ones: no backup /
// restore pass.  Observation data comes from copies sorted by point (pose index, u, v, information side by side: one round trip instead of three dependent
// ones), the poses from an LDS table.  Same LM schedule and the same arithmetic per edge as k_ba_lm.
constexpr int OP_NT = 512, OP_NW = OP_NT / 64, OP_NV = 64, OP_MAX_LDS_POSES = 512;
constexpr int OP_S0 = 32, OP_BAD = 59, OP_MAX = 63;          // accumulators: 0..20 Hpp, 21..26 bp | 32..52 Schur matrix terms, 53..58 rhs terms, 59 unsound point blocks | 63 largest diagonal entry
__host__ __device__ constexpr int op_slab_cap(int lgG) { return lgG == 0 ? 64 : 32; }     // entries of a wave's staging slab
constexpr size_t kOpLdsBytes = (((size_t)7 * OP_MAX_LDS_POSES + 2) + (size_t)OP_NW * 27 * 64) * sizeof(double);     // dynamic LDS at most: the pose table + the slabs (136 KB; ~11 KB are static)

// sum over a group of 2^lg neighbouring lanes (aligned), the result in every lane of the group: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror
__device__ __forceinline__ double group_sum_d(double v, int lg) {
    if (lg >= 1) v += dpp_d<0xB1>(v);
    if (lg >= 2) v += dpp_d<0x4E>(v);
    if (lg >= 3) v += dpp_d<0x141>(v);
    return v;
}
__device__ __forceinline__ int group_sum_i(int v, int lg) {
    if (lg >= 1) v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);
    if (lg >= 2) v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);
    if (lg >= 3) v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);
    return v;
}

// Hll + lambda I = L L^T (3 x 3, packed 00 01 02 11 12 22); returns false when a pivot is not positive
struct Chol3 { double i11, l21, l31, i22, l32, i33; };
__device__ __forceinline__ bool chol3(const double *H, double lambda, Chol3 &c) {
    const double a = H[0] + lambda, d = H[3] + lambda, f = H[5] + lambda;
    c.i11 = rsqrt_d(a); c.l21 = H[1] * c.i11; c.l31 = H[2] * c.i11;
    const double d2 = d - c.l21 * c.l21;
    c.i22 = rsqrt_d(d2); c.l32 = (H[4] - c.l31 * c.l21) * c.i22;
    const double d3 = f - c.l31 * c.l31 - c.l32 * c.l32;
    c.i33 = rsqrt_d(d3);
    return a > 0 && d2 > 0 && d3 > 0 && isfinite(c.i11 * c.i22 * c.i33);
}

// Sparse sums: a few lanes of a wave hold 27 values each whose sums go into acc[0 .. 27).  The contributors write their values side by side into the wave's
// slab ([27][cap], value-major: neighbouring entries in neighbouring banks; entry = a running index over the wave's contributors), then the wave adds the
// entries up -- value k by lanes 2k and 2k + 1 (even / odd entries) -- and issues one atomic per value.  A contributor beyond the slab's capacity adds its
// values with plain atomics.
__device__ __forceinline__ void slab_put(MS_LDS double *slab, int cap, MS_LDS double *acc, int idx, const double (&v)[27]) {
    if (idx < cap) {
#pragma unroll
        for (int k = 0; k < 27; ++k) slab[k * cap + idx] = v[k];
    } else {
#pragma unroll
        for (int k = 0; k < 27; ++k) lds_addd(acc + k, v[k]);
    }
}
__device__ __forceinline__ void slab_sum(MS_LDS double *slab, int cap, MS_LDS double *acc, int n, int lane) {      // wave-uniform call, n wave-uniform
    if (n == 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int ns = min(n, cap);
    if (lane < 54) {
        const int k = lane >> 1;
        double t = 0;
        for (int e = lane & 1; e < ns; e += 2) t += slab[k * cap + e];
        t += dpp_d<0xB1>(t);
        if ((lane & 1) == 0) lds_addd(acc + k, t);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int lanes_below(unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }

struct OpPoint { double X[3], H[6], bl[3], W[18]; int nf, i0, i1; bool pfree; };       // nf: the point's observations in the free keyframe (group total)

template <bool ONE>     // ONE: the launch has a lane group per point -- the point's record lives in registers for the whole solve
__global__ __launch_bounds__(OP_NT) void k_ba_one_pose(const BaProb *probs, int team, int lgG, int pose_doubles) {
    extern __shared__ __attribute__((aligned(16))) double op_lds[];      // [7 n_pose] the poses (when they fit), then the waves' staging slabs [8][27][cap]
    __shared__ double s_acc[OP_NV], s_sum[OP_NV], s_w[OP_NW * 2], s_part[OP_NW * OP_NV];
    __shared__ double s_eC[PO_MAXE][8], s_eM[PO_MAXE][8], s_eG[PO_MAXE][36], s_eW[PO_MAXE][36], s_Hc[24], s_const;
    __shared__ int s_eSide[PO_MAXE], s_ne;
    __shared__ double s_J[36];
    const long long t_kernel = clock64();
    const BaProb &P = probs[blockIdx.x / (unsigned)team];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rank = team > 1 ? (int)(blockIdx.x % (unsigned)team) : 0;
    const int G = 1 << lgG, gl = rank * OP_NT + tid, sub = gl & (G - 1), slot = gl >> lgG, nslot = (team * OP_NT) >> lgG;
    const int pi = P.free2pose[0], n_point = P.n_point, cap = op_slab_cap(lgG);
    const bool lds_poses = pose_doubles > 0;                              // (the host's decision for the whole launch: every problem's poses fit the table then)
    MS_LDS double *slab = (MS_LDS double *)op_lds + pose_doubles + wave * 27 * cap;
    MS_LDS double *acc = (MS_LDS double *)s_acc;
    const MS_GLOBAL int32_t *o_pose = (const MS_GLOBAL int32_t *)P.op_pose, *o_idx = (const MS_GLOBAL int32_t *)P.op_o, *pt_start = (const MS_GLOBAL int32_t *)P.pt_start;
    const MS_GLOBAL double *o_uvi = (const MS_GLOBAL double *)P.op_uvi;
    MS_GLOBAL double *rec = (MS_GLOBAL double *)P.op_rec;                 // (not ONE) [28][n_point]: Hll 0-5, bl 6-8, W 9-26, 27 = observations in the free keyframe, -1 for a fixed point
    MS_GLOBAL double *point = (MS_GLOBAL double *)P.point, *trial = (MS_GLOBAL double *)P.point_bk;
    const MS_GLOBAL uint8_t *pfix = (const MS_GLOBAL uint8_t *)P.point_fixed;
    const int nrounds = ONE ? 1 : (n_point + nslot - 1) / nslot;
    int seq = 0;
    // (the free pose's seven entries are written ONCE, at the end, by the launch's first lane: the team's barriers carry no cache maintenance, and two workgroups on
    //  different XCDs writing the same line -- one here, one at the end -- would leave the order of the two write-backs to chance)
    for (int i = gl; i < 7 * P.n_pose; i += team * OP_NT) if (i / 7 != pi) P.pose[i] = P.pose0[i];
    if (lds_poses) for (int i = tid; i < 7 * P.n_pose; i += OP_NT) op_lds[i] = P.pose0[i];
    OpPoint ps;
    double Xt[3] = {0, 0, 0};                                             // ONE: the trial point
    auto point_begin = [&](int l, bool from_point0) {                     // the point's observation range, its flag and its position
        ps.i0 = ps.i1 = 0; ps.pfree = false; ps.nf = 0; ps.X[0] = ps.X[1] = ps.X[2] = 0;
        if (l < n_point) {
            ps.i0 = pt_start[l]; ps.i1 = pt_start[l + 1]; ps.pfree = !(pfix && pfix[l]);
            const MS_GLOBAL double *src = from_point0 ? (const MS_GLOBAL double *)P.point0 : point;
            ps.X[0] = src[3 * (size_t)l]; ps.X[1] = src[3 * (size_t)l + 1]; ps.X[2] = src[3 * (size_t)l + 2];
        }
    };
    if (ONE) point_begin(slot, true);
    else for (int l = slot; l < n_point; l += nslot) if (sub == 0) { point[3 * (size_t)l] = P.point0[3 * (size_t)l]; point[3 * (size_t)l + 1] = P.point0[3 * (size_t)l + 1]; point[3 * (size_t)l + 2] = P.point0[3 * (size_t)l + 2]; }
    if (tid < OP_NV) s_acc[tid] = 0;
    if (tid < 24) s_Hc[tid] = 0;
    if (tid == 0) { s_ne = 0; s_const = 0; }
    __syncthreads();
    double pose[7];
#pragma unroll
    for (int a = 0; a < 7; ++a) pose[a] = P.pose0[7 * (size_t)pi + a];
    // ---- the SE3 edges: an edge between fixed poses is a constant, one that touches the free pose leaves its fixed side's transform, -J^T W and J^T W J
    //      in LDS (its Jacobian does not depend on the free pose), exactly as in k_ba_pose_only.  They belong to the LAST wave of the team's LAST workgroup:
    //      an edge is ~1 700 dependent instructions (quaternion products, the SE3 logarithm) in one lane, 17 k cycles per sweep, and on the team's first wave
    //      it sat in front of that wave's points -- the last lanes of a launch have the fewest points (none when the lanes outnumber them)
    const bool edge_wg = rank == team - 1;
    if (edge_wg && tid >= OP_NT - 64) {                                     // (the last wave: the one that takes the edges in every sweep)
        double cc = po_edges_setup(P, pi, tid - (OP_NT - 64), &s_ne, s_eSide, &s_eC[0][0], &s_eM[0][0], &s_eG[0][0], &s_eW[0][0], s_Hc, s_J);
        cc = wave_sum_d(cc);
        if (tid == OP_NT - 64) lds_addd((MS_LDS double *)&s_const, cc);
    }
    __syncthreads();
    const int ne = edge_wg ? s_ne : 0, et = tid - (OP_NT - 64);             // lane et of the last wave takes edge et
    // The workgroups of a team exchange nothing but their partial sums (points, records and trial points belong to the workgroup that owns the lane group):
    // these go through agent-scope atomic stores and loads, which are coherent across the XCDs' L2s by themselves, so the team barriers carry no L2 write-back
    // and no invalidate (team_sync_light) -- the observation data stays in the caches from sweep to sweep
    auto put = [](double *q, double v) { __hip_atomic_store(reinterpret_cast<unsigned long long *>(q), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto get = [](const double *q) { return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); };
    // ---- sums over the team: the LDS accumulators s_acc[lo .. hi) (contributions of this workgroup) -> s_sum[lo .. hi), the same bits in every
    //      workgroup (partials combined in rank order); slot OP_MAX is combined as a maximum
    // after the barrier every thread fetches one or two of the partials (value tid & 63 of ranks tid >> 6, + 8: the loads of one thread wait for each other),
    // the eight rows meet in LDS
    auto team_combine = [&](const double *part, double mine, bool mine_slot) {
        const int k = tid & 63, r0 = tid >> 6;
        double v = 0;
        for (int r = r0; r < team; r += OP_NW) { const double x = get(part + (size_t)r * OP_NV + k); v = k == OP_MAX ? fmax(v, x) : v + x; }
        s_part[r0 * OP_NV + k] = v;
        __syncthreads();
        if (mine_slot) {
            double t = s_part[tid];
            for (int r = 1; r < OP_NW; ++r) t = tid == OP_MAX ? fmax(t, s_part[r * OP_NV + tid]) : t + s_part[r * OP_NV + tid];
            mine = t;
        }
        return mine;
    };
    auto vec_reduce = [&](int lo, int hi, bool with_max) {
        __syncthreads();
        const bool mine_slot = (tid >= lo && tid < hi) || (with_max && tid == OP_MAX);
        double mine = 0;
        if (mine_slot) { mine = s_acc[tid]; s_acc[tid] = 0; }
        if (team > 1) {
            double *part = P.op_red + (size_t)(seq & 1) * team * OP_NV;
            if (mine_slot) put(part + (size_t)rank * OP_NV + tid, mine);
            team_sync_light(P, team);
            mine = team_combine(part, mine, mine_slot);
        }
        ++seq;
        if (mine_slot) s_sum[tid] = mine;
        __syncthreads();
    };
    // two plain sums (fixed order: lanes, waves, ranks) -> s_sum[28], s_sum[29]
    auto pair_reduce = [&](double a, double b) {
        a = wave_sum_d(a); b = wave_sum_d(b);
        __syncthreads();
        if (lane == 0) { s_w[2 * wave] = a; s_w[2 * wave + 1] = b; }
        __syncthreads();
        double mine = 0;
        const bool mine_slot = tid == 28 || tid == 29;
        if (mine_slot) { for (int w = 0; w < OP_NW; ++w) mine += s_w[2 * w + tid - 28]; }
        if (team > 1) {
            double *part = P.op_red + (size_t)(seq & 1) * team * OP_NV;
            if (mine_slot) put(part + (size_t)rank * OP_NV + tid, mine);
            team_sync_light(P, team);
            mine = team_combine(part, mine, mine_slot);
        }
        ++seq;
        if (mine_slot) s_sum[tid] = mine;
        __syncthreads();
    };
    auto load_pose = [&](int pc, const double (&cur)[7], double (&pz)[7]) {
        if (pc == pi) {
#pragma unroll
            for (int a = 0; a < 7; ++a) pz[a] = cur[a];
        } else if (lds_poses) {                                           // (explicit address spaces: a flat load would wait for the prefetched global data as well)
            const MS_LDS double *q = (const MS_LDS double *)op_lds + 7 * pc;
#pragma unroll
            for (int a = 0; a < 7; ++a) pz[a] = q[a];
        } else {
            const MS_GLOBAL double *q = (const MS_GLOBAL double *)P.pose0 + 7 * (size_t)pc;
#pragma unroll
            for (int a = 0; a < 7; ++a) pz[a] = q[a];
        }
    };
    // ---- robust chi2 of this lane's share of the observations [i0, i1) of a point at X, with the free pose at `cur`
    auto chi2_share = [&](int i0, int i1, const double (&X)[3], const double (&cur)[7], bool store) {
        double sum = 0;
        int ii = i0 + sub, pn = 0;
        double un = 0, vn = 0, fn = 0;
        if (ii < i1) { pn = o_pose[ii]; un = o_uvi[3 * (size_t)ii]; vn = o_uvi[3 * (size_t)ii + 1]; fn = o_uvi[3 * (size_t)ii + 2]; }
        while (ii < i1) {
            const int pc = pn, icur = ii;
            const double uvc[2] = {un, vn}, infc = fn;
            ii += G;
            if (ii < i1) { pn = o_pose[ii]; un = o_uvi[3 * (size_t)ii]; vn = o_uvi[3 * (size_t)ii + 1]; fn = o_uvi[3 * (size_t)ii + 2]; }
            double pz[7], e[2], r, w;
            load_pose(pc, cur, pz);
            proj_edge<false>(pz, X, uvc, e, nullptr, nullptr);
            const double chi2 = infc * (e[0] * e[0] + e[1] * e[1]);
            huber(chi2, P.huber, r, w);
            if (store) P.chi2_obs[o_idx[icur]] = chi2;
            sum += r;
        }
        return sum;
    };
    // the SE3 edges at the free pose `cur` (lanes < ne of the team's first workgroup): chi2, and with lin the gradient into the accumulators
    // (an edge's error at the accepted pose is the error of the trial that was accepted: it is kept, e_acc, and the linearisation only multiplies it)
    double e_acc[6] = {0, 0, 0, 0, 0, 0}, e_try[6] = {0, 0, 0, 0, 0, 0};
    auto edge_part = [&](const double (&cur)[7], bool lin) {
        double sum = 0;
        if (et >= 0 && et < ne) {
            if (lin) {
#pragma unroll
                for (int a = 0; a < 6; ++a) { double v = 0; for (int c = 0; c < 6; ++c) v += s_eG[et][6 * a + c] * e_acc[c]; lds_addd(acc + 21 + a, v); }
            } else {
                double Bm[7], We[6];
                if (s_eSide[et] == 0) se3_mul(s_eC[et], cur, Bm);
                else { double Tjinv[7], A2[7]; se3_inv(cur, Tjinv); se3_mul(Tjinv, s_eM[et], A2); se3_mul(A2, s_eC[et], Bm); }
                se3_log(Bm, e_try);
                for (int i = 0; i < 6; ++i) { double v = 0; for (int j = 0; j < 6; ++j) v += s_eW[et][6 * i + j] * e_try[j]; We[i] = v; }
                for (int i = 0; i < 6; ++i) sum += e_try[i] * We[i];
            }
        }
        if (!lin && edge_wg && tid == 0) sum += s_const;
        return sum;
    };
    auto total_chi2 = [&](const double (&cur)[7], bool store) {          // at the accepted state
        double sum = 0;
        for (int rnd = 0; rnd < nrounds; ++rnd) {
            if (!ONE) point_begin(slot + rnd * nslot, false);
            sum += chi2_share(ps.i0, ps.i1, ps.X, cur, store);
        }
        sum += edge_part(cur, false);
        pair_reduce(sum, 0.0);
        return s_sum[28];
    };
    // ---- the point's part of the damped system: -W (Hll + lambda I)^-1 W^T (upper triangle, 21) and -W (Hll + lambda I)^-1 bl (6)
    auto schur_point = [&](double lambda, double (&Sv)[27]) {
        Chol3 c;
        const bool sound = chol3(ps.H, lambda, c);
        const double u0 = ps.bl[0] * c.i11, u1 = (ps.bl[1] - c.l21 * u0) * c.i22, u2 = (ps.bl[2] - c.l31 * u0 - c.l32 * u1) * c.i33;
        double Z[18];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const double z0 = ps.W[3 * r] * c.i11, z1 = (ps.W[3 * r + 1] - z0 * c.l21) * c.i22, z2 = (ps.W[3 * r + 2] - z0 * c.l31 - z1 * c.l32) * c.i33;
            Z[3 * r] = z0; Z[3 * r + 1] = z1; Z[3 * r + 2] = z2;
            Sv[21 + r] = -(z0 * u0 + z1 * u1 + z2 * u2);
        }
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b2 = a; b2 < 6; ++b2) { Sv[k] = -(Z[3 * a] * Z[3 * b2] + Z[3 * a + 1] * Z[3 * b2 + 1] + Z[3 * a + 2] * Z[3 * b2 + 2]); ++k; }
        return sound;
    };
    // one point's Schur terms into the accumulators (the group's first lane contributes); wave-uniform call
    auto schur_stage = [&](bool live, double lambda) {
        double Sv[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) Sv[k] = 0;
        bool contributes = false;
        if (live && sub == 0 && ps.pfree) {
            if (ps.nf > 0) { contributes = true; if (!schur_point(lambda, Sv)) lds_addd(acc + OP_BAD, 1.0); }
            else { Chol3 c; if (!chol3(ps.H, lambda, c)) lds_addd(acc + OP_BAD, 1.0); }
        }
        const unsigned long long m = __ballot(contributes);
        if (contributes) slab_put(slab, cap, acc + OP_S0, lanes_below(m), Sv);
        slab_sum(slab, cap, acc + OP_S0, (int)__popcll(m), lane);
    };
    auto rec_store = [&](int l) {
#pragma unroll
        for (int q = 0; q < 6; ++q) rec[(size_t)q * n_point + l] = ps.H[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) rec[(size_t)(6 + q) * n_point + l] = ps.bl[q];
        if (ps.nf > 0) {
#pragma unroll
            for (int q = 0; q < 18; ++q) rec[(size_t)(9 + q) * n_point + l] = ps.W[q];
        }
        rec[(size_t)27 * n_point + l] = ps.pfree ? (double)ps.nf : -1.0;
    };
    auto rec_load = [&](int l) {
        const double nfv = rec[(size_t)27 * n_point + l];
        ps.nf = nfv > 0 ? (int)nfv : 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) ps.H[q] = rec[(size_t)q * n_point + l];
#pragma unroll
        for (int q = 0; q < 3; ++q) ps.bl[q] = rec[(size_t)(6 + q) * n_point + l];
        if (nfv > 0) {
#pragma unroll
            for (int q = 0; q < 18; ++q) ps.W[q] = rec[(size_t)(9 + q) * n_point + l];
        }
    };
    double lambda = 0, ni = 2;
    int it = 0, trials = 0, stop = 0;
    long long cyc[6] = {0, 0, 0, 0, 0, 0}, tq = clock64();                 // 0 chi2 sweeps, 1 linearise (+ Schur terms), 2 the reduction after it, 3 6 x 6 solve, 4 points + trial chi2, 5 the reduction after it
    const long long t_begin = tq;
#define OP_LAP(i) do { const long long t_ = clock64(); cyc[i] += t_ - tq; tq = t_; } while (0)
    const double chi2_init = total_chi2(pose, false);
#pragma unroll
    for (int a = 0; a < 6; ++a) e_acc[a] = e_try[a];
    OP_LAP(0);
    double chi2_carried = chi2_init;
    for (it = 0; it < P.max_iters; ++it) {
        double current = chi2_carried, temp = current;
        // ---- linearisation: per point Hll, bl, W; the free pose's block and gradient (A: 21 + 6, this lane's part).  From the second iteration on lambda is
        //      known and the points' Schur terms follow in the same pass: one reduction instead of two
        double md = 0;
        for (int rnd = 0; rnd < nrounds; ++rnd) {
            const int l = slot + rnd * nslot;
            const bool live = l < n_point;
            if (!ONE) point_begin(l, false);
#pragma unroll
            for (int q = 0; q < 6; ++q) ps.H[q] = 0;
#pragma unroll
            for (int q = 0; q < 3; ++q) ps.bl[q] = 0;
#pragma unroll
            for (int q = 0; q < 18; ++q) ps.W[q] = 0;
            const int i1 = ps.i1;
            int jj = i1, jj2 = i1;                                       // this lane's first and second observation in the free keyframe
            bool more = false;                                           // ... and there are further ones (found by scanning: never in a SLAM window, where a keyframe sees a point once)
            double fu = 0, fv = 0, finf = 0;                             // the first one's measurement stays in registers (a reload after the loop is a round trip to L2)
            bool fkept = false;
            if (ps.pfree) {                                              // the point's own block and gradient: every observation of the share
                int ii = ps.i0 + sub, pn = 0;
                double un = 0, vn = 0, fn = 0;
                if (ii < i1) { pn = o_pose[ii]; un = o_uvi[3 * (size_t)ii]; vn = o_uvi[3 * (size_t)ii + 1]; fn = o_uvi[3 * (size_t)ii + 2]; }
                while (ii < i1) {
                    const int pc = pn;
                    const double uvc[2] = {un, vn}, infc = fn;
                    if (pc == pi) { if (jj == i1) { jj = ii; fu = un; fv = vn; finf = fn; fkept = true; } else if (jj2 == i1) jj2 = ii; else more = true; }
                    ii += G;
                    if (ii < i1) { pn = o_pose[ii]; un = o_uvi[3 * (size_t)ii]; vn = o_uvi[3 * (size_t)ii + 1]; fn = o_uvi[3 * (size_t)ii + 2]; }
                    double pz[7], e[2], Jp[12], Jl[6], r, w;
                    load_pose(pc, pose, pz);
                    proj_edge<true>(pz, ps.X, uvc, e, Jp, Jl);
                    const double chi2 = infc * (e[0] * e[0] + e[1] * e[1]);
                    huber(chi2, P.huber, r, w);
                    const double wi = w * infc;
                    ps.H[0] += wi * (Jl[0] * Jl[0] + Jl[3] * Jl[3]); ps.H[1] += wi * (Jl[0] * Jl[1] + Jl[3] * Jl[4]); ps.H[2] += wi * (Jl[0] * Jl[2] + Jl[3] * Jl[5]);
                    ps.H[3] += wi * (Jl[1] * Jl[1] + Jl[4] * Jl[4]); ps.H[4] += wi * (Jl[1] * Jl[2] + Jl[4] * Jl[5]); ps.H[5] += wi * (Jl[2] * Jl[2] + Jl[5] * Jl[5]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) ps.bl[c] -= wi * (Jl[c] * e[0] + Jl[3 + c] * e[1]);
                }
            } else { jj = ps.i0 + sub; while (jj < i1 && o_pose[jj] != pi) jj += G; more = true; }     // (a fixed point: its share is scanned)
            // the observations in the free keyframe once more (one lane in four has one; a wave-uniform loop): the pose's block and gradient go straight into the
            // wave's slab, W = Jp^T w Jl stays with the point -- keeping 27 more sums in registers through the loop above made the kernel spill
            int nf = 0, cnt = 0;
            for (;;) {
                const bool has = jj < i1;
                const unsigned long long m = __ballot(has);
                if (m == 0) break;
                if (has) {
                    if (!fkept) { fu = o_uvi[3 * (size_t)jj]; fv = o_uvi[3 * (size_t)jj + 1]; finf = o_uvi[3 * (size_t)jj + 2]; }
                    fkept = false;
                    const double uvc[2] = {fu, fv}, infc = finf;
                    double e[2], Jp[12], Jl[6], r, w, A[27];
                    proj_edge<true>(pose, ps.X, uvc, e, Jp, Jl);
                    const double chi2 = infc * (e[0] * e[0] + e[1] * e[1]);
                    huber(chi2, P.huber, r, w);
                    const double wi = w * infc;
                    int k = 0;
#pragma unroll
                    for (int a = 0; a < 6; ++a) {
                        A[21 + a] = -(Jp[a] * e[0] + Jp[6 + a] * e[1]) * wi;
#pragma unroll
                        for (int b2 = a; b2 < 6; ++b2) { A[k] = wi * (Jp[a] * Jp[b2] + Jp[6 + a] * Jp[6 + b2]); ++k; }
                    }
                    slab_put(slab, cap, acc, cnt + lanes_below(m), A);
                    if (ps.pfree) {
                        ++nf;
#pragma unroll
                        for (int r2 = 0; r2 < 6; ++r2)
#pragma unroll
                            for (int c = 0; c < 3; ++c) ps.W[3 * r2 + c] += wi * (Jp[r2] * Jl[c] + Jp[6 + r2] * Jl[3 + c]);
                    }
                    if (more && jj2 == i1) { jj += G; while (jj < i1 && o_pose[jj] != pi) jj += G; }      // the rare cases: scan on
                    else { jj = jj2; jj2 = i1; }
                }
                cnt += (int)__popcll(m);
            }
            slab_sum(slab, cap, acc, cnt, lane);
            ps.nf = group_sum_i(nf, lgG);
#pragma unroll
            for (int q = 0; q < 6; ++q) ps.H[q] = group_sum_d(ps.H[q], lgG);
#pragma unroll
            for (int q = 0; q < 3; ++q) ps.bl[q] = group_sum_d(ps.bl[q], lgG);
            if (ps.nf > 0) {
#pragma unroll
                for (int q = 0; q < 18; ++q) ps.W[q] = group_sum_d(ps.W[q], lgG);
            }
            if (live && sub == 0) {
                if (!ONE) rec_store(l);
                if (ps.pfree) md = fmax(md, fmax(fabs(ps.H[0]), fmax(fabs(ps.H[3]), fabs(ps.H[5]))));
            }
            if (it > 0) schur_stage(live, lambda);
        }
        (void)edge_part(pose, true);
        OP_LAP(1);
        if (edge_wg && tid < 21) lds_addd(acc + tid, s_Hc[tid]);          // the edges' constant J^T W J: into the sums, so that every workgroup of the team gets it
        if (it == 0) {
            for (int off = 32; off > 0; off >>= 1) md = fmax(md, __shfl_xor(md, off, 64));
            if (lane == 0) (void)atomicMax(reinterpret_cast<unsigned long long *>(&s_acc[OP_MAX]), (unsigned long long)__double_as_longlong(md));
        }
        vec_reduce(0, it == 0 ? 27 : OP_BAD + 1, it == 0);
        OP_LAP(2);
        const double *Hp = s_sum, *bp = s_sum + 21;                         // (they stay in LDS: 27 doubles in every thread's registers were a part of the kernel's spills)
        if (it == 0) {                                                       // computeLambdaInit: 1e-5 x the largest diagonal entry of the whole system
            const double mdp = fmax(fmax(fmax(fabs(Hp[0]), fabs(Hp[6])), fmax(fabs(Hp[11]), fabs(Hp[15]))), fmax(fabs(Hp[18]), fabs(Hp[20])));
            lambda = 1e-5 * fmax(mdp, s_sum[OP_MAX]); ni = 2;
        }
        double rho = 0;
        int qmax = 0;
        bool have_schur = it > 0;                                            // the Schur terms at this lambda are in s_sum already
        do {
            if (!have_schur) {
                for (int rnd = 0; rnd < nrounds; ++rnd) {
                    const int l = slot + rnd * nslot;
                    const bool live = l < n_point;
                    if (!ONE) { ps.pfree = false; ps.nf = 0; if (live && sub == 0) { ps.pfree = !(pfix && pfix[l]); if (ps.pfree) rec_load(l); } }
                    schur_stage(live, lambda);
                }
                OP_LAP(1);
                vec_reduce(OP_S0, OP_BAD + 1, false);
                OP_LAP(2);
            }
            have_schur = false;
            // (S + lambda I) dp = y: the 6 x 6 Cholesky by every thread for itself, as in k_ba_pose_only
            double Lm[21], dpv[6], yv[6];
            bool ok2 = s_sum[OP_BAD] == 0.0;
            {
                int k = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int c = a; c < 6; ++c) { Lm[c * (c + 1) / 2 + a] = Hp[k] + s_sum[OP_S0 + k] + (a == c ? lambda : 0.0); ++k; }
#pragma unroll
                for (int a = 0; a < 6; ++a) yv[a] = bp[a] + s_sum[OP_S0 + 21 + a];
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double d = Lm[j * (j + 1) / 2 + j];
#pragma unroll
                for (int k = 0; k < j; ++k) d -= Lm[j * (j + 1) / 2 + k] * Lm[j * (j + 1) / 2 + k];
                if (!(d > 0) || !isfinite(d)) ok2 = false;
                const double inv = rsqrt_d(d);
                Lm[j * (j + 1) / 2 + j] = inv;
#pragma unroll
                for (int i = j + 1; i < 6; ++i) {
                    double v = Lm[i * (i + 1) / 2 + j];
#pragma unroll
                    for (int k = 0; k < j; ++k) v -= Lm[i * (i + 1) / 2 + k] * Lm[j * (j + 1) / 2 + k];
                    Lm[i * (i + 1) / 2 + j] = v * inv;
                }
            }
            {
                double y2[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    double v = yv[i];
#pragma unroll
                    for (int k = 0; k < i; ++k) v -= Lm[i * (i + 1) / 2 + k] * y2[k];
                    y2[i] = v * Lm[i * (i + 1) / 2 + i];
                }
#pragma unroll
                for (int i = 5; i >= 0; --i) {
                    double v = y2[i];
#pragma unroll
                    for (int k = i + 1; k < 6; ++k) v -= Lm[k * (k + 1) / 2 + i] * dpv[k];
                    dpv[i] = v * Lm[i * (i + 1) / 2 + i];
                }
            }
            double trial_pose[7];
#pragma unroll
            for (int a = 0; a < 7; ++a) trial_pose[a] = pose[a];
            OP_LAP(3);
            if (ok2) {
                double ex[7], sc = 0, sum = 0;
                se3_exp(dpv, ex);
                se3_mul(ex, pose, trial_pose);
                if (gl == 0) { for (int a = 0; a < 6; ++a) sc += dpv[a] * (lambda * dpv[a] + bp[a]); }
                // ---- the points follow: dl = (Hll + lambda I)^-1 (bl - W^T dp), the trial point, its share of the gain denominator and the chi2 of its observations
                for (int rnd = 0; rnd < nrounds; ++rnd) {
                    const int l = slot + rnd * nslot;
                    const bool live = l < n_point;
                    if (!ONE) { point_begin(l, false); if (live && ps.pfree) rec_load(l); }
                    double Xn[3] = {ps.X[0], ps.X[1], ps.X[2]};
                    if (live && ps.pfree) {
                        double r0 = ps.bl[0], r1 = ps.bl[1], r2 = ps.bl[2];
                        if (ps.nf > 0) {
#pragma unroll
                            for (int a = 0; a < 6; ++a) { r0 -= ps.W[3 * a] * dpv[a]; r1 -= ps.W[3 * a + 1] * dpv[a]; r2 -= ps.W[3 * a + 2] * dpv[a]; }
                        }
                        Chol3 c;
                        (void)chol3(ps.H, lambda, c);
                        const double v0 = r0 * c.i11, v1 = (r1 - c.l21 * v0) * c.i22, v2 = (r2 - c.l31 * v0 - c.l32 * v1) * c.i33;       // L^-1 r
                        const double d2 = v2 * c.i33, d1 = (v1 - c.l32 * d2) * c.i22, d0 = (v0 - c.l21 * d1 - c.l31 * d2) * c.i11;         // L^-T (L^-1 r)
                        if (sub == 0) sc += d0 * (lambda * d0 + ps.bl[0]) + d1 * (lambda * d1 + ps.bl[1]) + d2 * (lambda * d2 + ps.bl[2]);
                        Xn[0] += d0; Xn[1] += d1; Xn[2] += d2;
                    }
                    if (ONE) { Xt[0] = Xn[0]; Xt[1] = Xn[1]; Xt[2] = Xn[2]; }
                    else if (live && sub == 0) { trial[3 * (size_t)l] = Xn[0]; trial[3 * (size_t)l + 1] = Xn[1]; trial[3 * (size_t)l + 2] = Xn[2]; }
                    sum += chi2_share(ps.i0, ps.i1, Xn, trial_pose, false);
                }
                sum += edge_part(trial_pose, false);
                OP_LAP(4);
                pair_reduce(sum, sc);
                OP_LAP(5);
                temp = s_sum[28];
            } else temp = DBL_MAX;
            const double scale = (ok2 ? s_sum[29] : 0.0) + 1e-3;
            rho = (current - temp) / scale;
            if (trials < P.debug_reject) rho = -1.0;                // (test hook: drives the ten-rejections Terminate path)
            if (rho > 0 && isfinite(temp)) {
                const double t3 = 2 * rho - 1;
                double alpha = 1. - t3 * t3 * t3;                                          // (pow(x, 3) of the reference to an ulp or two)
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2; current = temp; chi2_carried = temp;
#pragma unroll
                for (int a = 0; a < 7; ++a) pose[a] = trial_pose[a];
#pragma unroll
                for (int a = 0; a < 6; ++a) e_acc[a] = e_try[a];
                if (ONE) { ps.X[0] = Xt[0]; ps.X[1] = Xt[1]; ps.X[2] = Xt[2]; }
                else {
                    for (int l = slot; l < n_point; l += nslot)
                        if (sub == 0) { point[3 * (size_t)l] = trial[3 * (size_t)l]; point[3 * (size_t)l + 1] = trial[3 * (size_t)l + 1]; point[3 * (size_t)l + 2] = trial[3 * (size_t)l + 2]; }
                    __syncthreads();                                        // the group's other lanes read the moved points next
                }
            } else {
                lambda *= ni; ni *= 2;
                if (!isfinite(lambda)) break;
            }
            ++qmax; ++trials;
        } while (rho < 0 && qmax < 10);
        if (qmax == 10 || rho == 0 || !isfinite(lambda)) { stop = 1; ++it; break; }
    }
    tq = clock64();
    const double chi2_final = total_chi2(pose, true);
    OP_LAP(0);
    if (ONE && slot < n_point && sub == 0) { point[3 * (size_t)slot] = ps.X[0]; point[3 * (size_t)slot + 1] = ps.X[1]; point[3 * (size_t)slot + 2] = ps.X[2]; }
    if (gl == 0) {
        const bool hung = team > 1 && __hip_atomic_load(P.flag + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;      // a team barrier gave up: the result is not to be trusted
        for (int a = 0; a < 7; ++a) P.pose[7 * (size_t)pi + a] = pose[a];
        P.stats[0] = it; P.stats[1] = trials; P.stats[2] = stop; P.stats[3] = lambda; P.stats[4] = chi2_init; P.stats[5] = hung ? NAN : chi2_final;
        P.stats[6] = (isfinite(chi2_final) && !hung) ? 1 : 0; P.stats[7] = hung ? 1 : 0;
        P.stats[15] = 0;
    }
    if (gl == 0) {                                                         // the phase stamps of the first wave
        P.stats[8] = (double)cyc[0]; P.stats[9] = (double)cyc[1]; P.stats[10] = (double)cyc[2]; P.stats[11] = (double)cyc[3]; P.stats[12] = (double)cyc[4];
        P.stats[13] = (double)(clock64() - t_begin); P.stats[14] = (double)cyc[5];
        P.stats[15] = (double)(t_begin - t_kernel);                           // what comes before the first sweep (not part of [13])
    }
#undef OP_LAP
}
