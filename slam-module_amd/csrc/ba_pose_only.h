#pragma once
// ba_pose_only.h -- pose-only problems: poseBundleAdjust.  k_ba_pose_only; po_edges_setup also serves k_ba_one_pose.
// Included by ba.hip only, inside its anonymous namespace, like ba_one_pose.h; both rely on ba.o's -ffp-contract=fast.

// ---------------------------------------------------------------- pose-only problems: poseBundleAdjust (bundle_adjuster.cpp:396-491)
// ONE free pose, every point fixed: the projection edges of the current frame (+ the odometry edge to the fixed previous keyframe, :440-447) give a 6 x 6
// system per trial.  The general kernel walks such a problem through ~20 phases with a workgroup barrier and a round trip to memory each (0.47 ms for
// 12 iterations of a 6-dof problem -- and poseBundleAdjust runs on EVERY non-keyframe, mapper_helpers.cpp:1043-1050); here a 256-thread workgroup keeps
// the trial in registers: one sweep over the observations accumulates H (21 entries), b and the robust chi2 per thread, one reduction, lane 0 factors the
// 6 x 6 matrix, one more sweep gives the chi2 of the moved pose.  Same LM schedule, same arithmetic per edge as k_ba_lm.
// Round 4: the stamps showed 45 % of the kernel in its reductions (28 sums x 6 ds_bpermute steps, three barriers per sweep), 20 % in the observations and 18 % in
// the one SE3 edge's logarithm on the thread that also had the most observations -- and two sweeps per iteration where one is enough:
//   * every sweep linearises.  The trial's sweep at the moved pose already holds H and b of the NEXT iteration when the trial is accepted (g2o linearises the
//     same state again, optimizable_graph / sparse_optimizer computeActiveErrors + linearizeSystem), and a rejected trial keeps the old H, b in registers: 1 + trials
//     sweeps instead of 2 + iterations + trials, and the per-observation chi2 of the accepted state stays in registers, so the closing sweep goes too;
//   * the 28 sums go through LDS transposed: every thread writes its 28 partial sums (value-major rows of PO_ROW doubles), 8 lanes per value add 32 entries each
//     and meet over the DPP network (3 steps): two barriers, ~100 instructions;
//   * waves 0-2 take the observations (PO_K per thread in registers), wave 3 takes the SE3 edges, so the logarithm runs beside the observations.  One wave per
//     SIMD: the whole 512-register file is each wave's (a 512-thread version, two waves per SIMD, spilled ~200 dwords per trial and was no faster than round 3's).
constexpr int PO_NT = 256, PO_OT = 192, PO_K = 8, PO_MAXE = 8, PO_NV = 28;       // threads; threads with observations; observations a thread keeps in registers; SE3 edges; sums per sweep
constexpr int PO_ROW = PO_NT + 8;                            // row stride (doubles) of the transposed partial sums: 8 mod 32, so the 8 values x 8 parts a wave reads spread over all banks
constexpr size_t kPoLdsBytes = (size_t)PO_NV * PO_ROW * sizeof(double);
static_assert(8 * PO_NV <= PO_NT, "stage 2 of the reduction: 8 lanes per sum");

// The SE3 edges of a problem with ONE free pose (k_ba_pose_only, k_ba_one_pose), once per solve, by ONE wave (all its lanes): an edge between fixed poses is a constant chi2
// (returned: every lane's share); one that touches
// the free pose leaves its fixed side's transform, G = -J^T W and J^T W J = -G J in LDS.  Only the free side's Jacobian is formed (Ji = adj(Tj^-1 M) or
// Jj = -adj(Ti^-1 M^-1): no logarithm), and the two 6 x 6 products are spread over the lanes -- as the work of one thread (two Jacobians in scratch, 970 dependent
// multiply-adds) this was 44 k cycles, a third of the whole kernel.
__device__ __noinline__ double po_edges_setup(const BaProb &P, int pi, int lane, int *s_ne, int *s_eSide, double *s_eC, double *s_eM, double *s_eG, double *s_eW, double *s_Hc, double *s_J) {
    double cacc = 0;
    int ne = 0;
    for (int k = lane; k < P.n_edge; k += 64) {                             // the edges between fixed poses (a window's stage 1 has ~50): one per lane
        const int vi = P.edge_i[k], vj = P.edge_j[k];
        if (vi == pi || vj == pi) continue;
        const double *W = P.edge_info + 36 * (size_t)k;
        double e[6];
        pose_edge(P.pose0 + 7 * (size_t)vi, P.pose0 + 7 * (size_t)vj, P.edge_meas + 7 * (size_t)k, e, nullptr, nullptr, false);
        for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) cacc += e[i] * W[6 * i + j] * e[j];
    }
    // the edges of the free pose: found 64 at a time (a ballot over the lanes' edges -- a scan with one dependent load per edge was 35 us for a window's 50 edges), then
    // taken by the wave together
    for (int k0 = 0; k0 < P.n_edge; k0 += 64) {
      const int kl = k0 + lane;
      unsigned long long touching = __ballot(kl < P.n_edge && (P.edge_i[kl] == pi || P.edge_j[kl] == pi));
      while (touching) {
        const int k = k0 + __builtin_ctzll(touching);
        touching &= touching - 1;
        const int vi = P.edge_i[k], vj = P.edge_j[k];
        const double *W = P.edge_info + 36 * (size_t)k, *M = P.edge_meas + 7 * (size_t)k, *Ti = P.pose0 + 7 * (size_t)vi, *Tj = P.pose0 + 7 * (size_t)vj;
        const int sl = ne++, side = vi == pi ? 0 : 1;
        double C7[7], J[36];
        if (side == 0) { double Tjinv[7]; se3_inv(Tj, Tjinv); se3_mul(Tjinv, M, C7); se3_adj(C7, J); }
        else { double Tiinv[7], Minv[7]; se3_inv(Ti, Tiinv); se3_inv(M, Minv); se3_mul(Tiinv, Minv, C7); se3_adj(C7, J); for (int i = 0; i < 36; ++i) J[i] = -J[i]; }
        if (lane == 0) {
            s_eSide[sl] = side;
            if (side == 0) for (int i = 0; i < 7; ++i) s_eC[8 * sl + i] = C7[i];
            else for (int i = 0; i < 7; ++i) { s_eC[8 * sl + i] = Ti[i]; s_eM[8 * sl + i] = M[i]; }
            for (int i = 0; i < 36; ++i) s_J[i] = J[i];
        }
        if (lane < 36) s_eW[36 * sl + lane] = W[lane];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
        if (lane < 36) {                                                    // G = -J^T W
            const int a2 = lane / 6, c = lane % 6;
            double v = 0;
            for (int r2 = 0; r2 < 6; ++r2) v += s_J[6 * r2 + a2] * s_eW[36 * sl + 6 * r2 + c];
            s_eG[36 * sl + lane] = -v;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
        if (lane < 21) {                                                    // J^T W J = -G J packed by (a <= b) at a (11 - a) / 2 + b; the value is entry (b, a), the LOWER
            int a2 = 0, rest = lane;                                        // triangle -- the one the general kernel's Cholesky and the oracle read: it matters for a W that
            while (rest >= 6 - a2) { rest -= 6 - a2; ++a2; }                // is not symmetric (mi355slam.h: W is taken as given)
            const int b2 = a2 + rest;
            double v = 0;
            for (int c = 0; c < 6; ++c) v += s_eG[36 * sl + 6 * b2 + c] * s_J[6 * c + a2];
            s_Hc[lane] -= v;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
      }
    }
    if (lane == 0) *s_ne = ne;
    return cacc;
}

__global__ __launch_bounds__(PO_NT) void k_ba_pose_only(const BaProb *probs) {
    extern __shared__ __attribute__((aligned(16))) double po_red[];         // [PO_NV][PO_ROW]
    __shared__ __attribute__((aligned(16))) double s_sum[2][32];       // the sums of the last two sweeps: [cur] belongs to the accepted state (its H and b), the other to the trial
    __shared__ double s_eC[PO_MAXE][8], s_eM[PO_MAXE][8], s_eG[PO_MAXE][36], s_eW[PO_MAXE][36], s_Hc[24], s_const;
    __shared__ int s_eSide[PO_MAXE], s_ne, s_any;
    __shared__ double s_J[36];
    const long long t_kernel = clock64();
    const BaProb &P = probs[blockIdx.x];
    const int tid = threadIdx.x, pi = P.free2pose[0];
    // the block ms_ba_download fetches -- [16 stats][7 n_pose poses][3 n_point points][n_obs chi2] -- is filled as the values arise (a single problem: BaProb::pack)
    MS_GLOBAL double *pk = (MS_GLOBAL double *)uglobal(P.pack);
    MS_GLOBAL double *pk_pose = pk + 16, *pk_point = pk_pose + 7 * P.n_pose, *pk_chi2 = pk_point + 3 * P.n_point;
    for (int i = tid; i < 7 * P.n_pose; i += PO_NT) { const double v = P.pose0[i]; P.pose[i] = v; if (pk) pk_pose[i] = v; }
    for (int i = tid; i < 3 * P.n_point; i += PO_NT) { const double v = P.point0[i]; P.point[i] = v; if (pk) pk_point[i] = v; }
    if (tid < 24) s_Hc[tid] = 0;
    if (tid == 0) { s_ne = 0; s_const = 0; s_any = P.n_obs; }
    __syncthreads();
    {   // the first observation of the free pose
        int mine = P.n_obs;
        for (int o = tid; o < P.n_obs; o += PO_NT) if (P.obs_pose[o] == pi) { mine = o; break; }
        if (mine < P.n_obs) atomicMin(&s_any, mine);
    }
    __syncthreads();
    double pose[7];
#pragma unroll
    for (int a = 0; a < 7; ++a) pose[a] = P.pose0[7 * (size_t)pi + a];
    // ---- what never changes: the observations of the free pose go into registers (PO_K per thread of waves 0-2), the others' chi2 and the edges between fixed
    //      poses into one constant; an edge that touches the free pose leaves its fixed side's transform, -J^T W and J^T W J in LDS (its Jacobian does not depend
    //      on the free pose: Ji = adj(Tj^-1 M), Jj = -adj(Ti^-1 M^-1)), so a sweep only takes its logarithm
    double X[PO_K][3], uv[PO_K][2], info[PO_K], c2[PO_K], c2t[PO_K], cacc = 0;
    unsigned have = 0;
    const int o_any = s_any;                                                // an observation of the free pose (n_obs: there is none)
    double Xd[3] = {0, 0, 1}, uvd[2] = {0, 0};
    if (o_any < P.n_obs) {
        const int l = P.obs_point[o_any];
        Xd[0] = P.point0[3 * (size_t)l]; Xd[1] = P.point0[3 * (size_t)l + 1]; Xd[2] = P.point0[3 * (size_t)l + 2];
        uvd[0] = P.obs_uv[2 * (size_t)o_any]; uvd[1] = P.obs_uv[2 * (size_t)o_any + 1];
    }
#pragma unroll
    for (int j = 0; j < PO_K; ++j) {
        const int o = tid + PO_OT * j;
        X[j][0] = Xd[0]; X[j][1] = Xd[1]; X[j][2] = Xd[2]; uv[j][0] = uvd[0]; uv[j][1] = uvd[1]; info[j] = c2[j] = c2t[j] = 0;
        if (tid < PO_OT && o < P.n_obs) {
            const int po = P.obs_pose[o], l = P.obs_point[o];
            if (po == pi) {
                have |= 1u << j;
                X[j][0] = P.point0[3 * (size_t)l]; X[j][1] = P.point0[3 * (size_t)l + 1]; X[j][2] = P.point0[3 * (size_t)l + 2];
                uv[j][0] = P.obs_uv[2 * (size_t)o]; uv[j][1] = P.obs_uv[2 * (size_t)o + 1]; info[j] = P.obs_info[o];
            }
        }
    }
    // slots this wave sweeps: observation tid + PO_OT j exists for j < (n_obs - tid) / PO_OT, most for the wave's first lane (wave 3, the edges' wave, and a problem
    // without observations of the free pose: none)
    const int w0 = __builtin_amdgcn_readfirstlane(tid & ~63);
    const int jn = (w0 < PO_OT && o_any < P.n_obs && P.n_obs > w0) ? min(PO_K, (P.n_obs - w0 + PO_OT - 1) / PO_OT) : 0;
    for (int o = tid; o < P.n_obs; o += PO_NT) {                            // observations from FIXED poses: constant
        const int po = P.obs_pose[o];
        if (po == pi) continue;
        double e[2], r, w;
        proj_edge<false>(P.pose0 + 7 * (size_t)po, P.point0 + 3 * (size_t)P.obs_point[o], P.obs_uv + 2 * (size_t)o, e, nullptr, nullptr);
        const double chi2 = P.obs_info[o] * (e[0] * e[0] + e[1] * e[1]);
        huber(chi2, P.huber, r, w);
        P.chi2_obs[o] = chi2;
        if (pk) pk_chi2[o] = chi2;
        cacc += r;
    }
    if (tid >= PO_OT) cacc += po_edges_setup(P, pi, tid - PO_OT, &s_ne, s_eSide, &s_eC[0][0], &s_eM[0][0], &s_eG[0][0], &s_eW[0][0], s_Hc, s_J);   // (wave 3, beside the observation loads)
    cacc = wave_sum_d(cacc);
    if ((tid & 63) == 0) lds_addd((MS_LDS double *)&s_const, cacc);
    __syncthreads();
    const int ne = s_ne;
    const bool overflow = P.n_obs > PO_OT * PO_K;                           // more observations than the registers take: those come from memory in every sweep
    const long long t_begin = clock64();
    int cur = 1;                                                            // which half of s_sum belongs to the accepted state
    // ---- one sweep over the free pose's edges at `pose`: the robust chi2 (returned), the upper triangle of H and b (left in s_sum[1 - cur][0 .. 27)), the chi2 per observation in c2t
    auto sweep = [&]() {
        double A[21], g[6], acc = 0;
#pragma unroll
        for (int a = 0; a < 21; ++a) A[a] = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) g[a] = 0;
        auto one = [&](const double *Xo, const double *uvo, double inf) {
            double e[2], Jp[12], Jl[6];
            proj_edge<true>(pose, Xo, uvo, e, Jp, Jl);
            const double chi2 = inf * (e[0] * e[0] + e[1] * e[1]);
            double r, w;
            huber(chi2, P.huber, r, w);
            acc += r;
            const double wi = w * inf;
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                g[a] += -(Jp[a] * e[0] + Jp[6 + a] * e[1]) * wi;
#pragma unroll
                for (int b2 = a; b2 < 6; ++b2) A[k++] += wi * (Jp[a] * Jp[b2] + Jp[6 + a] * Jp[6 + b2]);
            }
            return chi2;
        };
        // slots in pairs, both evaluations in one basic block so that the scheduler interleaves their chains (a lone wave per SIMD has nothing else to hide the
        // fp64 latency with); a slot without an observation holds a copy of a real one with information 0: finite arithmetic, nothing added
#pragma unroll
        for (int j = 0; j < PO_K; j += 2) {
            if (j + 1 < jn) { c2t[j] = one(X[j], uv[j], info[j]); c2t[j + 1] = one(X[j + 1], uv[j + 1], info[j + 1]); }
            else if (j < jn) c2t[j] = one(X[j], uv[j], info[j]);
        }
        if (overflow && tid < PO_OT)
            for (int o = tid + PO_OT * PO_K; o < P.n_obs; o += PO_OT) {
                if (P.obs_pose[o] != pi) continue;
                const double Xo[3] = {P.point0[3 * (size_t)P.obs_point[o]], P.point0[3 * (size_t)P.obs_point[o] + 1], P.point0[3 * (size_t)P.obs_point[o] + 2]};
                const double uvo[2] = {P.obs_uv[2 * (size_t)o], P.obs_uv[2 * (size_t)o + 1]};
                (void)one(Xo, uvo, P.obs_info[o]);
            }
        if (tid >= PO_OT && tid - PO_OT < ne) {                             // wave 3: the SE3 edges of the free pose
            const int k = tid - PO_OT;
            double Bm[7], e[6], We[6];
            if (s_eSide[k] == 0) se3_mul(s_eC[k], pose, Bm);                                      // (Tj^-1 M) Ti
            else { double Tjinv[7], A2[7]; se3_inv(pose, Tjinv); se3_mul(Tjinv, s_eM[k], A2); se3_mul(A2, s_eC[k], Bm); }
            se3_log(Bm, e);
            for (int i = 0; i < 6; ++i) { double v = 0; for (int j = 0; j < 6; ++j) v += s_eW[k][6 * i + j] * e[j]; We[i] = v; }
            for (int i = 0; i < 6; ++i) acc += e[i] * We[i];
            for (int a = 0; a < 6; ++a) { double v = 0; for (int c = 0; c < 6; ++c) v += s_eG[k][6 * a + c] * e[c]; g[a] += v; }
        }
        {
            MS_LDS double *row = (MS_LDS double *)po_red + tid;
#pragma unroll
            for (int a = 0; a < 21; ++a) row[a * PO_ROW] = A[a];
#pragma unroll
            for (int a = 0; a < 6; ++a) row[(21 + a) * PO_ROW] = g[a];
            row[27 * PO_ROW] = acc;
        }
        __syncthreads();
        if (tid < 8 * PO_NV) {                                              // lanes 8 v .. 8 v + 7 add row v up, each 32 entries, then among themselves
            const int v = tid >> 3, part = tid & 7;
            const MS_LDS double *row = (const MS_LDS double *)po_red + v * PO_ROW + part;
            double s0 = 0, s1 = 0;
#pragma unroll
            for (int k = 0; k < PO_NT / 8; k += 2) { s0 += row[8 * k]; s1 += row[8 * k + 8]; }
            double s = s0 + s1;
            s += dpp_d<0xB1>(s);                                            // quad_perm [1 0 3 2]
            s += dpp_d<0x4E>(s);                                            // quad_perm [2 3 0 1]
            s += dpp_d<0x141>(s);                                           // row_half_mirror
            if (part == 0) s_sum[1 - cur][v] = s + (v < 21 ? s_Hc[v] : (v == 27 ? s_const : 0.0));
        }
        __syncthreads();
        return s_sum[1 - cur][27];
    };
    double lambda = 0, ni = 2;
    int it = 0, trials = 0, stop = 0;
    auto accept = [&]() {                                                   // the swept state becomes the current one: its H, b (the other half of s_sum) and per-observation chi2
        cur = 1 - cur;
#pragma unroll
        for (int j = 0; j < PO_K; ++j) c2[j] = c2t[j];
    };
    const double chi2_init = sweep();
    accept();
    double chi2_carried = chi2_init;
    for (it = 0; it < P.max_iters; ++it) {
        double current = chi2_carried, temp = current;
        if (it == 0) {                                                       // computeLambdaInit: 1e-5 x the largest diagonal entry
            const double *H = s_sum[cur];
            const double md = fmax(fmax(fmax(fabs(H[0]), fabs(H[6])), fmax(fabs(H[11]), fabs(H[15]))), fmax(fabs(H[18]), fabs(H[20])));
            lambda = 1e-5 * md; ni = 2;
        }
        double rho = 0;
        int qmax = 0;
        do {
            // (H + lambda I) dp = b: Cholesky of the 6 x 6 matrix, by every thread for itself (fully unrolled: 21 + 6 registers, ~150 dependent operations --
            // cheaper than one thread doing it behind a barrier and a trip through LDS)
            double Lm[21], dpv[6], b[6];                                     // lower triangle, row-major: Lm[i (i + 1) / 2 + j]
            bool ok2 = true;
            const double *H = s_sum[cur];
#pragma unroll
            for (int a = 0; a < 6; ++a) b[a] = H[21 + a];
            {
                int k = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int c = a; c < 6; ++c) { Lm[c * (c + 1) / 2 + a] = H[k] + (a == c ? lambda : 0.0); ++k; }
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double d = Lm[j * (j + 1) / 2 + j];
#pragma unroll
                for (int k = 0; k < j; ++k) d -= Lm[j * (j + 1) / 2 + k] * Lm[j * (j + 1) / 2 + k];
                if (!(d > 0) || !isfinite(d)) ok2 = false;
                const double inv = rsqrt_d(d);
                Lm[j * (j + 1) / 2 + j] = inv;                               // the reciprocal pivot is what the substitutions use
#pragma unroll
                for (int i = j + 1; i < 6; ++i) {
                    double v = Lm[i * (i + 1) / 2 + j];
#pragma unroll
                    for (int k = 0; k < j; ++k) v -= Lm[i * (i + 1) / 2 + k] * Lm[j * (j + 1) / 2 + k];
                    Lm[i * (i + 1) / 2 + j] = v * inv;
                }
            }
            {
                double y[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    double v = b[i];
#pragma unroll
                    for (int k = 0; k < i; ++k) v -= Lm[i * (i + 1) / 2 + k] * y[k];
                    y[i] = v * Lm[i * (i + 1) / 2 + i];
                }
#pragma unroll
                for (int i = 5; i >= 0; --i) {
                    double v = y[i];
#pragma unroll
                    for (int k = i + 1; k < 6; ++k) v -= Lm[k * (k + 1) / 2 + i] * dpv[k];
                    dpv[i] = v * Lm[i * (i + 1) / 2 + i];
                }
            }
            double bk[7], sc = 0;
#pragma unroll
            for (int a = 0; a < 7; ++a) bk[a] = pose[a];                                    // push()
            if (ok2) {
                double dp[6], ex[7];
#pragma unroll
                for (int a = 0; a < 6; ++a) { dp[a] = dpv[a]; sc += dp[a] * (lambda * dp[a] + b[a]); }
                se3_exp(dp, ex);
                se3_mul(ex, bk, pose);                                                      // every thread moves its own copy of the pose: the same arithmetic, the same result
                temp = sweep();
            } else temp = DBL_MAX;
            const double scale = sc + 1e-3;
            rho = (current - temp) / scale;
            if (trials < P.debug_reject) rho = -1.0;                // (test hook: drives the ten-rejections Terminate path)
            if (rho > 0 && isfinite(temp)) {
                const double t3 = 2 * rho - 1;
                double alpha = 1. - t3 * t3 * t3;                                          // (pow(x, 3) of the reference to an ulp or two, without the ~300 instructions of pow)
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2; current = temp; chi2_carried = temp;
                accept();                                                                   // (the trial's half of s_sum becomes the current one; the next sweep writes the other, behind its first barrier)
            } else {
                lambda *= ni; ni *= 2;
#pragma unroll
                for (int a = 0; a < 7; ++a) pose[a] = bk[a];                                // pop()
                if (!isfinite(lambda)) break;
            }
            ++qmax; ++trials;
        } while (rho < 0 && qmax < 10);
        if (qmax == 10 || rho == 0 || !isfinite(lambda)) { stop = 1; ++it; break; }
    }
    // the chi2 per observation of the accepted state: from the registers; the observations beyond them are evaluated once more
#pragma unroll
    for (int j = 0; j < PO_K; ++j) if ((have >> j) & 1u) { P.chi2_obs[tid + PO_OT * j] = c2[j]; if (pk) pk_chi2[tid + PO_OT * j] = c2[j]; }
    if (overflow && tid < PO_OT)
        for (int o = tid + PO_OT * PO_K; o < P.n_obs; o += PO_OT) {
            if (P.obs_pose[o] != pi) continue;
            double e[2], Jp[12], Jl[6];
            proj_edge<true>(pose, P.point0 + 3 * (size_t)P.obs_point[o], P.obs_uv + 2 * (size_t)o, e, Jp, Jl);     // (the arithmetic of the sweeps)
            P.chi2_obs[o] = P.obs_info[o] * (e[0] * e[0] + e[1] * e[1]);
            if (pk) pk_chi2[o] = P.chi2_obs[o];
        }
    const double chi2_final = chi2_carried;                                 // the sweep that was accepted last evaluated exactly this state
    if (tid == PO_OT) { P.stats[9] = 0.0; if (pk) pk[9] = 0.0; }
    if (tid == 0) {
        // [8 .. 12] are zero ([9] is written by thread PO_OT, above); [13], [14]: cycles of the iterations and of what came before them
        const double st[16] = {(double)it, (double)trials, (double)stop, lambda, chi2_init, chi2_final, isfinite(chi2_final) ? 1.0 : 0.0, 0.0,
                               0.0, 0.0, 0.0, 0.0, 0.0, (double)(clock64() - t_begin), (double)(t_begin - t_kernel), 0.0};
        for (int a = 0; a < 7; ++a) { P.pose[7 * (size_t)pi + a] = pose[a]; if (pk) pk_pose[7 * (size_t)pi + a] = pose[a]; }
#pragma unroll
        for (int q = 0; q < 16; ++q) if (q != 9) { P.stats[q] = st[q]; if (pk) pk[q] = st[q]; }
    }
}
