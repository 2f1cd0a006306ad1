#pragma once
// ba_prep.h -- host side: what ms_ba_create builds per problem (the ba_* steps below, in the order they run) and the device block of a handle.
// Its last function names the three solvers: k_ba_lm, k_ba_pose_only, k_ba_one_pose.

// ---------------------------------------------------------------- what ms_ba_create builds per problem (the ba_* steps below, in the order they run)
// One pass set of the fused Schur phase on the host (FsSet is what the kernels see of it)
struct FsHost {
    bvec<int32_t> row0, row1, yoff, rowoff;                  // passes: their rows, their tile layout
    bvec<int32_t> batch_start, b_obs_start, b_run_start, b_fmt, pobs;
    bvec<double> puv;
    bvec<uint16_t> pairs;
    bool by_points = false;
};
struct Prep {
    int np_free = 0;
    bvec<int32_t> pidx, free2pose;                            // free-pose index
    bvec<int32_t> pt_start, pt_obs, fstart, fobs;             // CSR by point and by free pose
    int auto_team = 1;                                        // what ms_ba_solve will pick on its own (ba_auto_team): a handle that gets teams builds no streams, and only the fine pass set
    bvec<int32_t> fo_lo, op_pose, op_o;                       // the streams; the one-pose kernel's arrays
    bvec<double> fo_uvi, op_uvi;
    bool one_pose = false, pose_only = false;                 // the two shapes with ONE free pose: with free points (k_ba_one_pose), without (k_ba_pose_only)
    bool fused = false;                                       // the fused Schur pass (else the record-based list below)
    bvec<int32_t> chunk_items, seg_start, seg_pair;
    int n_chunks = 0, n_seg = 0;
    bvec<int32_t> env16, act_start, act_blk;                  // 16-row envelope and panel lists
    double chol_tiles = 0;
    bvec<int32_t> fs_cs;
    int fs_only = 0;                                          // the one pass set that is built
    FsHost fs[2];
    bvec<int32_t> cw_slot, cw_act_start, cw_act, cw_load_start, cw_load;      // windowed Cholesky
    int cw_W = 0;
    bool cw_zglobal = false, cw_meta_lds = false;
    size_t in_lo = 0, in_hi = 0, copy_lo = 0, copy_hi = 0;    // the problem's input range of the device block, and its entries of BaLayout::copies
};
// Envelope of the reduced camera matrix at pose level, and the free observations of every free point sorted by free pose (flat arrays: the fused Schur pass is built from them)
struct BaEnvelope {
    bvec<int> first;                                          // the first free pose each free pose is coupled with (a shared point or a pose-pose edge)
    bvec<int> hfirst;                                         // ... by a pose-pose EDGE (Hpp has nothing left of that block)
    bvec<int32_t> fp_start, fp_f, fp_o;
};
// MS_BA_TIMING: where the host time of a create goes.  A BaLap adds the time between its construction and its end to one slot.
struct BaTimes {
    enum Slot { kCsrEnvelope, kLists, kFused, kPasses, kPointKeys, kSort, kBatches, kValues, kSlots };
    const char *const mode = std::getenv("MS_BA_TIMING");     // prints the host index build and the allocation + upload time of every create to stderr
    double part[kSlots] = {};
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
};
struct BaLap {
    BaTimes &t;
    const int slot;
    const double t0;
    BaLap(BaTimes &times, int s) : t(times), slot(s), t0(times.mode ? BaTimes::now() : 0.0) {}
    ~BaLap() { if (t.mode) t.part[slot] += BaTimes::now() - t0; }
};
// The team size ms_ba_solve picks on its own for the general kernel: as many workgroups per problem as fit the chip beside the other problems, at most 32 (beyond that
// the single-workgroup Cholesky dominates); small problems are latency-bound on the barriers.  ms_ba_create builds for the regime this predicts.
static int ba_auto_team(int n_obs, int cus, int n) { return std::max(1, std::min(std::min(32, std::max(1, n_obs / 512)), cus / std::max(n, 1))); }
static int ba_check_problem(ms_ctx *c, const ms_ba_problem &Q, int p, Prep &R) {
    if (Q.n_pose < 1 || Q.n_point < 0 || Q.n_obs < 0 || Q.n_pose_edge < 0 || !Q.pose || !Q.pose_fixed || (Q.n_point && !Q.point) ||
        (Q.n_obs && (!Q.obs_pose || !Q.obs_point || !Q.obs_uv || !Q.obs_info)) || (Q.n_pose_edge && (!Q.edge_i || !Q.edge_j || !Q.edge_meas || !Q.edge_info)))
        return ms_fail(c, MS_ERR_INVALID, "ms_ba_create: problem %d has missing arrays", p);
    R.pidx.assign(Q.n_pose, -1);
    for (int i = 0; i < Q.n_pose; ++i) if (!Q.pose_fixed[i]) { R.pidx[i] = R.np_free++; R.free2pose.push_back(i); }
    if (R.np_free > kMaxFreePosesTeam) return ms_fail(c, MS_ERR_CAPACITY, "ms_ba_create: %d free poses (max %d in this version)", R.np_free, kMaxFreePosesTeam);
    for (int o = 0; o < Q.n_obs; ++o)
        if (Q.obs_pose[o] < 0 || Q.obs_pose[o] >= Q.n_pose || Q.obs_point[o] < 0 || Q.obs_point[o] >= Q.n_point)
            return ms_fail(c, MS_ERR_INVALID, "ms_ba_create: observation %d of problem %d indexes outside the problem", o, p);
    for (int k = 0; k < Q.n_pose_edge; ++k)
        if (Q.edge_i[k] < 0 || Q.edge_i[k] >= Q.n_pose || Q.edge_j[k] < 0 || Q.edge_j[k] >= Q.n_pose)
            return ms_fail(c, MS_ERR_INVALID, "ms_ba_create: pose edge %d of problem %d indexes outside the problem", k, p);
    return MS_OK;
}
// CSR by point and by free pose
static void ba_build_csr(const ms_ba_problem &Q, Prep &R) {
    R.pt_start.assign(Q.n_point + 1, 0);
    for (int o = 0; o < Q.n_obs; ++o) R.pt_start[Q.obs_point[o] + 1]++;
    for (int l = 0; l < Q.n_point; ++l) R.pt_start[l + 1] += R.pt_start[l];
    R.pt_obs.resize(Q.n_obs);
    { bvec<int32_t> cur(R.pt_start.begin(), R.pt_start.end() - 1); for (int o = 0; o < Q.n_obs; ++o) R.pt_obs[cur[Q.obs_point[o]]++] = o; }
    R.fstart.assign(R.np_free + 1, 0);
    for (int o = 0; o < Q.n_obs; ++o) { const int f = R.pidx[Q.obs_pose[o]]; if (f >= 0) R.fstart[f + 1]++; }
    for (int f = 0; f < R.np_free; ++f) R.fstart[f + 1] += R.fstart[f];
    R.fobs.resize(R.fstart[R.np_free]);
    { bvec<int32_t> cur(R.fstart.begin(), R.fstart.end() - 1); for (int o = 0; o < Q.n_obs; ++o) { const int f = R.pidx[Q.obs_pose[o]]; if (f >= 0) R.fobs[cur[f]++] = o; } }
    for (int o = 0; o < Q.n_obs; ++o) if (R.pidx[Q.obs_pose[o]] < 0) R.fobs.push_back(o);      // behind them: the observations of FIXED poses (fobs[fstart[np_free] .. n_obs))
}
// the fobs order as a stream of values (linearise_stream, eval_stream, backsub_stream): read by launches with ONE workgroup per window; a handle that will get teams
// (a window per keyframe) neither builds nor uploads them
static void ba_build_streams(const ms_ba_problem &Q, Prep &R) {
    if (R.auto_team != 1) return;
    R.fo_lo.resize(4 * (size_t)Q.n_obs); R.fo_uvi.assign(4 * (size_t)Q.n_obs, 0.0);
    for (int ii = 0; ii < Q.n_obs; ++ii) {
        const int o = R.fobs[ii];
        R.fo_lo[4 * (size_t)ii] = Q.obs_point[o]; R.fo_lo[4 * (size_t)ii + 1] = o | ((Q.point_fixed && Q.point_fixed[Q.obs_point[o]]) ? (int32_t)0x80000000 : 0); R.fo_lo[4 * (size_t)ii + 2] = Q.obs_pose[o]; R.fo_lo[4 * (size_t)ii + 3] = R.pidx[Q.obs_pose[o]];
        R.fo_uvi[4 * (size_t)ii] = Q.obs_uv[2 * (size_t)o]; R.fo_uvi[4 * (size_t)ii + 1] = Q.obs_uv[2 * (size_t)o + 1]; R.fo_uvi[4 * (size_t)ii + 2] = Q.obs_info[o];
    }
}
// The shapes with ONE free pose whose SE3 edges fit the PO_MAXE LDS slots (edges between fixed poses are constants: any number).  No free point: poseBundleAdjust,
// k_ba_pose_only.  At least one free point (stage 1 of localBundleAdjust): k_ba_one_pose reads the observations in point order, indices and values side by side.
static void ba_build_one_pose(const ms_ba_problem &Q, Prep &R) {
    if (R.np_free != 1 || ba_edges_at_free_pose(Q, R.free2pose[0]) > PO_MAXE) return;
    bool any_free_point = false;
    for (int l = 0; l < Q.n_point && !any_free_point; ++l) any_free_point = !(Q.point_fixed && Q.point_fixed[l]);
    R.pose_only = !any_free_point;
    R.one_pose = any_free_point && Q.n_pose_edge <= OP_NT;
    if (!R.one_pose) return;
    R.op_pose.resize(Q.n_obs); R.op_o.resize(Q.n_obs); R.op_uvi.resize(3 * (size_t)Q.n_obs);
    for (int ii = 0; ii < Q.n_obs; ++ii) {
        const int o = R.pt_obs[ii];
        R.op_pose[ii] = Q.obs_pose[o]; R.op_o[ii] = o;
        R.op_uvi[3 * (size_t)ii] = Q.obs_uv[2 * (size_t)o]; R.op_uvi[3 * (size_t)ii + 1] = Q.obs_uv[2 * (size_t)o + 1]; R.op_uvi[3 * (size_t)ii + 2] = Q.obs_info[o];
    }
}
// The pose-level envelope; decides whether the fused Schur pass applies (R.fused: no point with more than FS_OB free observations, no pose row wider than the LDS tile)
static void ba_build_envelope(const ms_ba_problem &Q, Prep &R, BaEnvelope &E) {
    E.first.resize(R.np_free); E.hfirst.resize(R.np_free); E.fp_start.assign(Q.n_point + 1, 0);
    bvec<int> &first = E.first, &hfirst = E.hfirst;
    bvec<int32_t> &fp_f = E.fp_f, &fp_o = E.fp_o;
    for (int f = 0; f < R.np_free; ++f) first[f] = hfirst[f] = f;
    int max_k = 0;
    for (int l = 0; l < Q.n_point; ++l) {
        E.fp_start[l] = (int32_t)fp_f.size();
        if (Q.point_fixed && Q.point_fixed[l]) continue;
        const size_t b0 = fp_f.size();
        for (int ii = R.pt_start[l]; ii < R.pt_start[l + 1]; ++ii) {
            const int o = R.pt_obs[ii], f = R.pidx[Q.obs_pose[o]];
            if (f < 0) continue;
            size_t at = fp_f.size();
            fp_f.push_back(f); fp_o.push_back(o);
            while (at > b0 && fp_f[at - 1] > f) { std::swap(fp_f[at - 1], fp_f[at]); std::swap(fp_o[at - 1], fp_o[at]); --at; }     // insertion: lists are short and mostly sorted
        }
        const int kk = (int)(fp_f.size() - b0);
        max_k = std::max(max_k, kk);
        if (kk) { const int fmin = fp_f[b0]; for (size_t a = b0; a < fp_f.size(); ++a) first[fp_f[a]] = std::min(first[fp_f[a]], fmin); }
    }
    E.fp_start[Q.n_point] = (int32_t)fp_f.size();
    for (int k = 0; k < Q.n_pose_edge; ++k) {
        const int fi = R.pidx[Q.edge_i[k]], fj = R.pidx[Q.edge_j[k]];
        if (fi >= 0 && fj >= 0) { first[std::max(fi, fj)] = std::min(first[std::max(fi, fj)], std::min(fi, fj)); hfirst[std::max(fi, fj)] = std::min(hfirst[std::max(fi, fj)], std::min(fi, fj)); }
    }
    bool ok = R.np_free > 0 && max_k <= FS_OB;
    for (int f = 0; f < R.np_free && ok; ++f) if (36 * (f - first[f] + 1) + 6 > kFsTileDoubles) ok = false;
    R.fused = ok;
}
// record-based Schur work list: for every free point, every ordered pair (a, b) of its observations with free poses fb <= fa,
// counting-sorted by (fa, fb), then cut into chunks of CH items of one pose pair
static void ba_build_record_list(const ms_ba_problem &Q, Prep &R) {
    const int np = R.np_free;
    bvec<int32_t> count((size_t)np * np + 1, 0);
    auto for_items = [&](auto &&fn) {
        for (int l = 0; l < Q.n_point; ++l) {
            if (Q.point_fixed && Q.point_fixed[l]) continue;
            for (int ia = R.pt_start[l]; ia < R.pt_start[l + 1]; ++ia) {
                const int a = R.pt_obs[ia], fa = R.pidx[Q.obs_pose[a]];
                if (fa < 0) continue;
                for (int ib = R.pt_start[l]; ib < R.pt_start[l + 1]; ++ib) {
                    const int b = R.pt_obs[ib], fb = R.pidx[Q.obs_pose[b]];
                    if (fb < 0 || fb > fa) continue;
                    fn(fa * np + fb, a, b);
                }
            }
        }
    };
    for_items([&](int key, int, int) { count[key + 1]++; });
    bvec<int32_t> kstart(count);
    for (size_t k = 1; k < kstart.size(); ++k) kstart[k] += kstart[k - 1];
    bvec<int32_t> sorted(2 * (size_t)kstart.back()), cur(kstart.begin(), kstart.end() - 1);
    for_items([&](int key, int a, int b) { const int pos = cur[key]++; sorted[2 * (size_t)pos] = a; sorted[2 * (size_t)pos + 1] = b; });
    R.seg_start.push_back(0);
    for (int key = 0; key < np * np; ++key) {
        const int lo = kstart[key], hi = kstart[key + 1];
        if (hi == lo) continue;
        for (int i = lo; i < hi; i += CH) {
            for (int t = 0; t < CH; ++t) {
                const bool in = i + t < hi;
                R.chunk_items.push_back(in ? sorted[2 * (size_t)(i + t)] : -1);
                R.chunk_items.push_back(in ? sorted[2 * (size_t)(i + t) + 1] : -1);
            }
            ++R.n_chunks;
        }
        R.seg_pair.push_back(((key / np) << 16) | (key % np));
        R.seg_start.push_back(R.n_chunks);
        ++R.n_seg;
    }
}
// envelope of the reduced camera matrix per 16-row block: the first structurally non-zero column.  Cholesky creates no fill left of it, so the
// factorisation skips everything outside.
static void ba_build_panel_lists(Prep &R, const BaEnvelope &E) {
    const int np = R.np_free, n6i = 6 * np;
    R.env16.assign(n6i / 16 + 2, 0);
    for (int b = 0; b < (int)R.env16.size(); ++b) {
        int e = n6i;
        for (int r = 16 * b; r < 16 * b + 16; ++r) e = r < n6i ? std::min(e, 6 * E.first[r / 6]) : 0;     // the rhs row (r = n6) is dense
        R.env16[b] = std::min(e, n6i);
    }
    // row tiles a Cholesky panel touches on average (those whose envelope reaches the panel): sizes the factorisation's sub-team
    const int nblk = n6i / 16 + 1;
    long long act = 0;
    for (int pb = 0; pb * 16 < n6i; ++pb) for (int b = pb; b <= nblk; ++b) act += R.env16[(size_t)std::min(b, (int)R.env16.size() - 1)] <= pb * 16 + 15;
    R.chol_tiles = n6i ? (double)act / ((n6i + 15) / 16) : 0.0;
    if (np > kMaxFreePoses) {                   // the distributed factorisation walks these lists
        R.act_start.push_back(0);
        for (int pb = 0; pb * 16 < n6i; ++pb) {
            const int m_rows = n6i - pb * 16 + 1;
            for (int rt = 0; rt * 16 < m_rows; ++rt) if (R.env16[(size_t)std::min(pb + rt, (int)R.env16.size() - 1)] <= pb * 16 + 15) R.act_blk.push_back(rt);
            R.act_start.push_back((int32_t)R.act_blk.size());
        }
    }
}
// A pass of the fused Schur phase, rows [r, r1): their envelope parts side by side in the tile, then the rhs segment
static void ba_add_pass(FsHost &F, const BaEnvelope &E, int r, int r1) {
    F.row0.push_back(r); F.row1.push_back(r1);
    F.yoff.push_back(0); F.yoff.push_back((int32_t)F.rowoff.size());
    int off2 = 0;
    for (int f = r; f < r1; ++f) { F.rowoff.push_back(off2); off2 += 36 * (f - E.first[f] + 1); }
    F.yoff[F.yoff.size() - 2] = off2;
}
// The fine set (teams): the POINTS are dealt out, not the rows -- a pass is a run of points (in the order of their first pose) with about 1 / team of the
// block products; its rows are the poses those points see (they overlap with the neighbours': the sums meet in S through atomics).  Every
// observation is then linearised once per damped solve.  (Row passes made each of the 32 workgroups re-evaluate every point that touches its
// one or two rows: 8x the observations, 75 batches per workgroup instead of 10.)  Leaves F.by_points false, and no pass, for a window it does not suit.
static void ba_choose_point_passes(const ms_ba_problem &Q, const Prep &R, const BaEnvelope &E, FsHost &F, bvec<bvec<int32_t>> &group_pts) {
    const int np = R.np_free, want_passes = std::max(1, std::min(R.auto_team, np));
    const bvec<int32_t> &fp_start = E.fp_start, &fp_f = E.fp_f;
    bvec<int32_t> need_pre(np + 1, 0);                        // tile doubles of rows [0, f): a pass's need is a difference
    for (int f = 0; f < np; ++f) need_pre[f + 1] = need_pre[f] + 36 * (f - E.first[f] + 1) + 6;
    auto tile_need = [&](int r, int r1) { return r1 > r ? need_pre[r1] - need_pre[r] : 0; };
    bvec<std::pair<uint32_t, int32_t>> order;      // (first pose << 16 | last pose, point)
    double total_cost = 0;
    for (int l = 0; l < Q.n_point; ++l) {
        const int k = fp_start[l + 1] - fp_start[l];
        if (k == 0) continue;
        order.emplace_back(((uint32_t)fp_f[fp_start[l]] << 16) | (uint32_t)fp_f[fp_start[l + 1] - 1], l);
        total_cost += 8.0 * k + 0.5 * k * (k + 1);
    }
    {   // by (first pose, last pose), then point: a counting sort over the np x np key space (std::sort of 2000 keys was 0.05 ms of the 0.45 ms create)
        const size_t nk = (size_t)np * np;
        if (order.size() > 64 && nk <= 65536) {
            bvec<int32_t> cnt(nk + 1, 0);
            auto key_of = [&](const std::pair<uint32_t, int32_t> &e) { return (size_t)(e.first >> 16) * np + (e.first & 0xFFFF); };
            for (const auto &e : order) cnt[key_of(e) + 1]++;
            for (size_t q = 0; q < nk; ++q) cnt[q + 1] += cnt[q];
            bvec<std::pair<uint32_t, int32_t>> sorted(order.size());
            for (const auto &e : order) sorted[cnt[key_of(e)]++] = e;      // (order is in point order: equal keys stay in it)
            order.swap(sorted);
        } else std::sort(order.begin(), order.end());
    }
    double acc_cost = 0;
    int g_lo = np, g_hi = 0;
    group_pts.emplace_back();
    for (const auto &e : order) {
        const int l = e.second, k = fp_start[l + 1] - fp_start[l], lo = std::min(g_lo, (int)(e.first >> 16)), hi = std::max(g_hi, (int)(e.first & 0xFFFF) + 1);
        const bool full = !group_pts.back().empty() && (tile_need(lo, hi) > kFsTileDoubles ||
                          ((int)group_pts.size() < want_passes && acc_cost >= total_cost * (double)group_pts.size() / want_passes));
        if (full) { ba_add_pass(F, E, g_lo, g_hi); group_pts.emplace_back(); g_lo = (int)(e.first >> 16); g_hi = (int)(e.first & 0xFFFF) + 1; }
        else { g_lo = lo; g_hi = hi; }
        group_pts.back().push_back(l);
        acc_cost += 8.0 * k + 0.5 * k * (k + 1);
    }
    if (!group_pts.back().empty()) ba_add_pass(F, E, g_lo, g_hi); else group_pts.pop_back();
    F.by_points = true;
    // a point seen from poses so far apart that the rows between them do not fit the tile (scattered covisibility): row passes for this window
    for (size_t ps = 0; ps < F.row0.size(); ++ps) if (tile_need(F.row0[ps], F.row1[ps]) > kFsTileDoubles) F.by_points = false;
    if (!F.by_points) { F.row0.clear(); F.row1.clear(); F.yoff.clear(); F.rowoff.clear(); group_pts.clear(); }
}
// Row passes (the coarse set, or a fine set by-points passes do not suit): greedy row ranges under the tile budget, as many rows per pass as the tile takes
static void ba_choose_row_passes(const Prep &R, const BaEnvelope &E, FsHost &F) {
    for (int r = 0; r < R.np_free;) {
        int r1 = r, used = 0;
        while (r1 < R.np_free) {
            const int need = 36 * (r1 - E.first[r1] + 1) + 6;
            if (used + need > kFsTileDoubles) break;
            used += need; ++r1;
        }
        ba_add_pass(F, E, r, r1);
        r = r1;
    }
}
typedef bvec<std::pair<uint64_t, int32_t>> BaPassPoints;      // (signature of the point's pose set, point)
// The points of pass ps, each with the signature of its free poses below the pass's last row (later poses have no pair with a row of this pass): points with the
// same set get the same key, and keys order roughly by position in the window.  A by-points pass owns the points it was dealt; a row pass visits every free point
// that one of its rows observes.
static void ba_pass_points(const ms_ba_problem &Q, const Prep &R, const BaEnvelope &E, const FsHost &F, size_t ps, const bvec<bvec<int32_t>> &group_pts, bvec<int32_t> &stamp, BaPassPoints &pts) {
    const int r0 = F.row0[ps], r1 = F.row1[ps];
    auto add = [&](int l, int r_end) {
        uint64_t h = 1469598103934665603ull; int fmin = 0x7fff, fmax = 0, kk = 0;
        for (int jj = E.fp_start[l]; jj < E.fp_start[l + 1] && E.fp_f[jj] < r_end; ++jj) { h = (h ^ (uint64_t)E.fp_f[jj]) * 1099511628211ull; fmin = std::min(fmin, (int)E.fp_f[jj]); fmax = E.fp_f[jj]; ++kk; }
        pts.emplace_back(((uint64_t)fmin << 48) | ((uint64_t)fmax << 32) | ((uint64_t)(kk & 0xFF) << 24) | (h & 0xFFFFFFull), l);
    };
    pts.clear();
    if (F.by_points) { for (int l : group_pts[ps]) add(l, INT32_MAX); return; }
    for (int fa = r0; fa < r1; ++fa)
        for (int ii = R.fstart[fa]; ii < R.fstart[fa + 1]; ++ii) {
            const int l = Q.obs_point[R.fobs[ii]];
            if (stamp[l] == (int32_t)ps || (Q.point_fixed && Q.point_fixed[l])) continue;
            stamp[l] = (int32_t)ps;
            add(l, r1);
        }
}
// Cuts the points of one pass (pts, sorted: points with the same set of poses next to each other) into batches of whole points with at most FS_OB observations,
// and appends every batch's lane slots, format and pair list to F
struct BaBatchCutter {
    const ms_ba_problem &Q; const BaEnvelope &E; FsHost &F;
    const BaPassPoints &pts;
    bvec<std::pair<int32_t, uint16_t>> &bp2;               // (block key, pair) of the open batch: scratch
    const int r0, r1;                                       // the pass's rows
    int in_batch = 0;
    bool uniform = true;                                    // every point of the open batch has the same pose set
    uint64_t batch_key = 0;
    int batch_k = 0, batch_first = -1;                      // poses per point / first point (index into pts) of the open batch
    int poses_below_r1(int l) const {
        const int j0 = E.fp_start[l];
        int kk = 0;
        while (j0 + kk < E.fp_start[l + 1] && E.fp_f[j0 + kk] < r1) ++kk;
        return kk;
    }
    void pad_pairs() { while (F.pairs.size() % 8) F.pairs.push_back((uint16_t)0xFFFF); }
    void pad_slots() {                                      // a batch owns FS_OB lane slots (the kernel addresses batch b at slot FS_OB b): the rest hold "no observation"
        const size_t at = F.pobs.size(), slots = at / 4, padded = (slots + FS_OB - 1) / FS_OB * FS_OB;
        if (padded == slots) return;
        F.pobs.resize(4 * padded);
        for (size_t q = slots; q < padded; ++q) { F.pobs[4 * q] = -1; F.pobs[4 * q + 1] = 0; F.pobs[4 * q + 2] = 0; F.pobs[4 * q + 3] = -1; }
    }
    void end_batch(int fmt) {
        pad_pairs();
        F.b_fmt.push_back(fmt);
        pad_slots();
        F.b_obs_start.push_back((int32_t)(F.pobs.size() / 4)); F.b_run_start.push_back((int32_t)F.pairs.size());
        in_batch = 0;
    }
    // the usual case: G points with the same k poses -> pairs in (a, b) position order are already grouped by block, blocks ascending
    void close_uniform(int pt_end) {
        const int G = pt_end - batch_first, k = batch_k, j0 = E.fp_start[pts[batch_first].second];
        int a0 = 0;
        while (a0 < k && E.fp_f[j0 + a0] < r0) ++a0;
        // (only for pass sets that own points = team launches: one window per keyframe, where the index build is a fifth of the call; a 256-window launch keeps the
        //  lists -- enumerating costs its Schur pass 4 %, 11.4 against 10.9 ms, and its handles are built once.  schur_fused<true> runs exactly these sets)
        if (F.by_points && k <= 31 && G <= 127) return end_batch(-1 - (G | (k << 7) | (a0 << 12)));      // the kernel enumerates the pairs of such a batch itself: nothing to build, nothing to upload
        const size_t n_pairs = (size_t)G * ((size_t)k * (k + 1) / 2 - (size_t)a0 * (a0 + 1) / 2);
        const size_t cap = std::min<size_t>(8, std::max<size_t>(1, (n_pairs + 63) / 64));
        const int single_fmt = n_pairs <= 64 ? (int)n_pairs : 0;
        for (int a = a0; a < k; ++a)
            for (int b2 = 0; b2 <= a; ++b2) {
                if (single_fmt) { for (int gp = 0; gp < G; ++gp) F.pairs.push_back((uint16_t)((gp * k + a) | ((gp * k + b2) << 8))); continue; }
                size_t in_chunk = 0;
                for (int gp = 0; gp < G; ++gp) {
                    if (in_chunk == cap) { pad_pairs(); in_chunk = 0; }
                    F.pairs.push_back((uint16_t)((gp * k + a) | ((gp * k + b2) << 8))); ++in_chunk;
                }
                pad_pairs();
            }
        end_batch(single_fmt);
    }
    // points with different pose sets: every pair with its block key, sorted by block
    void close_mixed(int pt_end) {
        bp2.clear();
        int base = 0;
        for (int q = batch_first; q < pt_end; ++q) {
            const int l = pts[q].second, j0 = E.fp_start[l], kk = poses_below_r1(l);
            for (int a = 0; a < kk; ++a) {
                const int fa = E.fp_f[j0 + a];
                if (fa < r0) continue;
                for (int b2 = 0; b2 < kk; ++b2)
                    if (E.fp_f[j0 + b2] <= fa) bp2.emplace_back((fa << 16) | E.fp_f[j0 + b2], (uint16_t)((base + a) | ((base + b2) << 8)));
            }
            base += kk;
        }
        std::stable_sort(bp2.begin(), bp2.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
        const int single_fmt = bp2.size() <= 64 ? (int)bp2.size() : 0;
        if (single_fmt) for (const auto &e : bp2) F.pairs.push_back(e.second);
        else {
            // chunks of <= 8 pairs of one block; when the batch has few pairs the chunks get shorter so that more lanes share them
            const size_t cap = std::min<size_t>(8, std::max<size_t>(1, (bp2.size() + 63) / 64));
            size_t in_chunk = 0;
            for (size_t i = 0; i < bp2.size(); ++i) {
                if (i && (bp2[i].first != bp2[i - 1].first || in_chunk == cap)) { pad_pairs(); in_chunk = 0; }
                F.pairs.push_back(bp2[i].second); ++in_chunk;
            }
        }
        end_batch(single_fmt);
    }
    void close_batch(int pt_end) {
        if (in_batch == 0) return;
        if (uniform) close_uniform(pt_end); else close_mixed(pt_end);
    }
    void add_point(int q) {
        const int l = pts[q].second, j0 = E.fp_start[l], kk = poses_below_r1(l);
        if (in_batch + kk > FS_OB) close_batch(q);
        if (in_batch == 0) { uniform = true; batch_key = pts[q].first; batch_k = kk; batch_first = q; }
        else if (pts[q].first != batch_key || kk != batch_k) uniform = false;
        if (uniform && q > batch_first) {                 // equal signatures: make sure the sets really are equal (the key holds a 24-bit hash)
            const int jb = E.fp_start[pts[batch_first].second];
            for (int a = 0; a < kk; ++a) if (E.fp_f[j0 + a] != E.fp_f[jb + a]) { uniform = false; break; }
        }
        const size_t at = F.pobs.size();
        F.pobs.resize(at + 4 * (size_t)kk);
        int32_t *w = F.pobs.data() + at;
        for (int a = 0; a < kk; ++a, w += 4) { const int o = E.fp_o[j0 + a]; w[0] = o; w[1] = Q.obs_pose[o]; w[2] = l; w[3] = E.fp_f[j0 + a]; }
        in_batch += kk;
    }
};
// fused Schur pass (schur_fused): pose rows -> passes whose envelope part fits the LDS tile, points -> batches of <= 64 observations.
// Only the set the launches will use is built (the other one aliases it: still correct, only slower, should ms_ba_set_team ask for the other regime later):
// a batch that fills the chip always runs one workgroup per problem and gets the coarse set 0, a handful of windows gets teams and the fine set 1.
static void ba_build_fused_passes(const ms_ba_problem &Q, Prep &R, const BaEnvelope &E, BaTimes &tm) {
    const int np = R.np_free;
    R.fs_cs.resize(2 * (size_t)np);                              // [np] first column of the row's envelope part, then [np] first column of the row's part of Hpp
    for (int f = 0; f < np; ++f) { R.fs_cs[f] = 6 * E.first[f]; R.fs_cs[(size_t)np + f] = 6 * E.hfirst[f]; }
    R.fs_only = R.auto_team == 1 ? 0 : 1;
    if (!R.fused) return;
    FsHost &F = R.fs[R.fs_only];
    bvec<int32_t> stamp(Q.n_point, -1);
    BaPassPoints pts;
    bvec<std::pair<int32_t, uint16_t>> bp2;
    bvec<bvec<int32_t>> group_pts;
    {
        BaLap lap(tm, BaTimes::kPasses);
        if (R.fs_only == 1) ba_choose_point_passes(Q, R, E, F, group_pts);
        if (!F.by_points) ba_choose_row_passes(R, E, F);
    }
    F.batch_start.push_back(0); F.b_obs_start.push_back(0); F.b_run_start.push_back(0);
    F.pobs.reserve(4 * E.fp_f.size() * 2); F.pairs.reserve(8 * E.fp_f.size());
    for (size_t ps = 0; ps < F.row0.size(); ++ps) {
        { BaLap lap(tm, BaTimes::kPointKeys); ba_pass_points(Q, R, E, F, ps, group_pts, stamp, pts); }
        { BaLap lap(tm, BaTimes::kSort); std::sort(pts.begin(), pts.end()); }      // points with the same set of poses next to each other: their pairs fall into the same blocks
        BaLap lap(tm, BaTimes::kBatches);
        BaBatchCutter cut{Q, E, F, pts, bp2, F.row0[ps], F.row1[ps]};
        for (int q = 0; q < (int)pts.size(); ++q) cut.add_point(q);
        cut.close_batch((int)pts.size());
        F.batch_start.push_back((int32_t)F.b_obs_start.size() - 1);
    }
    BaLap lap(tm, BaTimes::kValues);
    F.b_obs_start.push_back(F.b_obs_start.back());
    F.puv.assign(F.pobs.size(), 0.0);                         // per lane slot: u, v, information, 0
    for (size_t i = 0; i < F.pobs.size() / 4; ++i) {
        const int o = F.pobs[4 * i];
        if (o >= 0) { F.puv[4 * i] = Q.obs_uv[2 * (size_t)o]; F.puv[4 * i + 1] = Q.obs_uv[2 * (size_t)o + 1]; F.puv[4 * i + 2] = Q.obs_info[o]; }
    }
}
// windowed Cholesky (cholesky_window): active 16-row blocks per panel, LDS slots, tiles entering per panel
static void ba_build_chol_window(Prep &R, const BaEnvelope &E) {
    const int np = R.np_free, n6i = 6 * np, nblk = (n6i + 15) / 16;
    bvec<int32_t> &slot = R.cw_slot, &act_start = R.cw_act_start, &act = R.cw_act, &load_start = R.cw_load_start, &load = R.cw_load;
    bvec<int> ent(nblk, 0);
    for (int b = 0; b < nblk; ++b) {
        int e = n6i;
        for (int r = 16 * b; r < std::min(16 * b + 16, n6i); ++r) e = std::min(e, 6 * E.first[r / 6]);
        ent[b] = std::min(e / 16, b);
    }
    for (int b = nblk - 2; b >= 0; --b) ent[b] = std::min(ent[b], b);      // (a block is active at its own panel at the latest)
    slot.assign(nblk, 0);
    bvec<int> free_slots, active;
    int W = 0;
    bvec<bvec<int>> entering(nblk);
    for (int b = 0; b < nblk; ++b) entering[ent[b]].push_back(b);
    act_start.push_back(0); load_start.push_back(0);
    for (int pnl = 0; pnl < nblk; ++pnl) {
        if (pnl > 0) active.erase(std::find(active.begin(), active.end(), pnl - 1));      // block pnl-1 is factored ...
        if (pnl > 1) free_slots.push_back(slot[pnl - 2]);           // ... its slot is reused one panel later: panel pnl's tiles are fetched while pnl-1 is still updating
        std::sort(free_slots.begin(), free_slots.end(), std::greater<int>());
        for (int b : entering[pnl]) {
            int sl;
            if (!free_slots.empty()) { sl = free_slots.back(); free_slots.pop_back(); } else sl = W++;
            slot[b] = sl;
            active.push_back(b);
        }
        std::sort(active.begin(), active.end());
        for (int bi : active)
            for (int bj : active) {
                if (bj > bi) break;
                if (bi == bj && bi == pnl) continue;                       // the panel's own diagonal tile is fetched by the factoring wave
                if (ent[bi] == pnl || ent[bj] == pnl) { load.push_back(bi | (slot[bi] << 16)); load.push_back(bj | (slot[bj] << 16)); }
            }
        load_start.push_back((int32_t)load.size() / 2);
        for (int b : active) if (b != pnl) act.push_back(b | (slot[b] << 16));
        act_start.push_back((int32_t)act.size());
    }
    if (W < 3) W = 3;                                                // the back substitution keeps three columns (<= W tiles each) in the W x W tile area
    const size_t fixed = ((size_t)W * W * CT + 16 + 16 * (size_t)W + 32 + 256 + 16) * sizeof(double), zbytes = (size_t)((n6i + 15) & ~15) * sizeof(double);
    const bool fits = R.fused && nblk < 65536 && W >= 1 && W < 256;
    R.cw_W = fits && fixed <= kLdsBytes ? W : 0;
    R.cw_zglobal = fixed + zbytes > kLdsBytes;                       // a long trajectory: the tiles fit, the 8 n bytes of the rhs do not -- it stays in global memory
    const size_t meta = 4 * (slot.size() + act_start.size() + load_start.size() + act.size() + load.size());
    R.cw_meta_lds = R.cw_W > 0 && fixed + 2 * zbytes + meta <= kLdsBytes;      // (and the reciprocal pivots: another n doubles)
}

// ---------------------------------------------------------------- the device block of a handle: every array is named ONCE, in ba_lay_out
// input() / work() reserve an array's bytes (256-byte aligned, never less than one line), put the array's OFFSET into the descriptor's pointer member and note the
// member; relocate() turns the offsets into addresses once the block is known.  input() also notes what stage() copies into the problem's staging block.
// An absent array gets a null pointer and no copy; an absent INPUT still reserves its bytes, an absent WORK area only the minimum.
struct BaLayout {
    struct Copy { size_t at; const void *src; size_t bytes; };
    size_t total = 0, desc_at = 0;                            // bytes so far; where a single problem's two descriptors ride
    bvec<Copy> copies;
    bvec<void *> members;                                     // pointer members that hold an offset
    size_t reserve(size_t bytes) { const size_t o = total; total += ms_align_up(bytes ? bytes : 8, 256); return o; }
    template <class T> void note(T *&m, size_t at, bool present) {
        m = present ? reinterpret_cast<T *>(at) : nullptr;
        if (present) members.push_back(const_cast<void *>(static_cast<const void *>(&m)));
    }
    template <class T, class S> void input(T *&m, const S *src, size_t count, bool present = true, size_t slack = 0) {
        static_assert(sizeof(T) == sizeof(S), "an input array is uploaded as it is");
        const size_t at = reserve((count + slack) * sizeof(T));
        note(m, at, present);
        if (present && count) copies.push_back(Copy{at, src, count * sizeof(T)});
    }
    template <class T, class S> void input(T *&m, const bvec<S> &v, bool present = true, size_t slack = 0) { input(m, v.data(), v.size(), present, slack); }
    template <class T> void work(T *&m, size_t count, bool present = true) { note(m, reserve(present ? count * sizeof(T) : 0), present); }
    void relocate(char *base) const {
        for (void *m : members) { uintptr_t v; std::memcpy(&v, m, sizeof(v)); v += reinterpret_cast<uintptr_t>(base); std::memcpy(m, &v, sizeof(v)); }
    }
    void stage(const Prep &R, char *block) const {            // (block: the image of [R.in_lo, R.in_hi), zeroed)
        for (size_t i = R.copy_lo; i < R.copy_hi; ++i) std::memcpy(block + (copies[i].at - R.in_lo), copies[i].src, copies[i].bytes);
    }
};
// One problem's part of the device block and its descriptor H (A: the four arrays of its second linearisation set).  The ORDER is part of the format.
static void ba_lay_out(const ms_ba_problem &Q, Prep &R, bool single, size_t pack_doubles, BaLayout &L, BaProb &H, ms_ba::AltPtrs &A) {
    const size_t n6 = 6 * (size_t)R.np_free, n_point = Q.n_point, n_obs = Q.n_obs;
    const bool streams = !R.fo_lo.empty();
    H.n_pose = Q.n_pose; H.n_point = Q.n_point; H.n_obs = Q.n_obs; H.n_edge = Q.n_pose_edge; H.np_free = R.np_free; H.n6 = 6 * R.np_free;
    H.max_iters = Q.max_iters; H.huber = Q.huber_delta; H.team = 1; H.chol_team = 1; H.debug_reject = 0;
    H.n_chunks = R.n_chunks; H.n_seg = R.n_seg; H.fused = R.fused ? 1 : 0;
    H.cw_W = R.cw_W; H.cw_zglobal = R.cw_zglobal ? 1 : 0; H.cw_meta_lds = R.cw_meta_lds ? 1 : 0;
    // inputs first, contiguous: they go up in ONE host->device copy per problem
    R.in_lo = L.total; R.copy_lo = L.copies.size();
    L.input(H.pose0, Q.pose, 7 * Q.n_pose); L.input(H.point0, Q.point, 3 * n_point);
    L.input(H.pidx, R.pidx); L.input(H.point_fixed, Q.point_fixed, n_point, Q.point_fixed != nullptr);
    L.input(H.obs_pose, Q.obs_pose, n_obs); L.input(H.obs_point, Q.obs_point, n_obs); L.input(H.obs_uv, Q.obs_uv, 2 * n_obs); L.input(H.obs_info, Q.obs_info, n_obs);
    L.input(H.pt_start, R.pt_start); L.input(H.pt_obs, R.pt_obs); L.input(H.fstart, R.fstart); L.input(H.fobs, R.fobs);
    L.input(H.fo_lo, R.fo_lo, streams); L.input(H.fo_uvi, R.fo_uvi, streams);
    L.input(H.free2pose, R.free2pose);
    L.input(H.edge_i, Q.edge_i, Q.n_pose_edge); L.input(H.edge_j, Q.edge_j, Q.n_pose_edge); L.input(H.edge_meas, Q.edge_meas, 7 * Q.n_pose_edge); L.input(H.edge_info, Q.edge_info, 36 * Q.n_pose_edge);
    L.input(H.chunk_items, R.chunk_items); L.input(H.seg_start, R.seg_start); L.input(H.seg_pair, R.seg_pair);
    L.input(H.env16, R.env16); L.input(H.act_start, R.act_start); L.input(H.act_blk, R.act_blk);
    L.input(H.fs_cs, R.fs_cs);
    L.input(H.cw_slot, R.cw_slot); L.input(H.cw_act_start, R.cw_act_start); L.input(H.cw_act, R.cw_act); L.input(H.cw_load_start, R.cw_load_start); L.input(H.cw_load, R.cw_load);
    for (int set = 0; set < 2; ++set) {                      // (the set that was not built is empty here; ms_ba_create makes it an alias of the other)
        const FsHost &S = R.fs[set];
        FsSet &F = H.fs[set];
        const bool built = R.fused && set == R.fs_only;
        if (built) { F.n_pass = (int32_t)S.row0.size(); F.by_points = S.by_points ? 1 : 0; }
        L.input(F.row0, S.row0, built); L.input(F.row1, S.row1, built); L.input(F.batch_start, S.batch_start, built);
        L.input(F.b_obs_start, S.b_obs_start, built); L.input(F.b_run_start, S.b_run_start, built); L.input(F.b_fmt, S.b_fmt, built); L.input(F.pobs, S.pobs, built); L.input(F.puv, S.puv, built);
        L.input(F.pairs, S.pairs, built, 8); L.input(F.rowoff, S.rowoff, built); L.input(F.yoff, S.yoff, built);
    }
    L.input(H.op_pose, R.op_pose, R.one_pose); L.input(H.op_o, R.op_o, R.one_pose); L.input(H.op_uvi, R.op_uvi, R.one_pose);
    if (single) L.desc_at = L.reserve(2 * sizeof(BaProb));      // a single problem's two descriptors travel with its inputs: ONE copy per create
    R.in_hi = L.total; R.copy_hi = L.copies.size();
    // state and work areas
    L.work(H.pose, 7 * (size_t)Q.n_pose); L.work(H.pose_bk, 7 * (size_t)Q.n_pose); L.work(H.point, 3 * n_point); L.work(H.point_bk, 3 * n_point);
    L.work(H.Hpp, n6 * n6); L.work(H.S, n6 * n6); L.work(H.bp, n6); L.work(H.dp, n6); L.work(H.y, n6);
    L.work(H.Hll, 6 * n_point); L.work(H.bl, 3 * n_point); L.work(H.Hinv, 6 * n_point); L.work(H.Hpl, R.fused ? 1 : 18 * (n_obs + 1));      // (the fused pass keeps no Hpl / Y records)
    L.work(H.dl, 3 * n_point); L.work(H.chi2_obs, n_obs); L.work(H.stats, 16);
    L.work(H.Y, R.fused ? 1 : 18 * (n_obs + 1)); L.work(H.zrow, n6 + 16);
    L.work(H.dinv, n6 + 16);
    if (R.np_free > kMaxFreePoses) L.work(H.panG, (n6 + 17) * NB);
    L.work(H.bar, 64); L.work(H.red, 4 * kMaxTeam); L.work(H.flag, 64);     // team state on lines of their own (256 B each at least)
    L.work(H.op_rec, 28 * n_point, R.one_pose); L.work(H.op_red, 2 * (size_t)kMaxTeam * OP_NV, R.one_pose);
    // the second set of the linearisation's outputs (k_ba_lm's fused trial schedule): only for handles whose launches run one workgroup per problem on the streams
    const bool alt_set = streams && R.fused;
    L.work(A.Hpp, n6 * n6, alt_set); L.work(A.bp, n6, alt_set); L.work(A.Hll, 6 * n_point, alt_set); L.work(A.bl, 3 * n_point, alt_set);
    L.work(H.pack, pack_doubles, pack_doubles != 0);
}
// ONE device block per handle (arena + the problem descriptors behind it), taken from the context's cache of destroyed handles when one is large enough
static int ba_take_block(ms_ctx *c, ms_ba *B, size_t need) {
    // best fit among the kept blocks, but never one more than kBaCacheSlack times the request: a small window must not sit on the
    // gigabytes a global-BA handle left behind (that block waits for the next large request, or goes when the cache is trimmed)
    int best = -1;
    for (int i = 0; i < 4; ++i)
        if (c->ba_cache[i].p && c->ba_cache[i].bytes >= need && c->ba_cache[i].bytes / kBaCacheSlack <= need &&
            (best < 0 || c->ba_cache[i].bytes < c->ba_cache[best].bytes)) best = i;
    if (best >= 0) { B->d_arena = static_cast<char *>(c->ba_cache[best].p); B->arena_bytes = c->ba_cache[best].bytes; c->ba_cache[best] = {}; return MS_OK; }
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&B->d_arena), need);
    ++g_ba_host_allocs;
    if (e != hipSuccess) {                                  // out of memory with blocks kept for later: give them back and try once more
        (void)hipGetLastError();
        (void)hipStreamSynchronize(c->stream);
        for (auto &b : c->ba_cache) if (b.p) { (void)hipFree(b.p); b = {}; }
        e = hipMalloc(reinterpret_cast<void **>(&B->d_arena), need);
    }
    if (e != hipSuccess) { (void)hipGetLastError(); return ms_fail(c, MS_ERR_HIP, "ms_ba_create: cannot allocate %zu bytes: %s", need, hipGetErrorString(e)); }
    B->arena_bytes = need;
    return MS_OK;
}
// the context's page-locked staging block, free for this create and at least `need` bytes
static hipError_t ba_reserve_stage(ms_ctx *c, size_t need) {
    if (c->ba_stage_busy) { (void)hipEventSynchronize(c->ba_stage_ev); c->ba_stage_busy = false; }      // (the previous create's upload: long done)
    hipError_t e = hipSuccess;
    if (!c->ba_stage_ev) { e = hipEventCreateWithFlags(&c->ba_stage_ev, hipEventDisableTiming); ++g_ba_host_allocs; }
    if (e == hipSuccess && c->ba_stage_bytes < need) {
        if (c->ba_stage) (void)hipHostFree(c->ba_stage);
        c->ba_stage = nullptr; c->ba_stage_bytes = 0;
        const size_t want = std::min(kBaStageMax, ms_align_up(need + need / 4, (size_t)1 << 16));
        e = hipHostMalloc(&c->ba_stage, want, hipHostMallocDefault); ++g_ba_host_allocs;
        if (e == hipSuccess) c->ba_stage_bytes = want;
    }
    return e;
}
// the eager results of a single small problem (B->pack_doubles): a page-locked block that stays with the handle object
static hipError_t ba_reserve_result(ms_ba *B) {
    if (B->pack_doubles * sizeof(double) <= B->h_result_bytes) return hipSuccess;
    if (B->h_result) (void)hipHostFree(B->h_result);
    B->h_result = nullptr; B->h_result_bytes = 0;
    const size_t want = ms_align_up(B->pack_doubles * sizeof(double) * 2, (size_t)4096);
    const hipError_t e = hipHostMalloc(&B->h_result, want, hipHostMallocDefault); ++g_ba_host_allocs;
    if (e == hipSuccess) B->h_result_bytes = want;
    return e;
}
// the descriptors of a new handle (both sets) go up; stage_at: the end of the inputs in the context's staging block
static hipError_t ba_upload_new_descriptors(ms_ctx *c, ms_ba *B, bool staged, size_t stage_at) {
    const int n = B->n;
    hipError_t e;
    ba_make_alt(B);
    if (n == 1) {                                       // (went up with the inputs)
        e = staged ? hipEventRecord(c->ba_stage_ev, c->stream) : hipSuccess;
        if (staged) c->ba_stage_busy = e == hipSuccess;
    } else if (staged) {                                // the descriptors (both sets, side by side like on the device) follow the inputs out of the same block; its next user waits for ba_stage_ev
        char *at = static_cast<char *>(c->ba_stage) + stage_at;
        std::memcpy(at, B->host.data(), sizeof(BaProb) * n);
        std::memcpy(at + sizeof(BaProb) * n, B->host_alt.data(), sizeof(BaProb) * n);
        e = hipMemcpyAsync(B->d_probs, at, 2 * sizeof(BaProb) * n, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipEventRecord(c->ba_stage_ev, c->stream);
        c->ba_stage_busy = e == hipSuccess;
    } else {
        e = hipMemcpy(B->d_probs, B->host.data(), sizeof(BaProb) * n, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(B->d_probs_alt, B->host_alt.data(), sizeof(BaProb) * n, hipMemcpyHostToDevice);
    }
    return e;
}
// the solvers' dynamic LDS sizes: once per device and process
static hipError_t ba_set_lds_attributes(ms_ctx *c) {
    static std::atomic<unsigned long long> attr_done{0};
    if ((attr_done.load() >> (c->device & 63)) & 1ull) return hipSuccess;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_ba_lm), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_ba_pose_only), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPoLdsBytes) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_ba_one_pose<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kOpLdsBytes) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_ba_one_pose<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kOpLdsBytes) != hipSuccess) return hipErrorUnknown;
    attr_done.fetch_or(1ull << (c->device & 63));
    return hipSuccess;
}
