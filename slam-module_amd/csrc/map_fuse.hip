// map_fuse.hip -- the merge / replace half of replaceDuplication and the loop closer's merge loop on the device map tables, in place:
//   ms_map_fuse            the walk of keyframe_matcher.cpp:424-526 over the gated and scored entries of n_views views
//   ms_map_replace_pairs   "merge moved map points", loop_closer.cpp:531-546
// Both rest on replace(l, w) = MapPoint::replaceWith (map_point.cpp:118-156): one pass over kf_mp.  The walk is sequential across entries (an
// entry's decision reads the counts and the table as the entries before it left them), so ONE workgroup of 1024 lanes walks, as
// k_cull_keyframes does; what is parallel is the inside of a step.
//
// ms_map_fuse, three launches whatever n_views and n_entries are:
//   k_fuse_fill      cand = -1, the per-entry outputs' defaults, the "listed by K" marks = 0, the result block = 0
//   k_fuse_scatter   one workgroup column per view: kept query q -> cand[kept_entry[q]] = its best keypoint (detail::best_candidate), and the
//                    pre-pass checks (kept_entry inside the slice, top_idx inside [-1, stride), the valid entries of a walked slot are live),
//                    which only count into the result block
//   k_fuse_walk      nothing when the pre-pass counted a violation.  Per view: mark the rows K lists; read the slice in trips of 1024 entries;
//                    a lane decides codes 1 / 2 / 3 / 0 of its entry from the state at the trip's start; the entries with a candidate are
//                    compacted (block_rank, ms_scan.h) and stepped through in order.  A step's decision is made by every lane from the same
//                    addresses (so it is uniform and needs no broadcast), a barrier separates it from the step's writes and another one closes
//                    the step.  A step that takes a row out of K or erases it lets the later lanes of the trip that hold that row decide again.
//   replace          waves stride over the slots; a wave scans its row 64 entries at a time and finds l and w with ballots; the wave that
//                    owns the row rewrites it, so no two waves write one row.  n_obs is only ever touched by agent-scope atomics (adds,
//                    one exchange to zero, atomic loads): a plain load could be served from the CU's vector cache.
// All barriers are in uniform control flow: loop bounds are launch arguments, table values read by every lane behind a barrier, or block_rank's
// total (through LDS).  No workgroup waits for another.  Integer work only; the same input gives the same bits on every call.
//
// What stays with the caller (derived from erased_rows / erased_into and the per-entry outputs): keyPointToTrackId.erase (:142-144), the host
// MapPoint objects, fusedCount (codes 4-7).
#include "ms_internal.h"
#include "ms_scan.h"
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int kWalk = 1024;                                  // lanes of the one walking workgroup
constexpr int kDown = 3 + 8;                                 // n_erased, views_done, violations, counts[8]

struct FuseArgs {
    int32_t *kf_mp;
    uint8_t *mp_flags, *mp_live;
    int32_t *n_obs, *mp_track, *track_row;                   // the track tables are both null or both given
    const int32_t *kept_entry, *top_idx;
    const uint16_t *top_dist;
    const int32_t *mp_index;                                 // [n_entries], the workspace's copy
    const int4 *views;                                       // [n_views]: slot, first, count, n_kept
    const int2 *pairs;                                       // [n_pairs]: (loser, winner), the pairs that run
    int32_t *cand;                                           // [n_entries]: the entry's candidate keypoint, -1 for none
    uint8_t *in_k;                                           // [n_mp]: the row is a valid entry of the view's slot
    uint8_t *outcome;
    int32_t *kp, *other, *erased_rows, *erased_into;         // each may be null
    int32_t *down;                                           // [kDown]
    int32_t n_kf, stride, n_mp, n_entries, n_views, n_pairs, n_track, track_base, max_dist, source_slot;
};

__device__ __forceinline__ int obs_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(kBlock) void k_fuse_fill(const FuseArgs A) {
    const int i = blockIdx.x * kBlock + (int)threadIdx.x;
    if (i < A.n_entries) {
        A.cand[i] = -1;
        if (A.outcome) A.outcome[i] = 0;
        if (A.kp) A.kp[i] = -1;
        if (A.other) A.other[i] = -1;
    }
    if (i < A.n_mp) A.in_k[i] = 0;
    if (i < kDown) A.down[i] = 0;
}

// grid (x, view): lane j of the column is kept query j of the view and keypoint j of the view's slot
__global__ __launch_bounds__(kBlock) void k_fuse_scatter(const FuseArgs A) {
    const int4 V = A.views[blockIdx.y];
    const int j = blockIdx.x * kBlock + (int)threadIdx.x;
    bool bad = false;
    if (j < V.w) {                                           // V.w <= V.z and the slice lies inside [0, n_entries): validated on the host
        const int q = V.y + j;
        const int32_t e = A.kept_entry[q], t = A.top_idx[4 * (size_t)q];
        const bool e_ok = e >= V.y && e < V.y + V.z, t_ok = t >= -1 && t < A.stride;
        bad = !e_ok || !t_ok;
        if (!bad && t >= 0 && (int)A.top_dist[4 * (size_t)q] <= A.max_dist) A.cand[e] = t;
    }
    if (j < A.stride) {
        const uint32_t r = (uint32_t)A.kf_mp[(size_t)V.x * A.stride + j];
        if (r < (uint32_t)A.n_mp && !A.mp_live[r]) bad = true;
    }
    if (bad) atomicAdd(A.down + 2, 1);
}

// replaceWith(l -> w) on the tables; every lane of the walking workgroup calls it with the same arguments.  in_k is kept for slot K (-1: none).
// The caller puts a barrier behind it.  *s_stop = 1 when slot source_slot took w as a new entry.
__device__ inline void replace_row(const FuseArgs &A, int32_t l, int32_t w, int K, int32_t *s_stop) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = wave; s < A.n_kf; s += kWalk / 64) {
        int32_t *row = A.kf_mp + (size_t)s * A.stride;
        int n_l = 0;
        bool has_w = false;
        for (int j0 = 0; j0 < A.stride; j0 += 64) {
            const int j = j0 + lane;
            const int32_t r = j < A.stride ? row[j] : -1;
            n_l += __popcll(__ballot(r == l));
            has_w = has_w || __ballot(r == w) != 0ull;
        }
        if (!n_l) continue;                                  // wave-uniform
        for (int j0 = 0; j0 < A.stride; j0 += 64) {          // the wave that owns the row rewrites it
            const int j = j0 + lane;
            if (j < A.stride && row[j] == l) row[j] = has_w ? -1 : w;
        }
        if (lane == 0) {
            if (!has_w) atomicAdd(A.n_obs + w, n_l);
            if (s == K) { A.in_k[l] = 0; if (!has_w) A.in_k[w] = 1; }
            if (s == A.source_slot && !has_w) *s_stop = 1;
        }
    }
    if (threadIdx.x == kWalk - 1) {                          // the row itself: a lane of the last wave, which has the fewest slots
        A.mp_live[l] = 0; A.mp_flags[l] = 0;
        atomicExch(A.n_obs + l, 0);
        if (A.mp_track) {
            const int32_t t = A.mp_track[l];
            if (t != -1 && A.mp_track[w] == -1) {
                A.mp_track[w] = t;
                const uint32_t at = (uint32_t)t - (uint32_t)A.track_base;
                if (at < (uint32_t)A.n_track) A.track_row[at] = w;
            }
        }
    }
}

// codes 1 / 2 / 3 of the outcome table, 0 when none applies (the entry goes on to its candidate)
__device__ __forceinline__ int graph_filter(const FuseArgs &A, int32_t m) {
    if (!A.mp_live[m]) return 1;
    if (A.in_k[m]) return 2;
    if ((A.mp_flags[m] & 2) == 0) return 3;
    return 0;
}

__global__ __launch_bounds__(kWalk) void k_fuse_walk(const FuseArgs A) {
    __shared__ int32_t s_wave[kWalk / 64], s_cnt[8], s_stop;
    __shared__ uint16_t s_list[kWalk];
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_stop = 0;
    if (A.down[2]) return;                                   // uniform: written by the launch before
    __syncthreads();
    int n_erased = 0, views_done = 0;                        // the same in every lane
    for (int v = 0; v < A.n_views; ++v) {
        const int4 V = A.views[v];
        const int K = V.x;
        int32_t *krow = A.kf_mp + (size_t)K * A.stride;
        for (int j = threadIdx.x; j < A.stride; j += kWalk) {
            const uint32_t r = (uint32_t)krow[j];
            if (r < (uint32_t)A.n_mp) A.in_k[r] = 1;
        }
        __syncthreads();
        for (int t0 = 0; t0 < V.z; t0 += kWalk) {
            const int mine = t0 + (int)threadIdx.x;
            const bool valid = mine < V.z;
            const int32_t m = valid ? A.mp_index[V.y + mine] : -1;               // inside [0, n_mp): validated on the host
            const bool has = valid && A.cand[V.y + mine] >= 0;
            int code = valid && !has ? graph_filter(A, m) : 0;
            int total;
            const int rank = block_rank<kWalk>(has, s_wave, total);
            if (has) s_list[rank] = (uint16_t)threadIdx.x;
            __syncthreads();
            for (int i = 0; i < total; ++i) {
                const int at = s_list[i], e = V.y + t0 + at;
                const int32_t mm = A.mp_index[e], k = A.cand[e];                 // k inside [0, stride): the pre-pass
                int c = graph_filter(A, mm);
                int32_t x = -1;
                if (!c) {
                    x = krow[k];
                    if ((uint32_t)x >= (uint32_t)A.n_mp) { c = 4; x = -1; }
                    else if (obs_load(A.n_obs + mm) < obs_load(A.n_obs + x)) c = (A.mp_flags[x] & 2) == 0 ? 5 : 6;
                    else c = 7;
                }
                if (threadIdx.x == 0) {
                    atomicAdd(s_cnt + c, 1);
                    if (A.outcome) A.outcome[e] = (uint8_t)c;
                    if (c >= 4 && A.kp) A.kp[e] = k;
                    if (c >= 5 && A.other) A.other[e] = x;
                }
                if (c < 4) continue;                         // uniform; nothing was written that a decision reads
                __syncthreads();                             // every lane has decided
                if (c <= 5) {
                    if (threadIdx.x == 0) {
                        if (c == 5) { atomicSub(A.n_obs + x, 1); A.in_k[x] = 0; }
                        krow[k] = mm; A.in_k[mm] = 1;
                        atomicAdd(A.n_obs + mm, 1);
                    }
                } else {
                    const int32_t l = c == 6 ? mm : x, w = c == 6 ? x : mm;
                    replace_row(A, l, w, K, &s_stop);
                    if (threadIdx.x == 0) {
                        if (A.erased_rows) A.erased_rows[n_erased] = l;          // n_erased < n_entries: an entry erases at most one row
                        if (A.erased_into) A.erased_into[n_erased] = w;
                    }
                    ++n_erased;
                }
                __syncthreads();
                // x left K (5) or was erased (7): a later lane of this trip that holds x without a candidate decides again
                if (c != 6 && valid && !has && mine > t0 + at && m == x) code = graph_filter(A, m);
            }
            if (valid && !has) {
                if (A.outcome) A.outcome[V.y + mine] = (uint8_t)code;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = __popcll(__ballot(valid && !has && code == q));
                if ((threadIdx.x & 63) == 0 && n) atomicAdd(s_cnt + q, n);
            }
            __syncthreads();                                 // s_wave and s_list are free again
        }
        for (int j = threadIdx.x; j < A.stride; j += kWalk) {                    // the marks of what K lists now; a row that left K was unmarked then
            const uint32_t r = (uint32_t)krow[j];
            if (r < (uint32_t)A.n_mp) A.in_k[r] = 0;
        }
        views_done = v + 1;
        __syncthreads();
        if (s_stop) break;                                   // uniform: read behind the barrier, written before it
    }
    if (threadIdx.x == 0) { A.down[0] = n_erased; A.down[1] = views_done; }
    if (threadIdx.x < 8) A.down[3 + threadIdx.x] = s_cnt[threadIdx.x];
}

// grid over the rows of the pairs: a listed row that is not live
__global__ __launch_bounds__(kBlock) void k_pairs_check(const FuseArgs A, const int32_t *rows, int n) {
    const int i = blockIdx.x * kBlock + (int)threadIdx.x;
    if (i < n && !A.mp_live[rows[i]]) atomicAdd(A.down + 2, 1);
}

__global__ __launch_bounds__(kWalk) void k_pairs_walk(const FuseArgs A) {
    __shared__ int32_t s_stop;
    if (A.down[2]) return;
    for (int i = 0; i < A.n_pairs; ++i) {
        const int2 p = A.pairs[i];
        replace_row(A, p.x, p.y, -1, &s_stop);
        if (threadIdx.x == 0) {
            if (A.erased_rows) A.erased_rows[i] = p.x;
            if (A.erased_into) A.erased_into[i] = p.y;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) A.down[0] = A.n_pairs;
}

}  // namespace

extern "C" int ms_map_fuse(ms_ctx *c, int32_t *kf_mp, int n_kf, int stride, uint8_t *mp_flags, uint8_t *mp_live, int32_t *n_obs, int n_mp, int32_t *mp_track,
                           int32_t *track_row, int track_base, int n_track, const int32_t *kept_entry, const int32_t *top_idx, const uint16_t *top_dist,
                           const int32_t *mp_index, int n_entries, const ms_fuse_view *views, const int32_t *n_kept, int n_views, int max_dist, int source_slot,
                           uint8_t *outcome, int32_t *kp, int32_t *other, int32_t *erased_rows, int32_t *erased_into, int32_t *n_erased, int32_t *counts,
                           int32_t *views_done) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_map_fuse_check(kf_mp, n_kf, stride, mp_flags, mp_live, n_obs, n_mp, mp_track, track_row, track_base, n_track, kept_entry, top_idx, top_dist, mp_index,
                                n_entries, views, n_kept, n_views, max_dist, source_slot, n_erased, counts, views_done, c->err, sizeof(c->err))))
        return rc;
    *n_erased = 0;
    std::memset(counts, 0, 8 * sizeof(int32_t));
    *views_done = n_views;
    if (n_views == 0) return MS_OK;                          // nothing is walked: the per-entry outputs are not touched
    MsRange range("mapFuse");
    const size_t ne = (size_t)n_entries, nv = (size_t)n_views, nm = (size_t)n_mp;
    // upload block: mp_index | the views with their n_kept; then (host only) the results
    MsLayout up;
    const auto l_idx = up.array<int32_t>(ne);
    const auto l_views = up.array<int4>(nv);
    MsLayout host = up, dev = up;
    const auto l_down = host.array<int32_t>(kDown);
    // device-only block: results | candidates | the "listed by K" marks
    const auto l_res = dev.array<int32_t>(kDown);
    const auto l_cand = dev.array<int32_t>(ne);
    const auto l_ink = dev.array<uint8_t>(nm);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_MAP_FUSE];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    l_idx.fill(hs, mp_index);
    int4 *hv = l_views.at(hs);
    int max_count = 0;
    for (int v = 0; v < n_views; ++v) {
        hv[v] = make_int4(views[v].slot, views[v].first, views[v].count, n_kept[v]);
        max_count = std::max(max_count, n_kept[v]);
    }
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    FuseArgs A{};
    A.kf_mp = kf_mp; A.mp_flags = mp_flags; A.mp_live = mp_live; A.n_obs = n_obs; A.mp_track = mp_track; A.track_row = track_row;
    A.kept_entry = kept_entry; A.top_idx = top_idx; A.top_dist = top_dist;
    A.mp_index = l_idx.at(ds); A.views = l_views.at(ds);
    A.cand = l_cand.at(ds); A.in_k = l_ink.at(ds);
    A.outcome = outcome; A.kp = kp; A.other = other; A.erased_rows = erased_rows; A.erased_into = erased_into;
    A.down = l_res.at(ds);
    A.n_kf = n_kf; A.stride = stride; A.n_mp = n_mp; A.n_entries = n_entries; A.n_views = n_views; A.n_track = n_track; A.track_base = track_base;
    A.max_dist = max_dist; A.source_slot = source_slot;
    const dim3 block(kBlock);
    hipLaunchKernelGGL(k_fuse_fill, dim3((unsigned)ms_div_up(std::max(std::max(n_entries, n_mp), kDown), kBlock)), block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_fuse_fill");
    hipLaunchKernelGGL(k_fuse_scatter, dim3((unsigned)ms_div_up(std::max(max_count, stride), kBlock), (unsigned)n_views), block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_fuse_scatter");
    hipLaunchKernelGGL(k_fuse_walk, dim3(1), dim3(kWalk), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_fuse_walk");
    MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_res.at(ds), l_res.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *down = l_down.at(hs);
    if (down[2])
        return ms_fail(c, MS_ERR_INVALID, "map fuse: %d violations on the device (a kept_entry outside its view's slice, a top_idx outside [-1, %d), or a walked slot "
                       "that lists a row which is not live); the tables are untouched", down[2], stride);
    *n_erased = down[0]; *views_done = down[1];
    std::memcpy(counts, down + 3, 8 * sizeof(int32_t));
    return MS_OK;
}

extern "C" int ms_map_replace_pairs(ms_ctx *c, int32_t *kf_mp, int n_kf, int stride, uint8_t *mp_flags, uint8_t *mp_live, int32_t *n_obs, int n_mp, int32_t *mp_track,
                                    int32_t *track_row, int track_base, int n_track, const int32_t *pairs, int n_pairs, uint8_t *outcome, int32_t *erased_rows,
                                    int32_t *erased_into, int32_t *n_erased) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_map_replace_pairs_check(kf_mp, n_kf, stride, mp_flags, mp_live, n_obs, n_mp, mp_track, track_row, track_base, n_track, pairs, n_pairs, outcome, n_erased,
                                         c->err, sizeof(c->err))))
        return rc;
    *n_erased = 0;
    if (n_pairs == 0) return MS_OK;
    MsRange range("mapReplacePairs");
    const size_t np = (size_t)n_pairs;
    // upload block: every listed row | the pairs that run; then (host only) the results
    MsLayout up;
    const auto l_rows = up.array<int32_t>(2 * np);
    const auto l_pairs = up.array<int2>(np);
    MsLayout host = up, dev = up;
    const auto l_down = host.array<int32_t>(kDown);
    const auto l_res = dev.array<int32_t>(kDown);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_MAP_FUSE];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    l_rows.fill(hs, pairs);
    const int n_run = ms_pair_outcomes(pairs, n_pairs, outcome);
    int2 *run = l_pairs.at(hs);
    for (int i = 0, k = 0; i < n_pairs; ++i)
        if (outcome[i] == 0) run[k++] = make_int2(pairs[2 * i], pairs[2 * i + 1]);
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    FuseArgs A{};
    A.kf_mp = kf_mp; A.mp_flags = mp_flags; A.mp_live = mp_live; A.n_obs = n_obs; A.mp_track = mp_track; A.track_row = track_row;
    A.pairs = l_pairs.at(ds);
    A.erased_rows = erased_rows; A.erased_into = erased_into;
    A.down = l_res.at(ds);
    A.n_kf = n_kf; A.stride = stride; A.n_mp = n_mp; A.n_pairs = n_run; A.n_track = n_track; A.track_base = track_base; A.source_slot = -1;
    MS_HIP(c, hipMemsetAsync(l_res.at(ds), 0, l_res.bytes(), c->stream));
    hipLaunchKernelGGL(k_pairs_check, dim3((unsigned)ms_div_up(2 * n_pairs, kBlock)), dim3(kBlock), 0, c->stream, A, (const int32_t *)l_rows.at(ds), 2 * n_pairs);
    MS_KERNEL_CHECK(c, "k_pairs_check");
    hipLaunchKernelGGL(k_pairs_walk, dim3(1), dim3(kWalk), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_pairs_walk");
    MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_res.at(ds), l_res.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *down = l_down.at(hs);
    if (down[2]) return ms_fail(c, MS_ERR_INVALID, "map replace pairs: %d listed rows are not live; the tables are untouched", down[2]);
    *n_erased = down[0];
    return MS_OK;
}
