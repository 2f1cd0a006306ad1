// search_bind.hip -- the walk of searchByProjection behind its gates and its scoring, on the device map tables, in place:
//   ms_bound_mask    skip[j] = "keypoint j of slot K carries a map point" (keyframe_matcher.cpp:358), the t_skip of ms_projection_topk
//   ms_search_bind   the greedy walk of keyframe_matcher.cpp:349-389 over the kept queries of ONE view (detail::replay_search of the host
//                    mirror) and both addObservations (:388-389): kf_mp[K][best] = m, n_obs[m] += 1
// A query's decision reads the keypoints the queries before it bound, so ONE workgroup of 1024 lanes walks, as k_fuse_walk does; what is
// parallel is the settling of the queries that need no step, and the inside of a rescan.
//
// ms_search_bind, four launches whatever n_kept is:
//   k_sbind_fill    match_kp = -1, outcome = 0, the row marks = 0, the result block = 0
//   k_sbind_marks   lane j = keypoint j of K: marks the row K lists there, counts a skip[j] that disagrees with kf_mp[K][j]
//   k_sbind_check   lane q = kept query q: kept_entry inside the slice, the four top_idx inside [-1, n_kp) and not marked by skip, the row live,
//                   not listed by K, not named by an earlier query (one atomicOr per query on the row marks).  Both only count violations.
//   k_sbind_walk    nothing when a violation was counted.  The marks of the keypoints (bit 0 = skip, bit 1 = taken in this call) live in LDS, a
//                   byte per keypoint (n_kp <= MS_COVIS_MAX_STRIDE = 8192).  The queries are read in trips of 1024: a lane settles its own query
//                   when the list is empty (code 0) or its first entry is farther than 100 (code 1: every candidate, free or not, is at least
//                   that far); the others are compacted (block_rank, ms_scan.h) and stepped through in order.  A step's decision is made by
//                   every lane from the same addresses, so it is uniform and needs no broadcast; a barrier separates it from the step's
//                   writes and another one closes the step.  A step that binds nothing writes no state and takes no barrier.
//   rescan          a step whose list ran out (fewer than two free entries, n_scored > 4) scans the query's y band again against the marks
//                   as they stand: every lane bisects the same range, the lanes stride over it 1024 positions at a time with the float32
//                   arithmetic of k_projection_candidates, each keeps its two smallest keys (distance << 20 | position in the sorted array,
//                   the key of the top-4 lists), a butterfly reduces them inside a wave and 16 pairs go through LDS.  Positions stay below
//                   8192, so the 32-bit key never overflows and there is no wider fallback.
// All barriers are in uniform control flow: loop bounds are launch arguments, values every lane reads from the same address, or block_rank's
// total.  n_obs is touched only by an agent-scope atomic add.  Integer and correctly rounded float32 work: the same input gives the same bits on every call.
#include "ms_internal.h"
#include "ms_scan.h"
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int kWalk = 1024;                                  // lanes of the one walking workgroup
constexpr int kDown = 2 + 6;                                 // n_matched, violations, counts[6]
constexpr uint32_t kNoKey = 0xffffffffu;
constexpr int kMaxKp = MS_COVIS_MAX_STRIDE;                  // n_kp <= stride <= this: the LDS marks

struct BindArgs {
    int32_t *kf_mp;
    const uint8_t *mp_live;
    int32_t *n_obs;
    const int32_t *kept_entry;
    const float *q_x, *q_y, *q_radius;
    const int32_t *q_lo, *q_hi;                              // each may be null
    const uint32_t *q_desc;
    const int32_t *top_idx;
    const uint16_t *top_dist;
    const int32_t *top_octave, *n_scored;
    const uint8_t *skip;
    const float *sx, *sy;
    const int32_t *sidx;
    const uint32_t *t_desc;
    const int32_t *t_octave;
    const int32_t *rows;                                     // [count]: mp_index[first ...], the workspace's copy
    uint32_t *marks;                                         // [n_mp] bytes in words: bit 0 = K lists the row, bit 1 = a kept query names it
    int32_t *match_kp;                                       // each of the three may be null
    uint8_t *outcome, *usable;
    int32_t *down;                                           // [kDown]
    int32_t stride, n_mp, n_kp, first, count, n_kept, slot;
};

__global__ __launch_bounds__(kBlock) void k_bound_mask(const int32_t *krow, int n_kp, int n_mp, uint8_t *skip) {
    const int j = blockIdx.x * kBlock + (int)threadIdx.x;
    if (j < n_kp) skip[j] = (uint8_t)((uint32_t)krow[j] < (uint32_t)n_mp);
}

__global__ __launch_bounds__(kBlock) void k_sbind_fill(const BindArgs A) {
    const int i = blockIdx.x * kBlock + (int)threadIdx.x;
    if (i < A.count) {
        if (A.match_kp) A.match_kp[i] = -1;
        if (A.outcome) A.outcome[i] = 0;
    }
    if (i < (A.n_mp + 3) / 4) A.marks[i] = 0u;
    if (i < kDown) A.down[i] = 0;
}

__device__ __forceinline__ uint32_t mark_row(uint32_t *marks, int32_t m, uint32_t bit) { return atomicOr(marks + (m >> 2), bit << (8 * (m & 3))) >> (8 * (m & 3)); }

__global__ __launch_bounds__(kBlock) void k_sbind_marks(const BindArgs A) {
    const int j = blockIdx.x * kBlock + (int)threadIdx.x;
    if (j >= A.stride) return;
    const uint32_t r = (uint32_t)A.kf_mp[(size_t)A.slot * A.stride + j];
    const bool is_bound = r < (uint32_t)A.n_mp;
    if (is_bound) mark_row(A.marks, (int32_t)r, 1u);
    if (j < A.n_kp && (A.skip[j] != 0) != is_bound) atomicAdd(A.down + 1, 1);
}

__global__ __launch_bounds__(kBlock) void k_sbind_check(const BindArgs A) {
    const int q = blockIdx.x * kBlock + (int)threadIdx.x;
    if (q >= A.n_kept) return;
    const int32_t e = A.kept_entry[q];
    bool bad = e < A.first || e >= A.first + A.count;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int32_t t = A.top_idx[4 * (size_t)q + i];
        if (t < -1 || t >= A.n_kp) bad = true;
        else if (t >= 0 && A.skip[t]) bad = true;
    }
    if (e >= A.first && e < A.first + A.count) {
        const int32_t m = A.rows[e - A.first];                // inside [0, n_mp): validated on the host
        if (!A.mp_live[m]) bad = true;
        if (mark_row(A.marks, m, 2u) & 3u) bad = true;        // K lists it, or an earlier query named it
    }
    if (bad) atomicAdd(A.down + 1, 1);
}

__device__ __forceinline__ uint32_t hamming256(const uint32_t (&q)[8], const uint32_t *t) {
    const uint4 a = reinterpret_cast<const uint4 *>(t)[0], b = reinterpret_cast<const uint4 *>(t)[1];
    return __popc(q[0] ^ a.x) + __popc(q[1] ^ a.y) + __popc(q[2] ^ a.z) + __popc(q[3] ^ a.w) + __popc(q[4] ^ b.x) + __popc(q[5] ^ b.y) + __popc(q[6] ^ b.z) +
           __popc(q[7] ^ b.w);
}

// The two smallest keys of query q over its y band against the marks as they stand; every lane of the workgroup calls it with the same q
// and gets the same pair.  Two barriers, the second one behind the reads of s_key.
__device__ inline void rescan(const BindArgs &A, int q, const uint8_t *s_mark, uint32_t (*s_key)[2], uint32_t &k1, uint32_t &k2) {
    const uint4 qa = reinterpret_cast<const uint4 *>(A.q_desc)[2 * (size_t)q], qb = reinterpret_cast<const uint4 *>(A.q_desc)[2 * (size_t)q + 1];
    const uint32_t qd[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
    const float x = A.q_x[q], y = A.q_y[q], r = A.q_radius[q];
    const float ylo = __fsub_rn(y, r), yhi = __fadd_rn(y, r), r2 = __fmul_rn(r, r);
    const int lmin = A.q_lo ? A.q_lo[q] : -0x7fffffff, lmax = A.q_hi ? A.q_hi[q] : 0x7fffffff;
    int lo = 0, hi = A.n_kp;
    while (lo < hi) {                                        // first position whose y is not < qy - r; the same in every lane
        const int mid = (lo + hi) >> 1;
        if (A.sy[mid] < ylo) lo = mid + 1; else hi = mid;
    }
    uint32_t best = kNoKey, second = kNoKey;
    for (int p0 = lo; p0 < A.n_kp && A.sy[p0] <= yhi; p0 += kWalk) {             // uniform: sorted, so a trip whose first position is outside ends the band
        const int pos = p0 + (int)threadIdx.x;
        if (pos >= A.n_kp) continue;
        const float py = A.sy[pos];
        if (!(py <= yhi)) continue;
        const float dx = __fsub_rn(x, A.sx[pos]), dy = __fsub_rn(y, py);
        if (!(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < r2)) continue;
        const int j = A.sidx[pos];
        if (s_mark[j]) continue;                             // skipped by the scoring, or taken in this call
        const int o = A.t_octave[j];
        if (o < lmin || o > lmax) continue;
        const uint32_t key = (hamming256(qd, A.t_desc + 8 * (size_t)j) << 20) | (uint32_t)pos;
        const uint32_t l2 = min(best, key), h2 = max(best, key);
        second = min(second, h2);
        best = l2;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t ob = __shfl_xor(best, off, 64), os = __shfl_xor(second, off, 64);
        const uint32_t l2 = min(best, ob), h2 = max(best, ob);
        second = min(min(second, os), h2);
        best = l2;
    }
    // s_key is free: the reads of an earlier rescan lie in front of its last barrier
    if ((threadIdx.x & 63) == 0) { s_key[threadIdx.x >> 6][0] = best; s_key[threadIdx.x >> 6][1] = second; }
    __syncthreads();
    k1 = kNoKey; k2 = kNoKey;
#pragma unroll
    for (int w = 0; w < kWalk / 64; ++w) {
        const uint32_t ob = s_key[w][0], os = s_key[w][1];
        const uint32_t l2 = min(k1, ob), h2 = max(k1, ob);
        k2 = min(min(k2, os), h2);
        k1 = l2;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kWalk) void k_sbind_walk(const BindArgs A) {
    __shared__ int32_t s_wave[kWalk / 64], s_cnt[6];
    __shared__ uint16_t s_list[kWalk];
    __shared__ uint32_t s_key[kWalk / 64][2];
    __shared__ uint8_t s_mark[kMaxKp];
    if (A.down[1]) return;                                   // uniform: written by the launches before
    if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0;
    for (int j = threadIdx.x; j < A.n_kp; j += kWalk) s_mark[j] = A.skip[j] ? 1 : 0;
    __syncthreads();
    int32_t *krow = A.kf_mp + (size_t)A.slot * A.stride;
    int n_matched = 0;                                       // the same in every lane
    for (int t0 = 0; t0 < A.n_kept; t0 += kWalk) {
        const int mine = t0 + (int)threadIdx.x;
        const bool valid = mine < A.n_kept;
        int code = -1;
        if (valid) {
            if (A.top_idx[4 * (size_t)mine] < 0) code = 0;
            else if ((int)A.top_dist[4 * (size_t)mine] > MS_HAMMING_THR_HIGH) code = 1;
        }
        const bool stepped = valid && code < 0;
        int total;
        const int rank = block_rank<kWalk>(stepped, s_wave, total);
        if (stepped) s_list[rank] = (uint16_t)threadIdx.x;
        if (valid && !stepped && A.outcome) A.outcome[mine] = (uint8_t)code;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int n = __popcll(__ballot(valid && code == c));
            if ((threadIdx.x & 63) == 0 && n) atomicAdd(s_cnt + c, n);
        }
        __syncthreads();
        for (int i = 0; i < total; ++i) {
            const int q = t0 + (int)s_list[i];
            int best = -1, bd = 256, bd2 = 256, bl = -1, bl2 = -1, found = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int32_t j = A.top_idx[4 * (size_t)q + k];                  // inside [-1, n_kp): the pre-pass
                if (j < 0) break;
                if (found == 2 || (s_mark[j] & 2)) continue;
                const int d = A.top_dist[4 * (size_t)q + k], o = A.top_octave[4 * (size_t)q + k];
                if (found == 0) { best = j; bd = d; bl = o; } else { bd2 = d; bl2 = o; }
                ++found;
            }
            const bool again = found < 2 && A.n_scored[q] > 4;
            if (again) {                                     // uniform
                uint32_t k1, k2;
                rescan(A, q, s_mark, s_key, k1, k2);
                best = -1; bd = 256; bd2 = 256; bl = -1; bl2 = -1;
                if (k1 != kNoKey) { best = A.sidx[k1 & 0xFFFFFu]; bd = (int)(k1 >> 20); bl = A.t_octave[best]; }
                if (k2 != kNoKey) { bd2 = (int)(k2 >> 20); bl2 = A.t_octave[A.sidx[k2 & 0xFFFFFu]]; }
            }
            int c;
            if (best < 0) c = 0;
            else if (bd > MS_HAMMING_THR_HIGH) c = 1;
            else if (bl == bl2 && (double)bd > 0.8 * (double)bd2) c = 2;
            else c = again ? 4 : 3;
            if (threadIdx.x == 0) {
                atomicAdd(s_cnt + c, 1);
                if (again) atomicAdd(s_cnt + 5, 1);
                if (A.outcome) A.outcome[q] = (uint8_t)(c < 3 && again ? c | 8 : c);
            }
            if (c < 3) continue;                             // uniform; nothing was written that a decision reads
            __syncthreads();                                 // every lane has decided
            if (threadIdx.x == 0) {
                const int32_t e = A.kept_entry[q], m = A.rows[e - A.first];      // inside the slice: the pre-pass
                krow[best] = m;
                __hip_atomic_fetch_add(A.n_obs + m, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s_mark[best] |= 2;
                if (A.match_kp) A.match_kp[e - A.first] = best;
                if (A.usable) A.usable[best] = 0;
            }
            ++n_matched;
            __syncthreads();
        }
        __syncthreads();                                     // s_wave and s_list are free again
    }
    if (threadIdx.x == 0) A.down[0] = n_matched;
    if (threadIdx.x < 6) A.down[2 + threadIdx.x] = s_cnt[threadIdx.x];
}

}  // namespace

extern "C" int ms_bound_mask(ms_ctx *c, const int32_t *kf_mp, int n_kf, int stride, int n_mp, int slot, int n_kp, uint8_t *skip) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_bound_mask_check(kf_mp, n_kf, stride, n_mp, slot, n_kp, skip, c->err, sizeof(c->err)))) return rc;
    if (n_kp == 0) return MS_OK;
    MsRange range("boundMask");
    MS_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_bound_mask, dim3((unsigned)ms_div_up(n_kp, kBlock)), dim3(kBlock), 0, c->stream, kf_mp + (size_t)slot * stride, n_kp, n_mp, skip);
    MS_KERNEL_CHECK(c, "k_bound_mask");
    return MS_OK;                                            // in stream order with the scoring that reads it
}

extern "C" int ms_search_bind(ms_ctx *c, int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, int32_t *n_obs, int n_mp, const int32_t *kept_entry,
                              const float *q_x, const float *q_y, const float *q_radius, const int32_t *q_min_octave, const int32_t *q_max_octave, const uint32_t *q_desc,
                              const int32_t *top_idx, const uint16_t *top_dist, const int32_t *top_octave, const int32_t *n_scored, const uint8_t *skip,
                              const float *sorted_x, const float *sorted_y, const int32_t *sorted_idx, const uint32_t *t_desc, const int32_t *t_octave, int n_kp,
                              const int32_t *mp_index, int first, int count, int n_kept, int slot, int32_t *match_kp, uint8_t *outcome, uint8_t *usable,
                              int32_t *n_matched, int32_t *counts) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_search_bind_check(kf_mp, n_kf, stride, mp_live, n_obs, n_mp, kept_entry, q_x, q_y, q_radius, q_min_octave, q_max_octave, q_desc, top_idx, top_dist,
                                   top_octave, n_scored, skip, sorted_x, sorted_y, sorted_idx, t_desc, t_octave, n_kp, mp_index, first, count, n_kept, slot, n_matched,
                                   counts, c->err, sizeof(c->err))))
        return rc;
    *n_matched = 0;
    std::memset(counts, 0, 6 * sizeof(int32_t));
    if (count == 0) return MS_OK;                            // no entry: nothing is written
    MsRange range("searchBind");
    // upload block: the slice of mp_index; then (host only) the results
    MsLayout up;
    const auto l_rows = up.array<int32_t>((size_t)count);
    MsLayout host = up, dev = up;
    const auto l_down = host.array<int32_t>(kDown);
    // device-only block: results | the row marks, a byte per row in whole words
    const auto l_res = dev.array<int32_t>(kDown);
    const auto l_marks = dev.array<uint32_t>(((size_t)n_mp + 3) / 4);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_SEARCH_BIND];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    l_rows.fill(hs, mp_index + first);
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    BindArgs A{};
    A.kf_mp = kf_mp; A.mp_live = mp_live; A.n_obs = n_obs;
    A.kept_entry = kept_entry; A.q_x = q_x; A.q_y = q_y; A.q_radius = q_radius; A.q_lo = q_min_octave; A.q_hi = q_max_octave; A.q_desc = q_desc;
    A.top_idx = top_idx; A.top_dist = top_dist; A.top_octave = top_octave; A.n_scored = n_scored; A.skip = skip;
    A.sx = sorted_x; A.sy = sorted_y; A.sidx = sorted_idx; A.t_desc = t_desc; A.t_octave = t_octave;
    A.rows = l_rows.at(ds); A.marks = l_marks.at(ds);
    A.match_kp = match_kp; A.outcome = outcome; A.usable = usable;
    A.down = l_res.at(ds);
    A.stride = stride; A.n_mp = n_mp; A.n_kp = n_kp; A.first = first; A.count = count; A.n_kept = n_kept; A.slot = slot;
    const dim3 block(kBlock);
    hipLaunchKernelGGL(k_sbind_fill, dim3((unsigned)ms_div_up(std::max(std::max(count, (n_mp + 3) / 4), kDown), kBlock)), block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_sbind_fill");
    if (n_kept > 0) {
        hipLaunchKernelGGL(k_sbind_marks, dim3((unsigned)ms_div_up(stride, kBlock)), block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_sbind_marks");
        hipLaunchKernelGGL(k_sbind_check, dim3((unsigned)ms_div_up(n_kept, kBlock)), block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_sbind_check");
        hipLaunchKernelGGL(k_sbind_walk, dim3(1), dim3(kWalk), 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_sbind_walk");
    }
    MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_res.at(ds), l_res.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *down = l_down.at(hs);
    if (down[1])
        return ms_fail(c, MS_ERR_INVALID, "search bind: %d violations on the device (a kept_entry outside the slice, a top_idx outside [-1, %d) or marked by skip, "
                       "skip disagreeing with slot %d's row, or a row that is not live, that the slot already lists or that two kept queries name); the tables are "
                       "untouched", down[1], n_kp, slot);
    *n_matched = down[0];
    std::memcpy(counts, down + 2, 6 * sizeof(int32_t));
    return MS_OK;
}
