// map_cull.hip -- observation counts and the two culling passes of addKeyframeCommonInner on the keyframe table kf_mp (slot -> map-point rows):
//   ms_observation_count   mp.observations.size(), getFirstObservation / getLastObservation   map_point.cpp:45-63
//   ms_map_cull            cullMapPoints, then cullKeyframes                                   mapper_helpers.cpp:349-373, :433-482
//
// The device holds kf_mp and not its transpose, so "how many keyframes observe row r, and which is the oldest" is one pass over the table with
// integer atomics: add on n_obs[r], min / max on the slot's position in KfId order (the host sorts the slots by kf_id once per call and
// uploads position <-> slot, so the atomics stay 32 bits wide and the result does not depend on the order of arrival).  An entry r is used
// only after (uint32)r < n_mp held.
//
// ms_observation_count, three launches whatever the sizes:
//   k_obs_fill      n_obs = 0, first = none, last = -1 (and ms_map_cull's marks and result block)
//   k_obs_count     one lane per entry of every slot with kf_id >= 0: the three atomics; ms_map_cull also marks the rows of the current slot
//   k_obs_finish    position -> slot
// ms_map_cull, eight launches whatever n_mp, n_kf and n_cand are:
//   k_obs_fill, k_obs_count
//   k_cull_points   one lane per row: the decision of cullMapPoints depends on that row alone (left out for cull_points == 0)
//   k_cull_keyframes  ONE workgroup walks the candidates in descending KfId order; within a candidate the count over its entries and the
//                   decrements of their observation counts are parallel.  The decrements are agent-scope atomics and the counts of the next
//                   candidate are read with agent-scope atomic loads behind a workgroup barrier (a plain load may be served from the CU's L1)
//   k_cull_sweep    one lane per entry of the table: an entry whose row was removed becomes -1 (removeMapPoint's eraseObservation)
//   k_cull_count / k_cull_offsets / k_cull_pack   block_rank, per-workgroup count and block_offsets (ms_scan.h) over 256-row
//                   blocks: removed_rows is in ascending row order
// Nothing here depends on which lane's atomic arrives first: the same input gives the same bits on every call.
//
// What stays with the host mirror (it derives them from cand_removed and the downloaded removed_rows): the previousKfId / nextKfId links, the
// `uncertainty` accumulation, re-pointing referenceKeyframe, trackIdToMapPoint and bowIndex->remove.
#include "ms_internal.h"
#include "ms_scan.h"
#include <algorithm>
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int kWalk = 1024;                                  // lanes of the one workgroup of k_cull_keyframes

struct CullArgs {
    int32_t *kf_mp;
    uint8_t *mp_flags, *mp_live;
    const int32_t *slot_rank;            // [n_kf]: the slot's position in KfId order, -1 for an empty slot
    const int32_t *rank_slot;            // [slots with kf_id >= 0]: the inverse
    const double *kf_t;                  // [n_kf]
    const int2 *walk;                    // [n_walk]: (slot, the caller's position in cand), descending KfId, kept candidates dropped
    int32_t *n_obs, *first, *last;       // [n_mp]; first / last are positions in KfId order
    int32_t *first_slot, *last_slot;     // ms_observation_count's outputs, each may be null
    uint8_t *in_cur, *why1, *why3;       // [n_mp]: listed by the current slot | reason of pass 1 | 3 for a row orphaned in pass 2
    int32_t *blk_count, *blk_off;        // [n_blk]
    int32_t *removed_rows;
    uint8_t *removed_why;
    int32_t *down;                       // [2 + n_cand]: n_removed_rows, n_removed_kf, cand_removed in the caller's order
    double min_age, ratio;
    int32_t n_kf, stride, n_mp, n_blk, per_slot, n_walk, n_down, current_slot, min_obs, ratio_f32;
};

__global__ __launch_bounds__(kBlock) void k_obs_fill(const CullArgs A) {
    const int r = blockIdx.x * kBlock + (int)threadIdx.x;
    if (r < A.n_mp) {
        A.n_obs[r] = 0; A.first[r] = kNone; A.last[r] = -1;
        if (A.in_cur) { A.in_cur[r] = 0; A.why1[r] = 0; A.why3[r] = 0; }
    }
    if (r < A.n_down) A.down[r] = 0;
}

__global__ __launch_bounds__(kBlock) void k_obs_count(const CullArgs A) {
    const int slot = blockIdx.x / A.per_slot, j = (blockIdx.x % A.per_slot) * kBlock + (int)threadIdx.x;
    if (j >= A.stride) return;
    const int rank = A.slot_rank[slot];
    if (rank < 0) return;
    const uint32_t r = (uint32_t)A.kf_mp[(size_t)slot * A.stride + j];
    if (r >= (uint32_t)A.n_mp) return;
    atomicAdd(A.n_obs + r, 1);
    atomicMin(A.first + r, rank);
    atomicMax(A.last + r, rank);
    if (A.in_cur && slot == A.current_slot) A.in_cur[r] = 1;
}

__global__ __launch_bounds__(kBlock) void k_obs_finish(const CullArgs A) {
    const int r = blockIdx.x * kBlock + (int)threadIdx.x;
    if (r >= A.n_mp) return;
    const bool any = A.n_obs[r] > 0;
    if (A.first_slot) A.first_slot[r] = any ? A.rank_slot[A.first[r]] : -1;
    if (A.last_slot) A.last_slot[r] = any ? A.rank_slot[A.last[r]] : -1;
}

// cullMapPoints, mapper_helpers.cpp:357-371, for one row
__global__ __launch_bounds__(kBlock) void k_cull_points(const CullArgs A) {
    const int r = blockIdx.x * kBlock + (int)threadIdx.x;
    if (r >= A.n_mp || !A.mp_live[r]) return;
    uint8_t reason = 0;
    if (A.n_obs[r] == 0) reason = 1;                                                     // :359
    else if (!A.in_cur[r] && (A.mp_flags[r] & 1) == 0) {
        const int32_t age = (int32_t)__dsub_rn(A.kf_t[A.current_slot], A.kf_t[A.rank_slot[A.first[r]]]);        // const int obsAge: toward zero
        if ((double)age > A.min_age) reason = 2;                                         // :365
    }
    if (!reason) return;
    A.why1[r] = reason;
    A.mp_live[r] = 0; A.mp_flags[r] = 0; A.n_obs[r] = 0;
}

// cullKeyframes, mapper_helpers.cpp:447-481, and removeKeyframe's walk over the keyframe's map points (:391-405)
__global__ __launch_bounds__(kWalk) void k_cull_keyframes(const CullArgs A) {
    __shared__ int32_t s_mp[kWalk / 64], s_cr[kWalk / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n_removed = 0;
    for (int c = 0; c < A.n_walk; ++c) {
        const int2 cand = A.walk[c];
        int32_t *row = A.kf_mp + (size_t)cand.x * A.stride;
        int n_mp = 0, n_cr = 0;                              // wave totals
        for (int j0 = 0; j0 < A.stride; j0 += kWalk) {
            const int j = j0 + (int)threadIdx.x;
            bool is = false, critical = false;
            if (j < A.stride) {
                const uint32_t r = (uint32_t)row[j];
                if (r < (uint32_t)A.n_mp && !A.why1[r]) {
                    is = true;
                    critical = __hip_atomic_load(A.n_obs + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= A.min_obs;
                }
            }
            n_mp += __popcll(__ballot(is));
            n_cr += __popcll(__ballot(critical));
        }
        if (lane == 0) { s_mp[wave] = n_mp; s_cr[wave] = n_cr; }
        __syncthreads();
        int nMapPoints = 0, nCritical = 0;
#pragma unroll
        for (int w = 0; w < kWalk / 64; ++w) { nMapPoints += s_mp[w]; nCritical += s_cr[w]; }
        const bool remove = A.ratio_f32 ? (float)nCritical < __fmul_rn((float)nMapPoints, (float)A.ratio)
                                        : (double)nCritical < __dmul_rn((double)nMapPoints, A.ratio);             // :476
        if (remove) {
            for (int j = threadIdx.x; j < A.stride; j += kWalk) {
                const uint32_t r = (uint32_t)row[j];
                if (r < (uint32_t)A.n_mp && !A.why1[r]) {
                    const int before = atomicSub(A.n_obs + r, 1);                        // eraseObservation
                    if (before == 1 && A.mp_live[r]) {                                   // orphaned: only the lane that took the last one comes here
                        A.why3[r] = 3;
                        A.mp_live[r] = 0;
                        if (A.mp_flags) A.mp_flags[r] = 0;
                    }
                }
                row[j] = -1;
            }
            if (threadIdx.x == 0) { A.down[2 + cand.y] = 1; ++n_removed; }
        }
        __syncthreads();                                     // the next candidate's counts come after this one's decrements; s_mp / s_cr are free again
    }
    if (threadIdx.x == 0) A.down[1] = n_removed;
}

__global__ __launch_bounds__(kBlock) void k_cull_sweep(const CullArgs A) {
    const int slot = blockIdx.x / A.per_slot, j = (blockIdx.x % A.per_slot) * kBlock + (int)threadIdx.x;
    if (j >= A.stride) return;
    int32_t *e = A.kf_mp + (size_t)slot * A.stride + j;
    const uint32_t r = (uint32_t)*e;
    if (r < (uint32_t)A.n_mp && (A.why1[r] | A.why3[r])) *e = -1;
}

// the lane's row, its reason and its rank among the workgroup's removed rows, in row order; the workgroup's total through `total`
__device__ inline int cull_rank(const CullArgs &A, int32_t *s_wave, int &r, uint8_t &why, int &total) {
    r = blockIdx.x * kBlock + (int)threadIdx.x;
    why = r < A.n_mp ? (uint8_t)(A.why1[r] | A.why3[r]) : (uint8_t)0;      // a row has at most one of the two
    return block_rank<kBlock>(why != 0, s_wave, total);
}

__global__ __launch_bounds__(kBlock) void k_cull_count(const CullArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    int r, total;
    uint8_t why;
    cull_rank(A, s_wave, r, why, total);
    if (threadIdx.x == 0) A.blk_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_cull_offsets(const CullArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int removed = block_offsets<kBlock>(A.blk_count, A.blk_off, A.n_blk, s_wave);
    if (threadIdx.x == 0) A.down[0] = removed;
}

__global__ __launch_bounds__(kBlock) void k_cull_pack(const CullArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    int r, total;
    uint8_t why;
    const int rank = cull_rank(A, s_wave, r, why, total);
    if (!why) return;
    const size_t dst = (size_t)A.blk_off[blockIdx.x] + (size_t)rank;     // below n_mp: a prefix count of rows
    A.removed_rows[dst] = r;
    if (A.removed_why) A.removed_why[dst] = why;
}

}  // namespace

extern "C" int ms_observation_count(ms_ctx *c, const int32_t *kf_mp, int n_kf, int stride, int n_mp, const int32_t *kf_id, int32_t *n_obs, int32_t *first_slot,
                                    int32_t *last_slot) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_kf_table_check("observation count", kf_mp, n_kf, stride, n_mp, kf_id, c->err, sizeof(c->err)))) return rc;
    if (ms_map_over_capacity(n_kf, stride, n_mp, 0)) return ms_why_table_caps("observation count", n_kf, stride, n_mp, c->err, sizeof(c->err));
    const std::vector<int32_t> &order = ms_slots_by_id();    // the slots in KfId order, left by the validation
    if (n_mp == 0 || (!n_obs && !first_slot && !last_slot)) return MS_OK;
    MsRange range("observationCount");
    const size_t nk = (size_t)n_kf, nm = (size_t)n_mp;
    // upload block: slot -> position in KfId order | position -> slot
    MsLayout up;
    const auto l_sr = up.array<int32_t>(nk), l_rs = up.array<int32_t>(order.size());
    MsLayout dev = up;
    // device-only block: first / last positions | the counts when the caller does not want them
    const auto l_first = dev.array<int32_t>(nm), l_last = dev.array<int32_t>(nm), l_n = dev.array<int32_t>(n_obs ? 0 : nm);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_MAP_CULL];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    ms_fill_ranks(order, n_kf, l_sr.at(hs), l_rs.at(hs));
    if (up.end) MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    CullArgs A{};
    A.kf_mp = const_cast<int32_t *>(kf_mp);                  // read only here
    A.slot_rank = l_sr.at(ds); A.rank_slot = l_rs.at(ds);
    A.n_obs = n_obs ? n_obs : l_n.at(ds);
    A.first = l_first.at(ds); A.last = l_last.at(ds);
    A.first_slot = first_slot; A.last_slot = last_slot;
    A.n_kf = n_kf; A.stride = stride; A.n_mp = n_mp; A.per_slot = ms_div_up(stride, kBlock); A.current_slot = -1;
    const dim3 block(kBlock), by_row((unsigned)ms_div_up(n_mp, kBlock));
    hipLaunchKernelGGL(k_obs_fill, by_row, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_obs_fill");
    if (n_kf > 0) {
        hipLaunchKernelGGL(k_obs_count, dim3((unsigned)(nk * (size_t)A.per_slot)), block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_obs_count");
    }
    if (first_slot || last_slot) {
        hipLaunchKernelGGL(k_obs_finish, by_row, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_obs_finish");
    }
    MS_HIP(c, hipStreamSynchronize(c->stream));
    return MS_OK;
}

extern "C" int ms_map_cull(ms_ctx *c, int32_t *kf_mp, int n_kf, int stride, uint8_t *mp_flags, uint8_t *mp_live, int n_mp, const int32_t *kf_id, const double *kf_t,
                           const int32_t *cand, const uint8_t *cand_keep, int n_cand, const ms_cull_settings *s, int32_t *n_obs, int32_t *removed_rows, uint8_t *removed_why,
                           uint8_t *cand_removed, int32_t *n_removed_rows, int32_t *n_removed_kf) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_map_cull_check(kf_mp, n_kf, stride, mp_flags, mp_live, n_mp, kf_id, kf_t, cand, cand_keep, n_cand, s, removed_rows, cand_removed, n_removed_rows, n_removed_kf,
                                c->err, sizeof(c->err))))
        return rc;
    if (ms_map_over_capacity(n_kf, stride, n_mp, n_cand))
        return ms_fail(c, MS_ERR_CAPACITY, "map cull: %d slots / stride %d / %d map points / %d candidates, caps %d / %d / below %d / %d", n_kf, stride, n_mp, n_cand,
                       MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, MS_COVIS_MAX_QUERIES);
    if (n_mp == 0) {                                         // no entry can be valid: nMapPoints = 0 everywhere, and 0 < 0 * ratio never holds
        if (n_cand) std::memset(cand_removed, 0, (size_t)n_cand);
        *n_removed_rows = 0; *n_removed_kf = 0;
        return MS_OK;
    }
    MsRange range("mapCull");
    const std::vector<int32_t> &order = ms_slots_by_id();    // the slots in KfId order, left by the validation
    const size_t nk = (size_t)n_kf, nm = (size_t)n_mp, nc = (size_t)n_cand, n_blk = (nm + kBlock - 1) / kBlock;
    // upload block: slot -> position in KfId order | position -> slot | kf_t | the walk; then (host only) the results
    MsLayout up;
    const auto l_sr = up.array<int32_t>(nk), l_rs = up.array<int32_t>(order.size());
    const auto l_t = up.array<double>(nk);
    const auto l_walk = up.array<int2>(nc);
    MsLayout host = up, dev = up;
    const auto l_down = host.array<int32_t>(2 + nc);
    // device-only block: results | first / last positions | marks | block counts | block offsets | the counts when the caller does not want them
    const auto l_res = dev.array<int32_t>(2 + nc);
    const auto l_first = dev.array<int32_t>(nm), l_last = dev.array<int32_t>(nm);
    const auto l_cur = dev.array<uint8_t>(nm), l_w1 = dev.array<uint8_t>(nm), l_w3 = dev.array<uint8_t>(nm);
    const auto l_bc = dev.array<int32_t>(n_blk), l_bo = dev.array<int32_t>(n_blk);
    const auto l_n = dev.array<int32_t>(n_obs ? 0 : nm);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_MAP_CULL];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    ms_fill_ranks(order, n_kf, l_sr.at(hs), l_rs.at(hs));
    l_t.fill(hs, kf_t);
    // :445: descending KfId; :453-464: the kept ones never reach the device
    int2 *walk = l_walk.at(hs);
    int n_walk = 0;
    for (int i = 0; i < n_cand; ++i)
        if (!cand_keep || !cand_keep[i]) walk[n_walk++] = make_int2(cand[i], i);
    std::sort(walk, walk + n_walk, [&](const int2 &a, const int2 &b) { return kf_id[a.x] > kf_id[b.x]; });
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    CullArgs A{};
    A.kf_mp = kf_mp; A.mp_flags = mp_flags; A.mp_live = mp_live;
    A.slot_rank = l_sr.at(ds); A.rank_slot = l_rs.at(ds); A.kf_t = l_t.at(ds); A.walk = l_walk.at(ds);
    A.n_obs = n_obs ? n_obs : l_n.at(ds);
    A.first = l_first.at(ds); A.last = l_last.at(ds);
    A.in_cur = l_cur.at(ds); A.why1 = l_w1.at(ds); A.why3 = l_w3.at(ds);
    A.blk_count = l_bc.at(ds); A.blk_off = l_bo.at(ds);
    A.removed_rows = removed_rows; A.removed_why = removed_why;
    A.down = l_res.at(ds);
    A.min_age = s->min_age; A.ratio = s->max_critical_ratio;
    A.n_kf = n_kf; A.stride = stride; A.n_mp = n_mp; A.n_blk = (int32_t)n_blk; A.per_slot = ms_div_up(stride, kBlock);
    A.n_walk = n_walk; A.n_down = 2 + n_cand; A.current_slot = s->current_slot; A.min_obs = s->min_obs_for_ba; A.ratio_f32 = s->ratio_float32 != 0;
    const dim3 block(kBlock), by_row((unsigned)n_blk), by_entry((unsigned)(nk * (size_t)A.per_slot));
    hipLaunchKernelGGL(k_obs_fill, dim3((unsigned)std::max(n_blk, (2 + nc + kBlock - 1) / kBlock)), block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_obs_fill");
    hipLaunchKernelGGL(k_obs_count, by_entry, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_obs_count");
    if (s->cull_points) {
        hipLaunchKernelGGL(k_cull_points, by_row, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_cull_points");
    }
    hipLaunchKernelGGL(k_cull_keyframes, dim3(1), dim3(kWalk), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_cull_keyframes");
    hipLaunchKernelGGL(k_cull_sweep, by_entry, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_cull_sweep");
    hipLaunchKernelGGL(k_cull_count, by_row, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_cull_count");
    hipLaunchKernelGGL(k_cull_offsets, dim3(1), block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_cull_offsets");
    hipLaunchKernelGGL(k_cull_pack, by_row, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_cull_pack");
    MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_res.at(ds), l_res.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *down = l_down.at(hs);
    *n_removed_rows = down[0]; *n_removed_kf = down[1];
    for (int i = 0; i < n_cand; ++i) cand_removed[i] = (uint8_t)down[2 + i];
    return MS_OK;
}
