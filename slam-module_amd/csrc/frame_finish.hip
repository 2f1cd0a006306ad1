// frame_finish.hip -- the end of a frame on the device map tables: what the mapper does with every frame behind the pose adjustment.
//   setPointCloudOutput   mapper_helpers.cpp:484-497 (called at :1219-1221)   the frame's result point cloud
//   removeKeyframe        :375-431 (called at :1223-1226 and :1172-1183)      the table part: the slot's entries, orphaned map points
//
// ms_frame_finish, at most six launches whatever the sizes, one with n_remove == 0:
//   k_finish_cloud    ONE workgroup walks the slot's keypoints in trips of 256 and compacts the PRESENT and TRIANGULATED ones in keypoint order through the
//                     shared block rank, the count carried across trips (the gather of pose_tables.hip); it writes the block that goes down.  Launched
//                     first: it sees the tables before the removal
//   k_finish_fill     mark = none, remain = 0 (and the two removal counts)
//   k_finish_mark     one lane per entry of the whole table.  An entry of a removed slot: atomicMin(mark[r], its position in list order), the first claim;
//                     an entry of a remaining slot: atomicAdd(remain[r], 1).  Slots with kf_id < 0 are skipped.  The host uploads per slot its
//                     position in the list, kRemains or kEmpty
//   k_finish_count    one lane per entry of the removed slots: the first claimer of a live row nobody else lists is its owner; owners per workgroup
//   k_finish_offsets  ONE workgroup: block_offsets over those counts, the total to the head
//   k_finish_apply    as k_finish_count; returns at once when the total exceeds cap_removed (every verdict before any write).  The owner writes mp_live,
//                     mp_flags and removed_rows[offset + rank]; the first claimer writes n_obs; every lane clears its own entry
// Every position is decided by integer arithmetic and the atomics are integer min / add: nothing depends on which lane arrives first.  An entry r is
// used only after (uint32)r < n_mp held.
#include "ms_internal.h"
#include "ms_scan.h"
#include <algorithm>
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int32_t kRemains = -1, kEmpty = -2;                // slot_pos of a slot that is not in the list
constexpr int kHeadCloud = 0, kHeadRemoved = 1, kHeadErased = 2, kHeadInts = 4;

struct FinishArgs {
    int32_t *kf_mp;
    uint8_t *mp_flags, *mp_live;
    const double *mp_pos;
    const int32_t *mp_track;
    int32_t *n_obs;
    const int32_t *slot_pos;             // [n_kf]: position in remove_slots | kRemains | kEmpty
    const int32_t *list;                 // [n_remove]
    int32_t *mark, *remain;              // [n_mp]: the first claim's position (list index * stride + keypoint) | entries of remaining slots
    int32_t *blk_count, *blk_off;        // [n_remove * per_slot]
    int32_t *head;                       // [kHeadInts], the start of the block that goes down
    int32_t *cloud_row, *cloud_kp, *cloud_track;
    double *cloud_pos;
    int32_t *removed_rows;
    int32_t n_kf, stride, n_mp, per_slot, n_blk, cloud_slot, n_kp, cap_removed;
};

__global__ __launch_bounds__(kBlock) void k_finish_cloud(const FinishArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int tid = (int)threadIdx.x;
    const size_t row0 = (size_t)A.cloud_slot * A.stride;
    int n = 0;                                               // kept so far: the carry into the next trip
    for (int j0 = 0; j0 < A.n_kp; j0 += kBlock) {
        const int j = j0 + tid;
        int32_t r = -1;
        bool kept = false;
        if (j < A.n_kp) {
            r = A.kf_mp[row0 + j];
            kept = (uint32_t)r < (uint32_t)A.n_mp && (!A.mp_live || A.mp_live[r] != 0) && (A.mp_flags[r] & 1) != 0;      // :486-488
        }
        int total;
        const int k = n + block_rank<kBlock>(kept, s_wave, total);      // k < n_kp: a prefix count of keypoints
        if (kept) {
            A.cloud_row[k] = r;
            A.cloud_kp[k] = j;
            A.cloud_track[k] = A.mp_track ? A.mp_track[r] : -1;
            for (int a = 0; a < 3; ++a) A.cloud_pos[3 * (size_t)k + a] = A.mp_pos[3 * (size_t)r + a];
        }
        n += total;
        __syncthreads();                                     // s_wave is written again by the next trip
    }
    if (tid == 0) A.head[kHeadCloud] = n;
}

__global__ __launch_bounds__(kBlock) void k_finish_fill(const FinishArgs A) {
    const int r = blockIdx.x * kBlock + (int)threadIdx.x;
    if (r < A.n_mp) { A.mark[r] = kNone; A.remain[r] = 0; }
    if (r == 0) { A.head[kHeadRemoved] = 0; A.head[kHeadErased] = 0; }
}

__global__ __launch_bounds__(kBlock) void k_finish_mark(const FinishArgs A) {
    const int slot = blockIdx.x / A.per_slot, j = (blockIdx.x % A.per_slot) * kBlock + (int)threadIdx.x;
    const int32_t pos = A.slot_pos[slot];
    if (pos == kEmpty) return;                               // a stale entry is no observation
    uint32_t r = 0xffffffffu;
    if (j < A.stride) r = (uint32_t)A.kf_mp[(size_t)slot * A.stride + j];
    const bool valid = r < (uint32_t)A.n_mp;
    if (pos == kRemains) {
        if (valid) atomicAdd(A.remain + r, 1);
        return;
    }
    if (valid) atomicMin(A.mark + r, pos * A.stride + j);    // below MS_COVIS_MAX_QUERIES * MS_COVIS_MAX_STRIDE = 2^25
    const int n = __popcll(__ballot(valid));                 // the wave's erased entries
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(A.head + kHeadErased, n);
}

// The lane's entry of a removed slot: its address, its row, whether it is the row's first claim, and whether that row is orphaned; the lane's
// rank among the workgroup's orphans in claim order and their number.  Every lane of the workgroup calls it.
struct Entry {
    int32_t *at;
    uint32_t r;
    bool first, orphan;
};
__device__ inline int finish_rank(const FinishArgs &A, int32_t *s_wave, Entry &e, int &total) {
    const int i = blockIdx.x / A.per_slot, j = (blockIdx.x % A.per_slot) * kBlock + (int)threadIdx.x;
    e.at = nullptr; e.r = 0xffffffffu; e.first = e.orphan = false;
    if (j < A.stride) {
        e.at = A.kf_mp + (size_t)A.list[i] * A.stride + j;
        e.r = (uint32_t)*e.at;
        if (e.r < (uint32_t)A.n_mp) {
            e.first = A.mark[e.r] == i * A.stride + j;
            e.orphan = e.first && A.mp_live[e.r] != 0 && A.remain[e.r] == 0;      // :397-401; a row that is not live is never reported
        }
    }
    return block_rank<kBlock>(e.orphan, s_wave, total);
}

__global__ __launch_bounds__(kBlock) void k_finish_count(const FinishArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    Entry e;
    int total;
    finish_rank(A, s_wave, e, total);
    if (threadIdx.x == 0) A.blk_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_finish_offsets(const FinishArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int removed = block_offsets<kBlock>(A.blk_count, A.blk_off, A.n_blk, s_wave);
    if (threadIdx.x == 0) A.head[kHeadRemoved] = removed;
}

__global__ __launch_bounds__(kBlock) void k_finish_apply(const FinishArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    if (A.head[kHeadRemoved] > A.cap_removed) return;        // the same answer in every lane of the grid: nothing is written
    Entry e;
    int total;
    const int rank = finish_rank(A, s_wave, e, total);
    if (!e.at) return;
    if (e.orphan) {                                          // MapDB::removeMapPoint; only this lane read mp_live[r]
        A.removed_rows[(size_t)A.blk_off[blockIdx.x] + (size_t)rank] = (int32_t)e.r;      // below the total, which is at most cap_removed
        A.mp_live[e.r] = 0;
        A.mp_flags[e.r] = 0;
    }
    if (e.first && A.n_obs) A.n_obs[e.r] = A.remain[e.r];
    *e.at = -1;                                              // eraseObservation, and the slot is empty afterwards
}

}  // namespace

extern "C" int ms_frame_finish(ms_ctx *c, int32_t *kf_mp, int n_kf, int stride, uint8_t *mp_flags, uint8_t *mp_live, const double *mp_pos, const int32_t *mp_track,
                               int32_t *n_obs, int n_mp, const int32_t *kf_id, const int32_t *remove_slots, int n_remove, const ms_frame_finish_args *args,
                               int32_t *cloud_row, int32_t *cloud_kp, int32_t *cloud_track, double *cloud_pos, int32_t *removed_rows, int cap_removed, int32_t *counts) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_frame_finish_validate(kf_mp, n_kf, stride, mp_flags, mp_live, mp_pos, mp_track, n_obs, n_mp, kf_id, remove_slots, n_remove, args, cloud_row, cloud_kp,
                                       cloud_track, cloud_pos, removed_rows, cap_removed, counts, c->err, sizeof(c->err))))
        return rc;
    counts[0] = counts[1] = counts[2] = 0;
    const bool want_cloud = args->cloud_slot >= 0;
    if (!want_cloud && n_remove == 0) return MS_OK;
    MsRange range("frameFinish");
    const size_t nk = (size_t)n_kf, nm = (size_t)n_mp, nr = (size_t)n_remove, n_kp = want_cloud ? (size_t)args->n_kp : 0;
    const int per_slot = ms_div_up(stride, kBlock);
    const size_t n_blk = nr * (size_t)per_slot;
    // no more rows can be removed than the removed slots have entries, or the table has rows
    const size_t cap = std::min((size_t)cap_removed, std::min(nm, nr * (size_t)stride));
    // upload block (n_remove > 0): per slot its position in the list | the list
    MsLayout up;
    const auto l_pos = up.array<int32_t>(n_remove ? nk : 0), l_list = up.array<int32_t>(nr);
    MsLayout dev = up;
    // device-only block: first claims | entries of remaining slots | owners per workgroup | their offsets; then the block that goes down
    const auto l_mark = dev.array<int32_t>(n_remove ? nm : 0), l_remain = dev.array<int32_t>(n_remove ? nm : 0);
    const auto l_bc = dev.array<int32_t>(n_blk), l_bo = dev.array<int32_t>(n_blk);
    // the block that goes down: head | cloud rows | keypoints | tracks | positions | removed rows
    MsLayout down;
    const auto l_head = down.array<int32_t>(kHeadInts);
    const auto l_crow = down.array<int32_t>(n_kp), l_ckp = down.array<int32_t>(n_kp), l_ctrack = down.array<int32_t>(n_kp);
    const auto l_cpos = down.array<double>(3 * n_kp);
    const auto l_rows = down.array<int32_t>(cap);
    const size_t down_at = dev.take(down.end);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_FRAME_FINISH];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    if ((rc = ms_pinned(c, down.end))) return rc;
    void *hs = W.host, *ds = W.dev, *dd = ms_at<uint8_t>(W.dev, down_at);
    FinishArgs A{};
    A.kf_mp = kf_mp; A.mp_flags = mp_flags; A.mp_live = mp_live; A.mp_pos = mp_pos; A.mp_track = mp_track; A.n_obs = n_obs;
    A.slot_pos = l_pos.at(ds); A.list = l_list.at(ds); A.mark = l_mark.at(ds); A.remain = l_remain.at(ds); A.blk_count = l_bc.at(ds); A.blk_off = l_bo.at(ds);
    A.head = l_head.at(dd); A.cloud_row = l_crow.at(dd); A.cloud_kp = l_ckp.at(dd); A.cloud_track = l_ctrack.at(dd); A.cloud_pos = l_cpos.at(dd);
    A.removed_rows = l_rows.at(dd);
    A.n_kf = n_kf; A.stride = stride; A.n_mp = n_mp; A.per_slot = per_slot; A.n_blk = (int32_t)n_blk; A.cloud_slot = args->cloud_slot; A.n_kp = (int32_t)n_kp;
    A.cap_removed = cap_removed;
    const dim3 block(kBlock);
    if (want_cloud) {
        hipLaunchKernelGGL(k_finish_cloud, dim3(1), block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_finish_cloud");
    }
    if (n_remove > 0) {
        int32_t *pos = l_pos.at(hs);
        for (int k = 0; k < n_kf; ++k) pos[k] = kf_id[k] >= 0 ? kRemains : kEmpty;
        for (int i = 0; i < n_remove; ++i) pos[remove_slots[i]] = i;
        l_list.fill(hs, remove_slots);
        MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
        const dim3 by_row((unsigned)std::max<size_t>((nm + kBlock - 1) / kBlock, 1)), by_entry((unsigned)(nk * (size_t)per_slot)), by_removed((unsigned)n_blk);
        hipLaunchKernelGGL(k_finish_fill, by_row, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_finish_fill");
        hipLaunchKernelGGL(k_finish_mark, by_entry, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_finish_mark");
        hipLaunchKernelGGL(k_finish_count, by_removed, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_finish_count");
        hipLaunchKernelGGL(k_finish_offsets, dim3(1), block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_finish_offsets");
        hipLaunchKernelGGL(k_finish_apply, by_removed, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_finish_apply");
    }
    MS_HIP(c, hipMemcpyAsync(c->pinned, dd, down.end, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    void *ps = c->pinned;
    const int32_t *head = l_head.at(ps);
    const int n_cloud = want_cloud ? head[kHeadCloud] : 0, n_removed = n_remove ? head[kHeadRemoved] : 0;
    counts[0] = n_cloud; counts[1] = n_removed; counts[2] = n_remove ? head[kHeadErased] : 0;
    if (cloud_row) l_crow.get(ps, 0, cloud_row, (size_t)n_cloud);
    if (cloud_kp) l_ckp.get(ps, 0, cloud_kp, (size_t)n_cloud);
    if (cloud_track) l_ctrack.get(ps, 0, cloud_track, (size_t)n_cloud);
    if (cloud_pos) l_cpos.get(ps, 0, cloud_pos, 3 * (size_t)n_cloud);
    if (n_removed > cap_removed)
        return ms_fail(c, MS_ERR_CAPACITY, "frame finish: %d map points are removed, removed_rows holds %d (the tables are untouched)", n_removed, cap_removed);
    l_rows.get(ps, 0, removed_rows, (size_t)n_removed);
    return MS_OK;
}
