// obs_lists.hip -- ms_observation_lists: the transpose of the keyframe table kf_mp (slot -> map-point rows) for chosen rows, as CSR lists on
// the device.  A row's list is the reference's `std::map<KfId, KpId> observations` (map_point.hpp): the observing keyframes in
// ascending KfId order, with the keypoint's pixel, octave, depth and descriptor index gathered next to it, where ms_map_refresh_lists and
// ms_triangulate_lists read them.  An entry r of kf_mp or rows_in is used only after (uint32)r < n_mp held.
//
// Ten launches whatever the sizes:
//   k_ol_fill      n_obs = 0, first selecting position = none, output index = none; the result block = 0
//   k_ol_count     one lane per entry of every slot with kf_id >= 0: atomicAdd(n_obs[r]) -- the count kernel of map_cull.hip
//   k_ol_mark      one lane per position of the selection (rows_in[i], or keypoint i of the slot): atomicMin(sel[r], i), so a row is kept
//                  at its first occurrence whatever lane arrives first
//   k_ol_blocks / k_ol_offsets / k_ol_pack   block_rank, per-workgroup count and block_offsets (ms_scan.h) over 256 positions
//                  per block, with a second column through block_exclusive: the sum of the kept rows' list lengths, whose exclusive scan
//                  is obs_start.  k_ol_offsets scans the two columns of block totals one after the other
//   k_ol_scatter   one lane per entry: the entry's (KfId position, j) key goes behind an atomic cursor into its row's segment
//   k_ol_sort_short  a wave per kept row: segments of up to 64 keys are ranked inside the wave
//   k_ol_sort_long   the longer ones (listed by k_ol_pack) a workgroup each: up to kLds keys are ranked through LDS, beyond that from global
//                  memory (correct up to n_kf * stride keys, quadratic in the length).  Keys are distinct, so the rank of a key is its place
//   k_ol_gather    one lane per observation: key -> slot, j and the keypoint table's entries; one lane per row: first_octave
// The cursor decides only where a key waits for the sort; the sorted segment does not depend on it: the same input gives the same bits on
// every call and at any capacity.  Integer atomics only.  When the kept rows or their observations exceed the capacities, the totals are
// still computed and nothing behind the block scan writes.
#include "ms_internal.h"
#include "ms_scan.h"
#include <algorithm>
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int kLds = 1024;                                   // keys a workgroup ranks through LDS
constexpr int kLongGrid = 1024;                              // workgroups of k_ol_sort_long (they stride over the long rows)
constexpr int kJBits = 13;                                   // key = position in KfId order << kJBits | j
static_assert(MS_COVIS_MAX_STRIDE <= (1 << kJBits) && MS_COVIS_MAX_KF <= (1 << (31 - kJBits)), "the sort key is one int32");
constexpr int kMaxIn = 1 << 24;                              // entries of rows_in

struct ListArgs {
    const int32_t *kf_mp;
    const uint8_t *mp_flags;
    const float *kp_x, *kp_y, *kp_depth;
    const int32_t *kp_octave;
    const int32_t *slot_rank, *rank_slot, *desc_base;        // [n_kf], [slots with kf_id >= 0], [n_kf]
    const int32_t *rows_in;
    ms_obs_lists out;
    int32_t *n_obs, *sel, *dst_of;                           // [n_mp]: list length | first selecting position | index among the kept rows
    int32_t *blk_rows, *blk_obs, *off_rows, *off_obs;        // [n_blk]
    int32_t *cursor, *long_list;                             // [kept rows at most]
    int32_t *key, *sorted;                                   // [observations at most]
    int32_t *down;                                           // n_rows, n_obs, octave violations, rows of long_list
    int32_t n_kf, stride, n_mp, per_slot, n_pos, n_blk, slot, filter, drop_empty, n_levels, cap_rows, cap_obs;
};

__device__ __forceinline__ bool over(const ListArgs &A) { return A.down[0] > A.cap_rows || A.down[1] > A.cap_obs; }

__global__ __launch_bounds__(kBlock) void k_ol_fill(const ListArgs A) {
    const int r = blockIdx.x * kBlock + (int)threadIdx.x;
    if (r < A.n_mp) { A.n_obs[r] = 0; A.sel[r] = kNone; A.dst_of[r] = -1; }
    if (r < 4) A.down[r] = 0;
}

__global__ __launch_bounds__(kBlock) void k_ol_count(const ListArgs A) {
    const int slot = blockIdx.x / A.per_slot, j = (blockIdx.x % A.per_slot) * kBlock + (int)threadIdx.x;
    if (j >= A.stride || A.slot_rank[slot] < 0) return;
    const uint32_t r = (uint32_t)A.kf_mp[(size_t)slot * A.stride + j];
    if (r < (uint32_t)A.n_mp) atomicAdd(A.n_obs + r, 1);
}

// the row at position i of the selection (any int32: the caller compares it)
__device__ __forceinline__ uint32_t selected(const ListArgs &A, int i) {
    return (uint32_t)(A.slot >= 0 ? A.kf_mp[(size_t)A.slot * A.stride + i] : A.rows_in[i]);
}

__global__ __launch_bounds__(kBlock) void k_ol_mark(const ListArgs A) {
    const int i = blockIdx.x * kBlock + (int)threadIdx.x;
    if (i >= A.n_pos) return;
    const uint32_t r = selected(A, i);
    if (r < (uint32_t)A.n_mp) atomicMin(A.sel + r, i);
}

// Position i = this lane's: is its row kept, which row, how long is its list; then its rank among the workgroup's kept rows and the
// observations of the kept rows before it, in position order; the workgroup's totals through total_rows / total_obs.
__device__ inline bool list_rank(const ListArgs &A, int32_t (*s_wave)[kBlock / 64], uint32_t &r, int &n, int &rank, int &obs_before, int &total_rows, int &total_obs) {
    const int i = blockIdx.x * kBlock + (int)threadIdx.x;
    bool kept = false;
    r = 0; n = 0;
    if (i < A.n_pos) {
        r = selected(A, i);
        if (r < (uint32_t)A.n_mp && A.sel[r] == i) {
            n = A.n_obs[r];
            kept = true;
            if (A.filter == MS_OBS_REFRESH) kept = (A.mp_flags[r] & 2) != 0;                     // mapper_helpers.cpp:1066
            else if (A.filter == MS_OBS_RETRIANGULATE) kept = (A.mp_flags[r] & 1) == 0 || n >= 2;      // :1088
            if (A.drop_empty && n == 0) kept = false;
        }
    }
    rank = block_rank<kBlock>(kept, s_wave[0], total_rows);                    // an LDS array each: no barrier separates the two
    obs_before = block_exclusive<kBlock>(kept ? n : 0, s_wave[1], total_obs);
    return kept;
}

__global__ __launch_bounds__(kBlock) void k_ol_blocks(const ListArgs A) {
    __shared__ int32_t s_wave[2][kBlock / 64];
    uint32_t r;
    int n, rank, before, total_rows, total_obs;
    list_rank(A, s_wave, r, n, rank, before, total_rows, total_obs);
    if (threadIdx.x == 0) { A.blk_rows[blockIdx.x] = total_rows; A.blk_obs[blockIdx.x] = total_obs; }
}

__global__ __launch_bounds__(kBlock) void k_ol_offsets(const ListArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int carry_rows = block_offsets<kBlock>(A.blk_rows, A.off_rows, A.n_blk, s_wave);
    const int carry_obs = block_offsets<kBlock>(A.blk_obs, A.off_obs, A.n_blk, s_wave);
    if (threadIdx.x == 0) {
        A.down[0] = carry_rows; A.down[1] = carry_obs;
        if (carry_rows <= A.cap_rows && carry_obs <= A.cap_obs) A.out.obs_start[carry_rows] = carry_obs;      // obs_start holds cap_rows + 1
    }
}

__global__ __launch_bounds__(kBlock) void k_ol_pack(const ListArgs A) {
    __shared__ int32_t s_wave[2][kBlock / 64];
    uint32_t r;
    int n, rank, before, total_rows, total_obs;
    const bool kept = list_rank(A, s_wave, r, n, rank, before, total_rows, total_obs);
    if (!kept || over(A)) return;
    const int d = A.off_rows[blockIdx.x] + rank;             // below down[0] <= cap_rows
    A.out.rows[d] = (int32_t)r;
    A.out.obs_start[d] = A.off_obs[blockIdx.x] + before;
    if (A.out.n_obs_row) A.out.n_obs_row[d] = n;
    if (A.out.was_triangulated) A.out.was_triangulated[d] = (A.mp_flags[r] & 2) != 0;             // :607
    A.dst_of[r] = d;
    A.cursor[d] = 0;
    if (n > 64) A.long_list[atomicAdd(A.down + 3, 1)] = d;   // in any order: each segment is sorted on its own
}

__global__ __launch_bounds__(kBlock) void k_ol_scatter(const ListArgs A) {
    const int slot = blockIdx.x / A.per_slot, j = (blockIdx.x % A.per_slot) * kBlock + (int)threadIdx.x;
    if (j >= A.stride || over(A)) return;
    const int rank = A.slot_rank[slot];
    if (rank < 0) return;
    const uint32_t r = (uint32_t)A.kf_mp[(size_t)slot * A.stride + j];
    if (r >= (uint32_t)A.n_mp) return;
    const int d = A.dst_of[r];
    if (d < 0) return;
    const int p = atomicAdd(A.cursor + d, 1);
    const int at = A.out.obs_start[d] + p;
    if (p < A.n_obs[r] && at < A.cap_obs) A.key[at] = rank << kJBits | j;        // both hold while the table is the one k_ol_count read
}

__global__ __launch_bounds__(kBlock) void k_ol_sort_short(const ListArgs A) {
    const int d = blockIdx.x * (kBlock / 64) + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (over(A) || d >= A.down[0]) return;                   // whole waves leave
    const int s = A.out.obs_start[d], n = A.out.obs_start[d + 1] - s;
    if (n > 64) return;
    const int32_t k = lane < n ? A.key[s + lane] : kNone;
    int rank = 0;
    for (int i = 0; i < n; ++i) rank += __shfl(k, i) < k;
    if (lane < n) A.sorted[s + rank] = k;
}

__global__ __launch_bounds__(kBlock) void k_ol_sort_long(const ListArgs A) {
    __shared__ int32_t s_key[kLds];
    if (over(A)) return;
    const int n_long = A.down[3];
    for (int i = blockIdx.x; i < n_long; i += gridDim.x) {
        const int d = A.long_list[i];
        const int s = A.out.obs_start[d], n = A.out.obs_start[d + 1] - s;
        const int32_t *src = A.key + s;
        if (n <= kLds) {
            for (int e = threadIdx.x; e < n; e += kBlock) s_key[e] = src[e];
            __syncthreads();
            for (int e = threadIdx.x; e < n; e += kBlock) {
                const int32_t k = s_key[e];
                int rank = 0;
                for (int x = 0; x < n; ++x) rank += s_key[x] < k;
                A.sorted[s + rank] = k;
            }
            __syncthreads();                                 // the next row overwrites s_key
        } else {
            for (int e = threadIdx.x; e < n; e += kBlock) {
                const int32_t k = src[e];
                int rank = 0;
                for (int x = 0; x < n; ++x) rank += src[x] < k;
                A.sorted[s + rank] = k;
            }
        }
    }
}

// the octave of the keypoint at entry e of the table, inside [0, n_levels) when levels are given
__device__ __forceinline__ int32_t octave_at(const ListArgs &A, size_t e, bool count) {
    int32_t v = A.kp_octave[e];
    if (A.n_levels > 0 && (uint32_t)v >= (uint32_t)A.n_levels) {
        if (count) atomicAdd(A.down + 2, 1);
        v = v < 0 ? 0 : A.n_levels - 1;
    }
    return v;
}

__global__ __launch_bounds__(kBlock) void k_ol_gather(const ListArgs A) {
    const int o = blockIdx.x * kBlock + (int)threadIdx.x;
    if (over(A)) return;
    if (o < A.down[1]) {
        const int32_t k = A.sorted[o];
        const int slot = A.rank_slot[k >> kJBits], j = k & ((1 << kJBits) - 1);
        const size_t e = (size_t)slot * A.stride + j;
        if (A.out.obs_kf) A.out.obs_kf[o] = slot;
        if (A.out.obs_kp) A.out.obs_kp[o] = j;
        if (A.out.obs_x) A.out.obs_x[o] = A.kp_x[e];
        if (A.out.obs_y) A.out.obs_y[o] = A.kp_y[e];
        if (A.out.obs_octave) A.out.obs_octave[o] = octave_at(A, e, true);
        if (A.out.obs_depth) A.out.obs_depth[o] = A.kp_depth[e];
        if (A.out.obs_desc) { const int32_t base = A.desc_base[slot]; A.out.obs_desc[o] = base < 0 ? -1 : base + j; }
    }
    if (o < A.down[0] && A.out.first_octave) {
        const int s = A.out.obs_start[o];
        int32_t v = 0;
        if (A.out.obs_start[o + 1] > s) {
            const int32_t k = A.sorted[s];
            v = octave_at(A, (size_t)A.rank_slot[k >> kJBits] * A.stride + (k & ((1 << kJBits) - 1)), false);       // counted as an observation above, or not at all
        }
        A.out.first_octave[o] = v;
    }
}

}  // namespace

extern "C" int ms_observation_lists(ms_ctx *c, const int32_t *kf_mp, int n_kf, int stride, int n_mp, const int32_t *kf_id, const uint8_t *mp_flags, const float *kp_x,
                                    const float *kp_y, const int32_t *kp_octave, const float *kp_depth, const int32_t *kf_desc_base, const ms_obs_select *sel, int n_levels,
                                    const ms_obs_lists *out, int cap_rows, int cap_obs, int32_t *n_rows, int32_t *n_obs) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_observation_lists_check(kf_mp, n_kf, stride, n_mp, kf_id, mp_flags, kp_x, kp_y, kp_octave, kp_depth, kf_desc_base, sel, n_levels, out, cap_rows, cap_obs,
                                         n_rows, n_obs, c->err, sizeof(c->err))))
        return rc;
    const std::vector<int32_t> &order = ms_slots_by_id();    // the slots in KfId order, left by the validation
    const bool from_slot = sel->source == MS_OBS_FROM_SLOT;
    if (ms_map_over_capacity(n_kf, stride, n_mp, 0) || sel->n_in > kMaxIn)
        return ms_fail(c, MS_ERR_CAPACITY, "observation lists: %d slots / stride %d / %d map points / %d rows_in, caps %d / %d / below %d / %d", n_kf, stride, n_mp,
                       sel->n_in, MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, kMaxIn);
    const int n_pos = from_slot ? stride : sel->n_in;
    *n_rows = 0; *n_obs = 0;
    if (n_mp == 0 || n_pos == 0) {                           // no position can name a row: obs_start = {0}
        MS_HIP(c, hipSetDevice(c->device));
        MS_HIP(c, hipMemsetAsync(out->obs_start, 0, sizeof(int32_t), c->stream));
        MS_HIP(c, hipStreamSynchronize(c->stream));
        return MS_OK;
    }
    MsRange range("observationLists");
    const size_t nk = (size_t)n_kf, nm = (size_t)n_mp, n_blk = ((size_t)n_pos + kBlock - 1) / kBlock;
    const size_t max_rows = std::min((size_t)cap_rows, (size_t)n_pos), max_obs = std::min((size_t)cap_obs, nk * (size_t)stride);
    // upload block: slot -> position in KfId order | position -> slot | descriptor bases; then (host only) the result block
    MsLayout up;
    const auto l_sr = up.array<int32_t>(nk), l_rs = up.array<int32_t>(order.size()), l_base = up.array<int32_t>(kf_desc_base ? nk : 0);
    MsLayout host = up, dev = up;
    const auto l_down = host.array<int32_t>(4);
    // device-only block: results | lengths | selecting positions | output indices | block counts and offsets | cursors | long rows | keys, sorted keys
    const auto l_res = dev.array<int32_t>(4);
    const auto l_n = dev.array<int32_t>(nm), l_sel = dev.array<int32_t>(nm), l_dst = dev.array<int32_t>(nm);
    const auto l_br = dev.array<int32_t>(n_blk), l_bo = dev.array<int32_t>(n_blk), l_or = dev.array<int32_t>(n_blk), l_oo = dev.array<int32_t>(n_blk);
    const auto l_cur = dev.array<int32_t>(max_rows), l_long = dev.array<int32_t>(max_rows);
    const auto l_key = dev.array<int32_t>(max_obs), l_sorted = dev.array<int32_t>(max_obs);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_OBS_LISTS];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    ms_fill_ranks(order, n_kf, l_sr.at(hs), l_rs.at(hs));
    l_base.fill(hs, kf_desc_base);
    if (up.end) MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    ListArgs A{};
    A.kf_mp = kf_mp; A.mp_flags = mp_flags;
    A.kp_x = kp_x; A.kp_y = kp_y; A.kp_depth = kp_depth; A.kp_octave = kp_octave;
    A.slot_rank = l_sr.at(ds); A.rank_slot = l_rs.at(ds); A.desc_base = l_base.at(ds);
    A.rows_in = sel->rows_in;
    A.out = *out;
    A.n_obs = l_n.at(ds); A.sel = l_sel.at(ds); A.dst_of = l_dst.at(ds);
    A.blk_rows = l_br.at(ds); A.blk_obs = l_bo.at(ds); A.off_rows = l_or.at(ds); A.off_obs = l_oo.at(ds);
    A.cursor = l_cur.at(ds); A.long_list = l_long.at(ds);
    A.key = l_key.at(ds); A.sorted = l_sorted.at(ds);
    A.down = l_res.at(ds);
    A.n_kf = n_kf; A.stride = stride; A.n_mp = n_mp; A.per_slot = ms_div_up(stride, kBlock); A.n_pos = n_pos; A.n_blk = (int32_t)n_blk;
    A.slot = from_slot ? sel->slot : -1; A.filter = sel->filter; A.drop_empty = sel->drop_empty != 0; A.n_levels = n_levels;
    A.cap_rows = (int32_t)max_rows; A.cap_obs = (int32_t)max_obs;        // never more rows than positions, nor more observations than entries
    const dim3 block(kBlock), by_row((unsigned)ms_div_up(n_mp, kBlock)), by_pos((unsigned)n_blk), by_entry((unsigned)(nk * (size_t)A.per_slot));
    hipLaunchKernelGGL(k_ol_fill, by_row, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_ol_fill");
    if (n_kf > 0) {
        hipLaunchKernelGGL(k_ol_count, by_entry, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_ol_count");
    }
    hipLaunchKernelGGL(k_ol_mark, by_pos, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_ol_mark");
    hipLaunchKernelGGL(k_ol_blocks, by_pos, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_ol_blocks");
    hipLaunchKernelGGL(k_ol_offsets, dim3(1), block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_ol_offsets");
    hipLaunchKernelGGL(k_ol_pack, by_pos, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_ol_pack");
    if (n_kf > 0 && max_rows > 0 && max_obs > 0) {
        hipLaunchKernelGGL(k_ol_scatter, by_entry, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_ol_scatter");
        hipLaunchKernelGGL(k_ol_sort_short, dim3((unsigned)((max_rows + kBlock / 64 - 1) / (kBlock / 64))), block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_ol_sort_short");
        hipLaunchKernelGGL(k_ol_sort_long, dim3((unsigned)std::min((size_t)kLongGrid, max_rows)), block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_ol_sort_long");
    }
    if (max_rows > 0) {
        hipLaunchKernelGGL(k_ol_gather, dim3((unsigned)((std::max(max_rows, max_obs) + kBlock - 1) / kBlock)), block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_ol_gather");
    }
    MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_res.at(ds), l_res.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *down = l_down.at(hs);
    *n_rows = down[0]; *n_obs = down[1];
    if (down[0] > cap_rows || down[1] > cap_obs)
        return ms_fail(c, MS_ERR_CAPACITY, "observation lists: %d rows / %d observations, the outputs hold %d / %d", down[0], down[1], cap_rows, cap_obs);
    if (down[2] > 0) return ms_fail(c, MS_ERR_INVALID, "observation lists: %d gathered octaves outside [0, %d) (stored clamped)", down[2], n_levels);
    return MS_OK;
}
