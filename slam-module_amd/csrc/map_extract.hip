// map_extract.hip -- the partial map copy for the front end on the device map tables: copyMap (mapper.cpp:281-326) with
// copyPartialMapToFrontend, that is MapDB(mapDB, activeKeyframes) (mapdb.cpp:116-159) and MapPoint(mp, activeKeyframes) (map_point.cpp:22-43).
// The active keyframes of a SOURCE set of tables go into a DESTINATION set, compacted and renumbered; the source is only read.
//
// ms_map_extract, at most NINE launches whatever the sizes (seven without tracks and pool), no host wait between them:
//   k_extract_fill     cnt = 0 per source row, the head = 0
//   k_extract_mark     one lane per entry of the ACTIVE slots (not of the whole table): atomicAdd(cnt[r], 1) for a present row; the wave's kept
//                      entries and its valid entries of rows that are not live go to the head
//   k_extract_count    one lane per source row: active = cnt > 0; active rows per workgroup (block_rank)
//   k_extract_offsets  ONE workgroup: block_offsets over those counts, the total (n_rows) to the head
//   k_extract_place    as k_extract_count: d = offset + rank is the destination row; row_dst[r] = d | -1, row_src[d] = r
//   k_extract_rows     one lane per destination row: the row fields; every field's stores run over consecutive destination words of a workgroup's
//                      256 rows (a row of 3 doubles is written by 3 lanes), the loads gather whole source rows; the tail rows' defaults
//   k_extract_slots    one lane per entry of the destination table: the renumbered entry and the keypoint, the pose; the empty slots' defaults
//   k_extract_tracks   one lane per track of the window
//   k_extract_pool     one lane per 16 bytes of the active slots' descriptors
// Every kernel from k_extract_place on returns at once when n_rows exceeds the destination's rows: every verdict before any write.  Every position
// is a prefix count and the one atomic is an integer add: nothing depends on which lane arrives first.  An entry r is used only after
// (uint32)r < n_mp held; a destination row d only below n_rows <= min(n_mp, dst n_mp).
#include "ms_internal.h"
#include "ms_scan.h"
#include <algorithm>

namespace {

constexpr int kBlock = 256;
constexpr int kHeadRows = 0, kHeadKept = 1, kHeadDropped = 2, kHeadTracks = 3, kHeadInts = 4;

struct ExtractArgs {
    ms_map_extract_src S;
    ms_map_extract_dst D;
    const int32_t *list, *n_kp, *pool_src, *pool_dst;      // [n_active]: source slots | descriptors | first descriptor in either pool (pool_src < 0: none)
    int32_t *cnt, *rdst;                                     // [n_mp]: entries of the active slots per source row | its destination row or -1
    int32_t *rsrc;                                           // [min(n_mp, dst n_mp)]: the source row of a destination row
    int32_t *blk_count, *blk_off;                            // [n_blk]
    int32_t *head;                                           // [kHeadInts], the block that goes down
    int32_t n_active, per_slot, per_pool, n_blk;
};

__device__ inline bool present(const ExtractArgs &A, uint32_t r) { return r < (uint32_t)A.S.n_mp && (!A.S.mp_live || A.S.mp_live[r] != 0); }

__global__ __launch_bounds__(kBlock) void k_extract_fill(const ExtractArgs A) {
    const int r = blockIdx.x * kBlock + (int)threadIdx.x;
    if (r < A.S.n_mp) A.cnt[r] = 0;
    if (r < kHeadInts) A.head[r] = 0;
}

__global__ __launch_bounds__(kBlock) void k_extract_mark(const ExtractArgs A) {
    const int i = blockIdx.x / A.per_slot, j = (blockIdx.x % A.per_slot) * kBlock + (int)threadIdx.x;
    uint32_t r = 0xffffffffu;
    if (j < A.S.stride) r = (uint32_t)A.S.kf_mp[(size_t)A.list[i] * A.S.stride + j];
    const bool valid = r < (uint32_t)A.S.n_mp, kept = present(A, r);
    if (kept) atomicAdd(A.cnt + r, 1);
    const int n_kept = __popcll(__ballot(kept)), n_dropped = __popcll(__ballot(valid && !kept));
    if ((threadIdx.x & 63) == 0) {
        if (n_kept) atomicAdd(A.head + kHeadKept, n_kept);
        if (n_dropped) atomicAdd(A.head + kHeadDropped, n_dropped);
    }
}

// the lane's source row, whether it is active, and its rank among the workgroup's active rows; every lane of the workgroup calls it
__device__ inline int extract_rank(const ExtractArgs &A, int32_t *s_wave, int &r, bool &active, int &total) {
    r = blockIdx.x * kBlock + (int)threadIdx.x;
    active = r < A.S.n_mp && A.cnt[r] > 0;
    return block_rank<kBlock>(active, s_wave, total);
}

__global__ __launch_bounds__(kBlock) void k_extract_count(const ExtractArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    int r, total;
    bool active;
    extract_rank(A, s_wave, r, active, total);
    if (threadIdx.x == 0) A.blk_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_extract_offsets(const ExtractArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int n_rows = block_offsets<kBlock>(A.blk_count, A.blk_off, A.n_blk, s_wave);
    if (threadIdx.x == 0) A.head[kHeadRows] = n_rows;
}

__global__ __launch_bounds__(kBlock) void k_extract_place(const ExtractArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    if (A.head[kHeadRows] > A.D.n_mp) return;                // the same answer in every lane of the grid: nothing is written
    int r, total;
    bool active;
    const int rank = extract_rank(A, s_wave, r, active, total);
    if (r >= A.S.n_mp) return;
    const int32_t d = active ? A.blk_off[blockIdx.x] + rank : -1;      // below n_rows
    A.rdst[r] = d;
    if (A.D.row_dst) A.D.row_dst[r] = d;
    if (active) {
        A.rsrc[d] = r;
        if (A.D.row_src) A.D.row_src[d] = r;
    }
}

// W words of T per row for the workgroup's n rows from destination row d0 on: lane after lane writes consecutive destination words
template <class T, int W>
__device__ inline void gather_field(T *dst, const T *src, const int32_t *rsrc, int d0, int n) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int e = k * kBlock + (int)threadIdx.x;
        if (e < n * W) dst[(size_t)d0 * W + e] = src[(size_t)rsrc[d0 + e / W] * W + e % W];
    }
}

__global__ __launch_bounds__(kBlock) void k_extract_rows(const ExtractArgs A) {
    const int n_rows = A.head[kHeadRows];
    if (n_rows > A.D.n_mp) return;
    const ms_map_extract_src &S = A.S;
    const ms_map_extract_dst &D = A.D;
    const int d0 = blockIdx.x * kBlock, d = d0 + (int)threadIdx.x;
    const int n = min(n_rows - d0, kBlock);                  // the workgroup's copied rows (<= 0: none)
    if (n > 0) {
        gather_field<double, 3>(D.mp_pos, S.mp_pos, A.rsrc, d0, n);
        gather_field<float, 3>(D.mp_norm, S.mp_norm, A.rsrc, d0, n);
        gather_field<uint4, 2>(reinterpret_cast<uint4 *>(D.mp_desc), reinterpret_cast<const uint4 *>(S.mp_desc), A.rsrc, d0, n);
    }
    if (d >= D.n_mp) return;
    if (d < n_rows) {
        const int32_t r = A.rsrc[d];
        D.mp_min_dist[d] = S.mp_min_dist[r];
        D.mp_max_dist[d] = S.mp_max_dist[r];
        D.mp_flags[d] = S.mp_flags[r];
        D.mp_live[d] = 1;
        if (D.mp_track) D.mp_track[d] = S.mp_track[r];
        if (D.n_obs) D.n_obs[d] = A.cnt[r];
    } else {
        D.mp_flags[d] = 0;
        D.mp_live[d] = 0;
        if (D.mp_track) D.mp_track[d] = -1;
        if (D.n_obs) D.n_obs[d] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void k_extract_slots(const ExtractArgs A) {
    if (A.head[kHeadRows] > A.D.n_mp) return;
    const ms_map_extract_src &S = A.S;
    const ms_map_extract_dst &D = A.D;
    const int i = blockIdx.x / A.per_slot, j = (blockIdx.x % A.per_slot) * kBlock + (int)threadIdx.x;      // i < D.n_kf
    const bool copied = i < A.n_active;
    const int32_t slot = copied ? A.list[i] : 0;
    if (copied && D.kf_pose && blockIdx.x % A.per_slot == 0 && threadIdx.x < 12) D.kf_pose[(size_t)i * 12 + threadIdx.x] = S.kf_pose[(size_t)slot * 12 + threadIdx.x];
    if (j >= S.stride) return;
    const size_t to = (size_t)i * S.stride + j, from = (size_t)slot * S.stride + j;
    int32_t e = -1;
    if (copied) {
        const uint32_t r = (uint32_t)S.kf_mp[from];
        if (present(A, r)) e = A.rdst[r];                    // a present row of an active slot is active
    }
    D.kf_mp[to] = e;
    if (D.kp_x) {
        D.kp_x[to] = copied ? S.kp_x[from] : 0.0f;
        D.kp_y[to] = copied ? S.kp_y[from] : 0.0f;
        D.kp_octave[to] = copied ? S.kp_octave[from] : 0;
        D.kp_depth[to] = copied ? S.kp_depth[from] : 0.0f;
    }
}

__global__ __launch_bounds__(kBlock) void k_extract_tracks(const ExtractArgs A) {
    const bool fits = A.head[kHeadRows] <= A.D.n_mp;         // the count is wanted either way, the write is not
    const int t = blockIdx.x * kBlock + (int)threadIdx.x;
    bool kept = false;
    if (t < A.S.n_track) {
        const uint32_t r = (uint32_t)A.S.track_row[t];
        kept = present(A, r) && (long long)A.S.mp_track[r] == (long long)A.S.track_base + t && A.cnt[r] > 0;      // mapdb.cpp:141-145 under the presence rule
        if (fits) A.D.track_row[t] = kept ? A.rdst[r] : -1;
    }
    const int n = __popcll(__ballot(kept));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(A.head + kHeadTracks, n);
}

__global__ __launch_bounds__(kBlock) void k_extract_pool(const ExtractArgs A) {
    if (A.head[kHeadRows] > A.D.n_mp) return;
    const int i = blockIdx.x / A.per_pool, e = (blockIdx.x % A.per_pool) * kBlock + (int)threadIdx.x;      // 16 bytes each, two per descriptor
    const int32_t from = A.pool_src[i];
    if (from < 0 || e >= 2 * A.n_kp[i]) return;
    reinterpret_cast<uint4 *>(A.D.desc_pool)[(size_t)A.pool_dst[i] * 2 + e] = reinterpret_cast<const uint4 *>(A.S.desc_pool)[(size_t)from * 2 + e];
}

}  // namespace

extern "C" int ms_map_extract(ms_ctx *c, const ms_map_extract_src *src, const ms_map_extract_dst *dst, const int32_t *kf_id, const int32_t *active, int n_active,
                              const int32_t *desc_base, const int32_t *n_kp, int32_t *dst_desc_base, int32_t *counts) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_map_extract_validate(src, dst, kf_id, active, n_active, desc_base, n_kp, dst_desc_base, counts, c->err, sizeof(c->err)))) return rc;
    MsRange range("mapExtract");
    const bool with_pool = src->desc_pool != nullptr, with_tracks = src->track_row != nullptr;
    const size_t na = (size_t)n_active, nm = (size_t)src->n_mp;
    const int per_slot = ms_div_up(src->stride, kBlock), per_pool = ms_div_up(2 * src->stride, kBlock);
    const size_t n_blk = std::max<size_t>((nm + kBlock - 1) / kBlock, 1);
    // upload block: the list | with a pool: keypoint counts | first descriptor in the source pool | in the destination pool
    MsLayout up;
    const auto l_list = up.array<int32_t>(na), l_nkp = up.array<int32_t>(with_pool ? na : 0), l_psrc = up.array<int32_t>(with_pool ? na : 0),
               l_pdst = up.array<int32_t>(with_pool ? na : 0);
    // device-only block: entries per source row | its destination row | source row of a destination row | active rows per workgroup | their offsets | the head
    MsLayout dev = up;
    const auto l_cnt = dev.array<int32_t>(nm), l_rdst = dev.array<int32_t>(nm), l_rsrc = dev.array<int32_t>(std::min(nm, (size_t)dst->n_mp));
    const auto l_bc = dev.array<int32_t>(n_blk), l_bo = dev.array<int32_t>(n_blk), l_head = dev.array<int32_t>(kHeadInts);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_MAP_EXTRACT];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    if ((rc = ms_pinned(c, l_head.bytes()))) return rc;
    void *hs = W.host, *ds = W.dev;
    int32_t n_desc = 0;
    for (int i = 0; i < n_active; ++i) {
        const bool has = with_pool && desc_base[active[i]] >= 0;
        dst_desc_base[i] = has ? n_desc : -1;
        if (has) n_desc += n_kp[i];
    }
    if (n_active > 0) {
        l_list.fill(hs, active);
        if (with_pool) {
            l_nkp.fill(hs, n_kp);
            for (int i = 0; i < n_active; ++i) l_psrc.at(hs)[i] = desc_base[active[i]];
            l_pdst.fill(hs, dst_desc_base);
        }
        MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    }
    ExtractArgs A{};
    A.S = *src; A.D = *dst;
    A.list = l_list.at(ds); A.n_kp = l_nkp.at(ds); A.pool_src = l_psrc.at(ds); A.pool_dst = l_pdst.at(ds);
    A.cnt = l_cnt.at(ds); A.rdst = l_rdst.at(ds); A.rsrc = l_rsrc.at(ds); A.blk_count = l_bc.at(ds); A.blk_off = l_bo.at(ds); A.head = l_head.at(ds);
    A.n_active = n_active; A.per_slot = per_slot; A.per_pool = per_pool; A.n_blk = (int32_t)n_blk;
    const dim3 block(kBlock), by_row((unsigned)n_blk), by_active((unsigned)(na * (size_t)per_slot));
    const dim3 by_dst_row((unsigned)ms_div_up(dst->n_mp, kBlock)), by_dst_entry((unsigned)((size_t)dst->n_kf * (size_t)per_slot));
    const dim3 by_track((unsigned)ms_div_up(src->n_track, kBlock)), by_desc((unsigned)(na * (size_t)per_pool));
    hipLaunchKernelGGL(k_extract_fill, by_row, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_extract_fill");
    if (by_active.x) {
        hipLaunchKernelGGL(k_extract_mark, by_active, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_extract_mark");
    }
    hipLaunchKernelGGL(k_extract_count, by_row, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_extract_count");
    hipLaunchKernelGGL(k_extract_offsets, dim3(1), block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_extract_offsets");
    hipLaunchKernelGGL(k_extract_place, by_row, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_extract_place");
    if (by_dst_row.x) {
        hipLaunchKernelGGL(k_extract_rows, by_dst_row, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_extract_rows");
    }
    if (by_dst_entry.x) {
        hipLaunchKernelGGL(k_extract_slots, by_dst_entry, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_extract_slots");
    }
    if (with_tracks && by_track.x) {
        hipLaunchKernelGGL(k_extract_tracks, by_track, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_extract_tracks");
    }
    if (with_pool && by_desc.x) {
        hipLaunchKernelGGL(k_extract_pool, by_desc, block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_extract_pool");
    }
    MS_HIP(c, hipMemcpyAsync(c->pinned, A.head, l_head.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *head = static_cast<const int32_t *>(c->pinned);
    const bool fits = head[kHeadRows] <= dst->n_mp;
    counts[0] = head[kHeadRows]; counts[1] = head[kHeadKept]; counts[2] = head[kHeadDropped]; counts[3] = head[kHeadTracks]; counts[4] = n_desc;
    if (!fits)
        return ms_fail(c, MS_ERR_CAPACITY, "map extract: %d active map points, the destination holds %d (the destination is untouched)", head[kHeadRows], dst->n_mp);
    return MS_OK;
}
