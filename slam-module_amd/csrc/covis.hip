// covis.hip -- set queries over the keyframe table kf_mp (slot -> the map-point rows of Keyframe::mapPoints), for many queries in one call:
//   ms_covisibility      Keyframe::getNeighbors              keyframe.cpp:192-230
//   ms_map_point_union   localMps / adjacentMapPointsSet     mapper_helpers.cpp:241-261, :337-345
//                        loopMapPoints / localMapPoints      loop_closer.cpp:569-584, :418-433, :465-469
//
// An entry r of the table is used only after (uint32)r < n_mp held; everything else is "none".  Everything is integer work.
//
// ms_covisibility, four launches whatever the number of queries:
//   (memset)        the queries' bitmaps, n_mp bits each plus one word that stays zero (where the invalid entries of k_covis_count point)
//   k_covis_mark    one lane per (query, entry of its slot): OR the row's bit into the query's bitmap
//   k_covis_count   one workgroup per candidate slot: its entries are loaded once into registers (dwordx4 when the rows are 16-byte aligned),
//                   then for every query each lane tests its entries' bits; ballot + popcount per wave, the four wave totals of 64 queries
//                   at a time through LDS.  The table is read once per call, not once per query.
//   k_covis_pick    one wave per query walks the slots 64 at a time and packs the neighbours with a ballot prefix, ascending
// ms_map_point_union, six launches whatever the number of problems:
//   k_union_fill    mark[u][r] = kNone
//   k_union_mark    one lane per (list entry, entry of its slot): atomicMin(mark[u][r], position in the problem's list)
//   k_union_exclude the valid entries of the problem's exclude slot go back to kNone
//   k_union_count / k_union_offsets / k_union_pack   block_rank, per-workgroup count and block_offsets (ms_scan.h) over 256-row
//                   blocks: the packed order is ascending row order
// The only atomics are OR on bitmap words and MIN on owner words: no order of arrival decides anything.
#include "ms_internal.h"
#include "ms_scan.h"
#include <algorithm>
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int kQueryBatch = 64;                              // queries whose wave totals share one trip through LDS

struct QDev { int32_t slot, force_a, force_b, min_covis, require; };

struct CovisArgs {
    const int32_t *kf_mp;
    const uint8_t *mp_flags;
    const QDev *q;
    uint32_t *bitmap;                    // [n_q][words + 1]; word `words` of a query is never marked
    int32_t *count, *neighbours, *n_neighbours;
    int32_t n_kf, stride, n_mp, n_q, words;
    int32_t vec;                         // rows of kf_mp are 16-byte aligned
};

__global__ __launch_bounds__(kBlock) void k_covis_mark(const CovisArgs A) {
    const int q = blockIdx.y, j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= A.stride) return;
    const QDev Q = A.q[q];
    const uint32_t r = (uint32_t)A.kf_mp[(size_t)Q.slot * A.stride + j];
    if (r >= (uint32_t)A.n_mp) return;
    if (Q.require && (A.mp_flags[r] & Q.require) != Q.require) return;
    atomicOr(A.bitmap + (size_t)q * (A.words + 1) + (r >> 5), 1u << (r & 31));
}

template <int NV>                        // dwordx4 loads per lane: a slot of up to 1024 * NV entries lives in the workgroup's registers
__global__ __launch_bounds__(kBlock) void k_covis_count(const CovisArgs A) {
    __shared__ int32_t s_cnt[kBlock / 64][kQueryBatch];
    const int k = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t *row = A.kf_mp + (size_t)k * A.stride;
    const uint32_t none = 32u * (uint32_t)A.words;           // bit 0 of the word that stays zero
    uint32_t e[4 * NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int j = 4 * (v * kBlock + (int)threadIdx.x);
        int4 x = make_int4(-1, -1, -1, -1);
        if (A.vec) {                                         // stride is a multiple of 4 then: j < stride covers j + 3
            if (j < A.stride) x = *reinterpret_cast<const int4 *>(row + j);
        } else {
            if (j < A.stride) x.x = row[j];
            if (j + 1 < A.stride) x.y = row[j + 1];
            if (j + 2 < A.stride) x.z = row[j + 2];
            if (j + 3 < A.stride) x.w = row[j + 3];
        }
        e[4 * v] = (uint32_t)x.x < (uint32_t)A.n_mp ? (uint32_t)x.x : none;
        e[4 * v + 1] = (uint32_t)x.y < (uint32_t)A.n_mp ? (uint32_t)x.y : none;
        e[4 * v + 2] = (uint32_t)x.z < (uint32_t)A.n_mp ? (uint32_t)x.z : none;
        e[4 * v + 3] = (uint32_t)x.w < (uint32_t)A.n_mp ? (uint32_t)x.w : none;
    }
    for (int q0 = 0; q0 < A.n_q; q0 += kQueryBatch) {
        const int nb = min(kQueryBatch, A.n_q - q0);
        int mine = 0;                                        // lane i keeps the wave's total of query q0 + i
        for (int qi = 0; qi < nb; ++qi) {
            const uint32_t *bm = A.bitmap + (size_t)(q0 + qi) * (A.words + 1);
            int c = 0;
#pragma unroll
            for (int i = 0; i < 4 * NV; ++i) c += __popcll(__ballot((bm[e[i] >> 5] >> (e[i] & 31)) & 1u));
            if (lane == qi) mine = c;
        }
        s_cnt[wave][lane] = mine;
        __syncthreads();
        if ((int)threadIdx.x < nb) {
            int total = 0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; ++w) total += s_cnt[w][threadIdx.x];
            A.count[(size_t)(q0 + (int)threadIdx.x) * A.n_kf + k] = total;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void k_covis_pick(const CovisArgs A) {
    const int q = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= A.n_q) return;                                  // whole waves leave
    const QDev Q = A.q[q];
    const int32_t *cnt = A.count + (size_t)q * A.n_kf;
    int32_t *out = A.neighbours + (size_t)q * A.n_kf;
    int base = 0;
    for (int k0 = 0; k0 < A.n_kf; k0 += 64) {
        const int k = k0 + lane;
        bool is = false;
        if (k < A.n_kf && k != Q.slot) {
            const int c = cnt[k];
            is = k == Q.force_a || k == Q.force_b || (c >= 1 && c >= Q.min_covis);
        }
        const unsigned long long mask = __ballot(is);
        if (is) out[base + lanes_before(mask)] = k;
        base += __popcll(mask);
    }
    if (lane == 0) A.n_neighbours[q] = base;
}

struct UDev { int32_t exclude, require; };

struct UnionArgs {
    const int32_t *kf_mp;
    const uint8_t *mp_flags;
    const UDev *u;
    const int32_t *entry;                // per list entry of every problem: problem, position in its list, slot
    int32_t *mark;                       // [n_u][n_mp]
    int32_t *blk_count, *blk_off;        // [n_u][n_blk]
    int32_t *rows, *owner, *n_rows;
    int32_t n_kf, stride, n_mp, n_u, n_blk, per_slot;       // per_slot = workgroups per slot of kf_mp
};

__global__ __launch_bounds__(kBlock) void k_union_fill(const UnionArgs A, size_t n) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) A.mark[i] = kNone;
}

__global__ __launch_bounds__(kBlock) void k_union_mark(const UnionArgs A) {
    const int en = blockIdx.x / A.per_slot, j = (blockIdx.x % A.per_slot) * kBlock + (int)threadIdx.x;
    if (j >= A.stride) return;
    const int u = A.entry[3 * (size_t)en], p = A.entry[3 * (size_t)en + 1], slot = A.entry[3 * (size_t)en + 2];
    const uint32_t r = (uint32_t)A.kf_mp[(size_t)slot * A.stride + j];
    if (r >= (uint32_t)A.n_mp) return;
    const int require = A.u[u].require;
    if (require && (A.mp_flags[r] & require) != require) return;
    atomicMin(A.mark + (size_t)u * A.n_mp + r, p);
}

__global__ __launch_bounds__(kBlock) void k_union_exclude(const UnionArgs A) {
    const int u = blockIdx.y, j = blockIdx.x * kBlock + (int)threadIdx.x;
    const int slot = A.u[u].exclude;
    if (slot < 0 || j >= A.stride) return;
    const uint32_t r = (uint32_t)A.kf_mp[(size_t)slot * A.stride + j];
    if (r < (uint32_t)A.n_mp) A.mark[(size_t)u * A.n_mp + r] = kNone;
}

// the lane's row, its mark and its rank among the workgroup's kept rows, in row order; the workgroup's total through `total`
__device__ inline int union_rank(const UnionArgs &A, int32_t *s_wave, int u, int &r, int32_t &mark, int &total) {
    r = blockIdx.x * kBlock + (int)threadIdx.x;
    mark = r < A.n_mp ? A.mark[(size_t)u * A.n_mp + r] : kNone;
    return block_rank<kBlock>(mark != kNone, s_wave, total);
}

__global__ __launch_bounds__(kBlock) void k_union_count(const UnionArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    int r, total;
    int32_t mark;
    union_rank(A, s_wave, blockIdx.y, r, mark, total);
    if (threadIdx.x == 0) A.blk_count[(size_t)blockIdx.y * A.n_blk + blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_union_offsets(const UnionArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int u = blockIdx.x;
    const int rows = block_offsets<kBlock>(A.blk_count + (size_t)u * A.n_blk, A.blk_off + (size_t)u * A.n_blk, A.n_blk, s_wave);
    if (threadIdx.x == 0) A.n_rows[u] = rows;
}

__global__ __launch_bounds__(kBlock) void k_union_pack(const UnionArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int u = blockIdx.y;
    int r, total;
    int32_t mark;
    const int rank = union_rank(A, s_wave, u, r, mark, total);
    if (mark == kNone) return;
    const size_t dst = (size_t)u * A.n_mp + (size_t)A.blk_off[(size_t)u * A.n_blk + blockIdx.x] + (size_t)rank;
    A.rows[dst] = r;
    if (A.owner) A.owner[dst] = mark;
}

}  // namespace

extern "C" int ms_covisibility(ms_ctx *c, const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, int n_mp, const ms_covis_query *queries, int n_q,
                               int32_t *count, int32_t *neighbours, int32_t *n_neighbours) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_covisibility_check(kf_mp, n_kf, stride, mp_flags, n_mp, queries, n_q, neighbours, n_neighbours, c->err, sizeof(c->err)))) return rc;
    if (ms_map_over_capacity(n_kf, stride, n_mp, n_q))
        return ms_fail(c, MS_ERR_CAPACITY, "covisibility: %d slots / stride %d / %d map points / %d queries, caps %d / %d / below %d / %d", n_kf, stride, n_mp, n_q,
                       MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, MS_COVIS_MAX_QUERIES);
    if (n_q == 0) return MS_OK;
    MsRange range("covisibility");
    const size_t nq = (size_t)n_q, words = ((size_t)n_mp + 31) / 32;
    // upload block: queries; then (host only) the neighbour counts
    MsLayout up;
    const auto l_q = up.array<QDev>(nq);
    MsLayout host = up, dev = up;
    const auto l_down = host.array<int32_t>(nq);
    // device-only block: neighbour counts | bitmaps | counts when the caller does not want them
    const auto l_nn = dev.array<int32_t>(nq);
    const auto l_bm = dev.array<uint32_t>(nq * (words + 1));
    const auto l_cnt = dev.array<int32_t>(count ? 0 : nq * (size_t)n_kf);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_COVIS];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    QDev *hq = l_q.at(hs);
    for (int q = 0; q < n_q; ++q) hq[q] = QDev{queries[q].slot, queries[q].force_a, queries[q].force_b, queries[q].min_covis, (int32_t)queries[q].require};
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    CovisArgs A;
    A.kf_mp = kf_mp; A.mp_flags = mp_flags;
    A.q = l_q.at(ds);
    A.bitmap = l_bm.at(ds);
    A.count = count ? count : l_cnt.at(ds);
    A.neighbours = neighbours;
    A.n_neighbours = l_nn.at(ds);
    A.n_kf = n_kf; A.stride = stride; A.n_mp = n_mp; A.n_q = n_q; A.words = (int32_t)words;
    A.vec = stride % 4 == 0 && (reinterpret_cast<uintptr_t>(kf_mp) & 15u) == 0;
    MS_HIP(c, hipMemsetAsync(A.bitmap, 0, l_bm.bytes(), c->stream));
    hipLaunchKernelGGL(k_covis_mark, dim3(ms_div_up(stride, kBlock), (unsigned)n_q), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_covis_mark");
    const dim3 slots((unsigned)n_kf), block(kBlock);
    if (stride <= 1024) hipLaunchKernelGGL(k_covis_count<1>, slots, block, 0, c->stream, A);
    else if (stride <= 2048) hipLaunchKernelGGL(k_covis_count<2>, slots, block, 0, c->stream, A);
    else if (stride <= 4096) hipLaunchKernelGGL(k_covis_count<4>, slots, block, 0, c->stream, A);
    else hipLaunchKernelGGL(k_covis_count<8>, slots, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_covis_count");
    hipLaunchKernelGGL(k_covis_pick, dim3(ms_div_up(n_q, kBlock / 64)), block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_covis_pick");
    MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_nn.at(ds), l_nn.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(n_neighbours, l_down.at(hs), l_down.bytes());
    return MS_OK;
}

extern "C" int ms_map_point_union(ms_ctx *c, const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, int n_mp, const int32_t *kf_list, int n_list,
                                  const ms_union_problem *problems, int n_u, int32_t *rows, int32_t *owner, int32_t *n_rows) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_map_point_union_check(kf_mp, n_kf, stride, mp_flags, n_mp, kf_list, n_list, problems, n_u, rows, n_rows, c->err, sizeof(c->err)))) return rc;
    long long n_entries = 0;
    for (int u = 0; u < n_u; ++u) n_entries += problems[u].count;
    if (ms_map_over_capacity(n_kf, stride, n_mp, n_u) || n_entries > MS_UNION_MAX_ENTRIES)
        return ms_fail(c, MS_ERR_CAPACITY, "map point union: %d slots / stride %d / %d map points / %d problems / %lld list entries, caps %d / %d / below %d / %d / %d", n_kf,
                       stride, n_mp, n_u, n_entries, MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, MS_COVIS_MAX_QUERIES, MS_UNION_MAX_ENTRIES);
    if (n_u == 0) return MS_OK;
    if (n_mp == 0) {                                         // no row can be valid
        std::memset(n_rows, 0, 4 * (size_t)n_u);
        return MS_OK;
    }
    MsRange range("mapPointUnion");
    const size_t nu = (size_t)n_u, ne = (size_t)n_entries, n_blk = ((size_t)n_mp + kBlock - 1) / kBlock;
    // upload block: problems | list entries; then (host only) the row counts
    MsLayout up;
    const auto l_u = up.array<UDev>(nu);
    const auto l_en = up.array<int32_t>(3 * ne);
    MsLayout host = up, dev = up;
    const auto l_down = host.array<int32_t>(nu);
    // device-only block: row counts | marks | block counts | block offsets
    const auto l_nr = dev.array<int32_t>(nu), l_mark = dev.array<int32_t>(nu * (size_t)n_mp);
    const auto l_bc = dev.array<int32_t>(nu * n_blk), l_bo = dev.array<int32_t>(nu * n_blk);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_COVIS];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    UDev *hu = l_u.at(hs);
    int32_t *he = l_en.at(hs);
    bool any_exclude = false;
    for (int u = 0, at = 0; u < n_u; ++u) {
        const ms_union_problem &P = problems[u];
        hu[u] = UDev{P.exclude_slot, (int32_t)P.require};
        any_exclude |= P.exclude_slot >= 0;
        for (int p = 0; p < P.count; ++p, ++at) { he[3 * at] = u; he[3 * at + 1] = p; he[3 * at + 2] = kf_list[P.first + p]; }
    }
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    UnionArgs A;
    A.kf_mp = kf_mp; A.mp_flags = mp_flags;
    A.u = l_u.at(ds); A.entry = l_en.at(ds);
    A.mark = l_mark.at(ds); A.blk_count = l_bc.at(ds); A.blk_off = l_bo.at(ds);
    A.rows = rows; A.owner = owner;
    A.n_rows = l_nr.at(ds);
    A.n_kf = n_kf; A.stride = stride; A.n_mp = n_mp; A.n_u = n_u; A.n_blk = (int32_t)n_blk; A.per_slot = ms_div_up(stride, kBlock);
    const size_t n_mark = nu * (size_t)n_mp;
    const dim3 block(kBlock), by_row((unsigned)n_blk, (unsigned)n_u);
    hipLaunchKernelGGL(k_union_fill, dim3((unsigned)((n_mark + kBlock - 1) / kBlock)), block, 0, c->stream, A, n_mark);
    MS_KERNEL_CHECK(c, "k_union_fill");
    if (ne > 0) {
        hipLaunchKernelGGL(k_union_mark, dim3((unsigned)(ne * (size_t)A.per_slot)), block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_union_mark");
    }
    if (any_exclude && ne > 0) {
        hipLaunchKernelGGL(k_union_exclude, dim3((unsigned)A.per_slot, (unsigned)n_u), block, 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_union_exclude");
    }
    hipLaunchKernelGGL(k_union_count, by_row, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_union_count");
    hipLaunchKernelGGL(k_union_offsets, dim3((unsigned)n_u), block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_union_offsets");
    hipLaunchKernelGGL(k_union_pack, by_row, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_union_pack");
    MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_nr.at(ds), l_nr.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(n_rows, l_down.at(hs), l_down.bytes());
    return MS_OK;
}
