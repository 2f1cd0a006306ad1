// create_points.hip -- createNewMapPoints (mapper_helpers.cpp:271-318) on the device map tables: what the loop over the adjacent
// keyframes does between matchForTriangulationDBoW and the next adjacent, without the host.
//   ms_create_points_lists   the loop of :282-307 for one adjacent: every match of ms_match_triangulation becomes a provisional row with the two
//                            observations of :300-301 as an entry of ms_obs_lists, the form ms_triangulate_lists reads (:308)
//   ms_create_points_bind    :309-316 for the entries whose triangulation succeeded: both keyframes' entries, mp_live, the descriptor of two
//                            observations, the matcher's `usable` masks
//   ms_unbound_mask          the M2 mask of ms_match_frame ("has no map point", keyframe_matcher.cpp:205-221) of whole slots, from kf_mp
//
// The two walks have the shape of k_match_tracked: ONE workgroup of 256 lanes, trips of 256, block_rank (ms_scan.h) inside a trip and the
// running count carried across the trips.  k_create_lists decides and counts first (phase A writes nothing but its own workspace word per
// keypoint) and writes behind a barrier (phase B), only when phase A counted no violation and every capacity holds.  Each lane reads in B
// only what it wrote itself in A.  "A target named twice" is found with one LDS bit per keypoint of the adjacent keyframe and the value an
// atomicOr returns; no other atomic anywhere, no floating-point arithmetic: every output is an integer or a copy.
#include "ms_internal.h"
#include "ms_scan.h"
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int kDown = 8;                 // matches | violations: matched[j] out of range, target twice, bound entry, live new row, octave
constexpr int kMaskWords = MS_COVIS_MAX_STRIDE / 32;

struct ListsArgs {
    const int32_t *kf_mp;
    const uint8_t *mp_live;
    const float *kp_x, *kp_y, *kp_depth;
    const int32_t *kp_octave;
    const int32_t *matched, *new_rows;   // [n_kp1] the caller's | [n_new] uploaded
    int32_t *dst_of;                     // workspace [n_kp1]: the keypoint's position among the matches
    ms_obs_lists out;
    int32_t *match_kp1, *match_kp2;
    int32_t *down;                       // [kDown]
    int32_t stride, n_mp, n_kp1, n_kp2, n_new, cap_rows, cap_obs, n_levels;
    int32_t cur, adj, cur_first;         // cur_first: kf_id[cur] < kf_id[adj]
    int32_t base_cur, base_adj;          // kf_desc_base of the two slots, -1 for none
};

// the workgroup's sum of one int per lane, the same in every lane; ends with a barrier (s_wave is free again)
__device__ __forceinline__ int block_sum(int v, int32_t *s_wave) {
    int total;
    block_exclusive<kBlock>(v, s_wave, total);
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(kBlock) void k_create_lists(const ListsArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    __shared__ uint32_t s_named[kMaskWords];                 // one bit per keypoint of adj: some match names it
    for (int w = threadIdx.x; w < kMaskWords; w += kBlock) s_named[w] = 0u;
    __syncthreads();
    const int32_t *row_cur = A.kf_mp + (size_t)A.cur * A.stride, *row_adj = A.kf_mp + (size_t)A.adj * A.stride;
    const bool levels = A.n_levels > 0 && A.kp_octave != nullptr;
    // ---- phase A
    int n_matches = 0;                                       // running count, the same in every lane
    int v_range = 0, v_twice = 0, v_bound = 0, v_live = 0, v_octave = 0;      // this lane's
    for (int j0 = 0; j0 < A.n_kp1; j0 += kBlock) {
        const int j = j0 + (int)threadIdx.x;
        bool is_match = false;
        if (j < A.n_kp1) {
            const int32_t m = A.matched[j];
            if (m != -1) {
                if ((uint32_t)m >= (uint32_t)A.n_kp2) ++v_range;
                else {
                    is_match = true;
                    const uint32_t bit = 1u << (m & 31);
                    v_twice += (atomicOr(&s_named[m >> 5], bit) & bit) != 0u;
                    v_bound += (uint32_t)row_cur[j] < (uint32_t)A.n_mp;                                  // keyframe.cpp:275, both keyframes
                    v_bound += (uint32_t)row_adj[m] < (uint32_t)A.n_mp;
                    if (levels) {
                        v_octave += (uint32_t)A.kp_octave[(size_t)A.cur * A.stride + j] >= (uint32_t)A.n_levels;
                        v_octave += (uint32_t)A.kp_octave[(size_t)A.adj * A.stride + m] >= (uint32_t)A.n_levels;
                    }
                }
            }
        }
        int total;
        const int k = n_matches + block_rank<kBlock>(is_match, s_wave, total);
        n_matches += total;
        if (j < A.n_kp1) {
            A.dst_of[j] = is_match ? k : -1;
            if (is_match && k < A.n_new) v_live += A.mp_live[A.new_rows[k]] != 0;                         // in [0, n_mp): validated
        }
        __syncthreads();                                     // s_wave is written again in the next trip
    }
    v_range = block_sum(v_range, s_wave); v_twice = block_sum(v_twice, s_wave); v_bound = block_sum(v_bound, s_wave);
    v_live = block_sum(v_live, s_wave); v_octave = block_sum(v_octave, s_wave);
    if (threadIdx.x == 0) {
        A.down[0] = n_matches; A.down[1] = v_range; A.down[2] = v_twice; A.down[3] = v_bound; A.down[4] = v_live; A.down[5] = v_octave;
    }
    if (v_range | v_twice | v_bound | v_live | v_octave) return;             // the same in every lane
    if (n_matches > A.n_new || n_matches > A.cap_rows || 2 * (long long)n_matches > A.cap_obs) return;
    // ---- phase B (the last barrier above separates it from every read of phase A)
    const ms_obs_lists &L = A.out;
    if (threadIdx.x == 0) L.obs_start[n_matches] = 2 * n_matches;
    for (int j = threadIdx.x; j < A.n_kp1; j += kBlock) {    // the lane that decided keypoint j
        const int i = A.dst_of[j];
        if (i < 0) continue;
        const int m = A.matched[j];
        L.rows[i] = A.new_rows[i];
        L.obs_start[i] = 2 * i;
        if (L.n_obs_row) L.n_obs_row[i] = 2;
        if (L.was_triangulated) L.was_triangulated[i] = 0;
        if (A.match_kp1) A.match_kp1[i] = j;
        if (A.match_kp2) A.match_kp2[i] = m;
#pragma unroll
        for (int s = 0; s < 2; ++s) {                        // MapPoint::observations is a std::map<KfId, KpId>: ascending kf_id
            const bool of_cur = (s == 0) == (A.cur_first != 0);
            const int slot = of_cur ? A.cur : A.adj, p = of_cur ? j : m, base = of_cur ? A.base_cur : A.base_adj;
            const size_t e = (size_t)slot * A.stride + p;
            const int o = 2 * i + s;
            if (L.obs_kf) L.obs_kf[o] = slot;
            if (L.obs_kp) L.obs_kp[o] = p;
            if (L.obs_x) L.obs_x[o] = A.kp_x[e];
            if (L.obs_y) L.obs_y[o] = A.kp_y[e];
            if (L.obs_depth) L.obs_depth[o] = A.kp_depth[e];
            if (L.obs_desc) L.obs_desc[o] = base < 0 ? -1 : base + p;
            if (L.obs_octave || (s == 0 && L.first_octave)) {
                const int32_t octave = A.kp_octave[e];
                if (L.obs_octave) L.obs_octave[o] = octave;
                if (s == 0 && L.first_octave) L.first_octave[i] = octave;
            }
        }
    }
}

struct BindArgs {
    ms_obs_lists lists;                  // rows, obs_desc are read
    const int32_t *match_kp1, *match_kp2;
    const uint8_t *mp_flags;
    const uint32_t *desc_pool;
    int32_t *kf_mp;
    uint8_t *mp_live;
    uint32_t *mp_desc;
    int32_t *n_obs, *mp_track;
    uint8_t *usable1, *usable2;
    int32_t *created_rows, *created_kp1, *created_kp2;
    int32_t *down;                       // created | entries that name a row or a keypoint outside the tables
    int32_t n_matches, n_kp1, n_kp2, stride, n_mp, n_pool, cur, adj;
};

__global__ __launch_bounds__(kBlock) void k_create_bind(const BindArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    // the lists lie on the device and nothing checked them since they were written: every index is compared first, nothing is written otherwise
    int bad = 0;
    for (int i = threadIdx.x; i < A.n_matches; i += kBlock) {
        const bool ok = (uint32_t)A.lists.rows[i] < (uint32_t)A.n_mp && (uint32_t)A.match_kp1[i] < (uint32_t)A.n_kp1 && (uint32_t)A.match_kp2[i] < (uint32_t)A.n_kp2;      // n_kp <= stride: validated
        bool desc_ok = true;
        if (A.desc_pool && A.lists.obs_desc)
            for (int s = 0; s < 2; ++s) { const int32_t d = A.lists.obs_desc[2 * i + s]; desc_ok = desc_ok && (d == -1 || (uint32_t)d < (uint32_t)A.n_pool); }
        bad += !(ok && desc_ok);
    }
    bad = block_sum(bad, s_wave);
    if (bad) {
        if (threadIdx.x == 0) { A.down[0] = 0; A.down[1] = bad; }
        return;                                              // the same in every lane
    }
    int n_created = 0;
    for (int i0 = 0; i0 < A.n_matches; i0 += kBlock) {
        const int i = i0 + (int)threadIdx.x;
        int r = 0;
        bool kept = false;
        if (i < A.n_matches) {
            r = A.lists.rows[i];
            kept = A.mp_flags[r] != 0;                                                                   // :309, status != NOT_TRIANGULATED
        }
        int total;
        const int dst = n_created + block_rank<kBlock>(kept, s_wave, total);
        n_created += total;
        if (kept) {
            const int kp1 = A.match_kp1[i], kp2 = A.match_kp2[i];
            A.kf_mp[(size_t)A.cur * A.stride + kp1] = r;                                                 // :310-311
            A.kf_mp[(size_t)A.adj * A.stride + kp2] = r;
            A.mp_live[r] = 1;
            if (A.n_obs) A.n_obs[r] = 2;
            if (A.mp_track) A.mp_track[r] = -1;
            if (A.usable1) A.usable1[kp1] = 0;
            if (A.usable2) A.usable2[kp2] = 0;
            if (A.desc_pool && A.lists.obs_desc) {
                // updateDescriptor of two observations: the FIRST descriptor (the rule of k_match_finish, map_point.cpp:101-113); none: it stays
                for (int s = 0; s < 2; ++s) {
                    const int32_t d = A.lists.obs_desc[2 * i + s];
                    if (d == -1) continue;
                    const uint4 *src = reinterpret_cast<const uint4 *>(A.desc_pool + 8 * (size_t)d);
                    uint4 *out = reinterpret_cast<uint4 *>(A.mp_desc + 8 * (size_t)r);
                    const uint4 lo = src[0], hi = src[1];
                    out[0] = lo; out[1] = hi;
                    break;
                }
            }
            if (A.created_rows) A.created_rows[dst] = r;
            if (A.created_kp1) A.created_kp1[dst] = kp1;
            if (A.created_kp2) A.created_kp2[dst] = kp2;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { A.down[0] = n_created; A.down[1] = 0; }
}

struct MaskSlot {
    uint8_t *usable;
    int32_t slot, n_kp;
};

__global__ __launch_bounds__(kBlock) void k_unbound_mask(const int32_t *kf_mp, const MaskSlot *slots, int stride, int n_mp) {
    const MaskSlot S = slots[blockIdx.y];
    const int j = blockIdx.x * kBlock + (int)threadIdx.x;
    if (j < S.n_kp) S.usable[j] = (uint8_t)!((uint32_t)kf_mp[(size_t)S.slot * stride + j] < (uint32_t)n_mp);
}

}  // namespace

extern "C" int ms_create_points_lists(ms_ctx *c, const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, int n_mp, const int32_t *kf_id, const float *kp_x,
                                      const float *kp_y, const int32_t *kp_octave, const float *kp_depth, const int32_t *kf_desc_base, int cur, int adj,
                                      const int32_t *matched, int n_kp1, int n_kp2, const int32_t *new_rows, int n_new, int n_levels, const ms_obs_lists *lists, int cap_rows,
                                      int cap_obs, int32_t *match_kp1, int32_t *match_kp2, int32_t *n_matches) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_create_points_lists_check(kf_mp, n_kf, stride, mp_live, n_mp, kf_id, kp_x, kp_y, kp_octave, kp_depth, kf_desc_base, cur, adj, matched, n_kp1, n_kp2, new_rows,
                                           n_new, n_levels, lists, cap_rows, cap_obs, match_kp1, match_kp2, n_matches, c->err, sizeof(c->err))))
        return rc;
    *n_matches = 0;
    if (n_kp1 == 0) return MS_OK;
    MsRange range("createNewMapPointsLists");
    MsLayout up;
    const auto l_new = up.array<int32_t>((size_t)n_new);
    MsLayout host = up, dev = up;
    const auto l_down = host.array<int32_t>(kDown);
    const auto l_res = dev.array<int32_t>(kDown), l_dst = dev.array<int32_t>((size_t)n_kp1);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_CREATE_POINTS];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    l_new.fill(hs, new_rows);
    if (up.end) MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    ListsArgs A{};
    A.kf_mp = kf_mp; A.mp_live = mp_live; A.kp_x = kp_x; A.kp_y = kp_y; A.kp_depth = kp_depth; A.kp_octave = kp_octave;
    A.matched = matched; A.new_rows = l_new.at(ds); A.dst_of = l_dst.at(ds);
    A.out = *lists; A.match_kp1 = match_kp1; A.match_kp2 = match_kp2; A.down = l_res.at(ds);
    A.stride = stride; A.n_mp = n_mp; A.n_kp1 = n_kp1; A.n_kp2 = n_kp2; A.n_new = n_new; A.cap_rows = cap_rows; A.cap_obs = cap_obs; A.n_levels = n_levels;
    A.cur = cur; A.adj = adj; A.cur_first = kf_id[cur] < kf_id[adj];
    A.base_cur = kf_desc_base ? kf_desc_base[cur] : -1; A.base_adj = kf_desc_base ? kf_desc_base[adj] : -1;
    hipLaunchKernelGGL(k_create_lists, dim3(1), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_create_lists");
    MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_res.at(ds), l_res.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *down = l_down.at(hs);
    *n_matches = down[0];
    if (down[1] | down[2] | down[3] | down[4] | down[5])
        return ms_fail(c, MS_ERR_INVALID, "create points lists: %d matched entries outside [0, %d), %d targets named twice, %d matched keypoints whose kf_mp entry is already valid, "
                       "%d new rows that are live, %d octaves outside [0, %d) (nothing written)", down[1], n_kp2, down[2], down[3], down[4], down[5], n_levels);
    if (down[0] > n_new || down[0] > cap_rows || 2 * (long long)down[0] > cap_obs)
        return ms_fail(c, MS_ERR_CAPACITY, "create points lists: %d matches; new_rows holds %d, the lists %d rows and %d observations (nothing written)", down[0], n_new,
                       cap_rows, cap_obs);
    return MS_OK;
}

extern "C" int ms_create_points_bind(ms_ctx *c, int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, uint8_t *mp_live, uint32_t *mp_desc, int32_t *n_obs,
                                     int32_t *mp_track, int n_mp, const uint32_t *desc_pool, int n_pool, int cur, int adj, const ms_obs_lists *lists,
                                     const int32_t *match_kp1, const int32_t *match_kp2, int n_matches, int n_kp1, int n_kp2, uint8_t *usable1, uint8_t *usable2,
                                     int32_t *created_rows, int32_t *created_kp1, int32_t *created_kp2, int32_t *n_created) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_create_points_bind_check(kf_mp, n_kf, stride, mp_flags, mp_live, mp_desc, n_obs, mp_track, n_mp, desc_pool, n_pool, cur, adj, lists, match_kp1, match_kp2,
                                          n_matches, n_kp1, n_kp2, usable1, usable2, created_rows, created_kp1, created_kp2, n_created, c->err, sizeof(c->err))))
        return rc;
    *n_created = 0;
    if (n_matches == 0) return MS_OK;
    MsRange range("createNewMapPointsBind");
    MsLayout host, dev;
    const auto l_down = host.array<int32_t>(2), l_res = dev.array<int32_t>(2);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_CREATE_POINTS];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    BindArgs A{};
    A.lists = *lists; A.match_kp1 = match_kp1; A.match_kp2 = match_kp2; A.mp_flags = mp_flags; A.desc_pool = desc_pool;
    A.kf_mp = kf_mp; A.mp_live = mp_live; A.mp_desc = mp_desc; A.n_obs = n_obs; A.mp_track = mp_track; A.usable1 = usable1; A.usable2 = usable2;
    A.created_rows = created_rows; A.created_kp1 = created_kp1; A.created_kp2 = created_kp2; A.down = l_res.at(W.dev);
    A.n_matches = n_matches; A.n_kp1 = n_kp1; A.n_kp2 = n_kp2; A.stride = stride; A.n_mp = n_mp; A.n_pool = n_pool; A.cur = cur; A.adj = adj;
    hipLaunchKernelGGL(k_create_bind, dim3(1), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_create_bind");
    MS_HIP(c, hipMemcpyAsync(l_down.at(W.host), l_res.at(W.dev), l_res.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *down = l_down.at(W.host);
    if (down[1]) return ms_fail(c, MS_ERR_INVALID, "create points bind: %d entries name a row, a keypoint or a descriptor outside the tables (nothing written)", down[1]);
    *n_created = down[0];
    return MS_OK;
}

extern "C" int ms_unbound_mask(ms_ctx *c, const int32_t *kf_mp, int n_kf, int stride, int n_mp, const int32_t *slots, const int32_t *n_kp, uint8_t *const *usable,
                               int n_slots) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_unbound_mask_check(kf_mp, n_kf, stride, n_mp, slots, n_kp, usable, n_slots, c->err, sizeof(c->err)))) return rc;
    int longest = 0;
    for (int s = 0; s < n_slots; ++s) longest = n_kp[s] > longest ? n_kp[s] : longest;
    if (longest == 0) return MS_OK;
    MsRange range("unboundMask");
    MsLayout up;
    const auto l_slots = up.array<MaskSlot>((size_t)n_slots);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_CREATE_POINTS];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, up.end, false))) return rc;
    MaskSlot *S = l_slots.at(W.host);
    for (int s = 0; s < n_slots; ++s) { S[s].usable = usable[s]; S[s].slot = slots[s]; S[s].n_kp = n_kp[s]; }
    MS_HIP(c, hipMemcpyAsync(W.dev, W.host, up.end, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_unbound_mask, dim3(ms_div_up(longest, kBlock), n_slots), dim3(kBlock), 0, c->stream, kf_mp, l_slots.at(W.dev), stride, n_mp);
    MS_KERNEL_CHECK(c, "k_unbound_mask");
    MS_HIP(c, hipStreamSynchronize(c->stream));                // the staging block is written again by the next call
    return MS_OK;
}
