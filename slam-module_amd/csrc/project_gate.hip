// project_gate.hip -- the per-map-point gates in front of the projection-guided matchers, for many views in one call:
//   MS_GATE_SEARCH  searchByProjection         keyframe_matcher.cpp:313-345 (Keyframe::isInFrustum, keyframe.cpp:247-262, is the same gates)
//   MS_GATE_FUSE    replaceDuplication         keyframe_matcher.cpp:442-471
//   MS_GATE_SIM3    findMatchesTranformedMps   keyframe_matcher.cpp:573-596
//
// An entry is (view, map point): reprojection, viewing distance, viewing angle, MapPoint::predictScaleLevel (map_point.cpp:174-183) and the
// search radius, then the surviving entries of every view packed in entry order as the query arrays of ms_projection_topk.  Three launches,
// whatever the number of views:
//
//   k_gate          one lane per entry, 256-lane workgroups that never straddle two views (a block -> (view, first entry) table); the view
//                   record is staged in LDS once per workgroup.  Writes the per-entry outputs, the lane's rank among the workgroup's kept
//                   entries (block_rank of ms_scan.h) and the workgroup's kept count.
//   k_gate_offsets  one workgroup per view: block_offsets of the view's workgroup counts -> each workgroup's offset in the view's slice, n_kept.
//   k_gate_pack     one lane per entry again: a kept entry writes its query to slice position offset + rank and gathers its descriptor.
//
// Ranks and offsets are prefix sums in entry order, so the packed order is the walk order of the reference's loops and no atomic decides anything.
// Every floating-point operation is a single rounded IEEE operation (the library builds with -ffp-contract=off; the *_rn intrinsics pin the ones
// whose order matters; the float square root is sqrtf, which hipcc rounds correctly by default -- __fsqrt_rn is the native approximation here);
// logf is the one function whose last bit is the implementation's (near_level).
#include "ms_internal.h"
#include "ms_scan.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int32_t kNoWindowMin = -0x7fffffff, kNoWindowMax = 0x7fffffff;     // "no octave window", as mi355slam::RadiusQuery's defaults

struct GvDev {                           // one view as the kernels see it
    double R[9], t[3], c[3];             // c = -R^T t (SEARCH / FUSE)
    double fx, fy, cx, cy, w, h;
    float threshold, cos_limit;
    int32_t mode, first, count;
    int32_t blk0, nblk;                  // the view's workgroups in the block table
    int32_t pad;
};
static_assert(sizeof(GvDev) % 8 == 0, "GvDev is copied to LDS by words");

struct GateArgs {
    const GvDev *views;
    const int2 *blocks;                  // per workgroup: (view, first entry relative to the view's slice)
    const int32_t *mp_index;
    const float *sf;
    const double *mp_pos;
    const float *mp_norm, *mp_min, *mp_max;
    const uint32_t *mp_desc;
    int32_t n_levels;
    float scale_factor;
    uint8_t *status;
    float *x, *y, *dist;
    int32_t *level;
    float *radius;
    int32_t *rank;                       // workspace [n_entries]: rank among the workgroup's kept entries, -1 when rejected
    int32_t *blk_count, *blk_off;        // workspace [n_blocks]
    int32_t *n_kept;                     // [n_views]
    int32_t *kept_entry;
    float *q_x, *q_y, *q_radius;
    int32_t *q_min_octave, *q_max_octave;
    uint32_t *q_desc;
};

__global__ __launch_bounds__(kBlock) void k_gate(const GateArgs A) {
    __shared__ GvDev V;
    __shared__ int32_t s_wave[kBlock / 64];
    const int2 blk = A.blocks[blockIdx.x];
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(A.views + blk.x);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&V);
        for (int i = threadIdx.x; i < (int)(sizeof(GvDev) / 4); i += kBlock) dst[i] = src[i];
    }
    __syncthreads();
    const int k = blk.y + (int)threadIdx.x;                  // entry within the view
    const bool live = k < V.count;
    uint8_t status = 1;
    float xf = 0.f, yf = 0.f, dist = 0.f, radius = 0.f;
    int32_t level = -1;
    int e = 0;
    if (live) {
        e = V.first + k;
        const int m = A.mp_index[e];
        const double px = A.mp_pos[3 * (size_t)m], py = A.mp_pos[3 * (size_t)m + 1], pz = A.mp_pos[3 * (size_t)m + 2];
        // reprojectToImage (keyframe.cpp:340-356) for the pinhole stand-in, as loop_ransac.hip's project()
        const double cxp = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(V.R[0], px), __dmul_rn(V.R[1], py)), __dmul_rn(V.R[2], pz)), V.t[0]);
        const double cyp = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(V.R[3], px), __dmul_rn(V.R[4], py)), __dmul_rn(V.R[5], pz)), V.t[1]);
        const double czp = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(V.R[6], px), __dmul_rn(V.R[7], py)), __dmul_rn(V.R[8], pz)), V.t[2]);
        const double u = __dadd_rn(__dmul_rn(V.fx, __ddiv_rn(cxp, czp)), V.cx);
        const double v = __dadd_rn(__dmul_rn(V.fy, __ddiv_rn(cyp, czp)), V.cy);
        const bool visible = czp > 0.0 && u >= 0.0 && u < V.w && v >= 0.0 && v < V.h;
        if (visible) {
            xf = (float)u; yf = (float)v;
            const float dmin = A.mp_min[m], dmax = A.mp_max[m];
            float dx = 0.f, dy = 0.f, dz = 0.f;
            bool in_range;
            if (V.mode == MS_GATE_SIM3) {                    // :585-591: the distance stays a double for the comparison
                const double dd = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(cxp, cxp), __dmul_rn(cyp, cyp)), __dmul_rn(czp, czp)));
                in_range = !(dd < (double)dmin || (double)dmax < dd);
                dist = (float)dd;                            // predictScaleLevel takes a float
            } else {                                         // :323-326, :449-457
                dx = (float)__dsub_rn(V.c[0], px); dy = (float)__dsub_rn(V.c[1], py); dz = (float)__dsub_rn(V.c[2], pz);
                dist = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
                in_range = !(dist < dmin || dmax < dist);
            }
            status = 2;
            if (in_range) {
                float cosv = 1.f;
                status = 0;
                if (V.mode != MS_GATE_SIM3) {
                    const float nx = A.mp_norm[3 * (size_t)m], ny = A.mp_norm[3 * (size_t)m + 1], nz = A.mp_norm[3 * (size_t)m + 2];
                    if (V.mode == MS_GATE_FUSE && nx == 0.f && ny == 0.f && nz == 0.f) status = 3;       // :460
                    else {
                        cosv = __fadd_rn(__fadd_rn(__fmul_rn(__fdiv_rn(dx, dist), nx), __fmul_rn(__fdiv_rn(dy, dist), ny)), __fmul_rn(__fdiv_rn(dz, dist), nz));
                        if (cosv < (V.mode == MS_GATE_SEARCH ? V.cos_limit : 0.5f)) status = 4;           // :329, :464
                    }
                }
                if (status == 0) {
                    // predictScaleLevel (map_point.cpp:174-183); the reference's int conversion of +inf / NaN is undefined: +inf -> top level, NaN -> 0
                    const float ratio = __fdiv_rn(dmax, dist);
                    const float q = __fdiv_rn(logf(ratio), logf(A.scale_factor));
                    const float cq = ceilf(q);
                    const int top = A.n_levels - 1;
                    level = !(cq > 0.f) ? 0 : (cq >= (float)top ? top : (int)cq);
                    const float sl = A.sf[level], sref = A.sf[A.n_levels / 2];
                    if (V.mode == MS_GATE_SEARCH) {
                        const float mul = cosv > 0.998f ? 0.625f : 1.f;                                   // :335-337
                        radius = __fdiv_rn(__fmul_rn(__fmul_rn(mul, V.threshold), sl), sref);              // :342
                    } else if (V.mode == MS_GATE_FUSE) {
                        radius = __fmul_rn(__fdiv_rn(__fmul_rn(V.threshold, sl), sref), 2.4477f);          // :470-471
                    } else {
                        radius = __fmul_rn(V.threshold, sl);                                              // :596
                    }
                }
            }
        }
    }
    // rank among the workgroup's kept entries, in entry order
    const bool kept = live && status == 0;
    int total;
    const int rank = block_rank<kBlock>(kept, s_wave, total);
    if (threadIdx.x == 0) A.blk_count[blockIdx.x] = total;
    if (live) {
        A.rank[e] = kept ? rank : -1;
        if (A.status) A.status[e] = status;
        A.x[e] = xf; A.y[e] = yf; A.radius[e] = radius; A.level[e] = level;
        if (A.dist) A.dist[e] = dist;
    }
}

__global__ __launch_bounds__(kBlock) void k_gate_offsets(const GateArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int v = blockIdx.x;
    const int blk0 = A.views[v].blk0, nblk = A.views[v].nblk;
    const int kept = block_offsets<kBlock>(A.blk_count + blk0, A.blk_off + blk0, nblk, s_wave);
    if (threadIdx.x == 0) A.n_kept[v] = kept;
}

__global__ __launch_bounds__(kBlock) void k_gate_pack(const GateArgs A) {
    const int2 blk = A.blocks[blockIdx.x];
    const GvDev *V = A.views + blk.x;
    const int k = blk.y + (int)threadIdx.x;
    if (k >= V->count) return;
    const int first = V->first, e = first + k;
    const int r = A.rank[e];
    if (r < 0) return;
    const size_t dst = (size_t)first + (size_t)A.blk_off[blockIdx.x] + (size_t)r;
    if (A.kept_entry) A.kept_entry[dst] = e;
    if (A.q_x) A.q_x[dst] = A.x[e];
    if (A.q_y) A.q_y[dst] = A.y[e];
    if (A.q_radius) A.q_radius[dst] = A.radius[e];
    const bool window = V->mode == MS_GATE_SIM3;             // :611
    const int lv = A.level[e];
    if (A.q_min_octave) A.q_min_octave[dst] = window ? lv - 1 : kNoWindowMin;
    if (A.q_max_octave) A.q_max_octave[dst] = window ? lv : kNoWindowMax;
    if (A.q_desc) {
        const uint4 *src = reinterpret_cast<const uint4 *>(A.mp_desc + 8 * (size_t)A.mp_index[e]);
        uint4 *out = reinterpret_cast<uint4 *>(A.q_desc + 8 * dst);
        const uint4 lo = src[0], hi = src[1];
        out[0] = lo; out[1] = hi;
    }
}

}  // namespace

extern "C" int ms_project_gate(ms_ctx *c, const double *mp_pos, const float *mp_norm, const float *mp_min_dist, const float *mp_max_dist,
                               const uint32_t *mp_desc, int n_mp, const int32_t *mp_index, int n_entries, const ms_gate_view *views, int n_views,
                               const float *scale_factors, int n_levels, float scale_factor,
                               uint8_t *status, float *x, float *y, float *dist, int32_t *level, float *radius,
                               int32_t *kept_entry, float *q_x, float *q_y, float *q_radius, int32_t *q_min_octave, int32_t *q_max_octave,
                               uint32_t *q_desc, int32_t *n_kept) {
    if (!c) return MS_ERR_INVALID;
    if (n_mp < 0 || n_entries < 0 || n_views < 0 || (n_views > 0 && (!views || !n_kept)) || (n_entries > 0 && !mp_index) || !scale_factors)
        return ms_fail(c, MS_ERR_INVALID, "project gate: bad arguments");
    if (n_levels < 1 || !(scale_factor > 0.f) || scale_factor == 1.f || !std::isfinite(scale_factor))
        return ms_fail(c, MS_ERR_INVALID, "project gate: %d levels, scale factor %g", n_levels, (double)scale_factor);
    if (n_levels > MS_GATE_MAX_LEVELS || n_views > MS_GATE_MAX_VIEWS || n_entries >= MS_GATE_MAX_ENTRIES)
        return ms_fail(c, MS_ERR_CAPACITY, "project gate: %d levels / %d views / %d entries, caps %d / %d / below %d", n_levels, n_views, n_entries,
                       MS_GATE_MAX_LEVELS, MS_GATE_MAX_VIEWS, MS_GATE_MAX_ENTRIES);
    if (n_entries > 0 && (!mp_pos || !mp_min_dist || !mp_max_dist)) return ms_fail(c, MS_ERR_INVALID, "project gate: missing map-point table");
    if ((reinterpret_cast<uintptr_t>(mp_desc) | reinterpret_cast<uintptr_t>(q_desc)) & 15u)
        return ms_fail(c, MS_ERR_INVALID, "project gate: descriptor arrays must be 16-byte aligned");
    if (q_desc && !mp_desc && n_entries > 0) return ms_fail(c, MS_ERR_INVALID, "project gate: q_desc needs mp_desc");
    long long n_blocks = 0;
    bool need_norm = false;
    for (int v = 0; v < n_views; ++v) {
        const ms_gate_view &V = views[v];
        if (V.mode != MS_GATE_SEARCH && V.mode != MS_GATE_FUSE && V.mode != MS_GATE_SIM3) return ms_fail(c, MS_ERR_INVALID, "project gate: view %d: bad mode %d", v, V.mode);
        if (V.cam.width < 1 || V.cam.height < 1) return ms_fail(c, MS_ERR_INVALID, "project gate: view %d: bad camera", v);
        if (V.count < 0 || V.first < 0 || (long long)V.first + V.count > n_entries)
            return ms_fail(c, MS_ERR_INVALID, "project gate: view %d: slice [%d, %d + %d) outside [0, %d)", v, V.first, V.first, V.count, n_entries);
        n_blocks += ms_div_up(V.count, kBlock);
        need_norm |= V.mode != MS_GATE_SIM3 && V.count > 0;
        for (int i = V.first; i < V.first + V.count; ++i)       // entries in no slice are never read, so only the slices are checked
            if (mp_index[i] < 0 || mp_index[i] >= n_mp) return ms_fail(c, MS_ERR_INVALID, "project gate: entry %d: map point %d outside [0, %d)", i, mp_index[i], n_mp);
    }
    if (need_norm && !mp_norm) return ms_fail(c, MS_ERR_INVALID, "project gate: missing map-point normals");
    if (n_views == 0) return MS_OK;
    MsRange range("projectGate");
    // upload block: views | block table | mp_index | scale factors | (host only) the views ordered by `first`
    const size_t nb = (size_t)n_blocks, nv = (size_t)n_views, ne = (size_t)n_entries;
    MsLayout up;
    const auto l_view = up.array<GvDev>(nv);
    const auto l_blk = up.array<int2>(nb);
    const auto l_idx = up.array<int32_t>(ne);
    const auto l_sf = up.array<float>((size_t)n_levels);
    MsLayout host = up, dev = up;
    const auto l_order = host.array<int32_t>(nv), l_down = host.array<int32_t>(nv);
    // device-only block: n_kept | rank | block counts | block offsets | stand-ins for per-entry outputs the caller does not want
    const auto l_nk = dev.array<int32_t>(nv), l_rank = dev.array<int32_t>(ne), l_bc = dev.array<int32_t>(nb), l_bo = dev.array<int32_t>(nb);
    const auto l_x = dev.array<float>(ne), l_y = dev.array<float>(ne), l_r = dev.array<float>(ne);
    const auto l_l = dev.array<int32_t>(ne);
    MS_HIP(c, hipSetDevice(c->device));
    int rc;
    MsWorkspace &W = c->ws[MS_WS_PROJECT_GATE];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    void *hs = W.host;
    // overlapping slices: order the non-empty views by `first` (before anything is allocated on the device or written)
    int32_t *order = l_order.at(hs);
    int n_live = 0;
    for (int v = 0; v < n_views; ++v) if (views[v].count > 0) order[n_live++] = v;
    std::sort(order, order + n_live, [&](int32_t a, int32_t b) { return views[a].first < views[b].first; });
    for (int i = 1; i < n_live; ++i)
        if (views[order[i - 1]].first + views[order[i - 1]].count > views[order[i]].first)
            return ms_fail(c, MS_ERR_INVALID, "project gate: the slices of views %d and %d overlap", order[i - 1], order[i]);
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *ds = W.dev;
    GvDev *hv = l_view.at(hs);
    int2 *hb = l_blk.at(hs);
    int at = 0;
    for (int v = 0; v < n_views; ++v) {
        const ms_gate_view &V = views[v];
        GvDev &D = hv[v];
        std::memcpy(D.R, V.R_cw, sizeof(D.R));
        std::memcpy(D.t, V.t_cw, sizeof(D.t));
        for (int j = 0; j < 3; ++j) {                        // worldToCameraMatrixCameraCenter: -R^T t, summed left to right
            const double a = V.R_cw[j] * V.t_cw[0], b = V.R_cw[3 + j] * V.t_cw[1], d = V.R_cw[6 + j] * V.t_cw[2];
            D.c[j] = -((a + b) + d);
        }
        D.fx = V.cam.fx; D.fy = V.cam.fy; D.cx = V.cam.cx; D.cy = V.cam.cy; D.w = (double)V.cam.width; D.h = (double)V.cam.height;
        D.threshold = V.threshold; D.cos_limit = V.view_cos_limit;
        D.mode = V.mode; D.first = V.first; D.count = V.count;
        D.blk0 = at; D.nblk = ms_div_up(V.count, kBlock); D.pad = 0;
        for (int b = 0; b < D.nblk; ++b) hb[at++] = make_int2(v, b * kBlock);
    }
    l_idx.fill(hs, mp_index);
    l_sf.fill(hs, scale_factors);
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    GateArgs A;
    A.views = l_view.at(ds); A.blocks = l_blk.at(ds); A.mp_index = l_idx.at(ds); A.sf = l_sf.at(ds);
    A.mp_pos = mp_pos; A.mp_norm = mp_norm; A.mp_min = mp_min_dist; A.mp_max = mp_max_dist; A.mp_desc = mp_desc;
    A.n_levels = n_levels; A.scale_factor = scale_factor;
    A.status = status; A.dist = dist;
    A.x = x ? x : l_x.at(ds);
    A.y = y ? y : l_y.at(ds);
    A.radius = radius ? radius : l_r.at(ds);
    A.level = level ? level : l_l.at(ds);
    A.rank = l_rank.at(ds); A.blk_count = l_bc.at(ds); A.blk_off = l_bo.at(ds); A.n_kept = l_nk.at(ds);
    A.kept_entry = kept_entry; A.q_x = q_x; A.q_y = q_y; A.q_radius = q_radius; A.q_min_octave = q_min_octave; A.q_max_octave = q_max_octave; A.q_desc = q_desc;
    if (nb > 0) {
        hipLaunchKernelGGL(k_gate, dim3((unsigned)nb), dim3(kBlock), 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_gate");
    }
    hipLaunchKernelGGL(k_gate_offsets, dim3((unsigned)n_views), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_gate_offsets");
    if (nb > 0 && (kept_entry || q_x || q_y || q_radius || q_min_octave || q_max_octave || q_desc)) {
        hipLaunchKernelGGL(k_gate_pack, dim3((unsigned)nb), dim3(kBlock), 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_gate_pack");
    }
    MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_nk.at(ds), l_nk.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(n_kept, l_down.at(hs), l_down.bytes());
    return MS_OK;
}
