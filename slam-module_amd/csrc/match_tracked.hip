// match_tracked.hip -- matchTrackedFeatures (mapper_helpers.cpp:67-142) on the device map tables: the first step of
// addKeyframeCommonInner and the only one that runs for every frame.
//   ms_match_tracked         the walk of :76-141 over the current frame's keypoints: per keypoint its track's map point is looked up,
//                            bound (just tracked, or TRIANGULATED and through isInFrustum and checkReprojectionError) or created
//   ms_match_tracked_finish  what follows triangulateMapPointFirstLastObs (:90) for the just-tracked rows: the updateDescriptor of :811
//                            for the rows that are now UNSURE, and the rows of the refresh of :121-124
//
// One launch each: ONE workgroup of 256 lanes walks its positions in trips of 256, block_rank (ms_scan.h) inside a trip and running
// counts carried across the trips -- the shape of k_gate_offsets' block_offsets.  A per-frame call pays for launches, not for occupancy.
//
// k_match_tracked, phase A: every lane decides its keypoint's outcome from the tables as they are, ranks it among the created / just
// tracked / checked keypoints before it, counts the violations and writes nothing but `outcome` and its own two workspace words.  Behind
// a barrier phase B writes the tables and the packed lists -- only when phase A counted no violation and new_rows holds every created
// point.  Each lane reads in B only what it wrote itself in A; nothing B writes is read by A of another lane, because A is over.
//
// The two gates are restated here (DESIGN 9.4 SEARCH, statuses 1 / 2 / 4; 9.7 checkReprojectionError "with the reference's types"), every
// floating-point operation a single rounded IEEE operation (-ffp-contract=off; *_rn where project_gate.hip pins the order), no logf or
// other function whose last bit is the implementation's: every output is an integer, a copy or a comparison of exactly rounded values.
//
// Two keypoints cannot resolve to the same row: a present track t has mp_track[row] == t, and the validation holds the track ids of
// kp_track distinct; a created row that is also a present one is live, which is counted.
#include "ms_internal.h"
#include "ms_scan.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr double kChi2Inv2D = 5.991;     // CHI2_INV2D, mapper_helpers.cpp:26
constexpr int kDown = 8;                 // created, just tracked, checked, frustum, reprojection | violations: bound entry, live new row, octave

struct FrameDev {                        // the frame as the kernel sees it, copied to LDS once
    double P[12], c[3];                  // rows 0-2 of poseCW; c = -R^T t
    double fx, fy, cx, cy, w, h;
    float sigma[MS_TRI_MAX_LEVELS];
    float rel_thr, cos_limit;
    int32_t focal, n_levels, slot, desc_base, track_base, pad;
};
static_assert(sizeof(FrameDev) % 8 == 0, "FrameDev is copied to LDS by words");

struct TrackArgs {
    int32_t *kf_mp;
    uint8_t *mp_flags, *mp_live;
    const double *mp_pos;
    const float *mp_norm, *mp_min, *mp_max;
    uint32_t *mp_desc;
    int32_t *mp_track, *track_row;
    const float *kp_x, *kp_y;
    const int32_t *kp_octave;
    const uint32_t *desc_pool;
    const FrameDev *frame;
    const int32_t *kp_track, *new_rows;  // uploaded: [n_kp], [n_new]
    int32_t *row_of, *dst_of;            // workspace [n_kp]: the keypoint's row | its position in its packed list
    uint8_t *outcome;
    int32_t *created_rows, *created_kp, *tracked_rows, *checked_rows;
    int32_t *down;                       // [kDown]
    int32_t stride, n_mp, n_kp, n_new;
};

// isInFrustum (keyframe.cpp:247-262; the SEARCH gates of project_gate.hip) and then checkReprojectionError (mapper_helpers.cpp:576-598;
// check_observation of triangulate.hip) of map point r against keypoint (x, y, octave): 3 bound | 4 outside the frustum | 5 reprojection
__device__ int check_tracked(const TrackArgs &A, const FrameDev &V, int r, float x, float y, int octave) {
    const double px = A.mp_pos[3 * (size_t)r], py = A.mp_pos[3 * (size_t)r + 1], pz = A.mp_pos[3 * (size_t)r + 2];
    const double cxp = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(V.P[0], px), __dmul_rn(V.P[1], py)), __dmul_rn(V.P[2], pz)), V.P[3]);
    const double cyp = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(V.P[4], px), __dmul_rn(V.P[5], py)), __dmul_rn(V.P[6], pz)), V.P[7]);
    const double czp = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(V.P[8], px), __dmul_rn(V.P[9], py)), __dmul_rn(V.P[10], pz)), V.P[11]);
    const double u = __dadd_rn(__dmul_rn(V.fx, __ddiv_rn(cxp, czp)), V.cx);
    const double v = __dadd_rn(__dmul_rn(V.fy, __ddiv_rn(cyp, czp)), V.cy);
    if (!(czp > 0.0 && u >= 0.0 && u < V.w && v >= 0.0 && v < V.h)) return 4;                            // reproject, :249
    const float dx = (float)__dsub_rn(V.c[0], px), dy = (float)__dsub_rn(V.c[1], py), dz = (float)__dsub_rn(V.c[2], pz);
    const float dist = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
    if (dist < A.mp_min[r] || A.mp_max[r] < dist) return 4;                                              // :254
    const float nx = A.mp_norm[3 * (size_t)r], ny = A.mp_norm[3 * (size_t)r + 1], nz = A.mp_norm[3 * (size_t)r + 2];
    const float cosv = __fadd_rn(__fadd_rn(__fmul_rn(__fdiv_rn(dx, dist), nx), __fmul_rn(__fdiv_rn(dy, dist), ny)), __fmul_rn(__fdiv_rn(dz, dist), nz));
    if (cosv < V.cos_limit) return 4;                                                                    // :258
    // checkReprojectionError: the same camera point and pixel, so it is visible; the error in float32, the bound in float64
    const float du = __fsub_rn((float)u, x), dv = __fsub_rn((float)v, y);
    const float sq = __fadd_rn(__fmul_rn(du, du), __fmul_rn(dv, dv));
    const double rel_sigma_base = (double)__fmul_rn((float)V.focal, V.rel_thr);
    const double sigma2 = __dmul_rn(__dmul_rn((double)__fdiv_rn(V.sigma[octave], V.sigma[V.n_levels / 2]), rel_sigma_base), rel_sigma_base);
    return (double)sq <= __dmul_rn(kChi2Inv2D, sigma2) ? 3 : 5;
}

// the workgroup's sum of one int per lane, the same in every lane; ends with a barrier (s_wave is free again)
__device__ __forceinline__ int block_sum(int v, int32_t *s_wave) {
    int total;
    block_exclusive<kBlock>(v, s_wave, total);
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(kBlock) void k_match_tracked(const TrackArgs A) {
    __shared__ FrameDev V;
    __shared__ int32_t s_wave[3][kBlock / 64];
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(A.frame);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&V);
        for (int i = threadIdx.x; i < (int)(sizeof(FrameDev) / 4); i += kBlock) dst[i] = src[i];
    }
    __syncthreads();
    int32_t *row = A.kf_mp + (size_t)V.slot * A.stride;
    // ---- phase A
    int n_created = 0, n_tracked = 0, n_checked = 0;         // running counts, the same in every lane
    int n_frustum = 0, n_repro = 0, v_bound = 0, v_live = 0, v_octave = 0;      // this lane's
    for (int j0 = 0; j0 < A.n_kp; j0 += kBlock) {
        const int j = j0 + (int)threadIdx.x;
        int outcome = 0, r = -1;
        if (j < A.n_kp) {
            const int32_t t = A.kp_track[j];
            if (t >= 0) {                                                                                // :78
                const size_t e = (size_t)V.slot * A.stride + j;
                const int32_t octave = A.kp_octave[e];
                const bool octave_ok = (uint32_t)octave < (uint32_t)V.n_levels;
                v_octave += !octave_ok;
                r = A.track_row[t - V.track_base];
                const bool present = (uint32_t)r < (uint32_t)A.n_mp && A.mp_live[r] != 0 && A.mp_track[r] == t;          // :81
                if (!present) { outcome = V.desc_base >= 0 ? 1 : 6; r = -1; }                          // :126
                else if ((A.mp_flags[r] & 1) == 0) outcome = 2;                                          // :85
                else outcome = octave_ok ? check_tracked(A, V, r, A.kp_x[e], A.kp_y[e], octave) : 5;     // :96-113
            }
        }
        int t_created, t_tracked, t_checked;
        const int k_created = n_created + block_rank<kBlock>(outcome == 1, s_wave[0], t_created);
        const int k_tracked = n_tracked + block_rank<kBlock>(outcome == 2, s_wave[1], t_tracked);
        const int k_checked = n_checked + block_rank<kBlock>(outcome == 3, s_wave[2], t_checked);
        n_created += t_created; n_tracked += t_tracked; n_checked += t_checked;
        if (j < A.n_kp) {
            int dst = -1;
            if (outcome == 1) {
                dst = k_created;
                if (k_created < A.n_new) { r = A.new_rows[k_created]; v_live += A.mp_live[r] != 0; }     // in [0, n_mp): validated
            } else if (outcome == 2) dst = k_tracked;
            else if (outcome == 3) dst = k_checked;
            if (outcome >= 1 && outcome <= 3) v_bound += (uint32_t)row[j] < (uint32_t)A.n_mp;            // keyframe.cpp:275
            n_frustum += outcome == 4; n_repro += outcome == 5;
            A.outcome[j] = (uint8_t)outcome;
            A.row_of[j] = r; A.dst_of[j] = dst;
        }
        __syncthreads();                                     // s_wave is written again in the next trip
    }
    n_frustum = block_sum(n_frustum, s_wave[0]); n_repro = block_sum(n_repro, s_wave[0]);
    v_bound = block_sum(v_bound, s_wave[0]); v_live = block_sum(v_live, s_wave[0]); v_octave = block_sum(v_octave, s_wave[0]);
    if (threadIdx.x == 0) {
        A.down[0] = n_created; A.down[1] = n_tracked; A.down[2] = n_checked; A.down[3] = n_frustum; A.down[4] = n_repro;
        A.down[5] = v_bound; A.down[6] = v_live; A.down[7] = v_octave;
    }
    if (v_bound | v_live | v_octave || n_created > A.n_new) return;      // the same in every lane
    // ---- phase B (the last barrier above separates it from every read of phase A)
    for (int j = threadIdx.x; j < A.n_kp; j += kBlock) {     // the lane that decided keypoint j
        const int outcome = A.outcome[j];
        if (outcome < 1 || outcome > 3) continue;
        const int r = A.row_of[j], dst = A.dst_of[j];
        row[j] = r;                                                                                      // currentKeyframe.addObservation
        if (outcome == 1) {                                                                              // :128-137
            A.mp_live[r] = 1; A.mp_flags[r] = 0;
            const int32_t t = A.kp_track[j];
            A.mp_track[r] = t;
            A.track_row[t - V.track_base] = r;
            const uint4 *src = reinterpret_cast<const uint4 *>(A.desc_pool + 8 * ((size_t)V.desc_base + j));      // updateDescriptor of one observation
            uint4 *out = reinterpret_cast<uint4 *>(A.mp_desc + 8 * (size_t)r);
            const uint4 lo = src[0], hi = src[1];
            out[0] = lo; out[1] = hi;
            if (A.created_rows) A.created_rows[dst] = r;
            if (A.created_kp) A.created_kp[dst] = j;
        } else if (outcome == 2) {
            if (A.tracked_rows) A.tracked_rows[dst] = r;
        } else if (A.checked_rows) A.checked_rows[dst] = r;
    }
}

struct FinishArgs {
    ms_obs_lists lists;
    const uint8_t *mp_flags;
    const uint32_t *desc_pool;
    uint32_t *mp_desc;
    const int32_t *checked_rows;
    int32_t *refresh_rows, *down;
    int32_t n_rows, n_checked;
};

__global__ __launch_bounds__(kBlock) void k_match_finish(const FinishArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    int n_kept = 0;
    for (int i0 = 0; i0 < A.n_rows; i0 += kBlock) {
        const int i = i0 + (int)threadIdx.x;
        bool kept = false;
        int r = 0;
        if (i < A.n_rows) {
            r = A.lists.rows[i];
            const uint8_t f = A.mp_flags[r];
            kept = (f & 1) != 0;                                                                         // :121
            if (f == 2 && A.desc_pool && A.lists.obs_desc) {
                // updateDescriptor (:811) of an UNSURE point: it has exactly two observations (:810).  map_point.cpp:101-113 takes each
                // descriptor's median distance at index (unsigned)(0.5 * (n - 1)) = 0 of its sorted distances, which is the distance to
                // itself, 0, for both; the scan keeps the first index whose median is strictly below the best so far (256 at the start):
                // the FIRST descriptor.  With one descriptor it is that one; with none the point keeps what it has (:86).
                for (int o = A.lists.obs_start[i]; o < A.lists.obs_start[i + 1]; ++o) {
                    const int32_t d = A.lists.obs_desc[o];
                    if (d == -1) continue;
                    const uint4 *src = reinterpret_cast<const uint4 *>(A.desc_pool + 8 * (size_t)d);
                    uint4 *out = reinterpret_cast<uint4 *>(A.mp_desc + 8 * (size_t)r);
                    const uint4 lo = src[0], hi = src[1];
                    out[0] = lo; out[1] = hi;
                    break;
                }
            }
        }
        int total;
        const int rank = block_rank<kBlock>(kept, s_wave, total);
        if (kept) A.refresh_rows[n_kept + rank] = r;
        n_kept += total;
        __syncthreads();
    }
    for (int i = threadIdx.x; i < A.n_checked; i += kBlock) A.refresh_rows[n_kept + i] = A.checked_rows[i];
    if (threadIdx.x == 0) A.down[0] = n_kept + A.n_checked;
}

}  // namespace

extern "C" int ms_match_tracked(ms_ctx *c, int32_t *kf_mp, int n_kf, int stride, uint8_t *mp_flags, uint8_t *mp_live, const double *mp_pos, const float *mp_norm,
                                const float *mp_min_dist, const float *mp_max_dist, uint32_t *mp_desc, int32_t *mp_track, int n_mp, const float *kp_x, const float *kp_y,
                                const int32_t *kp_octave, const uint32_t *desc_pool, int n_pool, int32_t *track_row, int n_track, const ms_tracked_frame *f,
                                const int32_t *kp_track, int n_kp, const int32_t *new_rows, int n_new, uint8_t *outcome, int32_t *created_rows, int32_t *created_kp,
                                int32_t *tracked_rows, int32_t *checked_rows, int32_t *counts) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_match_tracked_check(kf_mp, n_kf, stride, mp_flags, mp_live, mp_pos, mp_norm, mp_min_dist, mp_max_dist, mp_desc, mp_track, n_mp, kp_x, kp_y, kp_octave,
                                     desc_pool, n_pool, track_row, n_track, f, kp_track, n_kp, new_rows, n_new, outcome, counts, c->err, sizeof(c->err))))
        return rc;
    std::memset(counts, 0, 5 * sizeof(int32_t));
    if (n_kp == 0) return MS_OK;
    MsRange range("matchTrackedFeatures");
    const size_t nk = (size_t)n_kp;
    // upload block: the frame record | kp_track | new_rows; then (host only) the result block
    MsLayout up;
    const auto l_frame = up.array<FrameDev>(1);
    const auto l_track = up.array<int32_t>(nk), l_new = up.array<int32_t>((size_t)n_new);
    MsLayout host = up, dev = up;
    const auto l_down = host.array<int32_t>(kDown);
    // device-only block: results | the keypoints' rows | their positions in the packed lists
    const auto l_res = dev.array<int32_t>(kDown), l_row = dev.array<int32_t>(nk), l_dst = dev.array<int32_t>(nk);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_MATCH_TRACKED];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    FrameDev &D = *l_frame.at(hs);
    std::memset(&D, 0, sizeof(D));
    std::memcpy(D.P, f->pose, sizeof(D.P));
    for (int j = 0; j < 3; ++j) {                            // worldToCameraMatrixCameraCenter: -R^T t, summed left to right (as ms_project_gate)
        const double a = f->pose[j] * f->pose[3], b = f->pose[4 + j] * f->pose[7], d = f->pose[8 + j] * f->pose[11];
        D.c[j] = -((a + b) + d);
    }
    D.fx = f->cam.fx; D.fy = f->cam.fy; D.cx = f->cam.cx; D.cy = f->cam.cy; D.w = (double)f->cam.width; D.h = (double)f->cam.height;
    std::memcpy(D.sigma, f->level_sigma_sq, (size_t)f->n_levels * sizeof(float));
    D.rel_thr = f->rel_reprojection_threshold; D.cos_limit = f->view_cos_limit;
    D.focal = f->focal; D.n_levels = f->n_levels; D.slot = f->slot; D.desc_base = f->desc_base < 0 ? -1 : f->desc_base; D.track_base = f->track_base;
    l_track.fill(hs, kp_track);
    l_new.fill(hs, new_rows);
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    TrackArgs A{};
    A.kf_mp = kf_mp; A.mp_flags = mp_flags; A.mp_live = mp_live;
    A.mp_pos = mp_pos; A.mp_norm = mp_norm; A.mp_min = mp_min_dist; A.mp_max = mp_max_dist; A.mp_desc = mp_desc;
    A.mp_track = mp_track; A.track_row = track_row;
    A.kp_x = kp_x; A.kp_y = kp_y; A.kp_octave = kp_octave; A.desc_pool = desc_pool;
    A.frame = l_frame.at(ds); A.kp_track = l_track.at(ds); A.new_rows = l_new.at(ds);
    A.row_of = l_row.at(ds); A.dst_of = l_dst.at(ds);
    A.outcome = outcome;
    A.created_rows = created_rows; A.created_kp = created_kp; A.tracked_rows = tracked_rows; A.checked_rows = checked_rows;
    A.down = l_res.at(ds);
    A.stride = stride; A.n_mp = n_mp; A.n_kp = n_kp; A.n_new = n_new;
    hipLaunchKernelGGL(k_match_tracked, dim3(1), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_match_tracked");
    MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_res.at(ds), l_res.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *down = l_down.at(hs);
    std::memcpy(counts, down, 5 * sizeof(int32_t));
    if (down[5] | down[6] | down[7])
        return ms_fail(c, MS_ERR_INVALID, "match tracked: %d bound keypoints whose kf_mp entry is already valid, %d new rows that are live, %d octaves outside [0, %d) (nothing written)",
                       down[5], down[6], down[7], f->n_levels);
    if (down[0] > n_new) return ms_fail(c, MS_ERR_CAPACITY, "match tracked: the frame creates %d map points, new_rows holds %d (nothing written)", down[0], n_new);
    return MS_OK;
}

extern "C" int ms_match_tracked_finish(ms_ctx *c, const ms_obs_lists *lists, int n_rows, const uint8_t *mp_flags, const uint32_t *desc_pool, uint32_t *mp_desc, int n_mp,
                                       const int32_t *checked_rows, int n_checked, int append_checked, int32_t *refresh_rows, int cap_refresh, int32_t *n_refresh) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_match_tracked_finish_check(lists, n_rows, mp_flags, desc_pool, mp_desc, n_mp, checked_rows, n_checked, append_checked, refresh_rows, cap_refresh, n_refresh,
                                            c->err, sizeof(c->err))))
        return rc;
    *n_refresh = 0;
    const int n_append = append_checked ? n_checked : 0;
    if (n_rows + n_append == 0) return MS_OK;
    MsRange range("matchTrackedFinish");
    MsLayout host, dev;
    const auto l_down = host.array<int32_t>(1), l_res = dev.array<int32_t>(1);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_MATCH_TRACKED];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    FinishArgs A{};
    if (lists) A.lists = *lists;
    A.mp_flags = mp_flags; A.desc_pool = desc_pool; A.mp_desc = mp_desc;
    A.checked_rows = checked_rows; A.refresh_rows = refresh_rows; A.down = l_res.at(W.dev);
    A.n_rows = n_rows; A.n_checked = n_append;
    hipLaunchKernelGGL(k_match_finish, dim3(1), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_match_finish");
    MS_HIP(c, hipMemcpyAsync(l_down.at(W.host), l_res.at(W.dev), l_res.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    *n_refresh = *l_down.at(W.host);
    return MS_OK;
}
