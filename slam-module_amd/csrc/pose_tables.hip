// pose_tables.hip -- poseBundleAdjust (bundle_adjuster.cpp:396-491) on the device map tables: the step that runs on every frame that
// is not a keyframe, behind ms_match_tracked, without the host ever seeing the frame's map points.
//   k_pose_gather   :403-407, :453-480: ONE workgroup walks the frame's kf_mp row in trips of 256 and writes the inputs of a pose-only solver handle
//                   (ms_ba_pose_tables_create, ba.hip) where k_ba_pose_only reads them: the two poses, the kept points, their observations,
//                   the odometry edge and the descriptor's sizes
//   k_ba_pose_only  the unchanged solver, on that problem
//   k_pose_apply    :485-489: the decision (enough points, a finite solve) and, if it falls that way, kf_pose[slot]; the small result record
// The frame travels as kernel arguments: nothing is uploaded.  The compaction keeps keypoint order through the shared block rank (ms_scan.h) with the
// count carried across trips; integer arithmetic decides every position, there is no atomic, and the float64 expressions are those of ba_window.hip
// (ba_window_dev.h), evaluated as written.
#include "ms_internal.h"
#include "ms_scan.h"
#include "ba_window_dev.h"
#include <cmath>
#include <cstring>

struct ms_pose_tables {
    ms_ctx *ctx = nullptr;
    ms_ba *ba = nullptr;
    MsBaPoseIo io{};
    int cap = 0, n_levels = 0;
    void *dev = nullptr;                 // the level sigmas | the result record
    float *d_sigma = nullptr;
    double *d_rec = nullptr;
    int last_n = 0;                      // observations the last gather wrote (0: none, or a call that ended in an error)
};

namespace {

constexpr int kBlock = 256;
// the result record, doubles: kept keypoints | kept keypoints with an octave outside the levels | ran | - | the solver's 16 status words | pose 0 | chi2 [cap]
constexpr int kRecN = 0, kRecBad = 1, kRecRan = 2, kRecStats = 4, kRecPose = 20, kRecChi2 = 27;

struct GatherArgs {
    const int32_t *kf_mp;
    const uint8_t *mp_flags, *mp_live;
    const double *mp_pos, *kf_pose;
    const float *kp_x, *kp_y;
    const int32_t *kp_octave;
    const float *sigma;
    MsBaPoseIo io;
    double *rec;
    double fx, fy, cx, cy, huber;
    double edge_meas[7], edge_info[36];
    int32_t focal, slot, prev_slot, n_kp, stride, n_mp, n_levels, cap, min_visible, max_iters;
};

__global__ __launch_bounds__(kBlock) void k_pose_gather(const GatherArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int tid = (int)threadIdx.x;
    const size_t row0 = (size_t)A.slot * A.stride;
    int n = 0;                                               // kept so far: the carry into the next trip
    bool bad = false;
    for (int j0 = 0; j0 < A.n_kp; j0 += kBlock) {
        const int j = j0 + tid;
        int32_t r = -1;
        bool kept = false;
        if (j < A.n_kp) {
            r = A.kf_mp[row0 + j];
            kept = (uint32_t)r < (uint32_t)A.n_mp && (!A.mp_live || A.mp_live[r] != 0) && (A.mp_flags[r] & 1) != 0;      // PRESENT and TRIANGULATED, :404, :455-461
        }
        int total;
        const int k = n + block_rank<kBlock>(kept, s_wave, total);
        if (kept) {
            int32_t octave = A.kp_octave[row0 + j];
            if ((uint32_t)octave >= (uint32_t)A.n_levels) { bad = true; octave = octave < 0 ? 0 : A.n_levels - 1; }
            if (k < A.cap) {
                for (int a = 0; a < 3; ++a) A.io.point0[3 * (size_t)k + a] = A.mp_pos[3 * (size_t)r + a];
                A.io.obs_point[k] = k;
                A.io.obs_pose[k] = 0;
                A.io.obs_uv[2 * (size_t)k] = obs_normalised(A.kp_x[row0 + j], A.cx, A.fx);
                A.io.obs_uv[2 * (size_t)k + 1] = obs_normalised(A.kp_y[row0 + j], A.cy, A.fy);
                A.io.obs_info[k] = obs_information(A.focal, A.sigma[octave]);
            }
        }
        n += total;
        __syncthreads();                                     // s_wave is written again by the next trip
    }
    int n_bad;
    block_rank<kBlock>(bad, s_wave, n_bad);
    // the vertices and the edge: pose 0 = the frame (free), pose 1 = the previous keyframe (fixed), :424-449
    if (tid < 2) pose_of_table(A.kf_pose + 12 * (size_t)(tid == 0 ? A.slot : A.prev_slot), A.io.pose0 + 7 * tid);
    if (tid >= 64 && tid < 64 + 7) A.io.edge_meas[tid - 64] = A.edge_meas[tid - 64];
    if (tid >= 128 && tid < 128 + 36) A.io.edge_info[tid - 128] = A.edge_info[tid - 128];
    if (tid == 0) {
        // a frame the apply will not write (too many points for the handle, a bad octave, too few points) is not iterated on: the solver evaluates it once
        const bool usable = n <= A.cap && n_bad == 0;
        A.io.edge_i[0] = 0; A.io.edge_j[0] = 1;
        *A.io.n_point = usable ? n : 0;
        *A.io.n_obs = usable ? n : 0;
        *A.io.max_iters = usable && n >= A.min_visible ? A.max_iters : 0;
        *A.io.huber = A.huber;
        A.rec[kRecN] = (double)n;
        A.rec[kRecBad] = (double)n_bad;
    }
}

struct ApplyArgs {
    MsBaPoseIo io;
    double *rec, *kf_pose;
    int32_t slot, cap, min_visible, want_chi2;
};

__global__ __launch_bounds__(kBlock) void k_pose_apply(const ApplyArgs A) {
    const int tid = (int)threadIdx.x;
    const int n = (int)A.rec[kRecN];
    const bool usable = n <= A.cap && A.rec[kRecBad] == 0.0;
    const bool ran = usable && n >= A.min_visible && A.io.stats[6] != 0.0;       // [6]: the solve ended in a finite state
    if (tid == 0) {
        if (ran) write_pose(A.io.pose, A.kf_pose + 12 * (size_t)A.slot);         // applyBundleAdjustResults, :485-489: the frame's pose alone
        A.rec[kRecRan] = ran ? 1.0 : 0.0;
        A.rec[kRecRan + 1] = 0.0;
    }
    if (tid >= 64 && tid < 64 + 16) A.rec[kRecStats + tid - 64] = A.io.stats[tid - 64];
    if (tid >= 128 && tid < 128 + 7) A.rec[kRecPose + tid - 128] = A.io.pose[tid - 128];
    if (A.want_chi2 && usable)
        for (int i = tid; i < n; i += kBlock) A.rec[kRecChi2 + i] = A.io.chi2_obs[i];
}

}  // namespace

extern "C" int ms_pose_tables_create(ms_ctx *c, int cap_obs, const float *level_sigma_sq, int n_levels, ms_pose_tables **out) {
    if (!c || !out) return MS_ERR_INVALID;
    *out = nullptr;
    if (cap_obs < 0 || cap_obs > MS_COVIS_MAX_STRIDE) return ms_fail(c, MS_ERR_INVALID, "pose tables: capacity %d outside [0, %d]", cap_obs, MS_COVIS_MAX_STRIDE);
    if (!level_sigma_sq || n_levels < 1 || n_levels > MS_TRI_MAX_LEVELS) return ms_fail(c, MS_ERR_INVALID, "pose tables: %d levels outside [1, %d], or no level_sigma_sq", n_levels, MS_TRI_MAX_LEVELS);
    for (int l = 0; l < n_levels; ++l)
        if (!(std::isfinite(level_sigma_sq[l]) && level_sigma_sq[l] > 0.f)) return ms_fail(c, MS_ERR_INVALID, "pose tables: level_sigma_sq[%d] = %g", l, (double)level_sigma_sq[l]);
    MS_HIP(c, hipSetDevice(c->device));
    ms_pose_tables *h = new ms_pose_tables();
    ++g_ms_host_allocs;
    h->ctx = c; h->cap = cap_obs; h->n_levels = n_levels;
    int rc = ms_ba_pose_tables_create(c, cap_obs, &h->ba, &h->io);
    if (rc != MS_OK) { delete h; return rc; }
    MsLayout dev;
    const auto l_sigma = dev.array<float>((size_t)n_levels);
    const auto l_rec = dev.array<double>((size_t)kRecChi2 + (size_t)cap_obs);
    hipError_t e = hipMalloc(&h->dev, dev.end);
    ++g_ms_host_allocs;
    if (e == hipSuccess) {
        h->d_sigma = l_sigma.at(h->dev); h->d_rec = l_rec.at(h->dev);
        e = hipMemcpyAsync(h->d_sigma, level_sigma_sq, l_sigma.bytes(), hipMemcpyHostToDevice, c->stream);     // once, here
        if (e == hipSuccess) e = hipMemsetAsync(h->d_rec, 0, l_rec.bytes(), c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (e == hipSuccess && ms_pinned(c, l_rec.bytes()) != MS_OK) e = hipErrorOutOfMemory;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ms_pose_tables_destroy(h);
        return ms_fail(c, MS_ERR_HIP, "pose tables: device setup failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return MS_OK;
}

extern "C" void ms_pose_tables_destroy(ms_pose_tables *h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    if (h->ba) ms_ba_destroy(h->ba);
    if (h->dev) { (void)hipStreamSynchronize(h->ctx->stream); (void)hipFree(h->dev); }
    delete h;
}

extern "C" int ms_pose_tables_solve(ms_pose_tables *h, const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const double *mp_pos,
                                    int n_mp, const float *kp_x, const float *kp_y, const int32_t *kp_octave, double *kf_pose, const ms_pose_tables_frame *f,
                                    ms_pose_tables_out *out, double *chi2) {
    if (!h) return MS_ERR_INVALID;
    ms_ctx *c = h->ctx;
    int rc;
    if ((rc = ms_pose_tables_solve_check(kf_mp, n_kf, stride, mp_flags, mp_live, mp_pos, n_mp, kp_x, kp_y, kp_octave, kf_pose, f, out, c->err, sizeof(c->err)))) return rc;
    out->ran = 0; out->n_triangulated = 0;
    h->last_n = 0;
    if (f->prev_slot == -1) return MS_OK;                    // :430-432
    MsRange range("poseBundleAdjust");
    MS_HIP(c, hipSetDevice(c->device));
    const size_t rec_doubles = (size_t)kRecChi2 + (chi2 ? (size_t)h->cap : 0);
    if ((rc = ms_pinned(c, rec_doubles * sizeof(double)))) return rc;
    GatherArgs G{};
    G.kf_mp = kf_mp; G.mp_flags = mp_flags; G.mp_live = mp_live; G.mp_pos = mp_pos; G.kf_pose = kf_pose;
    G.kp_x = kp_x; G.kp_y = kp_y; G.kp_octave = kp_octave; G.sigma = h->d_sigma;
    G.io = h->io; G.rec = h->d_rec;
    G.fx = f->cam.fx; G.fy = f->cam.fy; G.cx = f->cam.cx; G.cy = f->cam.cy; G.huber = f->huber_delta;
    std::memcpy(G.edge_meas, f->edge_meas, sizeof(G.edge_meas));
    std::memcpy(G.edge_info, f->edge_info, sizeof(G.edge_info));
    G.focal = f->focal; G.slot = f->slot; G.prev_slot = f->prev_slot; G.n_kp = f->n_kp; G.stride = stride; G.n_mp = n_mp; G.n_levels = h->n_levels; G.cap = h->cap;
    G.min_visible = f->min_visible; G.max_iters = f->max_iters;
    hipLaunchKernelGGL(k_pose_gather, dim3(1), dim3(kBlock), 0, c->stream, G);
    MS_KERNEL_CHECK(c, "k_pose_gather");
    if ((rc = ms_ba_pose_tables_launch(h->ba))) return rc;
    ApplyArgs P{};
    P.io = h->io; P.rec = h->d_rec; P.kf_pose = kf_pose; P.slot = f->slot; P.cap = h->cap; P.min_visible = f->min_visible; P.want_chi2 = chi2 ? 1 : 0;
    hipLaunchKernelGGL(k_pose_apply, dim3(1), dim3(kBlock), 0, c->stream, P);
    MS_KERNEL_CHECK(c, "k_pose_apply");
    MS_HIP(c, hipMemcpyAsync(c->pinned, h->d_rec, rec_doubles * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if ((rc = ms_ba_pose_tables_wait(h->ba))) return rc;
    const double *rec = static_cast<const double *>(c->pinned), *st = rec + kRecStats;
    const int n = (int)rec[kRecN], n_bad = (int)rec[kRecBad];
    out->n_triangulated = n;
    for (int k = 0; k < 8; ++k) out->result.phase_cycles[k] = st[8 + k];
    out->result.iterations = (int)st[0]; out->result.trials = (int)st[1]; out->result.stopped_early = (int)st[2]; out->result.final_lambda = st[3];
    out->result.chi2_initial = st[4]; out->result.chi2_final = st[5];
    if (n > h->cap)
        return ms_fail(c, MS_ERR_CAPACITY, "pose tables: the frame has %d triangulated map points, the handle holds %d (kf_pose untouched)", n, h->cap);
    if (n_bad)
        return ms_fail(c, MS_ERR_INVALID, "pose tables: %d kept keypoints with an octave outside [0, %d) (kf_pose untouched)", n_bad, h->n_levels);
    h->last_n = n;
    if (n < f->min_visible) {                                // :410-412
        std::memcpy(out->pose, rec + kRecPose, 7 * sizeof(double));
        return MS_OK;
    }
    if (st[6] == 0) return ms_fail(c, MS_ERR_NUMERIC, "pose tables: the solve ended in a non-finite state (kf_pose untouched)");
    std::memcpy(out->pose, rec + kRecPose, 7 * sizeof(double));
    if (chi2 && n) std::memcpy(chi2, rec + kRecChi2, (size_t)n * sizeof(double));
    out->ran = (int)rec[kRecRan];
    return MS_OK;
}

extern "C" int ms_pose_tables_problem(ms_pose_tables *h, double *pose, double *point, int32_t *obs_point, int32_t *obs_pose, double *obs_uv, double *obs_info, int32_t *n) {
    if (!h || !n) return MS_ERR_INVALID;
    ms_ctx *c = h->ctx;
    MS_HIP(c, hipSetDevice(c->device));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const size_t k = (size_t)h->last_n;
    *n = h->last_n;
    if (pose) MS_HIP(c, hipMemcpy(pose, h->io.pose0, 14 * sizeof(double), hipMemcpyDeviceToHost));
    if (k && point) MS_HIP(c, hipMemcpy(point, h->io.point0, 3 * k * sizeof(double), hipMemcpyDeviceToHost));
    if (k && obs_point) MS_HIP(c, hipMemcpy(obs_point, h->io.obs_point, k * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (k && obs_pose) MS_HIP(c, hipMemcpy(obs_pose, h->io.obs_pose, k * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (k && obs_uv) MS_HIP(c, hipMemcpy(obs_uv, h->io.obs_uv, 2 * k * sizeof(double), hipMemcpyDeviceToHost));
    if (k && obs_info) MS_HIP(c, hipMemcpy(obs_info, h->io.obs_info, k * sizeof(double), hipMemcpyDeviceToHost));
    return MS_OK;
}
