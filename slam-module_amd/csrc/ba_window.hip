// ba_window.hip -- the local BA window of localBundleAdjust (bundle_adjuster.cpp:141-394) on the device map tables: the two
// steps around the solve that still needed MapPoint::observations and Keyframe::mapPoints on the host.
//   ms_ba_window_lists   :245-290: the observation lists ms_observation_lists left for the rows of ms_map_point_union become the arrays of
//                        an ms_ba_problem (pose, point, obs_point, obs_pose, obs_uv, obs_info) on the HOST; the observations of slots
//                        that are not local are dropped (:275); the kept edges' table entries stay on the device for the second step
//   ms_ba_window_apply   :376-390 (MS_BA_APPLY_LOCAL) or :326-331 (MS_BA_APPLY_NEIGHBOR): outlier observations erased in both
//                        directions, the UNSURE demotion, positions and poses written back into the tables
//
// Both are a stream compaction over the edges: one thread per listed observation / edge, a workgroup's kept lanes counted with block_rank,
// the workgroups' totals scanned by ONE workgroup with block_offsets (ms_scan.h; a second trip beyond 65 536 listed observations, 32 768 edges in the apply), then the same decision
// again with the offset known.  Every decision is made before anything is written: a call that ends in MS_ERR_CAPACITY has written nothing.
// The only atomic is the integer decrement of n_obs in the apply; the float64 expressions are evaluated as written (no contraction).
#include "ms_internal.h"
#include "ms_scan.h"
#include "ba_window_dev.h"
#include <cmath>
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int kEdgeBlock = 128;          // the apply's edge kernels: two waves per workgroup; its offsets scan takes a second trip beyond 32 768 edges
constexpr int kHead = 8;                 // int32 in front of the downloaded block: lists n_edge | n_current; apply n_erased | n_stale
constexpr double kChi2Threshold = 5.991; // CHI2_THRESHOLD, bundle_adjuster.cpp:378

// ------------------------------------------------------------------------------------------------ gather
struct GatherArgs {
    const double *kf_pose, *mp_pos;
    ms_obs_lists lists;                  // rows, obs_start, obs_kf, obs_kp, obs_x, obs_y, obs_octave are read
    const int32_t *pose_index;           // [n_kf] the slot's position in local_slot, -1 for a slot that is not local
    const int32_t *local_slot, *focal;   // [n_local]
    const double *cam;                   // [n_local * 4] fx, fy, cx, cy
    const float *sigma;                  // [n_levels]
    int32_t *blk_cnt, *blk_cur;          // [n_blocks] kept edges | edges of the current keyframe, per workgroup; then their offsets
    int32_t *head;                       // [kHead]
    double *pose, *point, *uv, *info;    // the block that goes down, on the device
    int32_t *o_point, *o_pose;
    ms_ba_window_dev win;
    int32_t n_kf, n_mp, n_rows, n_obs, n_local, n_levels, current, cap_edge, n_blocks;
};

// the pose index of the slot that observes o, -1 when that slot is not local
__device__ __forceinline__ int pose_of(const GatherArgs &A, int o) {
    const int32_t slot = A.lists.obs_kf[o];
    return (uint32_t)slot < (uint32_t)A.n_kf ? A.pose_index[slot] : -1;
}

__global__ __launch_bounds__(kBlock) void k_window_count(const GatherArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int o = blockIdx.x * kBlock + (int)threadIdx.x;
    const int k = o < A.n_obs ? pose_of(A, o) : -1;
    int kept, cur;
    block_rank<kBlock>(k >= 0, s_wave, kept);
    __syncthreads();
    block_rank<kBlock>(k >= 0 && k == A.current, s_wave, cur);
    if (threadIdx.x == 0) { A.blk_cnt[blockIdx.x] = kept; A.blk_cur[blockIdx.x] = cur; }
}

// ONE workgroup: the per-workgroup counts become offsets, the totals go to the head
__global__ __launch_bounds__(kBlock) void k_window_offsets(int32_t *a, int32_t *b, int n, int32_t *head) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int total_a = block_offsets<kBlock>(a, a, n, s_wave);
    const int total_b = block_offsets<kBlock>(b, b, n, s_wave);
    if (threadIdx.x == 0) { head[0] = total_a; head[1] = total_b; }
}

__global__ __launch_bounds__(kBlock) void k_window_pack(const GatherArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    if (A.head[0] > A.cap_edge) return;                      // the same in every lane of every workgroup: nothing is written
    const int o = blockIdx.x * kBlock + (int)threadIdx.x;
    const int k = o < A.n_obs ? pose_of(A, o) : -1;
    int total;
    const int e = A.blk_cnt[blockIdx.x] + block_rank<kBlock>(k >= 0, s_wave, total);
    if (k < 0) return;
    int lo = 0, hi = A.n_rows;                               // the last row whose list starts at or before o (rows without observations share a start)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.lists.obs_start[mid] <= o) lo = mid; else hi = mid;
    }
    const int32_t slot = A.lists.obs_kf[o];
    A.o_point[e] = lo;
    A.o_pose[e] = k;
    const double fx = A.cam[4 * k], fy = A.cam[4 * k + 1], cx = A.cam[4 * k + 2], cy = A.cam[4 * k + 3];
    A.uv[2 * (size_t)e] = obs_normalised(A.lists.obs_x[o], cx, fx);
    A.uv[2 * (size_t)e + 1] = obs_normalised(A.lists.obs_y[o], cy, fy);
    int32_t octave = A.lists.obs_octave[o];
    octave = octave < 0 ? 0 : (octave >= A.n_levels ? A.n_levels - 1 : octave);  // ms_observation_lists stores them inside the range already
    A.info[e] = obs_information(A.focal[k], A.sigma[octave]);
    A.win.edge_slot[e] = slot;
    A.win.edge_kp[e] = A.lists.obs_kp[o];
    A.win.edge_point[e] = lo;
}

// thread i: the pose of local keyframe i (i < n_local) and the position of listed row i (i < n_rows, 0 when the points do not fit)
__global__ __launch_bounds__(kBlock) void k_window_vertices(const GatherArgs A, int n_rows) {
    const int i = blockIdx.x * kBlock + (int)threadIdx.x;
    if (i < A.n_local) {
        pose_of_table(A.kf_pose + 12 * (size_t)A.local_slot[i], A.pose + 7 * (size_t)i);
    }
    if (i < n_rows) {
        const int32_t r = A.lists.rows[i];
        const bool ok = (uint32_t)r < (uint32_t)A.n_mp;
        for (int a = 0; a < 3; ++a) A.point[3 * (size_t)i + a] = ok ? A.mp_pos[3 * (size_t)r + a] : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------ apply
struct ApplyArgs {
    int32_t *kf_mp;
    double *mp_pos, *kf_pose;
    uint8_t *mp_flags;
    int32_t *n_obs;
    const double *pose, *point, *chi2;   // uploaded: [n_local * 7], [n_rows * 3], [n_edge]
    const int32_t *local_slot;           // uploaded
    ms_ba_window_dev win;
    const int32_t *rows;
    int32_t *blk_cnt, *blk_stale, *lost, *head, *erased;
    int32_t n_kf, stride, n_mp, n_edge, n_rows, n_local, current, mode, cap_erased;
};

// 0: the edge stays | 1: it is erased | 2: its table entry no longer names its row (skipped and counted).  row / entry for the writer.
__device__ __forceinline__ int edge_verdict(const ApplyArgs &A, int e, int &p, int &row, size_t &entry) {
    const int32_t slot = A.win.edge_slot[e], kp = A.win.edge_kp[e];
    p = A.win.edge_point[e];
    if (!((uint32_t)slot < (uint32_t)A.n_kf && (uint32_t)kp < (uint32_t)A.stride && (uint32_t)p < (uint32_t)A.n_rows)) return 2;
    row = A.rows[p];
    entry = (size_t)slot * A.stride + kp;
    if (!((uint32_t)row < (uint32_t)A.n_mp) || A.kf_mp[entry] != row) return 2;
    return A.chi2[e] > kChi2Threshold ? 1 : 0;               // strict; a NaN keeps the edge
}

__global__ __launch_bounds__(kEdgeBlock) void k_apply_count(const ApplyArgs A) {
    __shared__ int32_t s_wave[kEdgeBlock / 64];
    const int e = blockIdx.x * kEdgeBlock + (int)threadIdx.x;
    int p, row; size_t entry;
    const int v = e < A.n_edge ? edge_verdict(A, e, p, row, entry) : 0;
    int erased, stale;
    block_rank<kEdgeBlock>(v == 1, s_wave, erased);
    __syncthreads();
    block_rank<kEdgeBlock>(v == 2, s_wave, stale);
    if (threadIdx.x == 0) { A.blk_cnt[blockIdx.x] = erased; A.blk_stale[blockIdx.x] = stale; }
}

// An erased edge writes its own table entry and nobody else's: the verdicts of the other lanes do not move while this kernel runs.
__global__ __launch_bounds__(kEdgeBlock) void k_apply_erase(const ApplyArgs A) {
    __shared__ int32_t s_wave[kEdgeBlock / 64];
    if (A.head[0] > A.cap_erased) return;                    // the same everywhere: nothing is written
    const int e = blockIdx.x * kEdgeBlock + (int)threadIdx.x;
    int p = 0, row = 0; size_t entry = 0;
    const int v = e < A.n_edge ? edge_verdict(A, e, p, row, entry) : 0;
    int total;
    const int dst = A.blk_cnt[blockIdx.x] + block_rank<kEdgeBlock>(v == 1, s_wave, total);
    if (v != 1) return;
    A.kf_mp[entry] = -1;                                     // Keyframe::eraseObservation, :383
    atomicSub(&A.n_obs[row], 1);                             // MapPoint::eraseObservation, :382
    A.lost[p] = 1;
    A.erased[dst] = e;
}

__global__ __launch_bounds__(kBlock) void k_apply_vertices(const ApplyArgs A) {
    const bool local = A.mode == MS_BA_APPLY_LOCAL;
    if (local && A.head[0] > A.cap_erased) return;
    const int i = blockIdx.x * kBlock + (int)threadIdx.x;
    if (i < A.n_rows) {
        const int32_t r = A.rows[i];
        if ((uint32_t)r < (uint32_t)A.n_mp) {
            if (local && A.lost[i] && A.n_obs[r] <= 2) A.mp_flags[r] = 2;        // :384-386; the check after each erase is monotone
            for (int a = 0; a < 3; ++a) A.mp_pos[3 * (size_t)r + a] = A.point[3 * (size_t)i + a];
        }
    }
    if (i < A.n_local && (local || i == A.current)) write_pose(A.pose + 7 * (size_t)i, A.kf_pose + 12 * (size_t)A.local_slot[i]);
}

}  // namespace

extern "C" int ms_ba_window_lists(ms_ctx *c, const double *kf_pose, int n_kf, const double *mp_pos, int n_mp, const ms_obs_lists *lists, int n_rows, int n_obs,
                                  const int32_t *local_slot, int n_local, int current_index, const ms_pinhole *kf_cam, const int32_t *kf_focal, const float *level_sigma_sq,
                                  int n_levels, double *pose, double *point, int32_t *obs_point, int32_t *obs_pose, double *obs_uv, double *obs_info, int cap_point, int cap_edge,
                                  const ms_ba_window_dev *window, int32_t *n_edge, int32_t *n_current) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_ba_window_lists_check(kf_pose, n_kf, mp_pos, n_mp, lists, n_rows, n_obs, local_slot, n_local, current_index, kf_cam, kf_focal, level_sigma_sq, n_levels, pose,
                                       point, obs_point, obs_pose, obs_uv, obs_info, cap_point, cap_edge, window, n_edge, n_current, c->err, sizeof(c->err))))
        return rc;
    MsRange range("baWindowLists");
    const bool points_fit = n_rows <= cap_point;
    const int n_blocks = ms_div_up(n_obs, kBlock), n_point = points_fit ? n_rows : 0, n_out = n_obs < cap_edge ? n_obs : cap_edge;       // n_edge <= n_obs
    MsLayout up;                                             // upload block: pose index | local slots | focal lengths | cameras | sigmas
    const auto l_index = up.array<int32_t>((size_t)n_kf), l_local = up.array<int32_t>((size_t)n_local), l_focal = up.array<int32_t>((size_t)n_local);
    const auto l_cam = up.array<double>(4 * (size_t)n_local);
    const auto l_sigma = up.array<float>((size_t)n_levels);
    MsLayout down;                                           // the block that goes down: head | poses | points | the edges' arrays
    const auto l_head = down.array<int32_t>(kHead);
    const auto l_pose = down.array<double>(7 * (size_t)n_local), l_point = down.array<double>(3 * (size_t)n_point);
    const auto l_opoint = down.array<int32_t>((size_t)n_out), l_opose = down.array<int32_t>((size_t)n_out);
    const auto l_uv = down.array<double>(2 * (size_t)n_out), l_info = down.array<double>((size_t)n_out);
    MsLayout dev = up;                                       // device block: the upload block | block counts | the block that goes down
    const auto l_cnt = dev.array<int32_t>((size_t)n_blocks), l_cur = dev.array<int32_t>((size_t)n_blocks);
    const size_t down_at = dev.take(down.end);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_BA_WINDOW];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    if ((rc = ms_pinned(c, down.end))) return rc;
    void *hs = W.host, *ds = W.dev, *dd = static_cast<uint8_t *>(W.dev) + down_at, *hd = c->pinned;
    int32_t *index = l_index.at(hs);
    for (int k = 0; k < n_kf; ++k) index[k] = -1;
    for (int k = 0; k < n_local; ++k) {
        const int32_t slot = local_slot[k];
        index[slot] = k;
        l_local.at(hs)[k] = slot;
        l_focal.at(hs)[k] = kf_focal[slot];
        double *K = l_cam.at(hs) + 4 * (size_t)k;
        K[0] = kf_cam[slot].fx; K[1] = kf_cam[slot].fy; K[2] = kf_cam[slot].cx; K[3] = kf_cam[slot].cy;
    }
    l_sigma.fill(hs, level_sigma_sq);
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    MS_HIP(c, hipMemsetAsync(l_head.at(dd), 0, l_head.bytes(), c->stream));
    GatherArgs A{};
    A.kf_pose = kf_pose; A.mp_pos = mp_pos;
    if (lists) A.lists = *lists;
    A.pose_index = l_index.at(ds); A.local_slot = l_local.at(ds); A.focal = l_focal.at(ds); A.cam = l_cam.at(ds); A.sigma = l_sigma.at(ds);
    A.blk_cnt = l_cnt.at(ds); A.blk_cur = l_cur.at(ds); A.head = l_head.at(dd);
    A.pose = l_pose.at(dd); A.point = l_point.at(dd); A.uv = l_uv.at(dd); A.info = l_info.at(dd); A.o_point = l_opoint.at(dd); A.o_pose = l_opose.at(dd);
    if (window) A.win = *window;
    A.n_kf = n_kf; A.n_mp = n_mp; A.n_rows = n_rows; A.n_obs = n_obs; A.n_local = n_local; A.n_levels = n_levels; A.current = current_index; A.cap_edge = cap_edge;
    A.n_blocks = n_blocks;
    if (n_blocks > 0) {
        hipLaunchKernelGGL(k_window_count, dim3(n_blocks), dim3(kBlock), 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_window_count");
        hipLaunchKernelGGL(k_window_offsets, dim3(1), dim3(kBlock), 0, c->stream, A.blk_cnt, A.blk_cur, n_blocks, A.head);
        MS_KERNEL_CHECK(c, "k_window_offsets");
        if (points_fit && cap_edge > 0) {
            hipLaunchKernelGGL(k_window_pack, dim3(n_blocks), dim3(kBlock), 0, c->stream, A);
            MS_KERNEL_CHECK(c, "k_window_pack");
        }
    }
    const int n_vertex = n_local > n_point ? n_local : n_point;
    if (n_vertex > 0) {
        hipLaunchKernelGGL(k_window_vertices, dim3(ms_div_up(n_vertex, kBlock)), dim3(kBlock), 0, c->stream, A, n_point);
        MS_KERNEL_CHECK(c, "k_window_vertices");
    }
    MS_HIP(c, hipMemcpyAsync(hd, dd, down.end, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *head = l_head.at(hd);
    *n_edge = head[0]; *n_current = head[1];
    if (!points_fit || head[0] > cap_edge)
        return ms_fail(c, MS_ERR_CAPACITY, "ba window lists: %d rows and %d edges; the caller's arrays hold %d points and %d edges (nothing written)", n_rows, head[0], cap_point,
                       cap_edge);
    l_pose.get(hd, 0, pose, 7 * (size_t)n_local);
    l_point.get(hd, 0, point, 3 * (size_t)n_rows);
    const size_t ne = (size_t)head[0];
    l_opoint.get(hd, 0, obs_point, ne); l_opose.get(hd, 0, obs_pose, ne); l_uv.get(hd, 0, obs_uv, 2 * ne); l_info.get(hd, 0, obs_info, ne);
    return MS_OK;
}

extern "C" int ms_ba_window_apply(ms_ctx *c, int32_t *kf_mp, int n_kf, int stride, double *mp_pos, uint8_t *mp_flags, int32_t *n_obs, int n_mp, double *kf_pose,
                                  const double *pose, int n_pose, const double *point, const double *chi2, const ms_ba_window_dev *window, int n_edge, const int32_t *rows,
                                  int n_rows, const int32_t *local_slot, int n_local, int current_index, int mode, int32_t *erased_edge, int cap_erased, int32_t *n_erased,
                                  int32_t *n_stale) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_ba_window_apply_check(kf_mp, n_kf, stride, mp_pos, mp_flags, n_obs, n_mp, kf_pose, pose, n_pose, point, chi2, window, n_edge, rows, n_rows, local_slot, n_local,
                                       current_index, mode, erased_edge, cap_erased, n_erased, n_stale, c->err, sizeof(c->err))))
        return rc;
    *n_erased = 0; *n_stale = 0;
    MsRange range("baWindowApply");
    const bool local = mode == MS_BA_APPLY_LOCAL;
    const int n_walk = local ? n_edge : 0, n_blocks = ms_div_up(n_walk, kEdgeBlock), n_out = n_walk < cap_erased ? n_walk : cap_erased;
    MsLayout up;                                             // upload block: poses | points | chi2 | local slots
    const auto l_pose = up.array<double>(7 * (size_t)n_local), l_point = up.array<double>(3 * (size_t)n_rows), l_chi2 = up.array<double>((size_t)n_walk);
    const auto l_local = up.array<int32_t>((size_t)n_local);
    MsLayout down;                                           // the block that goes down: head | erased edges
    const auto l_head = down.array<int32_t>(kHead);
    const auto l_erased = down.array<int32_t>((size_t)n_out);
    MsLayout dev = up;                                       // device block: the upload block | block counts | "lost an observation" marks | the block that goes down
    const auto l_cnt = dev.array<int32_t>((size_t)n_blocks), l_stale = dev.array<int32_t>((size_t)n_blocks);
    const auto l_lost = dev.array<int32_t>((size_t)(local ? n_rows : 0));
    const size_t down_at = dev.take(down.end);
    const size_t zero_bytes = down_at + ms_align_up(l_head.bytes(), MsLayout::kAlign) - l_lost.off;      // the marks and the head lie next to each other: one clear
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_BA_WINDOW];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    if ((rc = ms_pinned(c, down.end))) return rc;
    void *hs = W.host, *ds = W.dev, *dd = static_cast<uint8_t *>(W.dev) + down_at, *hd = c->pinned;
    l_pose.fill(hs, pose); l_point.fill(hs, point); l_chi2.fill(hs, chi2); l_local.fill(hs, local_slot);
    if (up.end) MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    MS_HIP(c, hipMemsetAsync(l_lost.at(ds), 0, zero_bytes, c->stream));
    ApplyArgs A{};
    A.kf_mp = kf_mp; A.mp_pos = mp_pos; A.kf_pose = kf_pose; A.mp_flags = mp_flags; A.n_obs = n_obs;
    A.pose = l_pose.at(ds); A.point = l_point.at(ds); A.chi2 = l_chi2.at(ds); A.local_slot = l_local.at(ds);
    if (window) A.win = *window;
    A.rows = rows; A.blk_cnt = l_cnt.at(ds); A.blk_stale = l_stale.at(ds); A.lost = l_lost.at(ds); A.head = l_head.at(dd); A.erased = l_erased.at(dd);
    A.n_kf = n_kf; A.stride = stride; A.n_mp = n_mp; A.n_edge = n_walk; A.n_rows = n_rows; A.n_local = n_local; A.current = current_index; A.mode = mode;
    A.cap_erased = cap_erased;
    if (n_blocks > 0) {
        hipLaunchKernelGGL(k_apply_count, dim3(n_blocks), dim3(kEdgeBlock), 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_apply_count");
        hipLaunchKernelGGL(k_window_offsets, dim3(1), dim3(kBlock), 0, c->stream, A.blk_cnt, A.blk_stale, n_blocks, A.head);
        MS_KERNEL_CHECK(c, "k_window_offsets");
        hipLaunchKernelGGL(k_apply_erase, dim3(n_blocks), dim3(kEdgeBlock), 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_apply_erase");
    }
    const int n_vertex = n_local > n_rows ? n_local : n_rows;
    if (n_vertex > 0) {
        hipLaunchKernelGGL(k_apply_vertices, dim3(ms_div_up(n_vertex, kBlock)), dim3(kBlock), 0, c->stream, A);
        MS_KERNEL_CHECK(c, "k_apply_vertices");
    }
    MS_HIP(c, hipMemcpyAsync(hd, dd, down.end, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *head = l_head.at(hd);
    *n_erased = head[0]; *n_stale = head[1];
    if (head[0] > cap_erased)
        return ms_fail(c, MS_ERR_CAPACITY, "ba window apply: %d erased edges, erased_edge holds %d (nothing written)", head[0], cap_erased);
    l_erased.get(hd, 0, erased_edge, (size_t)head[0]);
    if (head[1])
        return ms_fail(c, MS_ERR_INVALID, "ba window apply: %d edges whose table entry no longer names their row (skipped; the tables changed between gather and apply)",
                       head[1]);
    return MS_OK;
}
