// frame_admit.hip -- a frame that carries tracker features only, from the host's feature list to the device map tables: the piece of
// addKeyframeCommonOuter (mapper_helpers.cpp:1196) in front of ms_match_tracked for every front-end frame and every back-end frame that is no keyframe.
//   Keyframe::addTrackerFeatures   keyframe.cpp:118-133   the kept features become the keypoints, octave 0, keyPointToTrackId
//   processKeyPoints               keyframe.cpp:34-69     mapPoints = -1, keyPointDepth
//
// ms_frame_admit, TWO launches whatever the sizes:
//   k_frame_admit_rank    ONE workgroup walks the features in trips of 256: a feature is kept iff keep says so and the mask does; its keypoint index is
//                         its rank among the kept through the shared block rank, the count carried across trips.  The same workgroup then walks the
//                         slot's row and counts its VALID entries.  It writes per feature its keypoint index (or none) and the head of the block that
//                         goes down: n_kp, the two drop counts, the depths taken from the image, the bound entries of the row
//   k_frame_admit_write   one lane per feature or entry of the row, whichever is more.  Returns at once unless the head says that n_kp fits and the row
//                         is empty (every verdict before any write).  Then every write of the call: the keypoint's entries, its track id and feature
//                         index in the block that goes down, the cleared row, the pose
// Every position is an integer prefix count, there is no atomic, and no kernel reads what another lane of the same launch writes: the same inputs
// give the same bytes on every call.
#include "ms_internal.h"
#include "ms_scan.h"
#include <algorithm>
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int32_t kDropped = -1;                             // rank[i] of a feature that is no keypoint
// the head of the block that goes down
constexpr int kHeadKp = 0, kHeadKeep = 1, kHeadMask = 2, kHeadImage = 3, kHeadBadRow = 4, kHeadInts = 8;

struct FrameAdmitArgs {
    // the tables
    int32_t *kf_mp;
    float *kp_x, *kp_y, *kp_depth;
    int32_t *kp_octave;
    double *kf_pose;
    int32_t stride, n_mp, slot, cap_kp;
    double pose[12];
    // the features (device copies); keep is null when every feature passes
    const float *x, *y, *depth;
    const int32_t *id;
    const uint8_t *keep;
    int32_t n_tracks;
    // the depth image and the valid mask, each null when there is none
    const float *depth_image;
    int32_t depth_w, depth_h, depth_stride;
    const uint8_t *mask;
    int32_t mask_w, mask_h, mask_stride;
    int32_t *rank;                       // workspace [n_tracks]: the feature's keypoint index | kDropped
    // the block that goes down
    int32_t *head, *d_track, *d_feature;
};

// the rounded position of a keypoint: the rounding of the valid mask in ms_orb_set_valid_mask and of the depth sample in ms_keyframe_admit
__device__ __forceinline__ bool inside(float x, float y, int w, int h, int &ix, int &iy) {
    ix = __float2int_rn(x); iy = __float2int_rn(y);
    return ix >= 0 && ix < w && iy >= 0 && iy < h;
}

__device__ __forceinline__ bool admit_fits(const FrameAdmitArgs &A, int n_kp) { return n_kp <= A.stride && n_kp <= A.cap_kp; }

__global__ __launch_bounds__(kBlock) void k_frame_admit_rank(const FrameAdmitArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int tid = (int)threadIdx.x;
    int n_kp = 0;                                            // kept so far: the carry into the next trip
    int by_keep = 0, by_mask = 0, from_image = 0, bad_row = 0;      // this lane's share
    for (int i0 = 0; i0 < A.n_tracks; i0 += kBlock) {
        const int i = i0 + tid;
        bool kept = false;
        if (i < A.n_tracks) {
            const float x = A.x[i], y = A.y[i];
            int ix, iy;
            if (A.keep && A.keep[i] == 0) ++by_keep;
            else if (A.mask && !(inside(x, y, A.mask_w, A.mask_h, ix, iy) && A.mask[(size_t)iy * A.mask_stride + ix] != 0)) ++by_mask;
            else {
                kept = true;
                from_image += A.depth[i] < 0 && A.depth_image && inside(x, y, A.depth_w, A.depth_h, ix, iy);
            }
        }
        int total;
        const int k = n_kp + block_rank<kBlock>(kept, s_wave, total);      // k <= i < n_tracks
        if (i < A.n_tracks) A.rank[i] = kept ? k : kDropped;
        n_kp += total;
        __syncthreads();                                     // s_wave is written again by the next trip
    }
    for (int j = tid; j < A.stride; j += kBlock) bad_row += (uint32_t)A.kf_mp[(size_t)A.slot * A.stride + j] < (uint32_t)A.n_mp;
    // four sums of one int per lane over the workgroup; every lane learns each total
    const int share[4] = {by_keep, by_mask, from_image, bad_row};
    int sum[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        block_exclusive<kBlock>(share[q], s_wave, sum[q]);
        __syncthreads();                                     // s_wave is written again by the next sum
    }
    if (tid == 0) {
        A.head[kHeadKp] = n_kp; A.head[kHeadKeep] = sum[0]; A.head[kHeadMask] = sum[1]; A.head[kHeadImage] = sum[2]; A.head[kHeadBadRow] = sum[3];
        for (int q = kHeadBadRow + 1; q < kHeadInts; ++q) A.head[q] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void k_frame_admit_write(const FrameAdmitArgs A) {
    if (!admit_fits(A, A.head[kHeadKp]) || A.head[kHeadBadRow] != 0) return;      // the same answer in every lane of the grid: nothing is written
    const int j = blockIdx.x * kBlock + (int)threadIdx.x;
    if (j < A.stride) A.kf_mp[(size_t)A.slot * A.stride + j] = -1;
    if (j < 12) A.kf_pose[12 * (size_t)A.slot + j] = A.pose[j];
    if (j >= A.n_tracks) return;
    const int k = A.rank[j];
    if (k == kDropped) return;                               // otherwise k < n_kp <= min(stride, cap_kp)
    const float x = A.x[j], y = A.y[j];
    const size_t e = (size_t)A.slot * A.stride + k;
    A.kp_x[e] = x; A.kp_y[e] = y; A.kp_octave[e] = 0;        // keyframe.cpp:127
    float depth = A.depth[j];                                // keyframe.cpp:57-63
    if (depth < 0) {
        depth = -1.f;
        if (A.depth_image) {
            const int ix = __float2int_rn(x), iy = __float2int_rn(y);
            if (ix >= 0 && ix < A.depth_w && iy >= 0 && iy < A.depth_h) depth = A.depth_image[(size_t)iy * A.depth_stride + ix];
        }
    }
    A.kp_depth[e] = depth;
    A.d_track[k] = A.id[j];
    A.d_feature[k] = j;
}

}  // namespace

extern "C" int ms_frame_admit(ms_ctx *c, int32_t *kf_mp, int n_kf, int stride, int n_mp, float *kp_x, float *kp_y, int32_t *kp_octave, float *kp_depth, double *kf_pose,
                              const float *x, const float *y, const int32_t *id, const float *depth, const uint8_t *keep, int n_tracks, const ms_frame_admit_args *args,
                              int32_t *kp_track, int32_t *kp_feature, int cap_kp, int32_t *counts) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_frame_admit_validate(kf_mp, n_kf, stride, n_mp, kp_x, kp_y, kp_octave, kp_depth, kf_pose, x, y, id, depth, keep, n_tracks, args, kp_track, kp_feature, cap_kp,
                                      counts, c->err, sizeof(c->err))))
        return rc;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    MsRange range("frameAdmit");
    const size_t nt = (size_t)n_tracks;
    // no call admits more keypoints than it has features, the row holds or the caller's arrays hold: the bound of the arrays that go down
    const size_t bound = std::min(nt, (size_t)std::min(stride, cap_kp));
    // upload block: x | y | depth | id | keep
    MsLayout up;
    const auto l_x = up.array<float>(nt), l_y = up.array<float>(nt), l_depth = up.array<float>(nt);
    const auto l_id = up.array<int32_t>(nt);
    const auto l_keep = up.array<uint8_t>(keep ? nt : 0);
    MsLayout dev = up;
    // device-only block: the keypoint index per feature; then the block that goes down: head | track ids | feature indices
    const auto l_rank = dev.array<int32_t>(nt);
    MsLayout down;
    const auto l_head = down.array<int32_t>(kHeadInts);
    const auto l_dtrack = down.array<int32_t>(bound), l_dfeature = down.array<int32_t>(bound);
    const size_t down_at = dev.take(down.end);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_FRAME_ADMIT];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    if ((rc = ms_pinned(c, down.end))) return rc;
    void *hs = W.host, *ds = W.dev, *dd = ms_at<uint8_t>(W.dev, down_at);
    FrameAdmitArgs A{};
    A.kf_mp = kf_mp; A.kp_x = kp_x; A.kp_y = kp_y; A.kp_depth = kp_depth; A.kp_octave = kp_octave; A.kf_pose = kf_pose;
    A.stride = stride; A.n_mp = n_mp; A.slot = args->slot; A.cap_kp = cap_kp;
    std::memcpy(A.pose, args->pose, sizeof A.pose);
    A.x = l_x.at(ds); A.y = l_y.at(ds); A.depth = l_depth.at(ds); A.id = l_id.at(ds); A.keep = keep ? l_keep.at(ds) : nullptr; A.n_tracks = n_tracks;
    A.depth_image = args->depth_image; A.depth_w = args->depth_width; A.depth_h = args->depth_height; A.depth_stride = args->depth_stride;
    A.mask = args->valid_mask; A.mask_w = args->mask_width; A.mask_h = args->mask_height; A.mask_stride = args->mask_stride;
    A.rank = l_rank.at(ds);
    A.head = l_head.at(dd); A.d_track = l_dtrack.at(dd); A.d_feature = l_dfeature.at(dd);
    if (n_tracks > 0) {
        l_x.fill(hs, x); l_y.fill(hs, y); l_depth.fill(hs, depth); l_id.fill(hs, id);
        if (keep) l_keep.fill(hs, keep);
        MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    }
    const dim3 block(kBlock);
    const dim3 by_entry((unsigned)ms_div_up(std::max(stride, n_tracks), kBlock));
    hipLaunchKernelGGL(k_frame_admit_rank, dim3(1), block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_frame_admit_rank");
    hipLaunchKernelGGL(k_frame_admit_write, by_entry, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_frame_admit_write");
    MS_HIP(c, hipMemcpyAsync(c->pinned, dd, down.end, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    void *ps = c->pinned;
    const int32_t *head = l_head.at(ps);
    const int n_kp = head[kHeadKp];
    counts[0] = n_kp; counts[1] = head[kHeadKeep]; counts[2] = head[kHeadMask]; counts[3] = head[kHeadImage];
    if (n_kp > stride || n_kp > cap_kp)
        return ms_fail(c, MS_ERR_CAPACITY, "frame admit: %d keypoints; the row holds %d, the output arrays %d (nothing is written)", n_kp, stride, cap_kp);
    if (head[kHeadBadRow])
        return ms_fail(c, MS_ERR_INVALID, "frame admit: slot %d is not empty, %d of its entries are bound (nothing is written)", args->slot, head[kHeadBadRow]);
    if (kp_track) l_dtrack.get(ps, 0, kp_track, (size_t)n_kp);
    if (kp_feature) l_dfeature.get(ps, 0, kp_feature, (size_t)n_kp);
    return MS_OK;
}
