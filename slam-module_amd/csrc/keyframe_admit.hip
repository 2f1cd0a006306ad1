// keyframe_admit.hip -- a new keyframe from the extractor's output to the device map tables: the piece of addKeyframeCommonOuter
// (mapper_helpers.cpp:1186-1203) in front of every step of 9.4 - 9.18.
//   Keyframe::addFullFeatures   keyframe.cpp:95-116   keyPointTrackIds, FeatureSearch::create
//   processKeyPoints            keyframe.cpp:34-69    mapPoints = -1, keyPointDepth, KeyPoint::bearing
//   BowIndex::transform         bow_index.cpp:59-93   the descent; the FeatureVector as the ms_bow of an ms_match_frame
//
// ms_keyframe_admit, FOUR launches whatever the sizes; n = view.count[frame] is read by every kernel itself:
//   k_admit_descend   16 lanes per descriptor walk the vocabulary tree (bow_descend.h, the walk of ms_bow_transform) on the view's descriptors where
//                     they lie; without a vocabulary word = -1, weight = 0.  Lane 0 of the grid writes the head: n and zeroed verdict counters
//   k_admit_verdict   one lane per entry of the slot's row: counts into the head the non-finite coordinates, the valid entries already in the row
//                     and the tracked keypoints whose id is not listed; writes each keypoint's index into the track lists (the LAST equal id)
//   k_admit_write     returns at once unless every verdict is clean.  Every workgroup stages all y in LDS (32 KB at the cap of 8192) and each lane
//                     counts its position in FeatureSearch::create's order; the same again on the node keys for the position in (node, index) order.
//                     Then every write of the call but the node lists: keypoint table, depth, pool, frame arrays, the cleared row, the pose
//   k_admit_nodes     ONE workgroup walks the keypoints in node order in trips of 256: a segment head is a keypoint whose node differs from the one
//                     before it; heads are packed through the shared block rank, the count carried across trips
// Every position is an integer count, the only atomics are integer adds of the verdict counters, and no kernel reads what another lane of the
// same launch writes: the same inputs give the same bytes on every call.
#include "bow_descend.h"
#include "ms_bearing.h"
#include "ms_scan.h"
#include <algorithm>
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int kMaxKp = MS_COVIS_MAX_STRIDE;                  // n <= stride <= this: what the LDS staging of k_admit_write holds
constexpr int32_t kNoNode = 0x7fffffff;                      // the node key of a keypoint outside the node lists (weight <= 0, or no vocabulary)
constexpr int32_t kTrackNone = -1, kTrackMissing = -2;       // trk_idx of a keypoint without a track | whose id is not listed
// the head of the block that goes down
constexpr int kHeadN = 0, kHeadNodes = 1, kHeadKept = 2, kHeadBadXy = 3, kHeadBadRow = 4, kHeadBadTrack = 5, kHeadInts = 8;

struct AdmitArgs {
    // the view, offset to the frame
    const int32_t *count;                // &view.count[frame]
    const float *vx, *vy, *vangle;
    const int32_t *voctave, *vtrack;
    const uint32_t *vdesc;
    int32_t view_cap;
    // the tables
    int32_t *kf_mp;
    float *kp_x, *kp_y, *kp_depth;
    int32_t *kp_octave;
    uint32_t *desc_pool;
    double *kf_pose;
    int32_t stride, n_mp, n_pool, slot, desc_base;
    double pose[12];
    ms_pinhole cam;
    // the track lists (device copies) and the depth image
    const int32_t *track_ids;            // null: no lists
    const float *track_depth;
    int32_t n_tracks;
    const float *depth_image;            // null: no image
    int32_t depth_w, depth_h, depth_stride;
    // the vocabulary
    BowTree tree;
    int32_t has_tree, levels_up;
    ms_admit_frame out;
    // workspace [launch bound each]
    int32_t *word, *node, *trk_idx, *snode;
    double *weight;
    // the block that goes down; every array but the head may be null (not wanted)
    int32_t *head, *d_track, *d_word, *d_sidx, *d_octave;
    double *d_weight;
    float *d_sx, *d_sy;
    uint32_t *d_desc;
};

// what every kernel asks of n before it uses it: inside the view, the row, the frame arrays and the pool
__device__ __forceinline__ bool admit_fits(const AdmitArgs &A, int n) {
    return n >= 0 && n <= A.view_cap && n <= A.stride && n <= A.out.cap_kp && (long long)A.desc_base + n <= (long long)A.n_pool;
}
__device__ __forceinline__ bool admit_clean(const AdmitArgs &A) {
    return (A.head[kHeadBadXy] | A.head[kHeadBadRow] | A.head[kHeadBadTrack]) == 0;
}

__global__ __launch_bounds__(kBlock) void k_admit_descend(const AdmitArgs A) {
    const int n = *A.count;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        A.head[kHeadN] = n;
        for (int i = 1; i < kHeadInts; ++i) A.head[i] = 0;
    }
    const int i = blockIdx.x * 16 + ((int)threadIdx.x >> 4);
    const bool live = admit_fits(A, n) && i < n;             // i < n <= view_cap: inside the frame's descriptors
    if (A.has_tree) {
        bow_descend(A.tree, reinterpret_cast<const uint4 *>(A.vdesc), i, live, A.levels_up, A.word, A.weight, A.node);
    } else if (live && (threadIdx.x & 15) == 0) {
        A.word[i] = -1; A.weight[i] = 0.0; A.node[i] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void k_admit_verdict(const AdmitArgs A) {
    const int n = *A.count;
    if (!admit_fits(A, n)) return;                           // the host reports the capacity from n alone
    const int j = blockIdx.x * kBlock + (int)threadIdx.x;
    bool bad_xy = false, bad_row = false, bad_track = false;
    if (j < A.stride) bad_row = (uint32_t)A.kf_mp[(size_t)A.slot * A.stride + j] < (uint32_t)A.n_mp;
    if (j < n) {
        bad_xy = !(isfinite(A.vx[j]) && isfinite(A.vy[j]));
        const int32_t id = A.vtrack[j];
        int32_t at = kTrackNone;
        if (id >= 0 && A.track_ids) {
            at = kTrackMissing;
            for (int i = 0; i < A.n_tracks; ++i)
                if (A.track_ids[i] == id) at = i;            // the last one stays: trackIdToIndex[id] = idx overwrites
            bad_track = at == kTrackMissing;
        }
        A.trk_idx[j] = at;
    }
    const int n_xy = __popcll(__ballot(bad_xy)), n_row = __popcll(__ballot(bad_row)), n_track = __popcll(__ballot(bad_track));
    if ((threadIdx.x & 63) == 0) {
        if (n_xy) atomicAdd(A.head + kHeadBadXy, n_xy);
        if (n_row) atomicAdd(A.head + kHeadBadRow, n_row);
        if (n_track) atomicAdd(A.head + kHeadBadTrack, n_track);
    }
}

__global__ __launch_bounds__(kBlock) void k_admit_write(const AdmitArgs A) {
    __shared__ float4 s_stage[kMaxKp / 4];                   // all y, then all node keys: 32 KB
    const int n = *A.count;
    if (!admit_fits(A, n) || !admit_clean(A)) return;        // the same answer in every lane of the grid: nothing is written
    const int tid = (int)threadIdx.x, j = blockIdx.x * kBlock + tid;
    const int n4 = (n + 3) / 4;
    // ---- FeatureSearch::create: the position of j = #{k : y[k] < y[j] || (y[k] == y[j] && k < j)}
    {
        float *s_y = reinterpret_cast<float *>(s_stage);
        for (int k = tid; k < 4 * n4; k += kBlock) s_y[k] = k < n ? A.vy[k] : __builtin_nanf("");     // a NaN compares false both ways
    }
    __syncthreads();
    float x = 0.f, y = 0.f;
    if (j < n) {
        x = A.vx[j]; y = A.vy[j];
        int pos = 0;
        for (int q = 0; q < n4; ++q) {
            const float4 v = s_stage[q];
            const int k = 4 * q;
            pos += (v.x < y || (v.x == y && k < j)) + (v.y < y || (v.y == y && k + 1 < j)) + (v.z < y || (v.z == y && k + 2 < j)) + (v.w < y || (v.w == y && k + 3 < j));
        }
        // pos < n: j itself is not counted
        A.out.sorted_x[pos] = x; A.out.sorted_y[pos] = y; A.out.sorted_idx[pos] = j;
        if (A.d_sx) A.d_sx[pos] = x;
        if (A.d_sy) A.d_sy[pos] = y;
        if (A.d_sidx) A.d_sidx[pos] = j;
    }
    __syncthreads();                                         // the staging is written again
    // ---- the FeatureVector's order: keypoints with weight > 0 by (node, index)
    int32_t key = kNoNode;
    if (j < n && A.has_tree && A.weight[j] > 0.0) key = A.node[j];
    {
        int32_t *s_key = reinterpret_cast<int32_t *>(s_stage);
        for (int k = tid; k < 4 * n4; k += kBlock) s_key[k] = (k < n && A.has_tree && A.weight[k] > 0.0) ? A.node[k] : kNoNode;
    }
    __syncthreads();
    if (j < n) {
        const int4 *s_key4 = reinterpret_cast<const int4 *>(s_stage);
        int pos = 0, kept = 0;
        for (int q = 0; q < n4; ++q) {
            const int4 v = s_key4[q];
            const int k = 4 * q;
            pos += (v.x < key || (v.x == key && k < j)) + (v.y < key || (v.y == key && k + 1 < j)) + (v.z < key || (v.z == key && k + 2 < j)) + (v.w < key || (v.w == key && k + 3 < j));
            kept += (v.x != kNoNode) + (v.y != kNoNode) + (v.z != kNoNode) + (v.w != kNoNode);
        }
        if (key != kNoNode) { A.out.kp_idx[pos] = j; A.snode[pos] = key; }      // pos < kept <= n: the kept keys are all below kNoNode
        if (j == 0) A.head[kHeadKept] = kept;
    }
    // ---- the slot's row and pose
    if (j < A.stride) A.kf_mp[(size_t)A.slot * A.stride + j] = -1;
    if (j < 12) A.kf_pose[12 * (size_t)A.slot + j] = A.pose[j];
    if (j >= n) return;
    // ---- the keypoint's entries
    const size_t e = (size_t)A.slot * A.stride + j;
    const int32_t octave = A.voctave[j];
    A.kp_x[e] = x; A.kp_y[e] = y; A.kp_octave[e] = octave;
    float depth = -1.f;                                      // keyframe.cpp:57-63
    const int32_t at = A.trk_idx[j];
    if (at >= 0) depth = A.track_depth[at];
    if (depth < 0) {
        depth = -1.f;
        if (A.depth_image) {
            const int ix = __float2int_rn(x), iy = __float2int_rn(y);
            if (ix >= 0 && ix < A.depth_w && iy >= 0 && iy < A.depth_h) depth = A.depth_image[(size_t)iy * A.depth_stride + ix];
        }
    }
    A.kp_depth[e] = depth;
    const uint4 *src = reinterpret_cast<const uint4 *>(A.vdesc) + 2 * (size_t)j;
    const uint4 d0 = src[0], d1 = src[1];
    uint4 *pool = reinterpret_cast<uint4 *>(A.desc_pool) + 2 * ((size_t)A.desc_base + j), *fd = reinterpret_cast<uint4 *>(A.out.desc) + 2 * (size_t)j;
    pool[0] = d0; pool[1] = d1;
    fd[0] = d0; fd[1] = d1;
    if (A.d_desc) { uint32_t *dd = A.d_desc + 8 * (size_t)j; dd[0] = d0.x; dd[1] = d0.y; dd[2] = d0.z; dd[3] = d0.w; dd[4] = d1.x; dd[5] = d1.y; dd[6] = d1.z; dd[7] = d1.w; }
    A.out.angle[j] = A.vangle[j];
    A.out.octave[j] = octave;
    if (A.d_octave) A.d_octave[j] = octave;
    double xn, yn, b[3];
    ms_pinhole_bearing(A.cam, x, y, xn, yn, b);
    A.out.bearing[3 * (size_t)j] = b[0]; A.out.bearing[3 * (size_t)j + 1] = b[1]; A.out.bearing[3 * (size_t)j + 2] = b[2];
    A.out.usable[j] = 1;
    if (A.d_track) A.d_track[j] = A.vtrack[j];
    if (A.d_word) A.d_word[j] = A.word[j];
    if (A.d_weight) A.d_weight[j] = A.weight[j];
}

__global__ __launch_bounds__(kBlock) void k_admit_nodes(const AdmitArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int n = *A.count;
    if (!admit_fits(A, n) || !admit_clean(A)) return;
    const int kept = A.head[kHeadKept];                      // <= n <= cap_kp
    int n_nodes = 0;                                         // heads so far: the carry into the next trip
    for (int i0 = 0; i0 < kept; i0 += kBlock) {
        const int i = i0 + (int)threadIdx.x;
        int32_t node = 0;
        bool first = false;
        if (i < kept) {
            node = A.snode[i];
            first = i == 0 || A.snode[i - 1] != node;
        }
        int total;
        const int k = n_nodes + block_rank<kBlock>(first, s_wave, total);      // k <= i < cap_kp
        if (first) { A.out.node_id[k] = node; A.out.node_start[k] = i; }
        n_nodes += total;
        __syncthreads();                                     // s_wave is written again by the next trip
    }
    if (threadIdx.x == 0) {
        A.out.node_start[n_nodes] = kept;                    // n_nodes <= kept <= cap_kp: the array holds cap_kp + 1
        A.head[kHeadNodes] = n_nodes;
    }
}

}  // namespace

extern "C" int ms_keyframe_admit(ms_ctx *c, const ms_keypoints *view, int frame, int32_t *kf_mp, int n_kf, int stride, int n_mp, float *kp_x, float *kp_y,
                                 int32_t *kp_octave, float *kp_depth, uint32_t *desc_pool, int n_pool, double *kf_pose, const ms_admit_args *args,
                                 const ms_admit_frame *out, const ms_admit_host *host, int32_t *counts) {
    if (!c) return MS_ERR_INVALID;
    c->admit_n = -1;                                         // ms_keyframe_admit_words: nothing to hand out until this call has succeeded
    int rc;
    if ((rc = ms_keyframe_admit_validate(view, frame, kf_mp, n_kf, stride, n_mp, kp_x, kp_y, kp_octave, kp_depth, desc_pool, n_pool, kf_pose, args, out, host, counts, c->err,
                                         sizeof(c->err))))
        return rc;
    counts[0] = counts[1] = counts[2] = 0;
    MsRange range("keyframeAdmit");
    // no call admits more keypoints than the view, the row and the frame arrays hold: the launch bound of every per-keypoint array
    const size_t bound = (size_t)std::min(std::min(view->capacity, stride), out->cap_kp);
    const bool with_tracks = args->track_ids != nullptr && args->n_tracks > 0;
    const size_t nt = with_tracks ? (size_t)args->n_tracks : 0;
    static const ms_admit_host kNoHost = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const ms_admit_host &H = host ? *host : kNoHost;
    auto want = [&](const void *p) { return p ? bound : (size_t)0; };
    // upload block: track ids | depths
    MsLayout up;
    const auto l_ids = up.array<int32_t>(nt);
    const auto l_tdepth = up.array<float>(nt);
    MsLayout dev = up;
    // device-only block: word | node | track index | nodes in list order | weight
    const auto l_word = dev.array<int32_t>(bound), l_node = dev.array<int32_t>(bound), l_trk = dev.array<int32_t>(bound), l_snode = dev.array<int32_t>(bound);
    const auto l_weight = dev.array<double>(bound);
    // the block that goes down: head | track ids | words | weights | sorted x | y | index | octaves | descriptors
    MsLayout down;
    const auto l_head = down.array<int32_t>(kHeadInts);
    const auto l_dtrack = down.array<int32_t>(want(H.kp_track)), l_dword = down.array<int32_t>(want(H.word));
    const auto l_dweight = down.array<double>(want(H.weight));
    const auto l_dsx = down.array<float>(want(H.sorted_x)), l_dsy = down.array<float>(want(H.sorted_y));
    const auto l_dsidx = down.array<int32_t>(want(H.sorted_idx)), l_doct = down.array<int32_t>(want(H.octave));
    const auto l_ddesc = down.array<uint32_t>(8 * want(H.desc));
    const size_t down_at = dev.take(down.end);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_KEYFRAME_ADMIT];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    if ((rc = ms_pinned(c, down.end))) return rc;
    void *hs = W.host, *ds = W.dev, *dd = ms_at<uint8_t>(W.dev, down_at);
    AdmitArgs A{};
    const size_t f0 = (size_t)frame * (size_t)view->capacity;
    A.count = view->count + frame; A.vx = view->x + f0; A.vy = view->y + f0; A.vangle = view->angle + f0; A.voctave = view->octave + f0; A.vtrack = view->track_id + f0;
    A.vdesc = view->desc + 8 * f0; A.view_cap = view->capacity;
    A.kf_mp = kf_mp; A.kp_x = kp_x; A.kp_y = kp_y; A.kp_depth = kp_depth; A.kp_octave = kp_octave; A.desc_pool = desc_pool; A.kf_pose = kf_pose;
    A.stride = stride; A.n_mp = n_mp; A.n_pool = n_pool; A.slot = args->slot; A.desc_base = args->desc_base;
    std::memcpy(A.pose, args->pose, sizeof A.pose);
    A.cam = args->cam;
    A.track_ids = args->track_ids ? l_ids.at(ds) : nullptr; A.track_depth = l_tdepth.at(ds); A.n_tracks = (int32_t)nt;
    A.depth_image = args->depth_image; A.depth_w = args->depth_width; A.depth_h = args->depth_height; A.depth_stride = args->depth_stride;
    if (args->vocab) { A.tree = args->vocab->tree; A.has_tree = 1; A.levels_up = args->levels_up; }
    A.out = *out;
    A.word = l_word.at(ds); A.node = l_node.at(ds); A.trk_idx = l_trk.at(ds); A.snode = l_snode.at(ds); A.weight = l_weight.at(ds);
    A.head = l_head.at(dd);
    A.d_track = H.kp_track ? l_dtrack.at(dd) : nullptr; A.d_word = H.word ? l_dword.at(dd) : nullptr; A.d_weight = H.weight ? l_dweight.at(dd) : nullptr;
    A.d_sx = H.sorted_x ? l_dsx.at(dd) : nullptr; A.d_sy = H.sorted_y ? l_dsy.at(dd) : nullptr; A.d_sidx = H.sorted_idx ? l_dsidx.at(dd) : nullptr;
    A.d_octave = H.octave ? l_doct.at(dd) : nullptr; A.d_desc = H.desc ? l_ddesc.at(dd) : nullptr;
    if (with_tracks) {
        l_ids.fill(hs, args->track_ids);
        l_tdepth.fill(hs, args->track_depth);
        MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    }
    const dim3 block(kBlock);
    const dim3 by_group((unsigned)std::max<size_t>((bound + 15) / 16, 1)), by_entry((unsigned)ms_div_up(stride, kBlock));
    hipLaunchKernelGGL(k_admit_descend, by_group, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_admit_descend");
    hipLaunchKernelGGL(k_admit_verdict, by_entry, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_admit_verdict");
    hipLaunchKernelGGL(k_admit_write, by_entry, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_admit_write");
    hipLaunchKernelGGL(k_admit_nodes, dim3(1), block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_admit_nodes");
    MS_HIP(c, hipMemcpyAsync(c->pinned, dd, down.end, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    void *ps = c->pinned;
    const int32_t *head = l_head.at(ps);
    const int n = head[kHeadN];
    counts[0] = n;
    if (n < 0 || n > view->capacity) return ms_fail(c, MS_ERR_INVALID, "keyframe admit: the view counts %d keypoints in frame %d, its capacity is %d (nothing is written)", n, frame, view->capacity);
    if (n > stride || n > out->cap_kp || (long long)args->desc_base + n > (long long)n_pool)
        return ms_fail(c, MS_ERR_CAPACITY, "keyframe admit: %d keypoints; the row holds %d, the frame arrays %d, the pool %d from %d on (nothing is written)", n, stride,
                       out->cap_kp, n_pool - args->desc_base, args->desc_base);
    if (head[kHeadBadXy]) return ms_fail(c, MS_ERR_INVALID, "keyframe admit: %d of %d keypoints have a coordinate that is not finite (nothing is written)", head[kHeadBadXy], n);
    if (head[kHeadBadRow])
        return ms_fail(c, MS_ERR_INVALID, "keyframe admit: slot %d is not empty, %d of its entries are bound (nothing is written)", args->slot, head[kHeadBadRow]);
    if (head[kHeadBadTrack])
        return ms_fail(c, MS_ERR_INVALID, "keyframe admit: %d tracked keypoints have an id that is not in track_ids (nothing is written)", head[kHeadBadTrack]);
    counts[1] = head[kHeadNodes]; counts[2] = head[kHeadKept];
    const size_t m = (size_t)n;
    if (H.kp_track) l_dtrack.get(ps, 0, H.kp_track, m);
    if (H.word) l_dword.get(ps, 0, H.word, m);
    if (H.weight) l_dweight.get(ps, 0, H.weight, m);
    if (H.sorted_x) l_dsx.get(ps, 0, H.sorted_x, m);
    if (H.sorted_y) l_dsy.get(ps, 0, H.sorted_y, m);
    if (H.sorted_idx) l_dsidx.get(ps, 0, H.sorted_idx, m);
    if (H.octave) l_doct.get(ps, 0, H.octave, m);
    if (H.desc) l_ddesc.get(ps, 0, H.desc, 8 * m);
    c->admit_word = A.word; c->admit_weight = A.weight; c->admit_n = n;
    return MS_OK;
}

// The descent of the latest successful ms_keyframe_admit where it lies in the workspace: what ms_bow_db_add_words takes.
extern "C" int ms_keyframe_admit_words(ms_ctx *c, const int32_t **word, const double **weight, int32_t *n) {
    if (!c) return MS_ERR_INVALID;
    if (!word || !weight || !n) return ms_fail(c, MS_ERR_INVALID, "keyframe admit words: missing output");
    *word = nullptr; *weight = nullptr; *n = 0;
    if (c->admit_n < 0) return ms_fail(c, MS_ERR_INVALID, "keyframe admit words: no successful ms_keyframe_admit on this context since the last one that failed");
    *word = c->admit_word; *weight = c->admit_weight; *n = c->admit_n;
    return MS_OK;
}
