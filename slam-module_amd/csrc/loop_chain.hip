// loop_chain.hip -- the three pieces that join the batched solvers of LoopCloser::tryLoopClosure (loop_closer.cpp:126-378) on the device map
// tables: what still needed MapDB::mapPoints.at(...), observations.at(kf.id) and kf.mapPoints.at(i) on a host copy of the map.
//   ms_loop_usable_mask   the M1 masks of matchForLoopClosures ("has a TRIANGULATED map point", keyframe_matcher.cpp:79-84, :94-96) and the
//                         mps1 / mps2 rows of matchMapPointsSim3 (:568-571), for whole slots, in one launch
//   ms_loop_pairs         loop_closer.cpp:203-213 and the LoopRansac constructor (loop_ransac.cpp:17-41) for all candidates: matchedFeatureIds
//                         becomes the map-point pairs, the two camera-frame point clouds and the two threshold arrays, CSR over candidates
//   ms_loop_sim3_lists    optimize_transform.cpp:44-59 and :101-142 (getMpVertex and the two edges per match): the arrays of an
//                         ms_sim3_opt_problem for the final match lists
//
// ms_loop_pairs is a stream compaction per candidate, three launches whatever n_cand is:
//   k_pairs_count     ONE workgroup per candidate walks the current keyframe's keypoints in trips of 256, counts the kept pairs (block_rank,
//                     ms_scan.h, a carried count) and the violations; it writes nothing but those counts
//   k_pairs_offsets   ONE workgroup: block_offsets over the candidates' counts (a second trip beyond 256 candidates) -> pair_start, n_pairs
//   k_pairs_pack      nothing when a violation was counted or the pairs do not fit; else the same walk with the offset known, and the poses
// ms_loop_sim3_lists keeps the order of its input: one thread per listed match, one launch.  Its kernel writes into the workspace's staging
// block, not into anything of the caller's: a thread that finds a violation counts it and returns, the others still write their entries
// there, and "nothing written" holds because the host copies nothing out of the block when the count is not zero.
// Integer arithmetic decides every position, the compaction keeps keypoint order, the only atomics are integer counters; the float64
// expressions are written with *_rn intrinsics in the order the header pins.  The stores are plain vector stores.
#include "ms_internal.h"
#include "ms_scan.h"
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int kHead = 8;                 // int32 in front of the downloaded block: n_pairs | violations
constexpr float kChiSq2D = 9.21034f;     // CHI_SQ_2D, loop_ransac.cpp:28

__device__ __forceinline__ bool present(int32_t r, int n_mp, const uint8_t *live) { return (uint32_t)r < (uint32_t)n_mp && (!live || live[r] != 0); }

// poseCW * p: x_i = ((R[i][0] * p0 + R[i][1] * p1) + R[i][2] * p2) + t_i, float64, no contraction; P = rows 0-2 of poseCW, row-major 3 x 4
__device__ __forceinline__ void cam_point(const double *P, const double *p, double *out) {
    const double p0 = p[0], p1 = p[1], p2 = p[2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        out[i] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P[4 * i], p0), __dmul_rn(P[4 * i + 1], p1)), __dmul_rn(P[4 * i + 2], p2)), P[4 * i + 3]);
}

// ------------------------------------------------------------------------------------------------ masks
struct MaskSlot {
    uint8_t *usable;
    int32_t *tri_row;                    // may be null
    int32_t slot, n_kp, require, pad;
};

__global__ __launch_bounds__(kBlock) void k_loop_mask(const int32_t *kf_mp, const uint8_t *mp_flags, const uint8_t *mp_live, const MaskSlot *slots, int stride, int n_mp) {
    const MaskSlot S = slots[blockIdx.y];
    const int k = blockIdx.x * kBlock + (int)threadIdx.x;
    if (k >= S.n_kp) return;
    const int32_t r = kf_mp[(size_t)S.slot * stride + k];
    const bool there = present(r, n_mp, mp_live);
    const bool tri = there && mp_flags && (mp_flags[r] & 1);
    S.usable[k] = (uint8_t)(there && (!S.require || tri));
    if (S.tri_row) S.tri_row[k] = tri ? r : -1;
}

// ------------------------------------------------------------------------------------------------ pairs
struct PairCand {
    const int32_t *matched;              // DEVICE [n_kp_cur]
    int32_t slot, n_kp;
};

struct PairArgs {
    const int32_t *kf_mp;
    const uint8_t *mp_live;
    const double *mp_pos, *kf_pose;
    const int32_t *kp_octave;
    const PairCand *cand;                // [n_cand]
    const float *sigma;                  // [n_levels]
    int32_t *cnt;                        // [n_cand] kept pairs per candidate
    int32_t *head, *pair_start;          // the block that goes down, on the device
    int32_t *kp1, *kp2, *row1, *row2;
    double *pts1, *pts2;
    float *thr1, *thr2;
    double *cur_pose, *cand_pose;
    int32_t stride, n_mp, n_levels, cur, n_kp_cur, n_cand, cap_pairs;
};

// keypoint i of the current keyframe against candidate C: kept or dropped; `bad` for a matched value outside [-1, n_kp) or a kept pair's
// octave outside the levels.  Nothing outside the tables is read.
__device__ __forceinline__ bool pair_of(const PairArgs &A, const PairCand &C, int i, int32_t &m, int32_t &r1, int32_t &r2, int32_t &o1, int32_t &o2, bool &bad) {
    m = C.matched[i];
    if (m < -1 || m >= C.n_kp) { bad = true; return false; }
    if (m < 0) return false;
    r1 = A.kf_mp[(size_t)A.cur * A.stride + i];
    if (!present(r1, A.n_mp, A.mp_live)) return false;
    r2 = A.kf_mp[(size_t)C.slot * A.stride + m];
    if (!present(r2, A.n_mp, A.mp_live) || r1 == r2) return false;
    o1 = A.kp_octave[(size_t)A.cur * A.stride + i];
    o2 = A.kp_octave[(size_t)C.slot * A.stride + m];
    if ((uint32_t)o1 >= (uint32_t)A.n_levels || (uint32_t)o2 >= (uint32_t)A.n_levels) bad = true;
    return true;
}

__global__ __launch_bounds__(kBlock) void k_pairs_count(const PairArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const PairCand C = A.cand[blockIdx.x];
    int carry = 0;                                           // the same in every lane
    for (int i0 = 0; i0 < A.n_kp_cur; i0 += kBlock) {
        const int i = i0 + (int)threadIdx.x;
        int32_t m, r1, r2, o1, o2;
        bool bad = false;
        const bool kept = i < A.n_kp_cur && pair_of(A, C, i, m, r1, r2, o1, o2, bad);
        if (bad) atomicAdd(A.head + 1, 1);
        int total;
        block_rank<kBlock>(kept, s_wave, total);
        carry += total;
        __syncthreads();                                     // s_wave is free again
    }
    if (threadIdx.x == 0) A.cnt[blockIdx.x] = carry;
}

// ONE workgroup: the candidates' counts become pair_start, the total goes to the head
__global__ __launch_bounds__(kBlock) void k_pairs_offsets(const PairArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int total = block_offsets<kBlock>(A.cnt, A.pair_start, A.n_cand, s_wave);
    if (threadIdx.x == 0) { A.pair_start[A.n_cand] = total; A.head[0] = total; }
}

__global__ __launch_bounds__(kBlock) void k_pairs_pack(const PairArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    if (A.head[1] || A.head[0] > A.cap_pairs) return;        // the same in every lane of every workgroup: nothing is written
    const PairCand C = A.cand[blockIdx.x];
    const double *P1 = A.kf_pose + 12 * (size_t)A.cur, *P2 = A.kf_pose + 12 * (size_t)C.slot;
    if (threadIdx.x < 12) {
        A.cand_pose[12 * (size_t)blockIdx.x + threadIdx.x] = P2[threadIdx.x];
        if (blockIdx.x == 0) A.cur_pose[threadIdx.x] = P1[threadIdx.x];
    }
    int base = A.pair_start[blockIdx.x];                     // the same in every lane; inside [0, cap_pairs]
    for (int i0 = 0; i0 < A.n_kp_cur; i0 += kBlock) {
        const int i = i0 + (int)threadIdx.x;
        int32_t m = -1, r1 = -1, r2 = -1, o1 = 0, o2 = 0;
        bool bad = false;
        const bool kept = i < A.n_kp_cur && pair_of(A, C, i, m, r1, r2, o1, o2, bad);
        int total;
        const int e = base + block_rank<kBlock>(kept, s_wave, total);
        if (kept) {                                          // e < head[0] <= cap_pairs: the count pass made the same decisions
            A.kp1[e] = i; A.kp2[e] = m; A.row1[e] = r1; A.row2[e] = r2;
            cam_point(P1, A.mp_pos + 3 * (size_t)r1, A.pts1 + 3 * (size_t)e);
            cam_point(P2, A.mp_pos + 3 * (size_t)r2, A.pts2 + 3 * (size_t)e);
            A.thr1[e] = __fmul_rn(kChiSq2D, A.sigma[o1]);    // octaves inside the levels: a violation would have stopped the kernel
            A.thr2[e] = __fmul_rn(kChiSq2D, A.sigma[o2]);
        }
        base += total;
        __syncthreads();                                     // s_wave is free again
    }
}

// ------------------------------------------------------------------------------------------------ sim3 lists
struct SimCand {
    int32_t slot, n_kp;
    double fx, fy, cx, cy;
};

struct SimArgs {
    const int32_t *kf_mp;
    const uint8_t *mp_live;
    const double *mp_pos, *kf_pose;
    const float *kp_x, *kp_y;
    const int32_t *kp_octave;
    const SimCand *cand;                 // [n_cand + 1]: the candidates, then the current keyframe
    const float *sigma;
    const int32_t *kp1, *kp2, *ecand;    // [n_match]: the lists, and the candidate of each entry
    int32_t *head, *row1, *row2;         // the block that goes down, on the device
    double *pts1, *pts2, *obs1, *obs2;
    float *info1, *info2;
    int32_t stride, n_mp, n_levels, n_cand, n_match;
};

__global__ __launch_bounds__(kBlock) void k_sim3_lists(const SimArgs A) {
    const int e = blockIdx.x * kBlock + (int)threadIdx.x;
    if (e >= A.n_match) return;
    const SimCand K1 = A.cand[A.n_cand], K2 = A.cand[A.ecand[e]];                // ecand is the host's: inside [0, n_cand)
    const int32_t a = A.kp1[e], b = A.kp2[e];
    bool bad = (uint32_t)a >= (uint32_t)K1.n_kp || (uint32_t)b >= (uint32_t)K2.n_kp;
    int32_t r1 = -1, r2 = -1, o1 = 0, o2 = 0;
    const size_t at1 = (size_t)K1.slot * A.stride + (bad ? 0 : a), at2 = (size_t)K2.slot * A.stride + (bad ? 0 : b);
    if (!bad) {
        r1 = A.kf_mp[at1]; r2 = A.kf_mp[at2];
        bad = !present(r1, A.n_mp, A.mp_live) || !present(r2, A.n_mp, A.mp_live);
    }
    if (!bad) {
        o1 = A.kp_octave[at1]; o2 = A.kp_octave[at2];
        bad = (uint32_t)o1 >= (uint32_t)A.n_levels || (uint32_t)o2 >= (uint32_t)A.n_levels;
    }
    if (bad) { atomicAdd(A.head + 1, 1); return; }           // the other threads still fill the staging block; the host copies none of it out when the count is not zero
    A.row1[e] = r1; A.row2[e] = r2;
    cam_point(A.kf_pose + 12 * (size_t)K1.slot, A.mp_pos + 3 * (size_t)r1, A.pts1 + 3 * (size_t)e);
    cam_point(A.kf_pose + 12 * (size_t)K2.slot, A.mp_pos + 3 * (size_t)r2, A.pts2 + 3 * (size_t)e);
    A.obs1[2 * (size_t)e] = __ddiv_rn(__dsub_rn((double)A.kp_x[at1], K1.cx), K1.fx);                   // the obs_uv rule of ms_ba_window_lists
    A.obs1[2 * (size_t)e + 1] = __ddiv_rn(__dsub_rn((double)A.kp_y[at1], K1.cy), K1.fy);
    A.obs2[2 * (size_t)e] = __ddiv_rn(__dsub_rn((double)A.kp_x[at2], K2.cx), K2.fx);
    A.obs2[2 * (size_t)e + 1] = __ddiv_rn(__dsub_rn((double)A.kp_y[at2], K2.cy), K2.fy);
    A.info1[e] = A.sigma[o1];                                // optimize_transform.cpp:122, :137: multiplied by, not divided
    A.info2[e] = A.sigma[o2];
}

}  // namespace

extern "C" int ms_loop_usable_mask(ms_ctx *c, const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, int n_mp, const int32_t *slots,
                                   const int32_t *n_kp, const int32_t *require_triangulated, uint8_t *const *usable, int32_t *const *tri_row, int n_slots) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_loop_usable_mask_check(kf_mp, n_kf, stride, mp_flags, mp_live, n_mp, slots, n_kp, require_triangulated, usable, tri_row, n_slots, c->err, sizeof(c->err))))
        return rc;
    int longest = 0;
    for (int s = 0; s < n_slots; ++s) longest = n_kp[s] > longest ? n_kp[s] : longest;
    if (longest == 0) return MS_OK;
    MsRange range("loopUsableMask");
    MsLayout up;
    const auto l_slots = up.array<MaskSlot>((size_t)n_slots);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_LOOP_CHAIN];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, up.end, false))) return rc;
    MaskSlot *S = l_slots.at(W.host);
    for (int s = 0; s < n_slots; ++s) {
        S[s].usable = usable[s]; S[s].tri_row = tri_row ? tri_row[s] : nullptr;
        S[s].slot = slots[s]; S[s].n_kp = n_kp[s]; S[s].require = require_triangulated[s] != 0; S[s].pad = 0;
    }
    MS_HIP(c, hipMemcpyAsync(W.dev, W.host, up.end, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_loop_mask, dim3(ms_div_up(longest, kBlock), n_slots), dim3(kBlock), 0, c->stream, kf_mp, mp_flags, mp_live, l_slots.at(W.dev), stride, n_mp);
    MS_KERNEL_CHECK(c, "k_loop_mask");
    MS_HIP(c, hipStreamSynchronize(c->stream));                // the staging block is written again by the next call
    return MS_OK;
}

extern "C" int ms_loop_pairs(ms_ctx *c, const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const double *mp_pos, int n_mp, const double *kf_pose,
                             const int32_t *kp_octave, int cur, int n_kp_cur, const int32_t *cand_slot, const int32_t *n_kp_cand, const int32_t *const *matched, int n_cand,
                             const float *level_sigma_sq, int n_levels, int cap_pairs, int32_t *pair_start, int32_t *kp1, int32_t *kp2, int32_t *row1, int32_t *row2,
                             double *pts1, double *pts2, float *thr1, float *thr2, double *cur_pose, double *cand_pose, int32_t *n_pairs) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_loop_pairs_check(kf_mp, n_kf, stride, mp_live, mp_pos, n_mp, kf_pose, kp_octave, cur, n_kp_cur, cand_slot, n_kp_cand, matched, n_cand, level_sigma_sq,
                                  n_levels, cap_pairs, pair_start, kp1, kp2, row1, row2, pts1, pts2, thr1, thr2, cur_pose, cand_pose, n_pairs, c->err, sizeof(c->err))))
        return rc;
    if (n_cand == 0 || n_kp_cur == 0) {                      // no pair: no launch, the poses are not read
        *n_pairs = 0;
        std::memset(pair_start, 0, ((size_t)n_cand + 1) * sizeof(int32_t));
        return MS_OK;
    }
    MsRange range("loopPairs");
    const long long most = (long long)n_cand * n_kp_cur;     // n_pairs <= this
    const size_t n_out = (size_t)(most < cap_pairs ? most : cap_pairs);
    MsLayout up;                                             // upload block: candidate records | sigmas
    const auto l_cand = up.array<PairCand>((size_t)n_cand);
    const auto l_sigma = up.array<float>((size_t)n_levels);
    MsLayout down;                                           // the block that goes down: head | pair_start | the pairs' arrays | the poses
    const auto l_head = down.array<int32_t>(kHead);
    const auto l_start = down.array<int32_t>((size_t)n_cand + 1);
    const auto l_kp1 = down.array<int32_t>(n_out), l_kp2 = down.array<int32_t>(n_out), l_row1 = down.array<int32_t>(n_out), l_row2 = down.array<int32_t>(n_out);
    const auto l_pts1 = down.array<double>(3 * n_out), l_pts2 = down.array<double>(3 * n_out);
    const auto l_thr1 = down.array<float>(n_out), l_thr2 = down.array<float>(n_out);
    const auto l_cur = down.array<double>(12), l_pose = down.array<double>(12 * (size_t)n_cand);
    MsLayout dev = up;                                       // device block: the upload block | the candidates' counts | the block that goes down
    const auto l_cnt = dev.array<int32_t>((size_t)n_cand);
    const size_t down_at = dev.take(down.end);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_LOOP_CHAIN];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    if ((rc = ms_pinned(c, down.end))) return rc;
    void *hs = W.host, *ds = W.dev, *dd = static_cast<uint8_t *>(W.dev) + down_at, *hd = c->pinned;
    PairCand *C = l_cand.at(hs);
    for (int k = 0; k < n_cand; ++k) { C[k].matched = matched[k]; C[k].slot = cand_slot[k]; C[k].n_kp = n_kp_cand[k]; }
    l_sigma.fill(hs, level_sigma_sq);
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    MS_HIP(c, hipMemsetAsync(l_head.at(dd), 0, l_head.bytes(), c->stream));
    PairArgs A{};
    A.kf_mp = kf_mp; A.mp_live = mp_live; A.mp_pos = mp_pos; A.kf_pose = kf_pose; A.kp_octave = kp_octave;
    A.cand = l_cand.at(ds); A.sigma = l_sigma.at(ds); A.cnt = l_cnt.at(ds);
    A.head = l_head.at(dd); A.pair_start = l_start.at(dd);
    A.kp1 = l_kp1.at(dd); A.kp2 = l_kp2.at(dd); A.row1 = l_row1.at(dd); A.row2 = l_row2.at(dd);
    A.pts1 = l_pts1.at(dd); A.pts2 = l_pts2.at(dd); A.thr1 = l_thr1.at(dd); A.thr2 = l_thr2.at(dd);
    A.cur_pose = l_cur.at(dd); A.cand_pose = l_pose.at(dd);
    A.stride = stride; A.n_mp = n_mp; A.n_levels = n_levels; A.cur = cur; A.n_kp_cur = n_kp_cur; A.n_cand = n_cand; A.cap_pairs = cap_pairs;
    hipLaunchKernelGGL(k_pairs_count, dim3(n_cand), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_pairs_count");
    hipLaunchKernelGGL(k_pairs_offsets, dim3(1), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_pairs_offsets");
    hipLaunchKernelGGL(k_pairs_pack, dim3(n_cand), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_pairs_pack");
    MS_HIP(c, hipMemcpyAsync(hd, dd, down.end, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *head = l_head.at(hd);
    if (head[1])
        return ms_fail(c, MS_ERR_INVALID, "loop pairs: %d violations on the device (a matched value outside [-1, the candidate's keypoints) or a kept pair's octave "
                       "outside [0, %d)); nothing written", head[1], n_levels);
    *n_pairs = head[0];
    l_start.get(hd, 0, pair_start, (size_t)n_cand + 1);
    if (head[0] > cap_pairs) return ms_fail(c, MS_ERR_CAPACITY, "loop pairs: %d pairs, the caller's arrays hold %d (nothing written to them)", head[0], cap_pairs);
    const size_t n = (size_t)head[0];
    l_kp1.get(hd, 0, kp1, n); l_kp2.get(hd, 0, kp2, n); l_row1.get(hd, 0, row1, n); l_row2.get(hd, 0, row2, n);
    l_pts1.get(hd, 0, pts1, 3 * n); l_pts2.get(hd, 0, pts2, 3 * n); l_thr1.get(hd, 0, thr1, n); l_thr2.get(hd, 0, thr2, n);
    l_cur.get(hd, 0, cur_pose, 12); l_pose.get(hd, 0, cand_pose, 12 * (size_t)n_cand);
    return MS_OK;
}

extern "C" int ms_loop_sim3_lists(ms_ctx *c, const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const double *mp_pos, int n_mp, const double *kf_pose,
                                  const float *kp_x, const float *kp_y, const int32_t *kp_octave, int cur, int n_kp_cur, const int32_t *cand_slot, const int32_t *n_kp_cand,
                                  int n_cand, const ms_pinhole *kf_cam, const float *level_sigma_sq, int n_levels, const int32_t *kp1, const int32_t *kp2,
                                  const int32_t *match_start, double *pts1, double *pts2, double *obs1, double *obs2, float *info1, float *info2, int32_t *row1,
                                  int32_t *row2) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_loop_sim3_lists_check(kf_mp, n_kf, stride, mp_live, mp_pos, n_mp, kf_pose, kp_x, kp_y, kp_octave, cur, n_kp_cur, cand_slot, n_kp_cand, n_cand, kf_cam,
                                       level_sigma_sq, n_levels, kp1, kp2, match_start, pts1, pts2, obs1, obs2, info1, info2, row1, row2, c->err, sizeof(c->err))))
        return rc;
    const size_t n = (size_t)match_start[n_cand];            // <= n_cand * stride: the check
    if (n == 0) return MS_OK;
    MsRange range("loopSim3Lists");
    MsLayout up;                                             // upload block: candidate records, the current keyframe's last | sigmas | the lists | each entry's candidate
    const auto l_cand = up.array<SimCand>((size_t)n_cand + 1);
    const auto l_sigma = up.array<float>((size_t)n_levels);
    const auto l_a = up.array<int32_t>(n), l_b = up.array<int32_t>(n), l_of = up.array<int32_t>(n);
    MsLayout down;                                           // the block that goes down: head | rows | points | observations | informations
    const auto l_head = down.array<int32_t>(kHead);
    const auto l_row1 = down.array<int32_t>(n), l_row2 = down.array<int32_t>(n);
    const auto l_pts1 = down.array<double>(3 * n), l_pts2 = down.array<double>(3 * n), l_obs1 = down.array<double>(2 * n), l_obs2 = down.array<double>(2 * n);
    const auto l_info1 = down.array<float>(n), l_info2 = down.array<float>(n);
    MsLayout dev = up;
    const size_t down_at = dev.take(down.end);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_LOOP_CHAIN];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    if ((rc = ms_pinned(c, down.end))) return rc;
    void *hs = W.host, *ds = W.dev, *dd = static_cast<uint8_t *>(W.dev) + down_at, *hd = c->pinned;
    SimCand *C = l_cand.at(hs);
    for (int k = 0; k <= n_cand; ++k) {
        const int slot = k < n_cand ? cand_slot[k] : cur;
        C[k].slot = slot; C[k].n_kp = k < n_cand ? n_kp_cand[k] : n_kp_cur;
        C[k].fx = kf_cam[slot].fx; C[k].fy = kf_cam[slot].fy; C[k].cx = kf_cam[slot].cx; C[k].cy = kf_cam[slot].cy;
        if (k < n_cand)
            for (int e = match_start[k]; e < match_start[k + 1]; ++e) l_of.at(hs)[e] = k;
    }
    l_sigma.fill(hs, level_sigma_sq); l_a.fill(hs, kp1); l_b.fill(hs, kp2);
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    MS_HIP(c, hipMemsetAsync(l_head.at(dd), 0, l_head.bytes(), c->stream));
    SimArgs A{};
    A.kf_mp = kf_mp; A.mp_live = mp_live; A.mp_pos = mp_pos; A.kf_pose = kf_pose; A.kp_x = kp_x; A.kp_y = kp_y; A.kp_octave = kp_octave;
    A.cand = l_cand.at(ds); A.sigma = l_sigma.at(ds); A.kp1 = l_a.at(ds); A.kp2 = l_b.at(ds); A.ecand = l_of.at(ds);
    A.head = l_head.at(dd); A.row1 = l_row1.at(dd); A.row2 = l_row2.at(dd);
    A.pts1 = l_pts1.at(dd); A.pts2 = l_pts2.at(dd); A.obs1 = l_obs1.at(dd); A.obs2 = l_obs2.at(dd); A.info1 = l_info1.at(dd); A.info2 = l_info2.at(dd);
    A.stride = stride; A.n_mp = n_mp; A.n_levels = n_levels; A.n_cand = n_cand; A.n_match = (int32_t)n;
    hipLaunchKernelGGL(k_sim3_lists, dim3(ms_div_up((int)n, kBlock)), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_sim3_lists");
    MS_HIP(c, hipMemcpyAsync(hd, dd, down.end, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *head = l_head.at(hd);
    if (head[1])
        return ms_fail(c, MS_ERR_INVALID, "loop sim3 lists: %d violations on the device (a keypoint outside its keyframe, an entry whose row is not present or an octave "
                       "outside [0, %d)); nothing written", head[1], n_levels);
    l_row1.get(hd, 0, row1, n); l_row2.get(hd, 0, row2, n);
    l_pts1.get(hd, 0, pts1, 3 * n); l_pts2.get(hd, 0, pts2, 3 * n); l_obs1.get(hd, 0, obs1, 2 * n); l_obs2.get(hd, 0, obs2, 2 * n);
    l_info1.get(hd, 0, info1, n); l_info2.get(hd, 0, info2, n);
    return MS_OK;
}
