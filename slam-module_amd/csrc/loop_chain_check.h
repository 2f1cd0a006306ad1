// loop_chain_check.h -- the validation half of ms_loop_usable_mask, ms_loop_pairs and ms_loop_sim3_lists (loop_chain.hip).  Plain C++17, no HIP
// and no context: it reads the HOST arguments only and asks of the DEVICE arrays nothing but whether they are there, so a program can compile
// it alone (LOOP_CHAIN_HOST_ONLY) and run it under sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/mi355slam.h"

namespace ms_loopc {

inline int why_is(int code, char *why, size_t bytes, const char *fmt, ...) {
    if (why && bytes) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(why, bytes, fmt, ap);
        va_end(ap);
    }
    return code;
}

// what all three entry points ask of the tables' sizes: signs, the stride, the caps; n = the listed slots / candidates and its cap
inline int check_sizes(const char *who, int n_kf, int stride, int n_mp, int n, int n_cap, char *why, size_t bytes) {
    if (n_kf < 0 || n_mp < 0 || n < 0) return why_is(MS_ERR_INVALID, why, bytes, "%s: negative size (%d slots, %d map points, %d listed)", who, n_kf, n_mp, n);
    if (stride < 1) return why_is(MS_ERR_INVALID, why, bytes, "%s: stride %d", who, stride);
    if (n_kf > MS_COVIS_MAX_KF || stride > MS_COVIS_MAX_STRIDE || n_mp >= MS_COVIS_MAX_MP || n > n_cap)
        return why_is(MS_ERR_CAPACITY, why, bytes, "%s: %d slots / stride %d / %d map points / %d listed, caps %d / %d / below %d / %d", who, n_kf, stride, n_mp, n,
                      MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, n_cap);
    return MS_OK;
}

inline int check_mask(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, int n_mp, const int32_t *slots, const int32_t *n_kp,
                      const int32_t *require_triangulated, uint8_t *const *usable, int32_t *const *tri_row, int n_slots, char *why, size_t bytes) {
    (void)mp_live;                                           // may be NULL: every row is live
    int rc;
    if ((rc = check_sizes("loop mask", n_kf, stride, n_mp, n_slots, MS_COVIS_MAX_QUERIES, why, bytes))) return rc;
    if (n_slots > 0 && (!kf_mp || !slots || !n_kp || !require_triangulated || !usable))
        return why_is(MS_ERR_INVALID, why, bytes, "loop mask: missing array (kf_mp, slots, n_kp, require_triangulated or usable)");
    for (int s = 0; s < n_slots; ++s) {
        if (slots[s] < 0 || slots[s] >= n_kf) return why_is(MS_ERR_INVALID, why, bytes, "loop mask: slot %d outside [0, %d)", slots[s], n_kf);
        if (n_kp[s] < 0 || n_kp[s] > stride) return why_is(MS_ERR_INVALID, why, bytes, "loop mask: %d keypoints in a table of stride %d", n_kp[s], stride);
        if (n_kp[s] > 0 && !usable[s]) return why_is(MS_ERR_INVALID, why, bytes, "loop mask: missing array (usable of slot %d)", slots[s]);
        if (!mp_flags && (require_triangulated[s] || (tri_row && tri_row[s])))
            return why_is(MS_ERR_INVALID, why, bytes, "loop mask: slot %d requires TRIANGULATED or asks for tri_row with mp_flags == NULL", slots[s]);
    }
    return MS_OK;
}

// the current keyframe and the candidates: in range, distinct, cur not among them, keypoint counts inside the stride
inline int check_candidates(const char *who, int n_kf, int stride, int cur, int n_kp_cur, const int32_t *cand_slot, const int32_t *n_kp_cand, int n_cand, char *why,
                            size_t bytes) {
    if (cur < 0 || cur >= n_kf) return why_is(MS_ERR_INVALID, why, bytes, "%s: slot %d outside [0, %d)", who, cur, n_kf);
    if (n_kp_cur < 0 || n_kp_cur > stride) return why_is(MS_ERR_INVALID, why, bytes, "%s: %d keypoints in a table of stride %d", who, n_kp_cur, stride);
    if (n_cand > 0 && (!cand_slot || !n_kp_cand)) return why_is(MS_ERR_INVALID, why, bytes, "%s: missing array (cand_slot or n_kp_cand)", who);
    for (int c = 0; c < n_cand; ++c) {
        if (cand_slot[c] < 0 || cand_slot[c] >= n_kf) return why_is(MS_ERR_INVALID, why, bytes, "%s: slot %d outside [0, %d)", who, cand_slot[c], n_kf);
        if (cand_slot[c] == cur) return why_is(MS_ERR_INVALID, why, bytes, "%s: the current keyframe's slot %d is among the candidates", who, cur);
        if (n_kp_cand[c] < 0 || n_kp_cand[c] > stride) return why_is(MS_ERR_INVALID, why, bytes, "%s: %d keypoints in a table of stride %d", who, n_kp_cand[c], stride);
    }
    if (n_cand > 1) {
        std::vector<int32_t> sorted(cand_slot, cand_slot + n_cand);
        std::sort(sorted.begin(), sorted.end());
        for (int c = 1; c < n_cand; ++c)
            if (sorted[c] == sorted[c - 1]) return why_is(MS_ERR_INVALID, why, bytes, "%s: candidate slot %d is listed twice", who, sorted[c]);
    }
    return MS_OK;
}

inline int check_levels(const char *who, const float *level_sigma_sq, int n_levels, char *why, size_t bytes) {
    if (n_levels < 1 || n_levels > MS_TRI_MAX_LEVELS) return why_is(MS_ERR_INVALID, why, bytes, "%s: %d levels outside [1, %d]", who, n_levels, MS_TRI_MAX_LEVELS);
    if (!level_sigma_sq) return why_is(MS_ERR_INVALID, why, bytes, "%s: missing array (level_sigma_sq)", who);
    for (int l = 0; l < n_levels; ++l)
        if (!(std::isfinite(level_sigma_sq[l]) && level_sigma_sq[l] > 0.f))
            return why_is(MS_ERR_INVALID, why, bytes, "%s: level_sigma_sq[%d] = %g", who, l, (double)level_sigma_sq[l]);
    return MS_OK;
}

inline int check_pairs(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const double *mp_pos, int n_mp, const double *kf_pose, const int32_t *kp_octave,
                       int cur, int n_kp_cur, const int32_t *cand_slot, const int32_t *n_kp_cand, const int32_t *const *matched, int n_cand, const float *level_sigma_sq,
                       int n_levels, int cap_pairs, const int32_t *pair_start, const int32_t *kp1, const int32_t *kp2, const int32_t *row1, const int32_t *row2,
                       const double *pts1, const double *pts2, const float *thr1, const float *thr2, const double *cur_pose, const double *cand_pose, const int32_t *n_pairs,
                       char *why, size_t bytes) {
    (void)mp_live;                                           // may be NULL: every row is live
    int rc;
    if (cap_pairs < 0) return why_is(MS_ERR_INVALID, why, bytes, "loop pairs: negative size (capacity %d)", cap_pairs);
    if ((rc = check_sizes("loop pairs", n_kf, stride, n_mp, n_cand, MS_LOOP_MAX_CANDIDATES, why, bytes))) return rc;
    if (!kf_mp || !kf_pose || !kp_octave || (n_mp > 0 && !mp_pos)) return why_is(MS_ERR_INVALID, why, bytes, "loop pairs: missing array (kf_mp, kf_pose, kp_octave or mp_pos)");
    if (!pair_start || !n_pairs || !cur_pose || (n_cand > 0 && !cand_pose))
        return why_is(MS_ERR_INVALID, why, bytes, "loop pairs: missing array (pair_start, n_pairs, cur_pose or cand_pose)");
    if (cap_pairs > 0 && (!kp1 || !kp2 || !row1 || !row2 || !pts1 || !pts2 || !thr1 || !thr2))
        return why_is(MS_ERR_INVALID, why, bytes, "loop pairs: missing array (kp1, kp2, row1, row2, pts1, pts2, thr1 or thr2)");
    if ((rc = check_candidates("loop pairs", n_kf, stride, cur, n_kp_cur, cand_slot, n_kp_cand, n_cand, why, bytes))) return rc;
    if (n_cand > 0 && !matched) return why_is(MS_ERR_INVALID, why, bytes, "loop pairs: missing array (matched)");
    for (int c = 0; c < n_cand && n_kp_cur > 0; ++c)
        if (!matched[c]) return why_is(MS_ERR_INVALID, why, bytes, "loop pairs: missing array (matched of candidate slot %d)", cand_slot[c]);
    return check_levels("loop pairs", level_sigma_sq, n_levels, why, bytes);
}

inline int check_sim3_lists(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const double *mp_pos, int n_mp, const double *kf_pose, const float *kp_x,
                            const float *kp_y, const int32_t *kp_octave, int cur, int n_kp_cur, const int32_t *cand_slot, const int32_t *n_kp_cand, int n_cand,
                            const ms_pinhole *kf_cam, const float *level_sigma_sq, int n_levels, const int32_t *kp1, const int32_t *kp2, const int32_t *match_start,
                            const double *pts1, const double *pts2, const double *obs1, const double *obs2, const float *info1, const float *info2, const int32_t *row1,
                            const int32_t *row2, char *why, size_t bytes) {
    (void)mp_live;                                           // may be NULL: every row is live
    int rc;
    if ((rc = check_sizes("loop sim3 lists", n_kf, stride, n_mp, n_cand, MS_LOOP_MAX_CANDIDATES, why, bytes))) return rc;
    if (!kf_mp || !kf_pose || !kp_x || !kp_y || !kp_octave || !kf_cam || (n_mp > 0 && !mp_pos))
        return why_is(MS_ERR_INVALID, why, bytes, "loop sim3 lists: missing array (kf_mp, kf_pose, kp_x, kp_y, kp_octave, kf_cam or mp_pos)");
    if (!match_start) return why_is(MS_ERR_INVALID, why, bytes, "loop sim3 lists: missing array (match_start)");
    if ((rc = check_candidates("loop sim3 lists", n_kf, stride, cur, n_kp_cur, cand_slot, n_kp_cand, n_cand, why, bytes))) return rc;
    if (match_start[0] != 0) return why_is(MS_ERR_INVALID, why, bytes, "loop sim3 lists: match_start[0] = %d", match_start[0]);
    for (int c = 0; c < n_cand; ++c) {
        const long long n = (long long)match_start[c + 1] - match_start[c];
        if (n < 0) return why_is(MS_ERR_INVALID, why, bytes, "loop sim3 lists: match_start descends at candidate %d (%d after %d)", c, match_start[c + 1], match_start[c]);
        if (n > stride)
            return why_is(MS_ERR_CAPACITY, why, bytes, "loop sim3 lists: %lld matches for candidate slot %d, more than the stride of %d", n, cand_slot[c], stride);
    }
    if (match_start[n_cand] > 0 && (!kp1 || !kp2 || !pts1 || !pts2 || !obs1 || !obs2 || !info1 || !info2 || !row1 || !row2))
        return why_is(MS_ERR_INVALID, why, bytes, "loop sim3 lists: missing array (kp1, kp2, pts1, pts2, obs1, obs2, info1, info2, row1 or row2)");
    for (int c = -1; c < n_cand; ++c) {
        const int slot = c < 0 ? cur : cand_slot[c];
        const ms_pinhole &K = kf_cam[slot];
        if (!(std::isfinite(K.fx) && K.fx > 0.0 && std::isfinite(K.fy) && K.fy > 0.0))
            return why_is(MS_ERR_INVALID, why, bytes, "loop sim3 lists: the camera of slot %d has fx %g, fy %g", slot, K.fx, K.fy);
        if (!std::isfinite(K.cx) || !std::isfinite(K.cy)) return why_is(MS_ERR_INVALID, why, bytes, "loop sim3 lists: the camera of slot %d has cx %g, cy %g", slot, K.cx, K.cy);
    }
    return check_levels("loop sim3 lists", level_sigma_sq, n_levels, why, bytes);
}

}  // namespace ms_loopc

#ifdef LOOP_CHAIN_HOST_ONLY
// the exported validation entry points as the library defines them, for a program that carries its own copy
extern "C" int ms_loop_usable_mask_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, int n_mp, const int32_t *slots,
                                         const int32_t *n_kp, const int32_t *require_triangulated, uint8_t *const *usable, int32_t *const *tri_row, int n_slots, char *why,
                                         size_t why_bytes) {
    return ms_loopc::check_mask(kf_mp, n_kf, stride, mp_flags, mp_live, n_mp, slots, n_kp, require_triangulated, usable, tri_row, n_slots, why, why_bytes);
}
extern "C" int ms_loop_pairs_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const double *mp_pos, int n_mp, const double *kf_pose,
                                   const int32_t *kp_octave, int cur, int n_kp_cur, const int32_t *cand_slot, const int32_t *n_kp_cand, const int32_t *const *matched,
                                   int n_cand, const float *level_sigma_sq, int n_levels, int cap_pairs, const int32_t *pair_start, const int32_t *kp1, const int32_t *kp2,
                                   const int32_t *row1, const int32_t *row2, const double *pts1, const double *pts2, const float *thr1, const float *thr2,
                                   const double *cur_pose, const double *cand_pose, const int32_t *n_pairs, char *why, size_t why_bytes) {
    return ms_loopc::check_pairs(kf_mp, n_kf, stride, mp_live, mp_pos, n_mp, kf_pose, kp_octave, cur, n_kp_cur, cand_slot, n_kp_cand, matched, n_cand, level_sigma_sq, n_levels,
                                 cap_pairs, pair_start, kp1, kp2, row1, row2, pts1, pts2, thr1, thr2, cur_pose, cand_pose, n_pairs, why, why_bytes);
}
extern "C" int ms_loop_sim3_lists_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const double *mp_pos, int n_mp, const double *kf_pose,
                                        const float *kp_x, const float *kp_y, const int32_t *kp_octave, int cur, int n_kp_cur, const int32_t *cand_slot,
                                        const int32_t *n_kp_cand, int n_cand, const ms_pinhole *kf_cam, const float *level_sigma_sq, int n_levels, const int32_t *kp1,
                                        const int32_t *kp2, const int32_t *match_start, const double *pts1, const double *pts2, const double *obs1, const double *obs2,
                                        const float *info1, const float *info2, const int32_t *row1, const int32_t *row2, char *why, size_t why_bytes) {
    return ms_loopc::check_sim3_lists(kf_mp, n_kf, stride, mp_live, mp_pos, n_mp, kf_pose, kp_x, kp_y, kp_octave, cur, n_kp_cur, cand_slot, n_kp_cand, n_cand, kf_cam,
                                      level_sigma_sq, n_levels, kp1, kp2, match_start, pts1, pts2, obs1, obs2, info1, info2, row1, row2, why, why_bytes);
}
#endif
