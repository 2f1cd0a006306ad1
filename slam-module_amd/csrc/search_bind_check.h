// search_bind_check.h -- the validation half of ms_bound_mask and ms_search_bind (search_bind.hip).  Plain C++17, no HIP and no context: it
// reads the HOST arguments only and asks of the DEVICE arrays nothing but whether they are there, so a program can compile it alone
// (SEARCH_BIND_HOST_ONLY) and run it under sanitizers.
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "../../include/mi355slam.h"

namespace ms_sbind {

inline int why_is(int code, char *why, size_t bytes, const char *fmt, ...) {
    if (why && bytes) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(why, bytes, fmt, ap);
        va_end(ap);
    }
    return code;
}

// what both entry points ask of the keyframe table, of the slot and of its keypoint count
inline int check_slot(const char *who, const int32_t *kf_mp, int n_kf, int stride, int n_mp, int slot, int n_kp, char *why, size_t bytes) {
    if (n_kf < 0 || n_mp < 0 || n_kp < 0) return why_is(MS_ERR_INVALID, why, bytes, "%s: negative size (%d slots, %d map points, %d keypoints)", who, n_kf, n_mp, n_kp);
    if (stride < 1) return why_is(MS_ERR_INVALID, why, bytes, "%s: stride %d", who, stride);
    if (n_kf > MS_COVIS_MAX_KF || stride > MS_COVIS_MAX_STRIDE || n_mp >= MS_COVIS_MAX_MP)
        return why_is(MS_ERR_CAPACITY, why, bytes, "%s: %d slots / stride %d / %d map points, caps %d / %d / below %d", who, n_kf, stride, n_mp, MS_COVIS_MAX_KF,
                      MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP);
    if (!kf_mp) return why_is(MS_ERR_INVALID, why, bytes, "%s: missing array (kf_mp)", who);
    if (slot < 0 || slot >= n_kf) return why_is(MS_ERR_INVALID, why, bytes, "%s: slot %d outside [0, %d)", who, slot, n_kf);
    if (n_kp > stride) return why_is(MS_ERR_INVALID, why, bytes, "%s: %d keypoints for a stride of %d", who, n_kp, stride);
    return MS_OK;
}

inline int check_mask(const int32_t *kf_mp, int n_kf, int stride, int n_mp, int slot, int n_kp, const uint8_t *skip, char *why, size_t bytes) {
    int rc;
    if ((rc = check_slot("bound mask", kf_mp, n_kf, stride, n_mp, slot, n_kp, why, bytes))) return rc;
    if (n_kp > 0 && !skip) return why_is(MS_ERR_INVALID, why, bytes, "bound mask: missing array (skip)");
    return MS_OK;
}

inline int check_bind(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const int32_t *n_obs, int n_mp, const int32_t *kept_entry, const float *q_x,
                      const float *q_y, const float *q_radius, const uint32_t *q_desc, const int32_t *top_idx, const uint16_t *top_dist, const int32_t *top_octave,
                      const int32_t *n_scored, const uint8_t *skip, const float *sorted_x, const float *sorted_y, const int32_t *sorted_idx, const uint32_t *t_desc,
                      const int32_t *t_octave, int n_kp, const int32_t *mp_index, int first, int count, int n_kept, int slot, const int32_t *n_matched,
                      const int32_t *counts, char *why, size_t bytes) {
    int rc;
    if ((rc = check_slot("search bind", kf_mp, n_kf, stride, n_mp, slot, n_kp, why, bytes))) return rc;
    if (first < 0 || count < 0 || n_kept < 0) return why_is(MS_ERR_INVALID, why, bytes, "search bind: negative size (first %d, count %d, n_kept %d)", first, count, n_kept);
    if (count >= MS_GATE_MAX_ENTRIES || first >= MS_GATE_MAX_ENTRIES - count)
        return why_is(MS_ERR_CAPACITY, why, bytes, "search bind: a slice [%d, %d + %d), cap below %d entries", first, first, count, MS_GATE_MAX_ENTRIES);
    if (n_kept > count) return why_is(MS_ERR_INVALID, why, bytes, "search bind: n_kept %d for a slice of %d", n_kept, count);
    if (!n_matched || !counts) return why_is(MS_ERR_INVALID, why, bytes, "search bind: missing array (n_matched or counts)");
    if (n_mp > 0 && (!mp_live || !n_obs)) return why_is(MS_ERR_INVALID, why, bytes, "search bind: missing array (mp_live or n_obs)");
    if (count > 0 && !mp_index) return why_is(MS_ERR_INVALID, why, bytes, "search bind: missing array (mp_index)");
    if (n_kept > 0 && (!kept_entry || !q_x || !q_y || !q_radius || !q_desc || !top_idx || !top_dist || !top_octave || !n_scored))
        return why_is(MS_ERR_INVALID, why, bytes, "search bind: missing array (a list of the gate or of the scoring)");
    if (n_kept > 0 && n_kp > 0 && (!skip || !sorted_x || !sorted_y || !sorted_idx || !t_desc || !t_octave))
        return why_is(MS_ERR_INVALID, why, bytes, "search bind: missing array (skip or a keyframe array)");
    if (((uintptr_t)q_desc | (uintptr_t)t_desc) & 15) return why_is(MS_ERR_INVALID, why, bytes, "search bind: q_desc and t_desc must be 16-byte aligned");
    for (int e = first; e < first + count; ++e)
        if (mp_index[e] < 0 || mp_index[e] >= n_mp) return why_is(MS_ERR_INVALID, why, bytes, "search bind: entry %d is row %d outside [0, %d)", e, mp_index[e], n_mp);
    return MS_OK;
}

}  // namespace ms_sbind

#ifdef SEARCH_BIND_HOST_ONLY
// the exported validation entry points as the library defines them, for a program that carries its own copy
extern "C" int ms_bound_mask_check(const int32_t *kf_mp, int n_kf, int stride, int n_mp, int slot, int n_kp, const uint8_t *skip, char *why, size_t why_bytes) {
    return ms_sbind::check_mask(kf_mp, n_kf, stride, n_mp, slot, n_kp, skip, why, why_bytes);
}
extern "C" int ms_search_bind_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const int32_t *n_obs, int n_mp, const int32_t *kept_entry,
                                    const float *q_x, const float *q_y, const float *q_radius, const int32_t *q_min_octave, const int32_t *q_max_octave,
                                    const uint32_t *q_desc, const int32_t *top_idx, const uint16_t *top_dist, const int32_t *top_octave, const int32_t *n_scored,
                                    const uint8_t *skip, const float *sorted_x, const float *sorted_y, const int32_t *sorted_idx, const uint32_t *t_desc,
                                    const int32_t *t_octave, int n_kp, const int32_t *mp_index, int first, int count, int n_kept, int slot, const int32_t *n_matched,
                                    const int32_t *counts, char *why, size_t why_bytes) {
    (void)q_min_octave; (void)q_max_octave;                  // each may be NULL: no window on that side
    return ms_sbind::check_bind(kf_mp, n_kf, stride, mp_live, n_obs, n_mp, kept_entry, q_x, q_y, q_radius, q_desc, top_idx, top_dist, top_octave, n_scored, skip, sorted_x,
                                sorted_y, sorted_idx, t_desc, t_octave, n_kp, mp_index, first, count, n_kept, slot, n_matched, counts, why, why_bytes);
}
#endif
