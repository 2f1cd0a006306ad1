// map_cull_check.h -- the validation half of ms_observation_count and ms_map_cull (map_cull.hip).  Plain C++17, no HIP and no context:
// it reads the HOST arrays only, so tests/map_cull_smoke.cpp can compile it alone (MAP_CULL_HOST_ONLY) and run it under sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/mi355slam.h"

namespace ms_cull {

inline int why_is(int code, char *why, size_t bytes, const char *fmt, ...) {
    if (why && bytes) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(why, bytes, fmt, ap);
        va_end(ap);
    }
    return code;
}

// order[i] = the slots with kf_id >= 0 by ascending kf_id.  False when a non-negative id is listed twice (*twice = that id).  The vector
// is the caller's and only grows.
inline bool slots_by_id(const int32_t *kf_id, int n_kf, std::vector<int32_t> &order, int32_t *twice) {
    order.clear();
    for (int k = 0; k < n_kf; ++k) if (kf_id[k] >= 0) order.push_back(k);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return kf_id[a] < kf_id[b]; });
    for (size_t i = 1; i < order.size(); ++i)
        if (kf_id[order[i - 1]] == kf_id[order[i]]) { *twice = kf_id[order[i]]; return false; }
    return true;
}

// slot_rank / rank_slot of an upload block from the slots in KfId order
inline void fill_ranks(const std::vector<int32_t> &order, int n_kf, int32_t *slot_rank, int32_t *rank_slot) {
    for (int k = 0; k < n_kf; ++k) slot_rank[k] = -1;
    for (size_t i = 0; i < order.size(); ++i) { slot_rank[order[i]] = (int32_t)i; rank_slot[i] = order[i]; }
}

inline int check_table(const char *who, const int32_t *kf_mp, int n_kf, int stride, int n_mp, const int32_t *kf_id, std::vector<int32_t> &order, char *why, size_t bytes) {
    if (n_kf < 0 || n_mp < 0) return why_is(MS_ERR_INVALID, why, bytes, "%s: negative size (%d slots, %d map points)", who, n_kf, n_mp);
    if (stride < 1) return why_is(MS_ERR_INVALID, why, bytes, "%s: stride %d", who, stride);
    if (n_kf > 0 && (!kf_mp || !kf_id)) return why_is(MS_ERR_INVALID, why, bytes, "%s: missing array (kf_mp or kf_id)", who);
    int32_t twice = 0;
    if (!slots_by_id(kf_id, n_kf, order, &twice)) return why_is(MS_ERR_INVALID, why, bytes, "%s: kf_id %d is listed twice", who, twice);
    return MS_OK;
}

inline int check_cull(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, int n_mp, const int32_t *kf_id, const double *kf_t,
                      const int32_t *cand, const uint8_t *cand_keep, int n_cand, const ms_cull_settings *s, const int32_t *removed_rows, const uint8_t *cand_removed,
                      const int32_t *n_removed_rows, const int32_t *n_removed_kf, std::vector<int32_t> &order, std::vector<int32_t> &sorted, char *why, size_t bytes) {
    (void)cand_keep;
    if (n_cand < 0) return why_is(MS_ERR_INVALID, why, bytes, "map cull: negative size (%d candidates)", n_cand);
    if (!s || !kf_t || !n_removed_rows || !n_removed_kf || (n_cand > 0 && (!cand || !cand_removed)) || (n_mp > 0 && (!mp_live || !removed_rows)))
        return why_is(MS_ERR_INVALID, why, bytes, "map cull: missing array");
    int rc;
    if ((rc = check_table("map cull", kf_mp, n_kf, stride, n_mp, kf_id, order, why, bytes))) return rc;
    if (s->cull_points && !mp_flags) return why_is(MS_ERR_INVALID, why, bytes, "map cull: cull_points is set and there is no mp_flags");
    if (!std::isfinite(s->min_age) || !std::isfinite(s->max_critical_ratio))
        return why_is(MS_ERR_INVALID, why, bytes, "map cull: min_age %g or max_critical_ratio %g is not finite", s->min_age, s->max_critical_ratio);
    if (s->min_obs_for_ba < 0) return why_is(MS_ERR_INVALID, why, bytes, "map cull: min_obs_for_ba %d", s->min_obs_for_ba);
    const int32_t cur = s->current_slot;
    if (cur < 0 || cur >= n_kf) return why_is(MS_ERR_INVALID, why, bytes, "map cull: current slot %d outside [0, %d)", cur, n_kf);
    if (kf_id[cur] < 0) return why_is(MS_ERR_INVALID, why, bytes, "map cull: current slot %d is empty (kf_id %d)", cur, kf_id[cur]);
    for (int32_t k : order) {
        if (!std::isfinite(kf_t[k])) return why_is(MS_ERR_INVALID, why, bytes, "map cull: kf_t of slot %d is not finite", k);
        const double age = kf_t[cur] - kf_t[k];
        if (!(std::fabs(age) < 2147483648.0)) return why_is(MS_ERR_INVALID, why, bytes, "map cull: the age %g of slot %d is outside int32", age, k);
    }
    for (int i = 0; i < n_cand; ++i) {
        if (cand[i] < 0 || cand[i] >= n_kf) return why_is(MS_ERR_INVALID, why, bytes, "map cull: candidate %d: slot %d outside [0, %d)", i, cand[i], n_kf);
        if (cand[i] == cur) return why_is(MS_ERR_INVALID, why, bytes, "map cull: candidate %d is the current slot %d", i, cur);
        if (kf_id[cand[i]] < 0) return why_is(MS_ERR_INVALID, why, bytes, "map cull: candidate %d: slot %d is empty (kf_id %d)", i, cand[i], kf_id[cand[i]]);
    }
    sorted.assign(cand, cand + n_cand);
    std::sort(sorted.begin(), sorted.end());
    for (int i = 1; i < n_cand; ++i)
        if (sorted[i - 1] == sorted[i]) return why_is(MS_ERR_INVALID, why, bytes, "map cull: slot %d is a candidate twice", sorted[i]);
    return MS_OK;
}

}  // namespace ms_cull

#ifdef MAP_CULL_HOST_ONLY
// the exported validation entry point as the library defines it, for a program that carries its own copy
extern "C" int ms_map_cull_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, int n_mp, const int32_t *kf_id, const double *kf_t,
                                 const int32_t *cand, const uint8_t *cand_keep, int n_cand, const ms_cull_settings *settings, const int32_t *removed_rows,
                                 const uint8_t *cand_removed, const int32_t *n_removed_rows, const int32_t *n_removed_kf, char *why, size_t why_bytes) {
    std::vector<int32_t> order, sorted;
    return ms_cull::check_cull(kf_mp, n_kf, stride, mp_flags, mp_live, n_mp, kf_id, kf_t, cand, cand_keep, n_cand, settings, removed_rows, cand_removed, n_removed_rows,
                               n_removed_kf, order, sorted, why, why_bytes);
}
#endif
