// map_checks.cpp -- the host validation of every call on the device map tables: the 22 exported ms_*_check functions, in the order of
// mi355slam.h, and ms_frame_finish_validate, ms_keyframe_admit_validate, ms_bow_vector_validate, ms_map_extract_validate, ms_frame_admit_validate and ms_map_publish_validate behind them.  Each turns bad arguments away with a code and a message before any device call; its entry point (in the family's .hip file)
// calls it with the context's error buffer.  Plain C++17, no HIP and no context: the checks read the HOST arguments only and ask of the DEVICE
// arrays nothing but whether they are there, so this file compiles alone and runs under sanitizers (tests/map_checks_corpus.cpp).  The first
// failing statement decides the message, so the order of the statements inside a function is part of the interface.
#include "ms_check.h"
#include <algorithm>
#include <cmath>
#include <utility>

std::atomic<long long> g_ms_host_allocs{0};

#define INVALID(...) return ms_why(MS_ERR_INVALID, why, why_bytes, __VA_ARGS__)

namespace {

// the per-thread vectors of the validation: they only grow
std::vector<int32_t> &tl_order() { thread_local std::vector<int32_t> v; return v; }       // the slots in KfId order (ms_slots_by_id)
std::vector<int32_t> &tl_sorted() { thread_local std::vector<int32_t> v; return v; }      // sorted candidates, views, rows; the merged set of ms_pair_outcomes
std::vector<int32_t> &tl_ids() { thread_local std::vector<int32_t> v; return v; }         // the track ids of ms_match_tracked_check

// order[i] = the slots with kf_id >= 0 by ascending kf_id.  False when a non-negative id is listed twice (*twice = that id).
bool slots_by_id(const int32_t *kf_id, int n_kf, std::vector<int32_t> &order, int32_t *twice) {
    order.clear();
    for (int k = 0; k < n_kf; ++k) if (kf_id[k] >= 0) order.push_back(k);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return kf_id[a] < kf_id[b]; });
    for (size_t i = 1; i < order.size(); ++i)
        if (kf_id[order[i - 1]] == kf_id[order[i]]) { *twice = kf_id[order[i]]; return false; }
    return true;
}

}  // namespace

bool ms_distinct_in_range(const int32_t *idx, int n, int limit, int *bad) {
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= limit) { *bad = i; return false; }
    thread_local std::vector<int32_t> tmp;
    if (tmp.capacity() < (size_t)n) { tmp.reserve((size_t)n + (size_t)n / 2); ++g_ms_host_allocs; }
    tmp.assign(idx, idx + n);
    std::sort(tmp.begin(), tmp.end());
    for (int i = 1; i < n; ++i)
        if (tmp[i - 1] == tmp[i]) { *bad = -1 - tmp[i]; return false; }
    return true;
}

int ms_kf_table_check(const char *who, const int32_t *kf_mp, int n_kf, int stride, int n_mp, const int32_t *kf_id, char *why, size_t why_bytes) {
    if (n_kf < 0 || n_mp < 0) INVALID("%s: negative size (%d slots, %d map points)", who, n_kf, n_mp);
    if (stride < 1) return ms_why_stride(who, stride, why, why_bytes);
    if (n_kf > 0 && (!kf_mp || !kf_id)) INVALID("%s: missing array (kf_mp or kf_id)", who);
    int32_t twice = 0;
    if (!slots_by_id(kf_id, n_kf, tl_order(), &twice)) INVALID("%s: kf_id %d is listed twice", who, twice);
    return MS_OK;
}

const std::vector<int32_t> &ms_slots_by_id() { return tl_order(); }

int ms_pair_outcomes(const int32_t *pairs, int n_pairs, uint8_t *outcome) {
    std::vector<int32_t> &merged = tl_sorted();              // sorted insertion keeps it a set
    merged.clear();
    int n_run = 0;
    auto has = [&](int32_t r) { return std::binary_search(merged.begin(), merged.end(), r); };
    for (int i = 0; i < n_pairs; ++i) {
        const int32_t a = pairs[2 * i], b = pairs[2 * i + 1];
        if (a == b) outcome[i] = 1;
        else if (has(a) || has(b)) outcome[i] = 2;
        else {
            outcome[i] = 0;
            merged.insert(std::upper_bound(merged.begin(), merged.end(), a), a);
            ++n_run;
        }
    }
    return n_run;
}

// ------------------------------------------------------------------------------------------------ map_refresh.hip
extern "C" int ms_map_refresh_check(const double *mp_pos, const float *mp_norm, const float *mp_min_dist, const float *mp_max_dist, const uint32_t *mp_desc, int n_mp,
                                    const double *kf_pose, int n_kf, const uint32_t *desc_pool, int n_pool, const int32_t *rows, int n_rows,
                                    const int32_t *obs_start, const int32_t *obs_kf, const int32_t *obs_desc, const int32_t *first_octave,
                                    const float *scale_factors, int n_levels, char *why, size_t why_bytes) {
    if (n_mp < 0 || n_kf < 0 || n_pool < 0 || n_rows < 0 || n_levels < 1 || !scale_factors) INVALID("map refresh: bad arguments");
    if (n_rows == 0) return MS_OK;
    if (!mp_pos || !mp_norm || !mp_min_dist || !mp_max_dist || !kf_pose || !rows || !obs_start || !obs_kf || !first_octave) INVALID("map refresh: missing array");
    const bool with_desc = desc_pool != nullptr && obs_desc != nullptr;
    if (with_desc && !mp_desc) INVALID("map refresh: a descriptor pool without the table's descriptors");
    if (with_desc && ((reinterpret_cast<uintptr_t>(mp_desc) | reinterpret_cast<uintptr_t>(desc_pool)) & 15u)) INVALID("map refresh: descriptor arrays must be 16-byte aligned");
    if (obs_start[0] != 0) INVALID("map refresh: obs_start[0] = %d", obs_start[0]);
    for (int r = 0; r < n_rows; ++r) {
        if (obs_start[r + 1] < obs_start[r]) INVALID("map refresh: obs_start decreases at row entry %d", r);
        if (obs_start[r + 1] == obs_start[r]) INVALID("map refresh: row entry %d has no observations", r);
        if (first_octave[r] < 0 || first_octave[r] >= n_levels) INVALID("map refresh: row entry %d: octave %d outside [0, %d)", r, first_octave[r], n_levels);
    }
    for (int o = 0; o < obs_start[n_rows]; ++o) {
        if (obs_kf[o] < 0 || obs_kf[o] >= n_kf) INVALID("map refresh: observation %d: keyframe slot %d outside [0, %d)", o, obs_kf[o], n_kf);
        if (with_desc && (obs_desc[o] < -1 || obs_desc[o] >= n_pool)) INVALID("map refresh: observation %d: descriptor %d outside [0, %d)", o, obs_desc[o], n_pool);
    }
    int bad = 0;
    if (!ms_distinct_in_range(rows, n_rows, n_mp, &bad)) {
        if (bad >= 0) INVALID("map refresh: row entry %d: row %d outside [0, %d)", bad, rows[bad], n_mp);
        INVALID("map refresh: row %d is listed twice", -1 - bad);
    }
    return MS_OK;
}

extern "C" int ms_loop_correct_check(const double *kf_pose, int n_kf, const double *mp_pos, int n_mp, const double *T, const int32_t *kf_slot, const uint8_t *kf_rigid,
                                     const double *kf_lambda, int n_corr, const int32_t *mp_row, const int32_t *mp_ref, int n_pts, char *why, size_t why_bytes) {
    if (n_kf < 0 || n_mp < 0 || n_corr < 0 || n_pts < 0 || !T) INVALID("loop correct: bad arguments");
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(T[k])) INVALID("loop correct: T[%d] is not finite", k);
    if ((n_corr > 0 && (!kf_pose || !kf_slot || !kf_rigid || !kf_lambda)) || (n_pts > 0 && (!mp_pos || !mp_row || !mp_ref))) INVALID("loop correct: missing array");
    for (int i = 0; i < n_corr; ++i)                         // a rigid member's lambda is not read
        if (!kf_rigid[i] && !(kf_lambda[i] >= 0.0 && kf_lambda[i] <= 1.0)) INVALID("loop correct: keyframe entry %d: lambda %g outside [0, 1]", i, kf_lambda[i]);
    for (int j = 0; j < n_pts; ++j)
        if (mp_ref[j] < 0 || mp_ref[j] >= n_corr) INVALID("loop correct: point entry %d: reference %d outside [0, %d)", j, mp_ref[j], n_corr);
    int bad = 0;
    if (!ms_distinct_in_range(kf_slot, n_corr, n_kf, &bad)) {
        if (bad >= 0) INVALID("loop correct: keyframe entry %d: slot %d outside [0, %d)", bad, kf_slot[bad], n_kf);
        INVALID("loop correct: keyframe slot %d is listed twice", -1 - bad);
    }
    if (!ms_distinct_in_range(mp_row, n_pts, n_mp, &bad)) {
        if (bad >= 0) INVALID("loop correct: point entry %d: row %d outside [0, %d)", bad, mp_row[bad], n_mp);
        INVALID("loop correct: map-point row %d is listed twice", -1 - bad);
    }
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ covis.hip
// (the caps of these two are tested by their entry points, not here: DESIGN, the map side's source map)
extern "C" int ms_covisibility_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, int n_mp, const ms_covis_query *queries, int n_q,
                                     const int32_t *neighbours, const int32_t *n_neighbours, char *why, size_t why_bytes) {
    if (n_kf < 0 || n_mp < 0 || n_q < 0) INVALID("covisibility: negative count (%d slots, %d map points, %d queries)", n_kf, n_mp, n_q);
    if (stride < 1) return ms_why_stride("covisibility", stride, why, why_bytes);
    if (n_q == 0) return MS_OK;
    if (!kf_mp || !queries || !neighbours || !n_neighbours) INVALID("covisibility: missing array");
    for (int q = 0; q < n_q; ++q) {
        const ms_covis_query &Q = queries[q];
        if (Q.slot < 0 || Q.slot >= n_kf) INVALID("covisibility: query %d: slot %d outside [0, %d)", q, Q.slot, n_kf);
        if (Q.force_a < -1 || Q.force_a >= n_kf || Q.force_b < -1 || Q.force_b >= n_kf)
            INVALID("covisibility: query %d: forced slots %d, %d outside [-1, %d)", q, Q.force_a, Q.force_b, n_kf);
        if (Q.require && !mp_flags) INVALID("covisibility: query %d requires flags 0x%x and there is no mp_flags", q, (unsigned)Q.require);
    }
    return MS_OK;
}

extern "C" int ms_map_point_union_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, int n_mp, const int32_t *kf_list, int n_list,
                                        const ms_union_problem *problems, int n_u, const int32_t *rows, const int32_t *n_rows, char *why, size_t why_bytes) {
    if (n_kf < 0 || n_mp < 0 || n_list < 0 || n_u < 0)
        INVALID("map point union: negative count (%d slots, %d map points, %d list entries, %d problems)", n_kf, n_mp, n_list, n_u);
    if (stride < 1) return ms_why_stride("map point union", stride, why, why_bytes);
    if (n_u == 0) return MS_OK;
    if (!kf_mp || !problems || !rows || !n_rows || (n_list > 0 && !kf_list)) INVALID("map point union: missing array");
    for (int u = 0; u < n_u; ++u) {
        const ms_union_problem &P = problems[u];
        if (P.count < 0 || P.first < 0 || (long long)P.first + P.count > n_list)
            INVALID("map point union: problem %d: slice [%d, %d + %d) outside [0, %d)", u, P.first, P.first, P.count, n_list);
        if (P.exclude_slot < -1 || P.exclude_slot >= n_kf) INVALID("map point union: problem %d: exclude slot %d outside [-1, %d)", u, P.exclude_slot, n_kf);
        if (P.require && !mp_flags) INVALID("map point union: problem %d requires flags 0x%x and there is no mp_flags", u, (unsigned)P.require);
        for (int i = P.first; i < P.first + P.count; ++i)       // list entries in no slice are never read, so only the slices are checked
            if (kf_list[i] < 0 || kf_list[i] >= n_kf) INVALID("map point union: list entry %d: slot %d outside [0, %d)", i, kf_list[i], n_kf);
    }
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ map_cull.hip
extern "C" int ms_map_cull_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, int n_mp, const int32_t *kf_id, const double *kf_t,
                                 const int32_t *cand, const uint8_t *cand_keep, int n_cand, const ms_cull_settings *s, const int32_t *removed_rows,
                                 const uint8_t *cand_removed, const int32_t *n_removed_rows, const int32_t *n_removed_kf, char *why, size_t why_bytes) {
    (void)cand_keep;
    if (n_cand < 0) INVALID("map cull: negative size (%d candidates)", n_cand);
    if (!s || !kf_t || !n_removed_rows || !n_removed_kf || (n_cand > 0 && (!cand || !cand_removed)) || (n_mp > 0 && (!mp_live || !removed_rows)))
        INVALID("map cull: missing array");
    int rc;
    if ((rc = ms_kf_table_check("map cull", kf_mp, n_kf, stride, n_mp, kf_id, why, why_bytes))) return rc;
    if (s->cull_points && !mp_flags) INVALID("map cull: cull_points is set and there is no mp_flags");
    if (!std::isfinite(s->min_age) || !std::isfinite(s->max_critical_ratio))
        INVALID("map cull: min_age %g or max_critical_ratio %g is not finite", s->min_age, s->max_critical_ratio);
    if (s->min_obs_for_ba < 0) INVALID("map cull: min_obs_for_ba %d", s->min_obs_for_ba);
    const int32_t cur = s->current_slot;
    if (cur < 0 || cur >= n_kf) INVALID("map cull: current slot %d outside [0, %d)", cur, n_kf);
    if (kf_id[cur] < 0) INVALID("map cull: current slot %d is empty (kf_id %d)", cur, kf_id[cur]);
    for (int32_t k : tl_order()) {
        if (!std::isfinite(kf_t[k])) INVALID("map cull: kf_t of slot %d is not finite", k);
        const double age = kf_t[cur] - kf_t[k];
        if (!(std::fabs(age) < 2147483648.0)) INVALID("map cull: the age %g of slot %d is outside int32", age, k);
    }
    for (int i = 0; i < n_cand; ++i) {
        if (cand[i] < 0 || cand[i] >= n_kf) INVALID("map cull: candidate %d: slot %d outside [0, %d)", i, cand[i], n_kf);
        if (cand[i] == cur) INVALID("map cull: candidate %d is the current slot %d", i, cur);
        if (kf_id[cand[i]] < 0) INVALID("map cull: candidate %d: slot %d is empty (kf_id %d)", i, cand[i], kf_id[cand[i]]);
    }
    std::vector<int32_t> &sorted = tl_sorted();
    sorted.assign(cand, cand + n_cand);
    std::sort(sorted.begin(), sorted.end());
    for (int i = 1; i < n_cand; ++i)
        if (sorted[i - 1] == sorted[i]) INVALID("map cull: slot %d is a candidate twice", sorted[i]);
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ triangulate.hip
extern "C" int ms_triangulate_check(const double *mp_pos, int n_mp, const double *kf_pose, int n_kf, const ms_pinhole *kf_cam, const int32_t *kf_focal,
                                    const int32_t *rows, const uint8_t *was_triangulated, int n_rows, const int32_t *obs_start, const int32_t *obs_kf,
                                    const float *obs_x, const float *obs_y, const int32_t *obs_octave, const ms_tri_settings *settings, int mode, char *why,
                                    size_t why_bytes) {
    if (n_mp < 0 || n_kf < 0 || n_rows < 0) INVALID("triangulate: bad arguments");
    if (mode != MS_TRI_TME && mode != MS_TRI_MIDPOINT && mode != MS_TRI_FIRST_LAST) INVALID("triangulate: mode %d", mode);
    if (!settings || !settings->level_sigma_sq) INVALID("triangulate: missing settings");
    if (settings->n_levels < 1 || settings->n_levels > MS_TRI_MAX_LEVELS) INVALID("triangulate: n_levels %d outside [1, %d]", settings->n_levels, MS_TRI_MAX_LEVELS);
    if (!std::isfinite(settings->min_angle_two_obs) || !std::isfinite(settings->min_angle_multiple_obs) || !std::isfinite(settings->rel_reprojection_threshold))
        INVALID("triangulate: a setting is not finite");
    for (int l = 0; l < settings->n_levels; ++l)
        if (!std::isfinite(settings->level_sigma_sq[l])) INVALID("triangulate: level_sigma_sq[%d] is not finite", l);
    if (n_rows == 0) return MS_OK;
    if (n_rows > MS_TRI_MAX_ROWS) return ms_why(MS_ERR_CAPACITY, why, why_bytes, "triangulate: %d rows, at most %d per call", n_rows, MS_TRI_MAX_ROWS);
    if (!mp_pos || !kf_pose || !kf_cam || !kf_focal || !rows || !was_triangulated || !obs_start) INVALID("triangulate: missing array");
    if (obs_start[0] != 0) INVALID("triangulate: obs_start[0] = %d", obs_start[0]);
    for (int r = 0; r < n_rows; ++r)
        if (obs_start[r + 1] < obs_start[r]) INVALID("triangulate: obs_start decreases at row entry %d", r);
    const int n_obs = obs_start[n_rows];
    if (n_obs > MS_TRI_MAX_OBS) return ms_why(MS_ERR_CAPACITY, why, why_bytes, "triangulate: %d observations, at most %d per call", n_obs, MS_TRI_MAX_OBS);
    if (n_obs > 0 && (!obs_kf || !obs_x || !obs_y || !obs_octave)) INVALID("triangulate: missing array");
    for (int o = 0; o < n_obs; ++o) {
        if (obs_kf[o] < 0 || obs_kf[o] >= n_kf) INVALID("triangulate: observation %d: keyframe slot %d outside [0, %d)", o, obs_kf[o], n_kf);
        if (obs_octave[o] < 0 || obs_octave[o] >= settings->n_levels) INVALID("triangulate: observation %d: octave %d outside [0, %d)", o, obs_octave[o], settings->n_levels);
        const ms_pinhole &c = kf_cam[obs_kf[o]];
        if (c.width < 1 || c.height < 1 || !(c.fx > 0.0) || !(c.fy > 0.0) || !std::isfinite(c.fx) || !std::isfinite(c.fy) || !std::isfinite(c.cx) || !std::isfinite(c.cy))
            INVALID("triangulate: keyframe slot %d: bad camera (%d x %d, fx %g, fy %g)", obs_kf[o], c.width, c.height, c.fx, c.fy);
    }
    int bad = 0;
    if (!ms_distinct_in_range(rows, n_rows, n_mp, &bad)) {
        if (bad >= 0) INVALID("triangulate: row entry %d: row %d outside [0, %d)", bad, rows[bad], n_mp);
        INVALID("triangulate: row %d is listed twice", -1 - bad);
    }
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ obs_lists.hip
// (the caps are tested by the entry point, which words them with its own cap on rows_in)
extern "C" int ms_observation_lists_check(const int32_t *kf_mp, int n_kf, int stride, int n_mp, const int32_t *kf_id, const uint8_t *mp_flags, const float *kp_x,
                                          const float *kp_y, const int32_t *kp_octave, const float *kp_depth, const int32_t *kf_desc_base, const ms_obs_select *sel,
                                          int n_levels, const ms_obs_lists *out, int cap_rows, int cap_obs, const int32_t *n_rows, const int32_t *n_obs, char *why,
                                          size_t why_bytes) {
    if (!sel || !out || !n_rows || !n_obs) INVALID("observation lists: missing array (selection, outputs or counts)");
    if (cap_rows < 0 || cap_obs < 0 || n_levels < 0 || sel->n_in < 0)
        INVALID("observation lists: negative size (capacities %d / %d, %d levels, %d rows_in)", cap_rows, cap_obs, n_levels, sel->n_in);
    int rc;
    if ((rc = ms_kf_table_check("observation lists", kf_mp, n_kf, stride, n_mp, kf_id, why, why_bytes))) return rc;
    if (sel->source != MS_OBS_FROM_ROWS && sel->source != MS_OBS_FROM_SLOT) INVALID("observation lists: source %d", sel->source);
    if (sel->filter != MS_OBS_ALL && sel->filter != MS_OBS_REFRESH && sel->filter != MS_OBS_RETRIANGULATE) INVALID("observation lists: filter %d", sel->filter);
    if (sel->filter != MS_OBS_ALL && !mp_flags) INVALID("observation lists: filter %d reads flags and there is no mp_flags", sel->filter);
    if (sel->source == MS_OBS_FROM_SLOT) {
        if (sel->slot < 0 || sel->slot >= n_kf) INVALID("observation lists: slot %d outside [0, %d)", sel->slot, n_kf);
        if (kf_id[sel->slot] < 0) INVALID("observation lists: slot %d is empty (kf_id %d)", sel->slot, kf_id[sel->slot]);
    } else if (sel->n_in > 0 && !sel->rows_in) {
        INVALID("observation lists: missing array (rows_in)");
    }
    if ((cap_rows > 0 && !out->rows) || !out->obs_start) INVALID("observation lists: missing array (rows or obs_start)");
    if ((out->obs_x && !kp_x) || (out->obs_y && !kp_y) || ((out->obs_octave || out->first_octave) && !kp_octave) || (out->obs_depth && !kp_depth) ||
        (out->obs_desc && !kf_desc_base))
        INVALID("observation lists: missing array (an output is asked for without its keypoint table)");
    if (out->was_triangulated && !mp_flags) INVALID("observation lists: missing array (was_triangulated without mp_flags)");
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ match_tracked.hip
extern "C" int ms_match_tracked_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const double *mp_pos, const float *mp_norm,
                                      const float *mp_min_dist, const float *mp_max_dist, const uint32_t *mp_desc, const int32_t *mp_track, int n_mp, const float *kp_x,
                                      const float *kp_y, const int32_t *kp_octave, const uint32_t *desc_pool, int n_pool, const int32_t *track_row, int n_track,
                                      const ms_tracked_frame *f, const int32_t *kp_track, int n_kp, const int32_t *new_rows, int n_new, const uint8_t *outcome,
                                      const int32_t *counts, char *why, size_t why_bytes) {
    if (n_kf < 0 || n_mp < 0 || n_pool < 0 || n_track < 0 || n_kp < 0 || n_new < 0)
        INVALID("match tracked: negative size (%d slots, %d map points, %d pool descriptors, %d tracks, %d keypoints, %d new rows)", n_kf, n_mp, n_pool, n_track, n_kp, n_new);
    if (stride < 1) return ms_why_stride("match tracked", stride, why, why_bytes);
    if (!f || !counts) INVALID("match tracked: missing array (frame or counts)");
    if (f->slot < 0 || f->slot >= n_kf) INVALID("match tracked: slot %d outside [0, %d)", f->slot, n_kf);
    if (n_kp > stride) INVALID("match tracked: %d keypoints in a table of stride %d", n_kp, stride);
    if (!kf_mp || !kp_x || !kp_y || !kp_octave) INVALID("match tracked: missing array (kf_mp or the keypoint table)");
    if (n_mp > 0 && (!mp_flags || !mp_live || !mp_pos || !mp_norm || !mp_min_dist || !mp_max_dist || !mp_desc || !mp_track))
        INVALID("match tracked: missing array (the map-point table)");
    if (n_track > 0 && !track_row) INVALID("match tracked: missing array (track_row)");
    if (n_kp > 0 && (!kp_track || !outcome)) INVALID("match tracked: missing array (kp_track or outcome)");
    if (n_new > 0 && !new_rows) INVALID("match tracked: missing array (new_rows)");
    if (!f->level_sigma_sq) INVALID("match tracked: missing array (level_sigma_sq)");
    if (f->n_levels < 1 || f->n_levels > MS_TRI_MAX_LEVELS) INVALID("match tracked: %d levels outside [1, %d]", f->n_levels, MS_TRI_MAX_LEVELS);
    for (int l = 0; l < f->n_levels; ++l)
        if (!std::isfinite(f->level_sigma_sq[l])) INVALID("match tracked: level_sigma_sq[%d] is not finite", l);
    if (!std::isfinite(f->rel_reprojection_threshold) || !std::isfinite(f->view_cos_limit))
        INVALID("match tracked: rel_reprojection_threshold %g or view_cos_limit %g is not finite", (double)f->rel_reprojection_threshold, (double)f->view_cos_limit);
    if (f->cam.width < 1 || f->cam.height < 1 || !(f->cam.fx > 0.0) || !(f->cam.fy > 0.0) || !std::isfinite(f->cam.fx) || !std::isfinite(f->cam.fy) ||
        !std::isfinite(f->cam.cx) || !std::isfinite(f->cam.cy))
        INVALID("match tracked: bad camera");
    if (f->desc_base >= 0 && (!desc_pool || (long long)f->desc_base + n_kp > n_pool))
        INVALID("match tracked: descriptors [%d, %d + %d) outside the pool of %d", f->desc_base, f->desc_base, n_kp, desc_pool ? n_pool : 0);
    if ((reinterpret_cast<uintptr_t>(mp_desc) | reinterpret_cast<uintptr_t>(desc_pool)) & 15u) INVALID("match tracked: descriptor arrays must be 16-byte aligned");
    std::vector<int32_t> &ids = tl_ids();
    ids.clear();
    if (ids.capacity() < (size_t)n_kp) { ids.reserve((size_t)n_kp + (size_t)n_kp / 2); ++g_ms_host_allocs; }
    for (int j = 0; j < n_kp; ++j) {
        const int32_t t = kp_track[j];
        if (t < 0) continue;
        if (t < f->track_base || (long long)t - f->track_base >= n_track)
            INVALID("match tracked: keypoint %d: track id %d outside the window [%d, %d + %d)", j, t, f->track_base, f->track_base, n_track);
        ids.push_back(t);
    }
    std::sort(ids.begin(), ids.end());
    for (size_t i = 1; i < ids.size(); ++i)
        if (ids[i - 1] == ids[i]) INVALID("match tracked: track id %d is listed twice", ids[i]);
    int bad = 0;
    if (!ms_distinct_in_range(new_rows, n_new, n_mp, &bad)) {
        if (bad < 0) INVALID("match tracked: new row %d is listed twice", -1 - bad);
        INVALID("match tracked: new row %d outside [0, %d)", new_rows[bad], n_mp);
    }
    if (ms_map_over_capacity(n_kf, stride, n_mp, 0) || n_track > MS_TRACKED_MAX_WINDOW)
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "match tracked: %d slots / stride %d / %d map points / %d tracks, caps %d / %d / below %d / %d", n_kf, stride, n_mp,
                      n_track, MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, MS_TRACKED_MAX_WINDOW);
    return MS_OK;
}

extern "C" int ms_match_tracked_finish_check(const ms_obs_lists *lists, int n_rows, const uint8_t *mp_flags, const uint32_t *desc_pool, const uint32_t *mp_desc, int n_mp,
                                             const int32_t *checked_rows, int n_checked, int append_checked, const int32_t *refresh_rows, int cap_refresh,
                                             const int32_t *n_refresh, char *why, size_t why_bytes) {
    if (n_rows < 0 || n_checked < 0 || n_mp < 0 || cap_refresh < 0)
        INVALID("match tracked finish: negative size (%d rows, %d checked rows, %d map points, capacity %d)", n_rows, n_checked, n_mp, cap_refresh);
    if (!n_refresh) INVALID("match tracked finish: missing array (n_refresh)");
    if (n_rows > 0 && (!lists || !lists->rows || !lists->obs_start || !mp_flags)) INVALID("match tracked finish: missing array (rows, obs_start or mp_flags)");
    if (n_rows > 0 && desc_pool && lists->obs_desc && !mp_desc) INVALID("match tracked finish: missing array (mp_desc)");
    if (n_checked > 0 && !checked_rows) INVALID("match tracked finish: missing array (checked_rows)");
    if (n_rows + n_checked > 0 && !refresh_rows) INVALID("match tracked finish: missing array (refresh_rows)");
    if ((reinterpret_cast<uintptr_t>(mp_desc) | reinterpret_cast<uintptr_t>(desc_pool)) & 15u) INVALID("match tracked finish: descriptor arrays must be 16-byte aligned");
    const long long need = (long long)n_rows + (append_checked ? n_checked : 0);
    if (n_rows > MS_COVIS_MAX_STRIDE || n_checked > MS_COVIS_MAX_STRIDE || n_mp >= MS_COVIS_MAX_MP || need > cap_refresh)
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "match tracked finish: %d rows / %d checked rows / %d map points, caps %d / %d / below %d; refresh_rows holds %d of up to %lld",
                      n_rows, n_checked, n_mp, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, cap_refresh, need);
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ map_fuse.hip
namespace {

// what both entry points ask of the tables
int check_fuse_tables(const char *who, const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const int32_t *n_obs, int n_mp,
                      const int32_t *mp_track, const int32_t *track_row, int n_track, char *why, size_t why_bytes) {
    if (n_kf < 0 || n_mp < 0 || n_track < 0) INVALID("%s: negative size (%d slots, %d map points, %d tracks)", who, n_kf, n_mp, n_track);
    if (stride < 1) return ms_why_stride(who, stride, why, why_bytes);
    if ((n_kf > 0 && !kf_mp) || (n_mp > 0 && (!mp_flags || !mp_live || !n_obs))) INVALID("%s: missing array (kf_mp, mp_flags, mp_live or n_obs)", who);
    if ((mp_track != nullptr) != (track_row != nullptr)) INVALID("%s: one track table without the other", who);
    if (ms_map_over_capacity(n_kf, stride, n_mp, 0)) return ms_why_table_caps(who, n_kf, stride, n_mp, why, why_bytes);
    if (n_track > MS_TRACKED_MAX_WINDOW) return ms_why(MS_ERR_CAPACITY, why, why_bytes, "%s: a track window of %d, cap %d", who, n_track, MS_TRACKED_MAX_WINDOW);
    return MS_OK;
}

}  // namespace

extern "C" int ms_map_fuse_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const int32_t *n_obs, int n_mp,
                                 const int32_t *mp_track, const int32_t *track_row, int track_base, int n_track, const int32_t *kept_entry, const int32_t *top_idx,
                                 const uint16_t *top_dist, const int32_t *mp_index, int n_entries, const ms_fuse_view *views, const int32_t *n_kept, int n_views,
                                 int max_dist, int source_slot, const int32_t *n_erased, const int32_t *counts, const int32_t *views_done, char *why, size_t why_bytes) {
    (void)track_base;                                        // any base is fine: a track outside the window writes no track_row
    int rc;
    if ((rc = check_fuse_tables("map fuse", kf_mp, n_kf, stride, mp_flags, mp_live, n_obs, n_mp, mp_track, track_row, n_track, why, why_bytes))) return rc;
    if (n_entries < 0 || n_views < 0) INVALID("map fuse: negative size (%d entries, %d views)", n_entries, n_views);
    if (!n_erased || !counts || !views_done || (n_views > 0 && (!views || !n_kept)) || (n_entries > 0 && (!mp_index || !kept_entry || !top_idx || !top_dist)))
        INVALID("map fuse: missing array");
    if (n_views > MS_GATE_MAX_VIEWS || n_entries >= MS_GATE_MAX_ENTRIES)
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "map fuse: %d views / %d entries, caps %d / below %d", n_views, n_entries, MS_GATE_MAX_VIEWS, MS_GATE_MAX_ENTRIES);
    if (max_dist < 0 || max_dist > 256) INVALID("map fuse: max_dist %d outside [0, 256]", max_dist);
    if (source_slot < -1 || source_slot >= n_kf) INVALID("map fuse: source slot %d outside [-1, %d)", source_slot, n_kf);
    for (int v = 0; v < n_views; ++v) {
        const ms_fuse_view &V = views[v];
        if (V.slot < 0 || V.slot >= n_kf) INVALID("map fuse: view %d: slot %d outside [0, %d)", v, V.slot, n_kf);
        if (V.first < 0 || V.count < 0 || V.first > n_entries || V.count > n_entries - V.first)
            INVALID("map fuse: view %d: slice [%d, %d + %d) outside [0, %d)", v, V.first, V.first, V.count, n_entries);
        if (n_kept[v] < 0 || n_kept[v] > V.count) INVALID("map fuse: view %d: n_kept %d for a slice of %d", v, n_kept[v], V.count);
    }
    // overlapping slices: the non-empty ones in the order of their first entries
    std::vector<int32_t> &sorted = tl_sorted();
    sorted.clear();
    for (int v = 0; v < n_views; ++v) if (views[v].count > 0) sorted.push_back(v);
    std::sort(sorted.begin(), sorted.end(), [&](int32_t a, int32_t b) { return views[a].first < views[b].first; });
    for (size_t i = 1; i < sorted.size(); ++i) {
        const ms_fuse_view &A = views[sorted[i - 1]], &B = views[sorted[i]];
        if (A.first + A.count > B.first) INVALID("map fuse: the slices of views %d and %d overlap", sorted[i - 1], sorted[i]);
    }
    for (int v = 0; v < n_views; ++v) {
        const ms_fuse_view &V = views[v];
        for (int e = V.first; e < V.first + V.count; ++e)
            if (mp_index[e] < 0 || mp_index[e] >= n_mp) INVALID("map fuse: view %d: entry %d is row %d outside [0, %d)", v, e, mp_index[e], n_mp);
        sorted.assign(mp_index + V.first, mp_index + V.first + V.count);
        std::sort(sorted.begin(), sorted.end());
        for (int i = 1; i < V.count; ++i)
            if (sorted[i - 1] == sorted[i]) INVALID("map fuse: view %d lists row %d twice", v, sorted[i]);
    }
    return MS_OK;
}

extern "C" int ms_map_replace_pairs_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const int32_t *n_obs, int n_mp,
                                          const int32_t *mp_track, const int32_t *track_row, int track_base, int n_track, const int32_t *pairs, int n_pairs,
                                          const uint8_t *outcome, const int32_t *n_erased, char *why, size_t why_bytes) {
    (void)track_base;
    int rc;
    if ((rc = check_fuse_tables("map replace pairs", kf_mp, n_kf, stride, mp_flags, mp_live, n_obs, n_mp, mp_track, track_row, n_track, why, why_bytes))) return rc;
    if (n_pairs < 0) INVALID("map replace pairs: negative size (%d pairs)", n_pairs);
    if (!n_erased || (n_pairs > 0 && (!pairs || !outcome))) INVALID("map replace pairs: missing array");
    if (n_pairs >= MS_GATE_MAX_ENTRIES) return ms_why(MS_ERR_CAPACITY, why, why_bytes, "map replace pairs: %d pairs, cap below %d", n_pairs, MS_GATE_MAX_ENTRIES);
    for (int i = 0; i < 2 * n_pairs; ++i)
        if (pairs[i] < 0 || pairs[i] >= n_mp) INVALID("map replace pairs: pair %d: row %d outside [0, %d)", i / 2, pairs[i], n_mp);
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ create_points.hip
extern "C" int ms_create_points_lists_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, int n_mp, const int32_t *kf_id, const float *kp_x,
                                            const float *kp_y, const int32_t *kp_octave, const float *kp_depth, const int32_t *kf_desc_base, int cur, int adj,
                                            const int32_t *matched, int n_kp1, int n_kp2, const int32_t *new_rows, int n_new, int n_levels, const ms_obs_lists *out,
                                            int cap_rows, int cap_obs, const int32_t *match_kp1, const int32_t *match_kp2, const int32_t *n_matches, char *why,
                                            size_t why_bytes) {
    (void)match_kp1; (void)match_kp2;                        // each may be NULL
    if (n_kf < 0 || n_mp < 0 || n_kp1 < 0 || n_kp2 < 0 || n_new < 0 || cap_rows < 0 || cap_obs < 0 || n_levels < 0)
        INVALID("create points lists: negative size (%d slots, %d map points, %d and %d keypoints, %d new rows, capacities %d / %d, %d levels)", n_kf, n_mp, n_kp1, n_kp2, n_new,
                cap_rows, cap_obs, n_levels);
    if (stride < 1) return ms_why_stride("create points lists", stride, why, why_bytes);
    if (!n_matches || !kf_id) INVALID("create points lists: missing array (n_matches or kf_id)");
    if (cur < 0 || cur >= n_kf) INVALID("create points lists: slot %d outside [0, %d)", cur, n_kf);
    if (adj < 0 || adj >= n_kf) INVALID("create points lists: slot %d outside [0, %d)", adj, n_kf);
    if (cur == adj) INVALID("create points lists: the current and the adjacent keyframe are both slot %d", cur);
    if (kf_id[cur] < 0) INVALID("create points lists: slot %d has kf_id %d", cur, kf_id[cur]);
    if (kf_id[adj] < 0) INVALID("create points lists: slot %d has kf_id %d", adj, kf_id[adj]);
    if (kf_id[cur] == kf_id[adj]) INVALID("create points lists: slots %d and %d both have kf_id %d", cur, adj, kf_id[cur]);
    if (n_kp1 > stride || n_kp2 > stride) INVALID("create points lists: %d keypoints in a table of stride %d", n_kp1 > stride ? n_kp1 : n_kp2, stride);
    if (n_levels > MS_TRI_MAX_LEVELS) INVALID("create points lists: %d levels outside [0, %d]", n_levels, MS_TRI_MAX_LEVELS);
    if (!kf_mp || (n_mp > 0 && !mp_live)) INVALID("create points lists: missing array (kf_mp or mp_live)");
    if (n_kp1 > 0 && !matched) INVALID("create points lists: missing array (matched)");
    if (n_new > 0 && !new_rows) INVALID("create points lists: missing array (new_rows)");
    if (!out || !out->rows || !out->obs_start) INVALID("create points lists: missing array (rows or obs_start)");
    if ((out->obs_x && !kp_x) || (out->obs_y && !kp_y) || ((out->obs_octave || out->first_octave || n_levels > 0) && !kp_octave) || (out->obs_depth && !kp_depth) ||
        (out->obs_desc && !kf_desc_base))
        INVALID("create points lists: missing array (an output is asked for whose table is missing)");
    int bad = 0;
    if (!ms_distinct_in_range(new_rows, n_new, n_mp, &bad)) {
        if (bad < 0) INVALID("create points lists: new row %d is listed twice", -1 - bad);
        INVALID("create points lists: new row %d outside [0, %d)", new_rows[bad], n_mp);
    }
    if (ms_map_over_capacity(n_kf, stride, n_mp, 0)) return ms_why_table_caps("create points lists", n_kf, stride, n_mp, why, why_bytes);
    return MS_OK;
}

extern "C" int ms_create_points_bind_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const uint32_t *mp_desc,
                                           const int32_t *n_obs, const int32_t *mp_track, int n_mp, const uint32_t *desc_pool, int n_pool, int cur, int adj,
                                           const ms_obs_lists *lists, const int32_t *match_kp1, const int32_t *match_kp2, int n_matches, int n_kp1, int n_kp2,
                                           const uint8_t *usable1, const uint8_t *usable2, const int32_t *created_rows, const int32_t *created_kp1,
                                           const int32_t *created_kp2, const int32_t *n_created, char *why, size_t why_bytes) {
    (void)n_obs; (void)mp_track; (void)usable1; (void)usable2; (void)created_rows; (void)created_kp1; (void)created_kp2;      // each may be NULL
    if (n_kf < 0 || n_mp < 0 || n_pool < 0 || n_matches < 0 || n_kp1 < 0 || n_kp2 < 0)
        INVALID("create points bind: negative size (%d slots, %d map points, %d pool descriptors, %d matches, %d and %d keypoints)", n_kf, n_mp, n_pool, n_matches, n_kp1, n_kp2);
    if (stride < 1) return ms_why_stride("create points bind", stride, why, why_bytes);
    if (n_kp1 > stride || n_kp2 > stride) INVALID("create points bind: %d keypoints in a table of stride %d", n_kp1 > stride ? n_kp1 : n_kp2, stride);
    if (!n_created) INVALID("create points bind: missing array (n_created)");
    if (cur < 0 || cur >= n_kf) INVALID("create points bind: slot %d outside [0, %d)", cur, n_kf);
    if (adj < 0 || adj >= n_kf) INVALID("create points bind: slot %d outside [0, %d)", adj, n_kf);
    if (cur == adj) INVALID("create points bind: the current and the adjacent keyframe are both slot %d", cur);
    if (!kf_mp || !mp_flags || !mp_live) INVALID("create points bind: missing array (kf_mp, mp_flags or mp_live)");
    if (n_matches > 0 && (!lists || !lists->rows || !match_kp1 || !match_kp2)) INVALID("create points bind: missing array (rows, match_kp1 or match_kp2)");
    if (n_matches > 0 && desc_pool && lists->obs_desc && !mp_desc) INVALID("create points bind: missing array (mp_desc)");
    if ((reinterpret_cast<uintptr_t>(mp_desc) | reinterpret_cast<uintptr_t>(desc_pool)) & 15u) INVALID("create points bind: descriptor arrays must be 16-byte aligned");
    if (ms_map_over_capacity(n_kf, stride, n_mp, 0) || n_matches > MS_COVIS_MAX_STRIDE)
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "create points bind: %d slots / stride %d / %d map points / %d matches, caps %d / %d / below %d / %d", n_kf, stride, n_mp,
                      n_matches, MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, MS_COVIS_MAX_STRIDE);
    return MS_OK;
}

extern "C" int ms_unbound_mask_check(const int32_t *kf_mp, int n_kf, int stride, int n_mp, const int32_t *slots, const int32_t *n_kp, uint8_t *const *usable, int n_slots,
                                     char *why, size_t why_bytes) {
    if (n_kf < 0 || n_mp < 0 || n_slots < 0) INVALID("unbound mask: negative size (%d slots, %d map points, %d listed slots)", n_kf, n_mp, n_slots);
    if (stride < 1) return ms_why_stride("unbound mask", stride, why, why_bytes);
    if (n_slots > 0 && (!kf_mp || !slots || !n_kp || !usable)) INVALID("unbound mask: missing array (kf_mp, slots, n_kp or usable)");
    for (int s = 0; s < n_slots; ++s) {
        if (slots[s] < 0 || slots[s] >= n_kf) INVALID("unbound mask: slot %d outside [0, %d)", slots[s], n_kf);
        if (n_kp[s] < 0 || n_kp[s] > stride) INVALID("unbound mask: %d keypoints in a table of stride %d", n_kp[s], stride);
        if (n_kp[s] > 0 && !usable[s]) INVALID("unbound mask: missing array (usable of slot %d)", slots[s]);
    }
    if (ms_map_over_capacity(n_kf, stride, n_mp, n_slots))
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "unbound mask: %d slots / stride %d / %d map points / %d listed slots, caps %d / %d / below %d / %d", n_kf, stride, n_mp,
                      n_slots, MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, MS_COVIS_MAX_QUERIES);
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ search_bind.hip
namespace {

// what both entry points ask of the keyframe table, of the slot and of its keypoint count
int check_bind_slot(const char *who, const int32_t *kf_mp, int n_kf, int stride, int n_mp, int slot, int n_kp, char *why, size_t why_bytes) {
    if (n_kf < 0 || n_mp < 0 || n_kp < 0) INVALID("%s: negative size (%d slots, %d map points, %d keypoints)", who, n_kf, n_mp, n_kp);
    if (stride < 1) return ms_why_stride(who, stride, why, why_bytes);
    if (ms_map_over_capacity(n_kf, stride, n_mp, 0)) return ms_why_table_caps(who, n_kf, stride, n_mp, why, why_bytes);
    if (!kf_mp) INVALID("%s: missing array (kf_mp)", who);
    if (slot < 0 || slot >= n_kf) INVALID("%s: slot %d outside [0, %d)", who, slot, n_kf);
    if (n_kp > stride) INVALID("%s: %d keypoints for a stride of %d", who, n_kp, stride);
    return MS_OK;
}

}  // namespace

extern "C" int ms_bound_mask_check(const int32_t *kf_mp, int n_kf, int stride, int n_mp, int slot, int n_kp, const uint8_t *skip, char *why, size_t why_bytes) {
    int rc;
    if ((rc = check_bind_slot("bound mask", kf_mp, n_kf, stride, n_mp, slot, n_kp, why, why_bytes))) return rc;
    if (n_kp > 0 && !skip) INVALID("bound mask: missing array (skip)");
    return MS_OK;
}

extern "C" int ms_search_bind_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const int32_t *n_obs, int n_mp, const int32_t *kept_entry,
                                    const float *q_x, const float *q_y, const float *q_radius, const int32_t *q_min_octave, const int32_t *q_max_octave,
                                    const uint32_t *q_desc, const int32_t *top_idx, const uint16_t *top_dist, const int32_t *top_octave, const int32_t *n_scored,
                                    const uint8_t *skip, const float *sorted_x, const float *sorted_y, const int32_t *sorted_idx, const uint32_t *t_desc,
                                    const int32_t *t_octave, int n_kp, const int32_t *mp_index, int first, int count, int n_kept, int slot, const int32_t *n_matched,
                                    const int32_t *counts, char *why, size_t why_bytes) {
    (void)q_min_octave; (void)q_max_octave;                  // each may be NULL: no window on that side
    int rc;
    if ((rc = check_bind_slot("search bind", kf_mp, n_kf, stride, n_mp, slot, n_kp, why, why_bytes))) return rc;
    if (first < 0 || count < 0 || n_kept < 0) INVALID("search bind: negative size (first %d, count %d, n_kept %d)", first, count, n_kept);
    if (count >= MS_GATE_MAX_ENTRIES || first >= MS_GATE_MAX_ENTRIES - count)
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "search bind: a slice [%d, %d + %d), cap below %d entries", first, first, count, MS_GATE_MAX_ENTRIES);
    if (n_kept > count) INVALID("search bind: n_kept %d for a slice of %d", n_kept, count);
    if (!n_matched || !counts) INVALID("search bind: missing array (n_matched or counts)");
    if (n_mp > 0 && (!mp_live || !n_obs)) INVALID("search bind: missing array (mp_live or n_obs)");
    if (count > 0 && !mp_index) INVALID("search bind: missing array (mp_index)");
    if (n_kept > 0 && (!kept_entry || !q_x || !q_y || !q_radius || !q_desc || !top_idx || !top_dist || !top_octave || !n_scored))
        INVALID("search bind: missing array (a list of the gate or of the scoring)");
    if (n_kept > 0 && n_kp > 0 && (!skip || !sorted_x || !sorted_y || !sorted_idx || !t_desc || !t_octave)) INVALID("search bind: missing array (skip or a keyframe array)");
    if (((uintptr_t)q_desc | (uintptr_t)t_desc) & 15) INVALID("search bind: q_desc and t_desc must be 16-byte aligned");
    for (int e = first; e < first + count; ++e)
        if (mp_index[e] < 0 || mp_index[e] >= n_mp) INVALID("search bind: entry %d is row %d outside [0, %d)", e, mp_index[e], n_mp);
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ ba_window.hip
namespace {

// the local keyframes: in range, distinct, the current one among them
int check_local(const char *who, const int32_t *local_slot, int n_local, int n_kf, int current_index, char *why, size_t why_bytes) {
    if (n_local > 0 && !local_slot) INVALID("%s: missing array (local_slot)", who);
    int bad = 0;
    if (!ms_distinct_in_range(local_slot, n_local, n_kf, &bad)) {
        if (bad < 0) INVALID("%s: local slot %d is listed twice", who, -1 - bad);
        INVALID("%s: local slot %d outside [0, %d)", who, local_slot[bad], n_kf);
    }
    if (current_index < 0 || current_index >= n_local) INVALID("%s: current index %d outside [0, %d)", who, current_index, n_local);
    return MS_OK;
}

}  // namespace

extern "C" int ms_ba_window_lists_check(const double *kf_pose, int n_kf, const double *mp_pos, int n_mp, const ms_obs_lists *lists, int n_rows, int n_obs,
                                        const int32_t *local_slot, int n_local, int current_index, const ms_pinhole *kf_cam, const int32_t *kf_focal,
                                        const float *level_sigma_sq, int n_levels, const double *pose, const double *point, const int32_t *obs_point, const int32_t *obs_pose,
                                        const double *obs_uv, const double *obs_info, int cap_point, int cap_edge, const ms_ba_window_dev *window, const int32_t *n_edge,
                                        const int32_t *n_current, char *why, size_t why_bytes) {
    if (n_kf < 0 || n_mp < 0 || n_rows < 0 || n_obs < 0 || n_local < 0 || cap_point < 0 || cap_edge < 0)
        INVALID("ba window lists: negative size (%d slots, %d map points, %d rows, %d observations, %d local keyframes, capacities %d / %d)", n_kf, n_mp, n_rows, n_obs, n_local,
                cap_point, cap_edge);
    if (n_levels < 1 || n_levels > MS_TRI_MAX_LEVELS) INVALID("ba window lists: %d levels outside [1, %d]", n_levels, MS_TRI_MAX_LEVELS);
    if (!n_edge || !n_current) INVALID("ba window lists: missing array (n_edge or n_current)");
    if (!kf_pose || !kf_cam || !kf_focal || !level_sigma_sq || !pose) INVALID("ba window lists: missing array (kf_pose, kf_cam, kf_focal, level_sigma_sq or pose)");
    if (n_rows > 0 && (!mp_pos || !lists || !lists->rows || !lists->obs_start)) INVALID("ba window lists: missing array (mp_pos, rows or obs_start)");
    if (n_obs > 0 && (n_rows == 0 || !lists->obs_kf || !lists->obs_kp || !lists->obs_x || !lists->obs_y || !lists->obs_octave))
        INVALID("ba window lists: missing array (obs_kf, obs_kp, obs_x, obs_y or obs_octave)");
    if (cap_point > 0 && !point) INVALID("ba window lists: missing array (point)");
    if (cap_edge > 0 && (!obs_point || !obs_pose || !obs_uv || !obs_info || !window || !window->edge_slot || !window->edge_kp || !window->edge_point))
        INVALID("ba window lists: missing array (obs_point, obs_pose, obs_uv, obs_info or the window's edge arrays)");
    int rc;
    if ((rc = check_local("ba window lists", local_slot, n_local, n_kf, current_index, why, why_bytes))) return rc;
    for (int k = 0; k < n_local; ++k) {
        const ms_pinhole &K = kf_cam[local_slot[k]];
        if (!(std::isfinite(K.fx) && K.fx > 0.0 && std::isfinite(K.fy) && K.fy > 0.0))
            INVALID("ba window lists: the camera of local slot %d has fx %g, fy %g", local_slot[k], K.fx, K.fy);
        if (!std::isfinite(K.cx) || !std::isfinite(K.cy)) INVALID("ba window lists: the camera of local slot %d has cx %g, cy %g", local_slot[k], K.cx, K.cy);
    }
    for (int l = 0; l < n_levels; ++l)
        if (!(std::isfinite(level_sigma_sq[l]) && level_sigma_sq[l] > 0.f)) INVALID("ba window lists: level_sigma_sq[%d] = %g", l, (double)level_sigma_sq[l]);
    if (n_kf > MS_COVIS_MAX_KF || n_mp >= MS_COVIS_MAX_MP || n_rows > MS_TRI_MAX_ROWS || n_obs > MS_TRI_MAX_OBS)
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "ba window lists: %d slots / %d map points / %d rows / %d observations, caps %d / below %d / %d / %d", n_kf, n_mp, n_rows,
                      n_obs, MS_COVIS_MAX_KF, MS_COVIS_MAX_MP, MS_TRI_MAX_ROWS, MS_TRI_MAX_OBS);
    return MS_OK;
}

extern "C" int ms_ba_window_apply_check(const int32_t *kf_mp, int n_kf, int stride, const double *mp_pos, const uint8_t *mp_flags, const int32_t *n_obs, int n_mp,
                                        const double *kf_pose, const double *pose, int n_pose, const double *point, const double *chi2, const ms_ba_window_dev *window,
                                        int n_edge, const int32_t *rows, int n_rows, const int32_t *local_slot, int n_local, int current_index, int mode,
                                        const int32_t *erased_edge, int cap_erased, const int32_t *n_erased, const int32_t *n_stale, char *why, size_t why_bytes) {
    if (n_kf < 0 || n_mp < 0 || n_pose < 0 || n_edge < 0 || n_rows < 0 || n_local < 0 || cap_erased < 0)
        INVALID("ba window apply: negative size (%d slots, %d map points, %d poses, %d edges, %d rows, %d local keyframes, capacity %d)", n_kf, n_mp, n_pose, n_edge, n_rows,
                n_local, cap_erased);
    if (stride < 1) return ms_why_stride("ba window apply", stride, why, why_bytes);
    if (mode != MS_BA_APPLY_LOCAL && mode != MS_BA_APPLY_NEIGHBOR) INVALID("ba window apply: mode %d", mode);
    if (!n_erased || !n_stale) INVALID("ba window apply: missing array (n_erased or n_stale)");
    if (!kf_pose || !pose) INVALID("ba window apply: missing array (kf_pose or pose)");
    if (n_rows > 0 && (!mp_pos || !point || !rows)) INVALID("ba window apply: missing array (mp_pos, point or rows)");
    if (n_pose < n_local) INVALID("ba window apply: %d poses for %d local keyframes", n_pose, n_local);
    if (mode == MS_BA_APPLY_LOCAL) {
        if (!kf_mp || !mp_flags || !n_obs) INVALID("ba window apply: missing array (kf_mp, mp_flags or n_obs)");
        if (n_edge > 0 && (!chi2 || !window || !window->edge_slot || !window->edge_kp || !window->edge_point))
            INVALID("ba window apply: missing array (chi2 or the window's edge arrays)");
        if (n_edge > 0 && n_rows == 0) INVALID("ba window apply: %d edges without a row", n_edge);
        if (cap_erased > 0 && !erased_edge) INVALID("ba window apply: missing array (erased_edge)");
    }
    int rc;
    if ((rc = check_local("ba window apply", local_slot, n_local, n_kf, current_index, why, why_bytes))) return rc;
    if (ms_map_over_capacity(n_kf, stride, n_mp, 0) || n_rows > MS_TRI_MAX_ROWS || n_edge > MS_TRI_MAX_OBS)
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "ba window apply: %d slots / stride %d / %d map points / %d rows / %d edges, caps %d / %d / below %d / %d / %d", n_kf,
                      stride, n_mp, n_rows, n_edge, MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, MS_TRI_MAX_ROWS, MS_TRI_MAX_OBS);
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ loop_chain.hip
namespace {

// what all three entry points ask of the tables' sizes: signs, the stride, the caps; n = the listed slots / candidates and its cap
int check_loop_sizes(const char *who, int n_kf, int stride, int n_mp, int n, int n_cap, char *why, size_t why_bytes) {
    if (n_kf < 0 || n_mp < 0 || n < 0) INVALID("%s: negative size (%d slots, %d map points, %d listed)", who, n_kf, n_mp, n);
    if (stride < 1) return ms_why_stride(who, stride, why, why_bytes);
    if (ms_map_over_capacity(n_kf, stride, n_mp, 0) || n > n_cap)
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "%s: %d slots / stride %d / %d map points / %d listed, caps %d / %d / below %d / %d", who, n_kf, stride, n_mp, n,
                      MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, n_cap);
    return MS_OK;
}

// the current keyframe and the candidates: in range, distinct, cur not among them, keypoint counts inside the stride
int check_loop_candidates(const char *who, int n_kf, int stride, int cur, int n_kp_cur, const int32_t *cand_slot, const int32_t *n_kp_cand, int n_cand, char *why,
                          size_t why_bytes) {
    if (cur < 0 || cur >= n_kf) INVALID("%s: slot %d outside [0, %d)", who, cur, n_kf);
    if (n_kp_cur < 0 || n_kp_cur > stride) INVALID("%s: %d keypoints in a table of stride %d", who, n_kp_cur, stride);
    if (n_cand > 0 && (!cand_slot || !n_kp_cand)) INVALID("%s: missing array (cand_slot or n_kp_cand)", who);
    for (int c = 0; c < n_cand; ++c) {
        if (cand_slot[c] < 0 || cand_slot[c] >= n_kf) INVALID("%s: slot %d outside [0, %d)", who, cand_slot[c], n_kf);
        if (cand_slot[c] == cur) INVALID("%s: the current keyframe's slot %d is among the candidates", who, cur);
        if (n_kp_cand[c] < 0 || n_kp_cand[c] > stride) INVALID("%s: %d keypoints in a table of stride %d", who, n_kp_cand[c], stride);
    }
    if (n_cand > 1) {
        std::vector<int32_t> sorted(cand_slot, cand_slot + n_cand);
        std::sort(sorted.begin(), sorted.end());
        for (int c = 1; c < n_cand; ++c)
            if (sorted[c] == sorted[c - 1]) INVALID("%s: candidate slot %d is listed twice", who, sorted[c]);
    }
    return MS_OK;
}

int check_loop_levels(const char *who, const float *level_sigma_sq, int n_levels, char *why, size_t why_bytes) {
    if (n_levels < 1 || n_levels > MS_TRI_MAX_LEVELS) INVALID("%s: %d levels outside [1, %d]", who, n_levels, MS_TRI_MAX_LEVELS);
    if (!level_sigma_sq) INVALID("%s: missing array (level_sigma_sq)", who);
    for (int l = 0; l < n_levels; ++l)
        if (!(std::isfinite(level_sigma_sq[l]) && level_sigma_sq[l] > 0.f)) INVALID("%s: level_sigma_sq[%d] = %g", who, l, (double)level_sigma_sq[l]);
    return MS_OK;
}

}  // namespace

extern "C" int ms_loop_usable_mask_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, int n_mp, const int32_t *slots,
                                         const int32_t *n_kp, const int32_t *require_triangulated, uint8_t *const *usable, int32_t *const *tri_row, int n_slots, char *why,
                                         size_t why_bytes) {
    (void)mp_live;                                           // may be NULL: every row is live
    int rc;
    if ((rc = check_loop_sizes("loop mask", n_kf, stride, n_mp, n_slots, MS_COVIS_MAX_QUERIES, why, why_bytes))) return rc;
    if (n_slots > 0 && (!kf_mp || !slots || !n_kp || !require_triangulated || !usable))
        INVALID("loop mask: missing array (kf_mp, slots, n_kp, require_triangulated or usable)");
    for (int s = 0; s < n_slots; ++s) {
        if (slots[s] < 0 || slots[s] >= n_kf) INVALID("loop mask: slot %d outside [0, %d)", slots[s], n_kf);
        if (n_kp[s] < 0 || n_kp[s] > stride) INVALID("loop mask: %d keypoints in a table of stride %d", n_kp[s], stride);
        if (n_kp[s] > 0 && !usable[s]) INVALID("loop mask: missing array (usable of slot %d)", slots[s]);
        if (!mp_flags && (require_triangulated[s] || (tri_row && tri_row[s])))
            INVALID("loop mask: slot %d requires TRIANGULATED or asks for tri_row with mp_flags == NULL", slots[s]);
    }
    return MS_OK;
}

extern "C" int ms_loop_pairs_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const double *mp_pos, int n_mp, const double *kf_pose,
                                   const int32_t *kp_octave, int cur, int n_kp_cur, const int32_t *cand_slot, const int32_t *n_kp_cand, const int32_t *const *matched,
                                   int n_cand, const float *level_sigma_sq, int n_levels, int cap_pairs, const int32_t *pair_start, const int32_t *kp1, const int32_t *kp2,
                                   const int32_t *row1, const int32_t *row2, const double *pts1, const double *pts2, const float *thr1, const float *thr2,
                                   const double *cur_pose, const double *cand_pose, const int32_t *n_pairs, char *why, size_t why_bytes) {
    (void)mp_live;                                           // may be NULL: every row is live
    int rc;
    if (cap_pairs < 0) INVALID("loop pairs: negative size (capacity %d)", cap_pairs);
    if ((rc = check_loop_sizes("loop pairs", n_kf, stride, n_mp, n_cand, MS_LOOP_MAX_CANDIDATES, why, why_bytes))) return rc;
    if (!kf_mp || !kf_pose || !kp_octave || (n_mp > 0 && !mp_pos)) INVALID("loop pairs: missing array (kf_mp, kf_pose, kp_octave or mp_pos)");
    if (!pair_start || !n_pairs || !cur_pose || (n_cand > 0 && !cand_pose)) INVALID("loop pairs: missing array (pair_start, n_pairs, cur_pose or cand_pose)");
    if (cap_pairs > 0 && (!kp1 || !kp2 || !row1 || !row2 || !pts1 || !pts2 || !thr1 || !thr2))
        INVALID("loop pairs: missing array (kp1, kp2, row1, row2, pts1, pts2, thr1 or thr2)");
    if ((rc = check_loop_candidates("loop pairs", n_kf, stride, cur, n_kp_cur, cand_slot, n_kp_cand, n_cand, why, why_bytes))) return rc;
    if (n_cand > 0 && !matched) INVALID("loop pairs: missing array (matched)");
    for (int c = 0; c < n_cand && n_kp_cur > 0; ++c)
        if (!matched[c]) INVALID("loop pairs: missing array (matched of candidate slot %d)", cand_slot[c]);
    return check_loop_levels("loop pairs", level_sigma_sq, n_levels, why, why_bytes);
}

extern "C" int ms_loop_sim3_lists_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const double *mp_pos, int n_mp, const double *kf_pose,
                                        const float *kp_x, const float *kp_y, const int32_t *kp_octave, int cur, int n_kp_cur, const int32_t *cand_slot,
                                        const int32_t *n_kp_cand, int n_cand, const ms_pinhole *kf_cam, const float *level_sigma_sq, int n_levels, const int32_t *kp1,
                                        const int32_t *kp2, const int32_t *match_start, const double *pts1, const double *pts2, const double *obs1, const double *obs2,
                                        const float *info1, const float *info2, const int32_t *row1, const int32_t *row2, char *why, size_t why_bytes) {
    (void)mp_live;                                           // may be NULL: every row is live
    int rc;
    if ((rc = check_loop_sizes("loop sim3 lists", n_kf, stride, n_mp, n_cand, MS_LOOP_MAX_CANDIDATES, why, why_bytes))) return rc;
    if (!kf_mp || !kf_pose || !kp_x || !kp_y || !kp_octave || !kf_cam || (n_mp > 0 && !mp_pos))
        INVALID("loop sim3 lists: missing array (kf_mp, kf_pose, kp_x, kp_y, kp_octave, kf_cam or mp_pos)");
    if (!match_start) INVALID("loop sim3 lists: missing array (match_start)");
    if ((rc = check_loop_candidates("loop sim3 lists", n_kf, stride, cur, n_kp_cur, cand_slot, n_kp_cand, n_cand, why, why_bytes))) return rc;
    if (match_start[0] != 0) INVALID("loop sim3 lists: match_start[0] = %d", match_start[0]);
    for (int c = 0; c < n_cand; ++c) {
        const long long n = (long long)match_start[c + 1] - match_start[c];
        if (n < 0) INVALID("loop sim3 lists: match_start descends at candidate %d (%d after %d)", c, match_start[c + 1], match_start[c]);
        if (n > stride)
            return ms_why(MS_ERR_CAPACITY, why, why_bytes, "loop sim3 lists: %lld matches for candidate slot %d, more than the stride of %d", n, cand_slot[c], stride);
    }
    if (match_start[n_cand] > 0 && (!kp1 || !kp2 || !pts1 || !pts2 || !obs1 || !obs2 || !info1 || !info2 || !row1 || !row2))
        INVALID("loop sim3 lists: missing array (kp1, kp2, pts1, pts2, obs1, obs2, info1, info2, row1 or row2)");
    for (int c = -1; c < n_cand; ++c) {
        const int slot = c < 0 ? cur : cand_slot[c];
        const ms_pinhole &K = kf_cam[slot];
        if (!(std::isfinite(K.fx) && K.fx > 0.0 && std::isfinite(K.fy) && K.fy > 0.0)) INVALID("loop sim3 lists: the camera of slot %d has fx %g, fy %g", slot, K.fx, K.fy);
        if (!std::isfinite(K.cx) || !std::isfinite(K.cy)) INVALID("loop sim3 lists: the camera of slot %d has cx %g, cy %g", slot, K.cx, K.cy);
    }
    return check_loop_levels("loop sim3 lists", level_sigma_sq, n_levels, why, why_bytes);
}

// ------------------------------------------------------------------------------------------------ pose_tables.hip
extern "C" int ms_pose_tables_solve_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const double *mp_pos, int n_mp,
                                          const float *kp_x, const float *kp_y, const int32_t *kp_octave, const double *kf_pose, const ms_pose_tables_frame *f,
                                          const ms_pose_tables_out *out, char *why, size_t why_bytes) {
    (void)mp_live;                                           // may be NULL: every row is live
    if (n_kf < 0 || n_mp < 0) INVALID("pose tables: negative size (%d slots, %d map points)", n_kf, n_mp);
    if (stride < 1) return ms_why_stride("pose tables", stride, why, why_bytes);
    if (!f || !out) INVALID("pose tables: missing array (frame or out)");
    if (f->n_kp < 0) INVALID("pose tables: negative size (%d keypoints)", f->n_kp);
    if (f->n_kp > stride) INVALID("pose tables: %d keypoints in a table of stride %d", f->n_kp, stride);
    if (f->slot < 0 || f->slot >= n_kf) INVALID("pose tables: slot %d outside [0, %d)", f->slot, n_kf);
    if (f->prev_slot < -1 || f->prev_slot >= n_kf) INVALID("pose tables: previous slot %d outside [-1, %d)", f->prev_slot, n_kf);
    if (f->prev_slot == f->slot) INVALID("pose tables: slot %d is its own previous keyframe", f->slot);
    if (!kf_mp || !kp_x || !kp_y || !kp_octave || !kf_pose) INVALID("pose tables: missing array (kf_mp, the keypoint table or kf_pose)");
    if (n_mp > 0 && (!mp_flags || !mp_pos)) INVALID("pose tables: missing array (mp_flags or mp_pos)");
    const ms_pinhole &K = f->cam;
    if (K.width < 1 || K.height < 1 || !(K.fx > 0.0) || !(K.fy > 0.0) || !std::isfinite(K.fx) || !std::isfinite(K.fy) || !std::isfinite(K.cx) || !std::isfinite(K.cy))
        INVALID("pose tables: bad camera (%d x %d, fx %g, fy %g)", K.width, K.height, K.fx, K.fy);
    for (int i = 0; i < 7; ++i)
        if (!std::isfinite(f->edge_meas[i])) INVALID("pose tables: edge_meas[%d] is not finite", i);
    for (int i = 0; i < 36; ++i)
        if (!std::isfinite(f->edge_info[i])) INVALID("pose tables: edge_info[%d] is not finite", i);
    if (!std::isfinite(f->huber_delta)) INVALID("pose tables: huber_delta is not finite");
    if (f->max_iters < 0) INVALID("pose tables: max_iters %d", f->max_iters);
    if (ms_map_over_capacity(n_kf, stride, n_mp, 0)) return ms_why_table_caps("pose tables", n_kf, stride, n_mp, why, why_bytes);
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ frame_finish.hip
// (named _validate, not _check: the header says why)
extern "C" int ms_frame_finish_validate(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const double *mp_pos,
                                        const int32_t *mp_track, const int32_t *n_obs, int n_mp, const int32_t *kf_id, const int32_t *remove_slots, int n_remove,
                                        const ms_frame_finish_args *args, const int32_t *cloud_row, const int32_t *cloud_kp, const int32_t *cloud_track,
                                        const double *cloud_pos, const int32_t *removed_rows, int cap_removed, const int32_t *counts, char *why, size_t why_bytes) {
    (void)mp_track; (void)n_obs; (void)cloud_row; (void)cloud_kp; (void)cloud_track; (void)cloud_pos;      // each may be NULL
    if (n_remove < 0 || cap_removed < 0) INVALID("frame finish: negative size (%d removed slots, capacity %d)", n_remove, cap_removed);
    if (!args || !counts) INVALID("frame finish: missing array (args or counts)");
    if (n_remove > 0 && !remove_slots) INVALID("frame finish: missing array (remove_slots)");
    if (cap_removed > 0 && !removed_rows) INVALID("frame finish: missing array (removed_rows)");
    int rc;
    if ((rc = ms_kf_table_check("frame finish", kf_mp, n_kf, stride, n_mp, kf_id, why, why_bytes))) return rc;
    if (n_mp > 0 && (!mp_flags || !mp_pos)) INVALID("frame finish: missing array (mp_flags or mp_pos)");
    if (n_remove > 0 && !mp_live) INVALID("frame finish: mp_live == NULL with %d removed slots", n_remove);
    if (args->cloud_slot < -1 || args->cloud_slot >= n_kf) INVALID("frame finish: cloud slot %d outside [-1, %d)", args->cloud_slot, n_kf);
    if (args->cloud_slot >= 0 && kf_id[args->cloud_slot] < 0) INVALID("frame finish: cloud slot %d is empty (kf_id %d)", args->cloud_slot, kf_id[args->cloud_slot]);
    if (args->n_kp < 0 || args->n_kp > stride) INVALID("frame finish: %d keypoints in a table of stride %d", args->n_kp, stride);
    if (n_remove > MS_COVIS_MAX_QUERIES || ms_map_over_capacity(n_kf, stride, n_mp, 0))
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "frame finish: %d slots / stride %d / %d map points / %d removed slots, caps %d / %d / below %d / %d", n_kf, stride, n_mp,
                      n_remove, MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, MS_COVIS_MAX_QUERIES);
    int bad = 0;
    if (!ms_distinct_in_range(remove_slots, n_remove, n_kf, &bad)) {
        if (bad < 0) INVALID("frame finish: removed slot %d is listed twice", -1 - bad);
        INVALID("frame finish: removed slot %d outside [0, %d)", remove_slots[bad], n_kf);
    }
    for (int i = 0; i < n_remove; ++i)
        if (kf_id[remove_slots[i]] < 0) INVALID("frame finish: removed slot %d is empty (kf_id %d)", remove_slots[i], kf_id[remove_slots[i]]);
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ keyframe_admit.hip
// (named _validate, not _check: the header says why)
extern "C" int ms_keyframe_admit_validate(const ms_keypoints *view, int frame, const int32_t *kf_mp, int n_kf, int stride, int n_mp, const float *kp_x, const float *kp_y,
                                          const int32_t *kp_octave, const float *kp_depth, const uint32_t *desc_pool, int n_pool, const double *kf_pose,
                                          const ms_admit_args *args, const ms_admit_frame *out, const ms_admit_host *host, const int32_t *counts, char *why,
                                          size_t why_bytes) {
    (void)host;                                              // the struct and each member may be NULL
    if (n_kf < 0 || n_mp < 0 || n_pool < 0) INVALID("keyframe admit: negative size (%d slots, %d map points, %d pool entries)", n_kf, n_mp, n_pool);
    if (stride < 1) return ms_why_stride("keyframe admit", stride, why, why_bytes);
    if (!view || !args || !out || !counts) INVALID("keyframe admit: missing array (view, args, out or counts)");
    if (!view->count || !view->x || !view->y || !view->angle || !view->octave || !view->desc || !view->track_id)
        INVALID("keyframe admit: missing array (count, x, y, angle, octave, desc or track_id of the view)");
    if (!kf_mp || !kp_x || !kp_y || !kp_octave || !kp_depth || !desc_pool || !kf_pose)
        INVALID("keyframe admit: missing array (kf_mp, the keypoint table, desc_pool or kf_pose)");
    if (!out->desc || !out->angle || !out->octave || !out->bearing || !out->usable || !out->sorted_x || !out->sorted_y || !out->sorted_idx || !out->node_id ||
        !out->node_start || !out->kp_idx)
        INVALID("keyframe admit: missing array (a frame array of out)");
    if (view->capacity < 0 || out->cap_kp < 0 || args->n_tracks < 0)
        INVALID("keyframe admit: negative size (view capacity %d, cap_kp %d, %d tracks)", view->capacity, out->cap_kp, args->n_tracks);
    if (frame < 0 || frame >= MS_COVIS_MAX_KF) INVALID("keyframe admit: frame %d outside [0, %d)", frame, MS_COVIS_MAX_KF);
    if (args->slot < 0 || args->slot >= n_kf) INVALID("keyframe admit: slot %d outside [0, %d)", args->slot, n_kf);
    if (args->desc_base < 0 || args->desc_base > n_pool) INVALID("keyframe admit: desc_base %d outside [0, %d]", args->desc_base, n_pool);
    if ((reinterpret_cast<uintptr_t>(view->desc) | reinterpret_cast<uintptr_t>(desc_pool) | reinterpret_cast<uintptr_t>(out->desc)) & 15u)
        INVALID("keyframe admit: descriptor arrays must be 16-byte aligned");
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(args->pose[i])) INVALID("keyframe admit: pose[%d] is not finite", i);
    const ms_pinhole &K = args->cam;
    if (!(K.fx > 0.0) || !(K.fy > 0.0) || !std::isfinite(K.fx) || !std::isfinite(K.fy) || !std::isfinite(K.cx) || !std::isfinite(K.cy))
        INVALID("keyframe admit: bad camera (fx %g, fy %g, cx %g, cy %g)", K.fx, K.fy, K.cx, K.cy);
    if (args->vocab && args->levels_up < 0) INVALID("keyframe admit: levels_up %d", args->levels_up);
    if ((args->track_ids == nullptr) != (args->track_depth == nullptr)) INVALID("keyframe admit: missing array (track_ids or track_depth)");
    if (args->n_tracks > 0 && !args->track_ids) INVALID("keyframe admit: missing array (track_ids with %d tracks)", args->n_tracks);
    if (args->depth_image && (args->depth_width < 1 || args->depth_height < 1 || args->depth_stride < args->depth_width))
        INVALID("keyframe admit: a depth image of %d x %d, row stride %d", args->depth_width, args->depth_height, args->depth_stride);
    if (view->capacity > MS_COVIS_MAX_STRIDE || out->cap_kp > MS_COVIS_MAX_STRIDE || args->n_tracks > MS_COVIS_MAX_STRIDE)
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "keyframe admit: view capacity %d / cap_kp %d / %d tracks, caps %d each", view->capacity, out->cap_kp, args->n_tracks,
                      MS_COVIS_MAX_STRIDE);
    if (args->depth_image && ((long long)args->depth_stride * args->depth_height > 0x7fffffffLL))
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "keyframe admit: a depth image of %d rows of %d elements, caps below 2^31 elements", args->depth_height, args->depth_stride);
    if (ms_map_over_capacity(n_kf, stride, n_mp, 0)) return ms_why_table_caps("keyframe admit", n_kf, stride, n_mp, why, why_bytes);
    return MS_OK;
}

// ms_bow_vector.  word / weight / words / values are DEVICE arrays: only their presence and alignment is looked at.
extern "C" int ms_bow_vector_validate(const int32_t *word, const double *weight, int n, int vocab_words, int cap, const int32_t *words, const double *values,
                                      const int32_t *counts, char *why, size_t why_bytes) {
    if (n < 0 || cap < 0) INVALID("bow vector: negative size (%d keypoints, cap %d)", n, cap);
    if (vocab_words < 1) INVALID("bow vector: a vocabulary of %d words", vocab_words);
    if (!counts) INVALID("bow vector: missing array (counts)");
    if (n > 0 && (!word || !weight)) INVALID("bow vector: missing array (word or weight with %d keypoints)", n);
    if (cap > 0 && (!words || !values)) INVALID("bow vector: missing array (words or values with cap %d)", cap);
    if ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(values)) & 7u) INVALID("bow vector: weight and values must be 8-byte aligned");
    if (n > MS_COVIS_MAX_STRIDE || cap > MS_COVIS_MAX_STRIDE)
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "bow vector: %d keypoints / cap %d, caps %d each", n, cap, MS_COVIS_MAX_STRIDE);
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ map_extract.hip
// (named _validate, not _check: the header says why)
extern "C" int ms_map_extract_validate(const ms_map_extract_src *src, const ms_map_extract_dst *dst, const int32_t *kf_id, const int32_t *active, int n_active,
                                       const int32_t *desc_base, const int32_t *n_kp, const int32_t *dst_desc_base, const int32_t *counts, char *why, size_t why_bytes) {
    if (!src || !dst || !counts) INVALID("map extract: missing array (src, dst or counts)");
    const ms_map_extract_src &S = *src;
    const ms_map_extract_dst &D = *dst;
    if (n_active < 0 || S.n_track < 0 || S.pool_size < 0 || D.n_kf < 0 || D.n_mp < 0 || D.pool_size < 0)
        INVALID("map extract: negative size (%d active slots, %d tracks, pools of %d and %d, a destination of %d slots and %d map points)", n_active, S.n_track, S.pool_size,
                D.pool_size, D.n_kf, D.n_mp);
    int rc;
    if ((rc = ms_kf_table_check("map extract", S.kf_mp, S.n_kf, S.stride, S.n_mp, kf_id, why, why_bytes))) return rc;
    if (S.n_mp > 0 && (!S.mp_flags || !S.mp_pos || !S.mp_norm || !S.mp_min_dist || !S.mp_max_dist || !S.mp_desc)) INVALID("map extract: missing array (a source map-point array)");
    if (D.n_mp > 0 && (!D.mp_flags || !D.mp_live || !D.mp_pos || !D.mp_norm || !D.mp_min_dist || !D.mp_max_dist || !D.mp_desc))
        INVALID("map extract: missing array (a destination map-point array)");
    if (D.n_kf > 0 && !D.kf_mp) INVALID("map extract: missing array (the destination's kf_mp)");
    if (n_active > 0 && (!active || !dst_desc_base)) INVALID("map extract: missing array (active or dst_desc_base)");
    if (S.track_row && !S.mp_track) INVALID("map extract: track_row without mp_track");
    const int n_src_kp = (S.kp_x != nullptr) + (S.kp_y != nullptr) + (S.kp_octave != nullptr) + (S.kp_depth != nullptr);
    const int n_dst_kp = (D.kp_x != nullptr) + (D.kp_y != nullptr) + (D.kp_octave != nullptr) + (D.kp_depth != nullptr);
    if (n_src_kp % 4 || n_dst_kp % 4) INVALID("map extract: %d of the four keypoint arrays of the %s", n_src_kp % 4 ? n_src_kp : n_dst_kp, n_src_kp % 4 ? "source" : "destination");
    if (n_src_kp != n_dst_kp) INVALID("map extract: the keypoint arrays are given for the %s only", n_src_kp ? "source" : "destination");
    const struct { const char *name; const void *s, *d; } pairs[] = {
        {"mp_track", S.mp_track, D.mp_track}, {"kf_pose", S.kf_pose, D.kf_pose}, {"track_row", S.track_row, D.track_row}, {"desc_pool", S.desc_pool, D.desc_pool}};
    for (const auto &p : pairs)
        if ((p.s != nullptr) != (p.d != nullptr)) INVALID("map extract: %s is given for the %s only", p.name, p.s ? "source" : "destination");
    const struct { const char *name; const void *s, *d; } same[] = {
        {"kf_mp", S.kf_mp, D.kf_mp}, {"mp_flags", S.mp_flags, D.mp_flags}, {"mp_live", S.mp_live, D.mp_live}, {"mp_pos", S.mp_pos, D.mp_pos}, {"mp_norm", S.mp_norm, D.mp_norm},
        {"mp_min_dist", S.mp_min_dist, D.mp_min_dist}, {"mp_max_dist", S.mp_max_dist, D.mp_max_dist}, {"mp_desc", S.mp_desc, D.mp_desc}, {"mp_track", S.mp_track, D.mp_track},
        {"kp_x", S.kp_x, D.kp_x}, {"kp_y", S.kp_y, D.kp_y}, {"kp_octave", S.kp_octave, D.kp_octave}, {"kp_depth", S.kp_depth, D.kp_depth}, {"kf_pose", S.kf_pose, D.kf_pose},
        {"track_row", S.track_row, D.track_row}, {"desc_pool", S.desc_pool, D.desc_pool}};
    for (const auto &p : same)
        if (p.s && p.s == p.d) INVALID("map extract: the destination's %s is the source's", p.name);
    if ((reinterpret_cast<uintptr_t>(S.mp_desc) | reinterpret_cast<uintptr_t>(D.mp_desc) | reinterpret_cast<uintptr_t>(S.desc_pool) | reinterpret_cast<uintptr_t>(D.desc_pool)) & 15u)
        INVALID("map extract: descriptor arrays must be 16-byte aligned");
    if (ms_map_over_capacity(S.n_kf, S.stride, S.n_mp, 0)) return ms_why_table_caps("map extract", S.n_kf, S.stride, S.n_mp, why, why_bytes);
    if (ms_map_over_capacity(D.n_kf, S.stride, D.n_mp, 0)) return ms_why_table_caps("map extract: destination", D.n_kf, S.stride, D.n_mp, why, why_bytes);
    if (S.n_track > MS_TRACKED_MAX_WINDOW) return ms_why(MS_ERR_CAPACITY, why, why_bytes, "map extract: a track window of %d, cap %d", S.n_track, MS_TRACKED_MAX_WINDOW);
    if (n_active > D.n_kf) INVALID("map extract: %d active slots for a destination of %d slots", n_active, D.n_kf);
    int bad = 0;
    if (!ms_distinct_in_range(active, n_active, S.n_kf, &bad)) {
        if (bad < 0) INVALID("map extract: active slot %d is listed twice", -1 - bad);
        INVALID("map extract: active slot %d outside [0, %d)", active[bad], S.n_kf);
    }
    for (int i = 0; i < n_active; ++i)
        if (kf_id[active[i]] < 0) INVALID("map extract: active slot %d is empty (kf_id %d)", active[i], kf_id[active[i]]);
    if (!S.desc_pool) return MS_OK;
    if (n_active > 0 && (!desc_base || !n_kp)) INVALID("map extract: missing array (desc_base or n_kp with a pool)");
    long long total = 0;
    for (int i = 0; i < n_active; ++i) {
        if (n_kp[i] < 0 || n_kp[i] > S.stride) INVALID("map extract: active slot %d: %d keypoints in a table of stride %d", active[i], n_kp[i], S.stride);
        const int32_t base = desc_base[active[i]];
        if (base < 0) continue;
        if ((long long)base + n_kp[i] > S.pool_size) INVALID("map extract: active slot %d: descriptors [%d, %d + %d) outside the pool of %d", active[i], base, base, n_kp[i], S.pool_size);
        total += n_kp[i];
    }
    if (total > D.pool_size) INVALID("map extract: %lld descriptors for a destination pool of %d", total, D.pool_size);
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ frame_admit.hip
// (named _validate, not _check: the header says why)
extern "C" int ms_frame_admit_validate(const int32_t *kf_mp, int n_kf, int stride, int n_mp, const float *kp_x, const float *kp_y, const int32_t *kp_octave,
                                       const float *kp_depth, const double *kf_pose, const float *x, const float *y, const int32_t *id, const float *depth, const uint8_t *keep,
                                       int n_tracks, const ms_frame_admit_args *args, const int32_t *kp_track, const int32_t *kp_feature, int cap_kp, const int32_t *counts,
                                       char *why, size_t why_bytes) {
    (void)keep; (void)kp_track; (void)kp_feature;            // each may be NULL
    if (n_kf < 0 || n_mp < 0 || n_tracks < 0 || cap_kp < 0) INVALID("frame admit: negative size (%d slots, %d map points, %d features, cap_kp %d)", n_kf, n_mp, n_tracks, cap_kp);
    if (stride < 1) return ms_why_stride("frame admit", stride, why, why_bytes);
    if (!args || !counts) INVALID("frame admit: missing array (args or counts)");
    if (!kf_mp || !kp_x || !kp_y || !kp_octave || !kp_depth || !kf_pose) INVALID("frame admit: missing array (kf_mp, the keypoint table or kf_pose)");
    if (n_tracks > 0 && (!x || !y || !id || !depth)) INVALID("frame admit: missing array (x, y, id or depth with %d features)", n_tracks);
    if (args->slot < 0 || args->slot >= n_kf) INVALID("frame admit: slot %d outside [0, %d)", args->slot, n_kf);
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(args->pose[i])) INVALID("frame admit: pose[%d] is not finite", i);
    if (args->depth_image && (args->depth_width < 1 || args->depth_height < 1 || args->depth_stride < args->depth_width))
        INVALID("frame admit: a depth image of %d x %d, row stride %d", args->depth_width, args->depth_height, args->depth_stride);
    if (args->valid_mask && (args->mask_width < 1 || args->mask_height < 1 || args->mask_stride < args->mask_width))
        INVALID("frame admit: a valid mask of %d x %d, row stride %d", args->mask_width, args->mask_height, args->mask_stride);
    if (n_tracks > MS_COVIS_MAX_STRIDE || cap_kp > MS_COVIS_MAX_STRIDE)
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "frame admit: %d features / cap_kp %d, caps %d each", n_tracks, cap_kp, MS_COVIS_MAX_STRIDE);
    if (args->depth_image && ((long long)args->depth_stride * args->depth_height > 0x7fffffffLL))
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "frame admit: a depth image of %d rows of %d elements, caps below 2^31 elements", args->depth_height, args->depth_stride);
    if (args->valid_mask && ((long long)args->mask_stride * args->mask_height > 0x7fffffffLL))
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "frame admit: a valid mask of %d rows of %d bytes, caps below 2^31 bytes", args->mask_height, args->mask_stride);
    if (ms_map_over_capacity(n_kf, stride, n_mp, 0)) return ms_why_table_caps("frame admit", n_kf, stride, n_mp, why, why_bytes);
    for (int i = 0; i < n_tracks; ++i) {
        if (!std::isfinite(x[i]) || !std::isfinite(y[i])) INVALID("frame admit: feature %d has a coordinate that is not finite", i);
        if (id[i] < 0) INVALID("frame admit: feature %d has the id %d (a negative id reads as no track)", i, id[i]);
    }
    std::vector<int32_t> &ids = tl_ids();
    if (ids.capacity() < (size_t)n_tracks) { ids.reserve((size_t)n_tracks + (size_t)n_tracks / 2); ++g_ms_host_allocs; }
    ids.assign(id, id + n_tracks);
    std::sort(ids.begin(), ids.end());
    for (int i = 1; i < n_tracks; ++i)
        if (ids[i - 1] == ids[i]) INVALID("frame admit: track id %d is listed twice", ids[i]);
    return MS_OK;
}

// ------------------------------------------------------------------------------------------------ map_publish.hip
// (named _validate, not _check: the header says why)
extern "C" int ms_map_publish_validate(const double *mp_pos, const float *mp_norm, const uint8_t *mp_flags, const uint8_t *mp_live, const int32_t *n_obs, const uint8_t *mp_color,
                                       int n_mp, const int32_t *kf_mp, int n_kf, int stride, const double *kf_pose, const int32_t *local_rows, int n_local, const float *rec_pos,
                                       const uint8_t *rec_state, const ms_map_publish_args *args, const int32_t *kf_list, int n_list, const int32_t *pub_row, const float *pub_pos,
                                       const float *pub_norm, const float *pub_color, const uint8_t *pub_status, const uint8_t *pub_bits, int cap_pub, const int32_t *ev_row,
                                       const uint8_t *ev_kind, const float *ev_pos, const float *ev_norm, int cap_ev, const float *pose_wc, const int32_t *counts, char *why,
                                       size_t why_bytes) {
    (void)mp_color;                                          // may be NULL
    if (n_mp < 0 || n_kf < 0 || n_local < 0 || n_list < 0 || cap_pub < 0 || cap_ev < 0)
        INVALID("map publish: negative size (%d map points, %d slots, %d local rows, %d listed slots, cap_pub %d, cap_ev %d)", n_mp, n_kf, n_local, n_list, cap_pub, cap_ev);
    if (stride < 1) return ms_why_stride("map publish", stride, why, why_bytes);
    if (!args || !counts) INVALID("map publish: missing array (args or counts)");
    if (args->what < 1 || args->what > (MS_PUBLISH_VIEW | MS_PUBLISH_RECORD)) INVALID("map publish: what %d outside 1 .. 3", args->what);
    if (args->min_record_obs < 0) INVALID("map publish: min_record_obs %d", args->min_record_obs);
    const bool view = (args->what & MS_PUBLISH_VIEW) != 0, record = (args->what & MS_PUBLISH_RECORD) != 0;
    if (n_mp > 0 && (!mp_pos || !mp_norm || !mp_flags || !mp_live)) INVALID("map publish: missing array (mp_pos, mp_norm, mp_flags or mp_live)");
    if (n_kf > 0 && (!kf_mp || !kf_pose)) INVALID("map publish: missing array (kf_mp or kf_pose)");
    if (n_local > 0 && !local_rows) INVALID("map publish: missing array (local_rows with %d entries)", n_local);
    if (n_list > 0 && (!kf_list || !pose_wc)) INVALID("map publish: missing array (kf_list or pose_wc with %d listed slots)", n_list);
    if (record && n_mp > 0 && (!n_obs || !rec_pos || !rec_state)) INVALID("map publish: missing array (n_obs, rec_pos or rec_state with MS_PUBLISH_RECORD)");
    if (view && cap_pub > 0 && (!pub_row || !pub_pos || !pub_norm || !pub_color || !pub_status || !pub_bits)) INVALID("map publish: missing array (a pub_ array with cap_pub %d)", cap_pub);
    if (record && cap_ev > 0 && (!ev_row || !ev_kind || !ev_pos || !ev_norm)) INVALID("map publish: missing array (an ev_ array with cap_ev %d)", cap_ev);
    if (args->current_slot < -1 || args->current_slot >= n_kf) INVALID("map publish: current slot %d outside [-1, %d)", args->current_slot, n_kf);
    if (n_local >= MS_COVIS_MAX_MP || n_list > MS_COVIS_MAX_KF || ms_map_over_capacity(n_kf, stride, n_mp, 0))
        return ms_why(MS_ERR_CAPACITY, why, why_bytes, "map publish: %d slots / stride %d / %d map points / %d local rows / %d listed slots, caps %d / %d / below %d / below %d / %d", n_kf,
                      stride, n_mp, n_local, n_list, MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, MS_COVIS_MAX_MP, MS_COVIS_MAX_KF);
    int bad = 0;
    if (!ms_distinct_in_range(kf_list, n_list, n_kf, &bad)) {
        if (bad < 0) INVALID("map publish: listed slot %d is listed twice", -1 - bad);
        INVALID("map publish: listed slot %d outside [0, %d)", kf_list[bad], n_kf);
    }
    return MS_OK;
}
