// map_fuse_check.h -- the validation half of ms_map_fuse and ms_map_replace_pairs (map_fuse.hip).  Plain C++17, no HIP and no context: it
// reads the HOST arrays only and asks of the DEVICE arrays nothing but whether they are there, so a program can compile it alone
// (MAP_FUSE_HOST_ONLY) and run it under sanitizers.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>
#include "../../include/mi355slam.h"

namespace ms_fuse {

inline int why_is(int code, char *why, size_t bytes, const char *fmt, ...) {
    if (why && bytes) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(why, bytes, fmt, ap);
        va_end(ap);
    }
    return code;
}

// what both entry points ask of the tables
inline int check_tables(const char *who, const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const int32_t *n_obs, int n_mp,
                        const int32_t *mp_track, const int32_t *track_row, int n_track, char *why, size_t bytes) {
    if (n_kf < 0 || n_mp < 0 || n_track < 0) return why_is(MS_ERR_INVALID, why, bytes, "%s: negative size (%d slots, %d map points, %d tracks)", who, n_kf, n_mp, n_track);
    if (stride < 1) return why_is(MS_ERR_INVALID, why, bytes, "%s: stride %d", who, stride);
    if ((n_kf > 0 && !kf_mp) || (n_mp > 0 && (!mp_flags || !mp_live || !n_obs)))
        return why_is(MS_ERR_INVALID, why, bytes, "%s: missing array (kf_mp, mp_flags, mp_live or n_obs)", who);
    if ((mp_track != nullptr) != (track_row != nullptr)) return why_is(MS_ERR_INVALID, why, bytes, "%s: one track table without the other", who);
    if (n_kf > MS_COVIS_MAX_KF || stride > MS_COVIS_MAX_STRIDE || n_mp >= MS_COVIS_MAX_MP)
        return why_is(MS_ERR_CAPACITY, why, bytes, "%s: %d slots / stride %d / %d map points, caps %d / %d / below %d", who, n_kf, stride, n_mp, MS_COVIS_MAX_KF,
                      MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP);
    if (n_track > MS_TRACKED_MAX_WINDOW) return why_is(MS_ERR_CAPACITY, why, bytes, "%s: a track window of %d, cap %d", who, n_track, MS_TRACKED_MAX_WINDOW);
    return MS_OK;
}

// `sorted` is the caller's scratch and only grows
inline int check_fuse(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const int32_t *n_obs, int n_mp, const int32_t *mp_track,
                      const int32_t *track_row, int n_track, const int32_t *kept_entry, const int32_t *top_idx, const uint16_t *top_dist, const int32_t *mp_index,
                      int n_entries, const ms_fuse_view *views, const int32_t *n_kept, int n_views, int max_dist, int source_slot, const int32_t *n_erased,
                      const int32_t *counts, const int32_t *views_done, std::vector<int32_t> &sorted, char *why, size_t bytes) {
    int rc;
    if ((rc = check_tables("map fuse", kf_mp, n_kf, stride, mp_flags, mp_live, n_obs, n_mp, mp_track, track_row, n_track, why, bytes))) return rc;
    if (n_entries < 0 || n_views < 0) return why_is(MS_ERR_INVALID, why, bytes, "map fuse: negative size (%d entries, %d views)", n_entries, n_views);
    if (!n_erased || !counts || !views_done || (n_views > 0 && (!views || !n_kept)) || (n_entries > 0 && (!mp_index || !kept_entry || !top_idx || !top_dist)))
        return why_is(MS_ERR_INVALID, why, bytes, "map fuse: missing array");
    if (n_views > MS_GATE_MAX_VIEWS || n_entries >= MS_GATE_MAX_ENTRIES)
        return why_is(MS_ERR_CAPACITY, why, bytes, "map fuse: %d views / %d entries, caps %d / below %d", n_views, n_entries, MS_GATE_MAX_VIEWS, MS_GATE_MAX_ENTRIES);
    if (max_dist < 0 || max_dist > 256) return why_is(MS_ERR_INVALID, why, bytes, "map fuse: max_dist %d outside [0, 256]", max_dist);
    if (source_slot < -1 || source_slot >= n_kf) return why_is(MS_ERR_INVALID, why, bytes, "map fuse: source slot %d outside [-1, %d)", source_slot, n_kf);
    for (int v = 0; v < n_views; ++v) {
        const ms_fuse_view &V = views[v];
        if (V.slot < 0 || V.slot >= n_kf) return why_is(MS_ERR_INVALID, why, bytes, "map fuse: view %d: slot %d outside [0, %d)", v, V.slot, n_kf);
        if (V.first < 0 || V.count < 0 || V.first > n_entries || V.count > n_entries - V.first)
            return why_is(MS_ERR_INVALID, why, bytes, "map fuse: view %d: slice [%d, %d + %d) outside [0, %d)", v, V.first, V.first, V.count, n_entries);
        if (n_kept[v] < 0 || n_kept[v] > V.count) return why_is(MS_ERR_INVALID, why, bytes, "map fuse: view %d: n_kept %d for a slice of %d", v, n_kept[v], V.count);
    }
    // overlapping slices: the non-empty ones in the order of their first entries
    sorted.clear();
    for (int v = 0; v < n_views; ++v) if (views[v].count > 0) sorted.push_back(v);
    std::sort(sorted.begin(), sorted.end(), [&](int32_t a, int32_t b) { return views[a].first < views[b].first; });
    for (size_t i = 1; i < sorted.size(); ++i) {
        const ms_fuse_view &A = views[sorted[i - 1]], &B = views[sorted[i]];
        if (A.first + A.count > B.first) return why_is(MS_ERR_INVALID, why, bytes, "map fuse: the slices of views %d and %d overlap", sorted[i - 1], sorted[i]);
    }
    for (int v = 0; v < n_views; ++v) {
        const ms_fuse_view &V = views[v];
        for (int e = V.first; e < V.first + V.count; ++e)
            if (mp_index[e] < 0 || mp_index[e] >= n_mp)
                return why_is(MS_ERR_INVALID, why, bytes, "map fuse: view %d: entry %d is row %d outside [0, %d)", v, e, mp_index[e], n_mp);
        sorted.assign(mp_index + V.first, mp_index + V.first + V.count);
        std::sort(sorted.begin(), sorted.end());
        for (int i = 1; i < V.count; ++i)
            if (sorted[i - 1] == sorted[i]) return why_is(MS_ERR_INVALID, why, bytes, "map fuse: view %d lists row %d twice", v, sorted[i]);
    }
    return MS_OK;
}

inline int check_pairs(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const int32_t *n_obs, int n_mp,
                       const int32_t *mp_track, const int32_t *track_row, int n_track, const int32_t *pairs, int n_pairs, const uint8_t *outcome,
                       const int32_t *n_erased, char *why, size_t bytes) {
    int rc;
    if ((rc = check_tables("map replace pairs", kf_mp, n_kf, stride, mp_flags, mp_live, n_obs, n_mp, mp_track, track_row, n_track, why, bytes))) return rc;
    if (n_pairs < 0) return why_is(MS_ERR_INVALID, why, bytes, "map replace pairs: negative size (%d pairs)", n_pairs);
    if (!n_erased || (n_pairs > 0 && (!pairs || !outcome))) return why_is(MS_ERR_INVALID, why, bytes, "map replace pairs: missing array");
    if (n_pairs >= MS_GATE_MAX_ENTRIES) return why_is(MS_ERR_CAPACITY, why, bytes, "map replace pairs: %d pairs, cap below %d", n_pairs, MS_GATE_MAX_ENTRIES);
    for (int i = 0; i < 2 * n_pairs; ++i)
        if (pairs[i] < 0 || pairs[i] >= n_mp)
            return why_is(MS_ERR_INVALID, why, bytes, "map replace pairs: pair %d: row %d outside [0, %d)", i / 2, pairs[i], n_mp);
    return MS_OK;
}

// The `merged` rule of loop_closer.cpp:533-542 on the list alone: outcome 0 replaced | 1 equal | 2 skipped because the first or the second row
// was the FIRST row of a pair replaced earlier.  `merged` is the caller's scratch (sorted insertion keeps it a set).
inline int pair_outcomes(const int32_t *pairs, int n_pairs, uint8_t *outcome, std::vector<int32_t> &merged) {
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

}  // namespace ms_fuse

#ifdef MAP_FUSE_HOST_ONLY
// the exported validation entry points as the library defines them, for a program that carries its own copy
extern "C" int ms_map_fuse_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const int32_t *n_obs, int n_mp,
                                 const int32_t *mp_track, const int32_t *track_row, int track_base, int n_track, const int32_t *kept_entry, const int32_t *top_idx,
                                 const uint16_t *top_dist, const int32_t *mp_index, int n_entries, const ms_fuse_view *views, const int32_t *n_kept, int n_views,
                                 int max_dist, int source_slot, const int32_t *n_erased, const int32_t *counts, const int32_t *views_done, char *why, size_t why_bytes) {
    (void)track_base;
    std::vector<int32_t> sorted;
    return ms_fuse::check_fuse(kf_mp, n_kf, stride, mp_flags, mp_live, n_obs, n_mp, mp_track, track_row, n_track, kept_entry, top_idx, top_dist, mp_index, n_entries, views,
                               n_kept, n_views, max_dist, source_slot, n_erased, counts, views_done, sorted, why, why_bytes);
}
extern "C" int ms_map_replace_pairs_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const int32_t *n_obs, int n_mp,
                                          const int32_t *mp_track, const int32_t *track_row, int track_base, int n_track, const int32_t *pairs, int n_pairs,
                                          const uint8_t *outcome, const int32_t *n_erased, char *why, size_t why_bytes) {
    (void)track_base;
    return ms_fuse::check_pairs(kf_mp, n_kf, stride, mp_flags, mp_live, n_obs, n_mp, mp_track, track_row, n_track, pairs, n_pairs, outcome, n_erased, why, why_bytes);
}
#endif
