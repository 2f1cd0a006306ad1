// ms_check.h -- what the host validation of the map entry points shares (map_checks.cpp holds the ms_*_check functions themselves).  Plain
// C++17, no HIP and no context: everything here reads HOST arguments only, so a program can compile map_checks.cpp alone and run it under
// sanitizers (tests/map_checks_corpus.cpp).  ms_internal.h includes this header.
#pragma once
#include <atomic>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/mi355slam.h"

// every allocation the library makes on the host or the device after a context exists (handle objects, host scratch growth, device blocks, pinned staging, events):
// a per-keyframe path must leave it unchanged after warm-up (ms_debug_host_allocs).  Defined in map_checks.cpp, whose scratch vectors count into it.
extern std::atomic<long long> g_ms_host_allocs;

// ms_fail for the *_check entry points, which report into the caller's buffer (may be null)
inline int ms_why(int code, char *why, size_t bytes, const char *fmt, ...) {
    if (why && bytes) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(why, bytes, fmt, ap);
        va_end(ap);
    }
    return code;
}

// the sizes every entry point over the keyframe table kf_mp accepts; n = its queries, problems or candidates
inline bool ms_map_over_capacity(int n_kf, int stride, int n_mp, int n) {
    return n_kf > MS_COVIS_MAX_KF || stride > MS_COVIS_MAX_STRIDE || n_mp >= MS_COVIS_MAX_MP || n > MS_COVIS_MAX_QUERIES;
}

// the two lines every family words alike (`who` = the family's prefix): a stride below 1, and a table beyond the three caps above
inline int ms_why_stride(const char *who, int stride, char *why, size_t bytes) { return ms_why(MS_ERR_INVALID, why, bytes, "%s: stride %d", who, stride); }
inline int ms_why_table_caps(const char *who, int n_kf, int stride, int n_mp, char *why, size_t bytes) {
    return ms_why(MS_ERR_CAPACITY, why, bytes, "%s: %d slots / stride %d / %d map points, caps %d / %d / below %d", who, n_kf, stride, n_mp, MS_COVIS_MAX_KF,
                  MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP);
}

// true when idx[0 .. n) are distinct values of [0, limit).  Otherwise *bad = the first entry outside the range, or -1 - v for a value v that is
// listed twice (entries are ranged before duplicates are looked for).  The sorted copy lives in a per-thread vector that only grows.
bool ms_distinct_in_range(const int32_t *idx, int n, int limit, int *bad);

// ---- what an entry point reuses of what its check computed (hidden: the library exports nothing new for them)
#define MS_HIDDEN __attribute__((visibility("hidden")))
// What ms_observation_count, ms_map_cull_check and ms_observation_lists_check ask of the keyframe table and of kf_id: signs, the stride, the two
// arrays, no kf_id >= 0 listed twice.  It leaves the slot order behind (below).
MS_HIDDEN int ms_kf_table_check(const char *who, const int32_t *kf_mp, int n_kf, int stride, int n_mp, const int32_t *kf_id, char *why, size_t bytes);
// the slots with kf_id >= 0 by ascending kf_id, as the last of those three left them on this thread (a per-thread vector that only grows)
MS_HIDDEN const std::vector<int32_t> &ms_slots_by_id();
// slot_rank / rank_slot of an upload block from the slots in KfId order
inline void ms_fill_ranks(const std::vector<int32_t> &order, int n_kf, int32_t *slot_rank, int32_t *rank_slot) {
    for (int k = 0; k < n_kf; ++k) slot_rank[k] = -1;
    for (size_t i = 0; i < order.size(); ++i) { slot_rank[order[i]] = (int32_t)i; rank_slot[i] = order[i]; }
}
// The `merged` rule of loop_closer.cpp:533-542 on the list of ms_map_replace_pairs alone: outcome 0 replaced | 1 equal | 2 skipped because the
// first or the second row was the FIRST row of a pair replaced earlier.  Returns the number of pairs that run.
MS_HIDDEN int ms_pair_outcomes(const int32_t *pairs, int n_pairs, uint8_t *outcome);
