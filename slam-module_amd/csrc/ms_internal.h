// ms_internal.h -- shared internals of libmi355slam (product code; never includes oracle/).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/mi355slam.h"
#include "ms_check.h"
#include "ms_geometry.h"      // msgeo::* (geometry.cpp), ms_div_up
#include "ms_layout.h"

struct MsWorkspace {
    void *dev = nullptr, *host = nullptr;
    size_t dev_bytes = 0, host_bytes = 0;
};
enum MsWorkspaceId {
    MS_WS_LOOP_RANSAC,      // ms_loop_ransac (loop_ransac.hip): device inputs / work / results
    MS_WS_SIM3_OPT,         // ms_sim3_optimize (sim3_opt.hip): device inputs / results
    MS_WS_PROJECT_GATE,     // ms_project_gate (project_gate.hip): device tables / ranks / offsets
    MS_WS_MAP_REFRESH,      // ms_map_refresh and ms_loop_correct (map_refresh.hip): device lists / centres / packed descriptors / previous poses
    MS_WS_COVIS,            // ms_covisibility and ms_map_point_union (covis.hip): device queries / bitmaps / owner marks / block counts
    MS_WS_TRIANGULATE,      // ms_triangulate (triangulate.hip): device lists / cameras / rays / results
    MS_WS_MAP_CULL,         // ms_observation_count and ms_map_cull (map_cull.hip): device KfId order / walk / first and last positions / marks / block counts
    MS_WS_OBS_LISTS,        // ms_observation_lists (obs_lists.hip): device KfId order / descriptor bases / lengths / marks / block counts / cursors / sort keys
    MS_WS_MATCH_TRACKED,    // ms_match_tracked and ms_match_tracked_finish (match_tracked.hip): device frame record / track ids / new rows / per-keypoint rows and positions
    MS_WS_MAP_FUSE,         // ms_map_fuse and ms_map_replace_pairs (map_fuse.hip): device entry rows / views / pairs / candidates / "listed by K" marks / results
    MS_WS_CREATE_POINTS,    // ms_create_points_lists, ms_create_points_bind and ms_unbound_mask (create_points.hip): device new rows / per-keypoint positions / results / slot records
    MS_WS_BA_WINDOW,        // ms_ba_window_lists and ms_ba_window_apply (ba_window.hip): device pose index / cameras / results in; block counts / marks / the block that goes down
    MS_WS_SEARCH_BIND,      // ms_search_bind (search_bind.hip): device slice of mp_index / results / row marks
    MS_WS_LOOP_CHAIN,       // ms_loop_usable_mask, ms_loop_pairs and ms_loop_sim3_lists (loop_chain.hip): device slot / candidate records, sigmas, match lists; counts; the block that goes down
    MS_WS_FRAME_FINISH,     // ms_frame_finish (frame_finish.hip): device list positions / list; first claims / remaining entries / block counts; the block that goes down
    MS_WS_KEYFRAME_ADMIT,   // ms_keyframe_admit (keyframe_admit.hip): device track ids / depths; word / weight / node / track index / sorted nodes; the block that goes down
    MS_WS_BOW_VECTOR,       // ms_bow_vector (bow_vector.hip): the device head {n_words, n_bad} that goes down
    MS_WS_MAP_EXTRACT,      // ms_map_extract (map_extract.hip): device list / keypoint counts / pool offsets; entries per row / row maps / block counts; the head that goes down
    MS_WS_FRAME_ADMIT,      // ms_frame_admit (frame_admit.hip): device features (x / y / depth / id / keep); the keypoint index per feature; the block that goes down
    MS_WS_MAP_PUBLISH,      // ms_map_publish (map_publish.hip): device listed slots; mark bitmaps / block counts / offsets; the head with pose_wc and the packed streams that go down
    MS_WS_COUNT
};

// The vocabulary tree as ms_bow_vocab_create lays it out on the device (bow.hip): breadth-first, every node's children adjacent.  The walk is
// bow_descend.h's; bow.hip and keyframe_admit.hip run it.
struct BowTree {
    const int32_t *first_child;    // [n] internal index of the first child (children are contiguous)
    const int32_t *n_children;     // [n]
    const uint4 *desc;             // [n][2]
    const int32_t *orig_id;        // [n] node id of the caller's numbering
    const int32_t *word;           // [n] word id (-1 for inner nodes)
    const double *weight;          // [n]
    int depth_levels, max_depth;
};
struct ms_bow_vocab {
    ms_ctx *ctx = nullptr;
    void *slab = nullptr;
    BowTree tree{};
    int n_nodes = 0, max_children = 0;
};

struct ms_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t slots[1024] = {nullptr};     // ms_event_mark: created on first use
    int n_cu = 0;
    void *scratch = nullptr;      // growable device scratch for small per-call argument tables
    size_t scratch_bytes = 0;
    int hamming_path = 0;         // 0 = automatic (matrix-core kernel for unmasked searches), 1 = popcount kernel for everything (ms_hamming_set_path)
    bool greedy_attr_done[2] = {false, false};   // dynamic-LDS attribute of k_greedy_big_nodes<false/true> set on this context's device
    int greedy_path = 0;          // 0 = node-parallel greedy matchers (sequential redo of pairs that need it), 1 = one wave per pair, sequential (ms_match_set_path)
    // device blocks of destroyed bundle-adjustment handles, kept for the next ms_ba_create on this context: a window per keyframe then allocates nothing after
    // warm-up (hipFree synchronises the whole device -- with one sequence per context that stalled every other sequence's stream once per keyframe)
    struct BaBlock { void *p = nullptr; size_t bytes = 0; } ba_cache[4];
    // asynchronous downloads (ms_dev_download_async): a stream of their own, ordered after the work enqueued before them; work that overwrites what
    // they read is ordered after them on the device (ms_ctx_order_after_downloads, called by ms_orb_extract)
    hipStream_t d2h_stream = nullptr;
    hipEvent_t ev_d2h_gate = nullptr, ev_d2h_done = nullptr;
    bool d2h_pending = false;
    void *pinned = nullptr;       // page-locked host staging of small result blocks (ms_pinned), grow-only
    size_t pinned_bytes = 0;
    // page-locked staging of ms_ba_create's small uploads (the inputs of all its problems and their descriptors, copied asynchronously: the solver launch follows
    // in stream order, nobody waits); ba_stage_ev = the end of the last upload from it, waited for before the block is written again
    void *ba_stage = nullptr;
    size_t ba_stage_bytes = 0;
    hipEvent_t ba_stage_ev = nullptr;
    bool ba_stage_busy = false;
    void *ba_handle_pool[4] = {nullptr, nullptr, nullptr, nullptr};      // destroyed bundle-adjustment handle OBJECTS (their vectors keep their capacity, their event stays): ms_ba_create takes one back
    // grow-only workspaces of the map-side entry points: a device block and its page-locked staging each (ms_grow; laid out with ms_layout.h)
    MsWorkspace ws[MS_WS_COUNT];
    // the descent of the latest successful ms_keyframe_admit where it lies in that call's workspace (ms_keyframe_admit_words); admit_n = -1: none
    const int32_t *admit_word = nullptr;
    const double *admit_weight = nullptr;
    int32_t admit_n = -1;
    char err[512] = {0};
};

void ms_ba_release_pool(ms_ctx *ctx);      // ba.hip: deletes the pooled handle objects (ms_ctx_destroy)

// ba.hip, for pose_tables.hip: a pose-only handle of capacity cap_obs -- two poses (0 free, 1 fixed), up to cap_obs fixed points with
// one observation each from pose 0, one SE3 edge -- whose inputs are WRITTEN BY A KERNEL: the device block ms_ba_create lays out for that shape, with
// no host array staged.  MsBaPoseIo names what the gather writes and what the apply reads, all DEVICE pointers into the handle's block.
struct MsBaPoseIo {
    double *pose0, *point0, *obs_uv, *obs_info, *edge_meas, *edge_info;    // [2 * 7], [cap * 3], [cap * 2], [cap], [7], [36]
    int32_t *obs_pose, *obs_point, *edge_i, *edge_j;                       // [cap], [cap], [1], [1]
    int32_t *n_point, *n_obs, *max_iters;                                  // fields of the descriptor k_ba_pose_only reads
    double *huber;
    const double *pose, *chi2_obs, *stats;                                 // the solver's state [2 * 7], chi2 per observation [cap], status record [16]
};
int ms_ba_pose_tables_create(ms_ctx *ctx, int cap_obs, ms_ba **out, MsBaPoseIo *io);
int ms_ba_pose_tables_launch(ms_ba *ba);   // k_ba_pose_only on the handle's problem as the device holds it: one launch, nothing else
int ms_ba_pose_tables_wait(ms_ba *ba);     // records the handle's event behind everything enqueued so far and waits for it politely (ba_wait_event)

// bow_vector.hip, for bowdb.hip: enqueues k_bow_vector on the context stream, nothing else.  word / weight [n] and head [2] =
// {n_words, n_bad} are DEVICE arrays, 0 <= n <= MS_COVIS_MAX_STRIDE.  With seg the vector goes into seg in the word pool's layout (ceil(len / 2)
// cells of words, then len cells of values; seg holds the cells of n words) and words / values are not used.
int ms_bow_vector_enqueue(ms_ctx *ctx, const int32_t *word, const double *weight, int n, int vocab_words, int cap, int32_t *words, double *values,
                          unsigned long long *seg, int32_t *head);

// page-locked host staging of at least `bytes` in ctx->pinned (contents are valid until the next call that uses it)
int ms_pinned(ms_ctx *ctx, size_t bytes);

// makes the context stream wait (on the device) for the asynchronous downloads issued so far
int ms_ctx_order_after_downloads(ms_ctx *ctx);

// device scratch of at least `bytes`, reused across calls on the context stream
int ms_scratch(ms_ctx *ctx, size_t bytes, void **out);

// grow-only block of a workspace: at least `bytes` in p (device memory, or page-locked host memory with `pinned`), capacity in cap.  Growing waits
// for the context stream, frees the block and allocates half as much again as asked for; the contents are not kept.
int ms_grow(ms_ctx *ctx, void *&p, size_t &cap, size_t bytes, bool pinned);

inline int ms_fail(ms_ctx *ctx, int code, const char *fmt, ...) {
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define MS_HIP(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e__ = (call);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return ms_fail((ctx), MS_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                           __FILE__, __LINE__);                                                    \
    } while (0)

#define MS_KERNEL_CHECK(ctx, name)                                                                 \
    do {                                                                                           \
        hipError_t e__ = hipGetLastError();                                                        \
        if (e__ != hipSuccess)                                                                     \
            return ms_fail((ctx), MS_ERR_HIP, "launch of %s failed: %s", name, hipGetErrorString(e__)); \
    } while (0)

// Stage ranges for a profiler's marker trace (ms_set_trace_ranges): roctxRangePushA / roctxRangePop, resolved at run time from
// librocprofiler-sdk-roctx / libroctx64 -- no link dependency, nothing happens (one relaxed load) while they are off.
void ms_range_push(const char *name);
void ms_range_pop();
struct MsRange {
    explicit MsRange(const char *name) { ms_range_push(name); }
    ~MsRange() { end(); }
    void end() { if (open_) { ms_range_pop(); open_ = false; } }      // close before the scope does (an early return still closes it)
    bool open_ = true;
    MsRange(const MsRange &) = delete;
    MsRange &operator=(const MsRange &) = delete;
};
