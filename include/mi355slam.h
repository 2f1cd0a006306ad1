/*
 * mi355slam.h -- C ABI of libmi355slam.so: the MI355X (gfx950) implementation of the
 * AaltoML/SLAM-module hot path (image pyramid + ORB extraction, Hamming matching, local BA).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Each entry point
 * names the reference interface it replaces (file:line relative to the reference tree).
 * Host-side C++ shims with the reference's own signatures live in slam-module_amd/host/.
 *
 * Conventions
 *   - every function returns MS_OK (0) or a negative ms_status; ms_last_error() gives the text.
 *     Nothing throws across the ABI (the reference itself has no exceptions / error codes:
 *     assert + bool/empty returns, e.g. bundle_adjuster.cpp:239,411).
 *   - a ms_ctx owns one HIP stream on one device; objects created from it are single-threaded
 *     (the reference calls this path from one backend thread, mapper.cpp:229-279).  Distinct
 *     contexts may be used concurrently from different threads.
 *   - "device pointer" arguments must be memory of the context's device; "host pointer"
 *     arguments are ordinary memory (pinned memory makes the copies asynchronous).
 *   - there is NO CPU fallback: without a usable gfx950 device ms_ctx_create() fails.
 */
#ifndef MI355SLAM_H
#define MI355SLAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MS_MAX_LEVELS 16
#define MS_ORB_PATCH_RADIUS 19       /* static_settings.hpp:14 */
#define MS_HAMMING_THR_LOW 50        /* keyframe_matcher.hpp:10 */
#define MS_HAMMING_THR_HIGH 100      /* keyframe_matcher.hpp:11 */
#define MS_HAMMING_MAX 256           /* keyframe_matcher.hpp:12 */

typedef enum {
    MS_OK = 0,
    MS_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
    MS_ERR_NO_DEVICE = -2,    /* no gfx950 device, or HIP runtime failure at init */
    MS_ERR_HIP = -3,          /* a HIP call failed; see ms_last_error */
    MS_ERR_CAPACITY = -4,     /* a fixed capacity given at create time was exceeded */
    MS_ERR_NUMERIC = -5,      /* BA: non-finite state */
    MS_ERR_TOO_LATE = -6      /* ms_prepare_process: the GPU runtime of this process is already up; the call can no longer have an effect */
} ms_status;

typedef struct ms_ctx ms_ctx;
typedef struct ms_orb ms_orb;

/* ---------------------------------------------------------------------------------------------
 * Context
 * ------------------------------------------------------------------------------------------- */
/* Optional, once per process, BEFORE the first HIP call of the process (ms_ctx_create included): tells the runtime how many contexts (= sequences, each
 * with its own stream) will drive the same GPU at the same time.  The HIP runtime maps streams onto a handful of hardware queues (4 by default), and kernels
 * of streams that share a queue run one after the other -- a 1.8 ms local-BA launch of one sequence then holds up the 10 us front-end kernels of another:
 * eight sequences on one GPU measured 4 300 frames/s with 4 queues, 5 600 with 8 and 8 400 - 8 700 with 12 ... 32 (the process holds more streams than its sequences' -- a context's
 * download stream, the application's own --, and with exactly one queue per context two sequences share one; tools/hw_queue_sweep.sh).  Sets GPU_MAX_HW_QUEUES to max(4, min(2 * concurrent_contexts, 32)) unless the variable is already set (the caller's own setting wins: MS_OK, nothing changed).  Once the runtime is
 * initialised -- by this library or by anybody else in the process: the kernel driver's device node is open -- the variable has been read and the call returns
 * MS_ERR_TOO_LATE without touching the environment, so a host that calls it late learns that it runs on the default number of queues.  (The reference has no
 * counterpart: its back end is one CPU thread per sequence, mapper.cpp:268-269.) */
int ms_prepare_process(int concurrent_contexts);
int ms_ctx_create(int device, ms_ctx **out);
void ms_ctx_destroy(ms_ctx *ctx);
int ms_ctx_sync(ms_ctx *ctx);                 /* hipStreamSynchronize on the context stream */
void *ms_ctx_stream(ms_ctx *ctx);             /* the hipStream_t, for event timing by the caller */
const char *ms_last_error(const ms_ctx *ctx); /* never NULL; valid until the next call on ctx */

/* Stage ranges in a profiler's marker trace (rocprofv3 --marker-trace): with on = 1 the entry points below bracket their work with roctx ranges named
 * like the reference's own timers where it has them (mapper_helpers.cpp:1044 "poseBundleAdjust", :1080 "localBundleAdjust", :1193 "Bow index
 * transform") and by stage elsewhere ("pyramid", "detect", "describe" inside ms_orb_extract; "match"; "ms_ba_create", "ms_ba_solve",
 * "ms_ba_download" -- the host mirrors wrap those in "localBundleAdjust" / "poseBundleAdjust" / "globalBundleAdjust").  The ranges mark where
 * the work is ENQUEUED on the calling thread.  Process-wide, off by default (also switched on by MS_TRACE_RANGES=1 in the environment); the roctx
 * library is looked up at run time, MS_ERR_INVALID if there is none.  ms_trace_range_push / pop let a caller (the host mirrors do) add its own. */
int ms_set_trace_ranges(int on);
void ms_trace_range_push(const char *name);
void ms_trace_range_pop(void);
const char *ms_version(void);
/* HIP-event timing on the context stream (bench.py measures the hot path with these). */
int ms_timer_start(ms_ctx *ctx);
int ms_timer_stop_ms(ms_ctx *ctx, float *ms); /* records, synchronises, returns elapsed ms */
/* 1024 general event slots (created on first use): mark = hipEventRecord on the context stream; elapsed synchronises on slot b. */
int ms_event_mark(ms_ctx *ctx, int slot);
int ms_event_elapsed_ms(ms_ctx *ctx, int slot_a, int slot_b, float *ms);
/* plain device memory helpers so a C caller needs no HIP headers */
int ms_dev_alloc(ms_ctx *ctx, size_t bytes, void **out);
int ms_dev_free(ms_ctx *ctx, void *p);
/* Page-locked host memory for frames going in and results coming out: copies from / to it are truly asynchronous (the copy engines read it
 * directly), which is what lets ms_orb_extract overlap a batch's copies with its kernels and ms_dev_download_async run under the next batch. */
int ms_host_alloc(ms_ctx *ctx, size_t bytes, void **out);
int ms_host_free(ms_ctx *ctx, void *p);
int ms_dev_upload(ms_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int ms_dev_download(ms_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* The same copy without waiting for it: it runs on a stream of its own, after everything enqueued on the context stream so far, while the context
 * stream goes on (the next batch's kernels and copies run under it).  `dst` should be pinned host memory (pageable memory is staged by the runtime and
 * the call then waits).  What the copy READS must stay intact until it is done: ms_orb_extract orders itself after the downloads issued so far (it
 * is the call that overwrites the extractor's outputs, and everything enqueued after it is ordered behind it); other writers of the source are the
 * caller's business.  ms_dev_download_wait blocks the host until every asynchronous download has arrived (ms_ctx_sync does, too). */
int ms_dev_download_async(ms_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int ms_dev_download_wait(ms_ctx *ctx);

/* ---------------------------------------------------------------------------------------------
 * S1/S2: pyramid geometry -- replaces StaticSettings (static_settings.cpp:9-60) and the level
 * sizing of image_pyramid.cpp:76-78.  Host-only arithmetic, exposed so callers size buffers.
 * ------------------------------------------------------------------------------------------- */
int ms_scale_factors(int levels, float scale_factor, float *out);
int ms_level_sigma_sq(int levels, float scale_factor, float *out);
int ms_level_quotas(int levels, float scale_factor, int max_kpts, int32_t *out);
int ms_level_sizes(int levels, float scale_factor, int width, int height, int32_t *w, int32_t *h);

/* ---------------------------------------------------------------------------------------------
 * ORB extractor -- replaces OrbExtractor::build / detectAndExtract (orb_extractor.hpp:11-30,
 * orb_extractor.cpp:73-164), ImagePyramid (image_pyramid.hpp:16-30, image_pyramid.cpp:68-86) and
 * FeatureDetector (feature_detector.hpp:15-24, feature_detector.cpp:68-134).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t width, height;     /* frame size (fixed per extractor, like the lazily-built pyramid) */
    int32_t levels;            /* parameters.slam.orbScaleLevels */
    float scale_factor;        /* parameters.slam.orbScaleFactor */
    int32_t max_kpts;          /* parameters.slam.maxKeypoints */
    int32_t lk_track_level;    /* parameters.slam.orbLkTrackLevel */
    int32_t fast_threshold;    /* this build's detector: FAST-9/16 threshold (score > threshold) */
    int32_t max_tracks;        /* capacity for tracker features per frame */
    int32_t max_batch;         /* frames per ms_orb_extract call (>= 1) */
    float min_distance;        /* parameters.tracker.gfttMinDistance (feature_detector.cpp:79-82): keypoints of a level keep
                                  floor(min_distance * min(w,h)/720 * 0.8 + 0.5) pixels apart; 0 = no suppression */
} ms_orb_config;

/* Per-frame outputs, structure-of-arrays, `capacity` = max_tracks + max(max_kpts, sum of the per-level quotas) slots per frame
 * (ms_orb_capacity; the quotas are rounded level by level, static_settings.cpp:52, and may add up to a few more than max_kpts).
 * Frame f's keypoint i is element f*capacity + i of each array (desc: 8 words per slot).
 * Order inside a frame: tracker features first, then detected points level-major
 * (orb_extractor.cpp:136-162); each level ordered by (FAST score desc, y*w+x asc). */
typedef struct {
    int32_t capacity;
    int32_t *count;      /* [batch] */
    float *x, *y;        /* level-0 pixel coordinates (KeyPoint::pt, key_point.hpp:14) */
    float *angle;        /* degrees [0,360) (KeyPoint::angle) */
    int32_t *octave;     /* KeyPoint::octave */
    uint32_t *desc;      /* KeyPoint::descriptor, std::array<uint32_t,8> (key_point.hpp:19-20) */
    int32_t *track_id;   /* keyPointTrackIds: tracker id or -1 (orb_extractor.cpp:122,161) */
} ms_keypoints;

int ms_orb_create(ms_ctx *ctx, const ms_orb_config *cfg, ms_orb **out);
void ms_orb_destroy(ms_orb *orb);

/* Optional camera validity mask (stand-in for tracker::Camera::isValidPixel, orb_extractor.cpp:101,
 * :231): width*height bytes in host memory, 0 = invalid.  NULL clears it (all pixels valid).  The mask is sampled at the
 * rounded level-0 position of a keypoint; the reference evaluates the camera model at the sub-pixel position, so the two can
 * differ at the rim of the valid region.  host/mi355slam/orb_extractor.hpp's predicate overload of detectAndExtract applies the
 * model itself to the output coordinates and reproduces the reference exactly. */
int ms_orb_set_valid_mask(ms_orb *orb, const uint8_t *mask_host);

/* detectAndExtract for a batch of frames.
 *   images        : frame f starts at images + f*frame_stride, rows `row_stride` bytes apart.
 *   images_on_device != 0: `images` is device memory and is used IN PLACE as pyramid level 0
 *                   (needs a 16-byte aligned base and row_stride % 16 == 0, else it is copied on
 *                   the device); it must stay valid until the call's work has completed.
 *   track_xy      : optional [n_frames][max_tracks][2] level-0 coords (host), track_id [n_frames][max_tracks],
 *                   n_tracks [n_frames].  NULL = no tracker features.
 * Asynchronous on the context stream; results are read with ms_orb_download / ms_orb_device_view
 * after ms_ctx_sync (ms_orb_download synchronises itself).
 * Which launches a call issues depends on where its frames live: frames in device memory, and host batches of fewer than 32 frames, are one
 * piece, and a piece large enough runs level 0's corner detection beside the resize chain (ms_orb_set_fast_overlap).  A HOST batch of 32 frames
 * or more, pinned or pageable, on an extractor with max_batch >= 32 and profiling off comes in as four pieces on the extractor's copy stream, each
 * piece's kernels under the next piece's copy; those pieces never split automatically.  The results are the same bit for bit either way. */
int ms_orb_extract(ms_orb *orb, const uint8_t *images, int images_on_device, int n_frames,
                   size_t frame_stride, size_t row_stride,
                   const float *track_xy, const int32_t *track_id, const int32_t *n_tracks);

/* Device-resident results of the last ms_orb_extract (pointers are device memory owned by orb). */
int ms_orb_device_view(ms_orb *orb, ms_keypoints *view);
/* Copy frame `frame`'s keypoints to caller-owned host arrays (each sized >= capacity); returns count in *n. */
int ms_orb_download(ms_orb *orb, int frame, float *x, float *y, float *angle, int32_t *octave,
                    uint32_t *desc, int32_t *track_id, int32_t *n);
int ms_orb_capacity(const ms_orb *orb);

/* N4, serialization half: KeyPoint::serialize (key_point.hpp:22-25) writes `ar(pt.x, pt.y, angle, octave, octave, bearing, descriptor)`
 * for every element of KeyframeShared::keyPoints (keyframe.hpp:80-93).  ms_keypoints_pack lays the first n keypoints of frame `frame`
 * of a device SoA view (ms_orb_device_view, or any ms_keypoints of device arrays) out in exactly that field order, 76 bytes per keypoint with no
 * padding -- x, y, angle as f32; octave as i32 TWICE (the reference's own quirk); bearing as 3 x f64 (`bearing`: device array [n*3] =
 * KeyPoint::bearing, which the caller computes, keyframe.cpp:55-68; NULL writes zeros); descriptor as 8 x u32 -- on the device, and
 * copies the records to `records_host` with one transfer (synchronises).  ms_keypoints_unpack is the inverse on the host (any output may
 * be NULL; MS_ERR_INVALID if the two octave copies of a record differ).  What is NOT known here: the archive framing around the records
 * (cereal's size tag of the vector and the Eigen::Vector3d serializer live in the parent project's util/serialization.hpp, not in the
 * reference tree); the record body above is what a binary archive writes for arithmetic fields and std::array<uint32_t, 8>. */
#define MS_KEYPOINT_RECORD_BYTES 76
int ms_keypoints_pack(ms_ctx *ctx, const ms_keypoints *view, int frame, int n, const double *bearing, uint8_t *records_host);
int ms_keypoints_unpack(const uint8_t *records, int n, float *x, float *y, float *angle, int32_t *octave, double *bearing, uint32_t *desc);

/* How many keypoints a wave of the describe kernel walks one after another (a test hook; outputs are bit for bit the same for every value).
 * 0 = the automatic launch plan (the default: long strips first, a tail of one-keypoint blocks; a small launch is one keypoint per wave);
 * 1 .. 8 = every workgroup uses r, no taper.  MS_ERR_INVALID for anything else.  Holds for the calls that follow. */
int ms_orb_set_describe_strip(ms_orb *orb, int r);

/* Which resize kernel builds the pyramid, and which workgroup takes which tile (a test hook; outputs are bit for bit the same for every value).
 * px: 0 = automatic (8 destination pixels per lane on every level whose tables allow it, for launches that fill the device; a frame or a
 * few run the 4-pixel kernel), 4 = the 4-pixel kernel everywhere, 8 = the 8-pixel kernel on every eligible level whatever the launch's size
 * (levels that are not eligible run the 4-pixel kernel).  map, for the 8-pixel kernel: 0 = automatic (by frame for batches of
 * 32 frames and more), 1 = tiles dealt across the whole device, 2 = by frame (all tiles of a frame on one XCD).
 * MS_ERR_INVALID for anything else.  Holds for the calls that follow. */
int ms_orb_set_resize_plan(ms_orb *orb, int px, int map);

/* Which workgroup of the describe kernel describes which keypoint, and when (a test hook; outputs are bit for bit the same for every value).
 * Bit 0: the workgroups dealt to one XCD take a contiguous run of the launch plan's blocks (whole frames through one L2).
 * Bit 1: a level's detections are visited in a spatial order (row bands, x inside a band) instead of score order; each still lands in its slot.
 * The default is 1 (the visit order costs the slot kernel what it saves the describe kernel).  MS_ERR_INVALID for anything outside 0 .. 3.  Holds for the calls that follow. */
int ms_orb_set_describe_order(ms_orb *orb, int mode);

/* Whether corner detection on pyramid level 0 (the caller's image, which needs no resized level) runs beside the resize chain, on a side stream of
 * the extractor (its copy stream where it has one) that forks from the context stream at the start of the call's kernels and joins it in front of
 * the selection (a test hook; outputs are bit for bit the same for every value).  0 = automatic: only in calls where each of the two detector
 * launches, level 0 and the other levels, has more workgroups than the detector's pruning rule asks for (17 frames and more at 1280 x 720 x 8
 * levels), and not in the pieces of a batch of host frames, whose kernels already run beside the next piece's copy; 1 = never: one launch on the
 * context stream; 2 = always, where the pyramid has more than one level (the side stream is created on this request if the extractor has none); a
 * one-level pyramid keeps its single launch.  MS_ERR_INVALID for anything else.  Holds for the calls that follow. */
int ms_orb_set_fast_overlap(ms_orb *orb, int mode);
/* How the last ms_orb_extract launched the corner detector: *launches = its launches (1 = one launch over all levels, 2 = level 0 beside the
 * resize chain and the other levels behind it; a host batch that came in as pieces counts every piece's), *pruning = how many of them were the
 * instantiation that raises its threshold from what the launch has found (launches of more than 2048 workgroups).  Host bookkeeping, no wait. */
int ms_orb_last_fast_launches(const ms_orb *orb, int32_t *launches, int32_t *pruning);

/* Per-kernel timing of ms_orb_extract with HIP events on the context stream (off by default).
 * Stage order: 0 resize (all levels), 1 blur, 2 fast, 3 select, 4 tracks, 5 describe.
 * ms_orb_stage_ms synchronises and returns the durations of the LAST ms_orb_extract call.
 * The events are all on the context stream, so the six times add up to the call's span.  In a call that runs level 0's detection beside the
 * resize chain (ms_orb_set_fast_overlap), `resize` therefore contains level 0's detection and `fast` is the other levels plus the wait for the
 * side stream; the time of each kernel alone is what a kernel trace shows. */
#define MS_ORB_STAGES 6
int ms_orb_set_profiling(ms_orb *orb, int enable);
int ms_orb_stage_ms(ms_orb *orb, float *ms /* [MS_ORB_STAGES] */);
/* The same for an earlier profiled call: calls_back = 0 is the last one, up to 127 back (each profiled call records into the next set of a ring), so a
 * run of calls can be enqueued without a host wait in between and read afterwards. */
int ms_orb_stage_ms_back(ms_orb *orb, int calls_back, float *ms /* [MS_ORB_STAGES] */);
/* ImagePyramid::getLevel / getBlurredLevel (image_pyramid.hpp:24-25): copy one level of one frame
 * of the last batch to host, tightly packed w*h bytes (debug / parity testing).
 * LIFETIME of device inputs: frames handed to ms_orb_extract in device memory (16-byte aligned base and strides) are used IN PLACE as
 * level 0 -- they are not copied.  Level 0, and every BLURRED level (the blurred pyramid is produced on demand, by k_blur over the levels
 * of the last batch), therefore read the caller's buffer at the time of THIS call: it must still hold the frames of the last
 * ms_orb_extract, unchanged and not freed, until the next ms_orb_extract or until the caller stops asking for level 0 / blurred levels.
 * Host inputs and unaligned device inputs are copied into the extractor's own memory and carry no such requirement. */
int ms_orb_level_size(const ms_orb *orb, int level, int32_t *w, int32_t *h);
int ms_orb_download_level(ms_orb *orb, int frame, int level, int blurred, uint8_t *dst_host);
/* FeatureDetector::detect (feature_detector.cpp:20-28): per-level detector output of the last batch
 * BEFORE orientation: integer level coordinates + FAST score, `*n` points (<= quota of the level). */
int ms_orb_download_detections(ms_orb *orb, int frame, int level, int32_t *x, int32_t *y, int32_t *score, int32_t *n);
/* How many candidates (3x3 non-maximum-suppressed corners) the detector appended per (frame, level) in the last ms_orb_extract, BEFORE the selection.
 * Within a batch the detector raises a tile's threshold to the score that the level's quota already excludes, so these counts are at most the number
 * of NMS maxima above fast_threshold and vary from run to run; the selected keypoints do not.  A one-frame call finds all of them. */
int ms_orb_last_candidate_counts(ms_orb *orb, int32_t *out /* [n_frames * levels] */);

/* ---------------------------------------------------------------------------------------------
 * Descriptor matching -- the scoring core of keyframe_matcher.cpp (compute_descriptor_distance_32,
 * openvslam/match_base.h:18-39) as device primitives.
 * ------------------------------------------------------------------------------------------- */
/* Per-context choice of the kernel behind the UNMASKED searches: 0 = automatic (the i8 matrix-core kernel), 1 = the popcount
 * kernel (v_xor / v_bcnt, wave reductions) that the masked searches always use.  Both give identical results; the switch exists to
 * cross-check one against the other and to time them side by side (bench.py reports both). */
int ms_hamming_set_path(ms_ctx *ctx, int path);

/* Brute-force best / second-best of every query against every target, for `n_pairs` independent
 * (query set, target set) pairs laid out back to back: pair p uses q + p*nq*8 and t + p*nt*8.
 * Update rule of keyframe_matcher.cpp:106-112 (strict '<': lowest index wins ties).
 * Optional masks (device pointers or NULL): q_bucket/t_bucket [n_pairs*nq]/[n_pairs*nt] -- only equal
 * bucket ids are compared (DBoW2 node gate, keyframe_matcher.cpp:74); t_valid [n_pairs*nt] -- 0 skips the
 * target (map-point gates, keyframe_matcher.cpp:94-100).
 * Outputs (device): best_idx (-1 if none), best_dist, second_dist (256 if none). All device pointers. */
int ms_hamming_best2(ms_ctx *ctx, const uint32_t *q, int nq, const uint32_t *t, int nt, int n_pairs,
                     const int32_t *q_bucket, const int32_t *t_bucket, const uint8_t *t_valid,
                     int32_t *best_idx, uint16_t *best_dist, uint16_t *second_dist);

/* Same search over SETS of descriptors kept in two pools (e.g. the per-frame outputs of ms_orb_extract,
 * ms_keypoints.desc with stride = capacity and count = ms_keypoints.count): set s of a pool starts at
 * pool + s*stride*8 words and holds count[s] rows (count == NULL: stride rows).  Pair p compares set
 * pair_q[p] of the query pool with set pair_t[p] of the target pool (NULL: set p).  Outputs are
 * [n_pairs * q_stride]; rows beyond a set's count get (-1, 256, 256).  All pointers are device memory. */
int ms_hamming_best2_sets(ms_ctx *ctx, const uint32_t *q_pool, int q_stride, const int32_t *q_count,
                          const uint32_t *t_pool, int t_stride, const int32_t *t_count,
                          const int32_t *pair_q, const int32_t *pair_t, int n_pairs,
                          int32_t *best_idx, uint16_t *best_dist, uint16_t *second_dist);

/* Accept rule of matchForLoopClosures without the greedy state (keyframe_matcher.cpp:115-122):
 * match[i] = best_idx if best <= max_dist and NOT (ratio * second < (float)best), else -1.  Device pointers.
 * Arithmetic of the product: float32 (`lowe_ratio` is a float here, the product is one rounded float32 multiply).  The reference writes
 * `parameters.loopClosureFeatureMatchLoweRatio * second_best_hamm_dist < static_cast<float>(best_hamm_dist)` (:120); the parameter's type lives in
 * the parent project (not in the tree).  If it is a double there, the reference's product is exact in double and the two can differ for a ratio
 * that float32 cannot represent, exactly at the boundary ratio * second == best (0.75, 0.5, 0.8125 ... are exact either way; 0.8 or 0.7 are not).
 * The same holds for ms_match_loop_closure's lowe_ratio. */
int ms_ratio_test(ms_ctx *ctx, const int32_t *best_idx, const uint16_t *best_dist, const uint16_t *second_dist,
                  int n, float lowe_ratio, int max_dist, int32_t *match);

/* Scoring core of the projection-guided matchers searchByProjection / replaceDuplication / findMatchesTranformedMps
 * (keyframe_matcher.cpp:349-378, :479-494, :600-623): query i (a map point's descriptor) against ITS OWN candidate list
 * cand_idx[cand_start[i] .. cand_start[i+1]) (keypoint indices from the radius query, Keyframe::getFeaturesAround).
 * t_skip marks targets to ignore (already bound features, :358-360); t_octave gives KeyPoint::octave so the caller can apply
 * the same-level ratio rule (:382-386).  Outputs follow the reference's sequential scan exactly: best = first minimum,
 * second = next smallest; *_octave are -1 when absent.  All pointers are device memory. */
int ms_hamming_candidates(ms_ctx *ctx, const uint32_t *q_desc, int nq, const uint32_t *t_desc,
                          const int32_t *cand_start, const int32_t *cand_idx, const uint8_t *t_skip, const int32_t *t_octave,
                          int32_t *best_idx, uint16_t *best_dist, uint16_t *second_dist, int32_t *best_octave, int32_t *second_octave,
                          int32_t *second_idx /* may be NULL */);

/* Representative descriptor of many map points at once (MapPoint::updateDescriptor, map_point.cpp:75-116): for map point p
 * with observations obs_idx[obs_start[p] .. obs_start[p+1]) (indices into desc_pool, 8 words each), the observation whose
 * median Hamming distance to all of the point's observations is smallest (median = sorted[(n-1)/2], self distance 0
 * included; lowest index wins ties; only a median < 256 replaces index 0).  best_local[p] = position in the point's list,
 * best_pool[p] = the pool index (either may be NULL); both -1 for a point without observations (the reference returns
 * early, :86).  max_obs >= the longest list, at most MS_MEDOID_MAX_OBS (a longer list yields -2
 * for that point).  All pointers are device memory. */
#define MS_MEDOID_MAX_OBS 256
int ms_descriptor_medoid(ms_ctx *ctx, const uint32_t *desc_pool, const int32_t *obs_start, const int32_t *obs_idx, int n_points,
                         int max_obs, int32_t *best_local, int32_t *best_pool);

/* ---- N3: vocabulary-tree descent behind BowIndex::transform (bow_index.cpp:59-93) -------------------------------------
 * The reference hands every keypoint descriptor to DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>::transform(features,
 * bowVector, featureVector, levelsup = 4) (bow_index.cpp:86-92; DBoW2 is an external library, not in the reference tree).
 * ms_bow_vocab_create takes the loaded vocabulary the way DBoW2 stores it -- HOST arrays: parent[i] = parent node id
 * (node 0 = root, parent[0] ignored, every parent id smaller than its children's ids, as DBoW2's loaders and k-means builder
 * produce), node_desc[i] = the node's 256-bit descriptor, node_weight[i] = its weight, node_word[i] = its word id for a leaf
 * (-1 for inner nodes), depth_levels = the vocabulary's L -- and keeps a device copy laid out for the descent.
 * ms_bow_transform walks n descriptors (DEVICE memory, 8 words each, 16-byte aligned) down the tree: at every level the child
 * with the smallest Hamming distance, the first child (lowest node id) on ties; word[i] / weight[i] are the reached leaf's,
 * node[i] is the node passed at level depth_levels - levels_up (0 = root when that level is <= 0; the leaf's own id when the
 * leaf lies above that level, where DBoW2 leaves the value unset).  word = -1, weight = 0 for a vocabulary without words.
 * weight / node may be NULL.  The BowVector / FeatureVector maps are assembled from these arrays by the host mirror
 * (mi355slam::BowIndex::transform) in feature order, so the sums match the reference's; ms_bow_vector (below) assembles the
 * BowVector from word / weight on the device with the same sums. */
typedef struct ms_bow_vocab ms_bow_vocab;
int ms_bow_vocab_create(ms_ctx *ctx, int n_nodes, const int32_t *parent, const uint32_t *node_desc, const double *node_weight,
                        const int32_t *node_word, int depth_levels, ms_bow_vocab **out);
void ms_bow_vocab_destroy(ms_bow_vocab *vocab);
int ms_bow_transform(ms_ctx *ctx, const ms_bow_vocab *vocab, const uint32_t *desc, int n, int levels_up,
                     int32_t *word, double *weight, int32_t *node);

/* ---- N3b: keyframe database behind BowIndex::add / remove / getBowSimilar (bow_index.cpp:44-57, :95-176) ---------------
 * The reference keeps an inverted index std::vector<std::list<MapKf>> over every vocabulary word and scores candidates with
 * DBoW2's L1Scoring.  ms_bow_db keeps, on the device, one entry per keyframe: (map_id, kf_id) and its BowVector (the sparse,
 * L1-normalised map the host mirror assembles after ms_bow_transform: words strictly ascending in [0, n_words), finite values).
 * Queries scan the live entries; results are bit-identical to the reference: the same entries in the same order with the same
 * float scores (order among equal scores: (map_id, kf_id) ascending, the std::map order the reference's std::sort starts from).
 * All arguments are HOST pointers (but the descent ms_bow_db_add_words takes).  add / remove enqueue their work and return; a query synchronises once and fills its outputs.
 * Capacity is grow-only; a steady add / remove / query cycle allocates nothing after warm-up (ms_debug_host_allocs). */
typedef struct ms_bow_db ms_bow_db;
/* An empty database for a vocabulary of n_words words, sized for initial_entries entries of initial_words words in all (grows as needed). */
int ms_bow_db_create(ms_ctx *ctx, int n_words, int initial_entries, long long initial_words, ms_bow_db **out);
void ms_bow_db_destroy(ms_bow_db *db);
/* BowIndex::add (bow_index.cpp:44-48): enter (map_id, kf_id) with its n words / values.  MS_ERR_INVALID, database unchanged, for
 * words out of order or range, a non-finite value, or an id that is already live (the reference never adds one twice).  n = 0 is
 * allowed: such an entry shares no word with anything. */
int ms_bow_db_add(ms_bow_db *db, int32_t map_id, int32_t kf_id, int n, const int32_t *words, const double *values);
/* BowIndex::remove (bow_index.cpp:50-57): O(1); an id that is not live is ignored (MS_OK), like the reference's loop. */
int ms_bow_db_remove(ms_bow_db *db, int32_t map_id, int32_t kf_id);
/* Live entries (MS_ERR_INVALID for NULL). */
int ms_bow_db_size(const ms_bow_db *db);
/* BowIndex::getBowSimilar (bow_index.cpp:95-176) for a BowVector given by the caller (validated like ms_bow_db_add).
 * (ex_map, ex_kf) is excluded from counting and scoring (:100, :113); ex_kf = -1: nothing excluded.
 *   common(e)   = the number of words the query and the entry share; maxInCommon = max over entries with common > 0 (:136-139); none: empty result
 *   minInCommon = (unsigned)(min_in_common_ratio * (float)maxInCommon); an entry survives if common > minInCommon (:143-151)
 *   score       = (float)(-s / 2.0), s = sum over common words in ascending word order of fabs(vi - wi) - fabs(vi) - fabs(wi),
 *                 in double, vi the query's value (DBoW2 L1Scoring::score) (:149)
 *   order       = score descending, then (map_id, kf_id) ascending (:165-166); the entries with score < best * score_ratio (float)
 *                 are cut (:169-173).
 * *n_total = the number of results; the first min(n_total, max_out) are written to out_map / out_kf / out_score. */
int ms_bow_db_query(ms_bow_db *db, int n, const int32_t *words, const double *values, int32_t ex_map, int32_t ex_kf,
                    float min_in_common_ratio, float score_ratio,
                    int max_out, int32_t *out_map, int32_t *out_kf, float *out_score, int *n_total);
/* getBowSimilar for q entries already in the database, each query excluding its own id (loop_closer.cpp:132, :139-141 for a batch):
 * the query vectors are read where they lie, nothing is uploaded.  MS_ERR_INVALID if an id is not live.  Output in CSR form:
 * query i's first min(n_total[i], max_out_per_query) results follow those of query i - 1 in out_map / out_kf / out_score (which hold
 * q * max_out_per_query entries); n_total[q] = each query's full count. */
int ms_bow_db_query_ids(ms_bow_db *db, int q, const int32_t *map_ids, const int32_t *kf_ids,
                        float min_in_common_ratio, float score_ratio, int max_out_per_query,
                        int32_t *out_map, int32_t *out_kf, float *out_score, int *n_total);

/* ---- the BowVector on the device --------------------------------------------------------------------------
 * DBoW2's BowVector::addWeight sums and normalize(L1) (the batch transform behind bow_index.cpp:86-92, mirrored by
 * mi355slam::BowIndex::assembleVector) for a descent that lies on the device.  tests/bow_vector_ref.py restates the rule and is the
 * specification.  word (int32) / weight (float64) [n] are DEVICE arrays in the form ms_bow_transform and ms_keyframe_admit write them:
 *   keep       keypoint i is kept iff weight[i] > 0 as written: a NaN, a zero, a negative weight and a stop word are skipped and their
 *              word is never read (word = -1 with weight = 0 is legal)
 *   entries    one per distinct word of the kept keypoints, in ascending word order
 *   value      starts at 0.0 and adds the kept weights of its word one by one in ascending i, float64, no contraction
 *   norm       starts at 0.0 and adds fabs(value) entry by entry in ascending word order; iff norm > 0.0 every value becomes
 *              value / norm (IEEE double division)
 *   n_bad      the kept keypoints whose word lies outside [0, vocab_words), plus the final values that are not finite
 * ms_bow_vector writes words [cap] (strictly ascending) and values [cap] (DEVICE) and counts (HOST [2]) = n_words, n_bad.
 * 0 <= n <= MS_COVIS_MAX_STRIDE, 0 <= cap <= MS_COVIS_MAX_STRIDE.  Every verdict is taken before any output byte is written:
 * MS_ERR_INVALID when n_bad > 0, MS_ERR_CAPACITY with the needed count in counts[0] when n_words > cap; the outputs keep their bytes
 * in both cases (n_bad is judged first).  Before any device call (ms_bow_vector_validate, the host validation alone: no context, no
 * device; `why` receives the message): MS_ERR_INVALID for a negative n or cap, vocab_words < 1, a missing array (counts; word or weight
 * with n > 0; words or values with cap > 0), weight or values not 8-byte aligned; MS_ERR_CAPACITY beyond the caps.
 * ONE launch whatever n is (k_bow_vector: one workgroup sorts the keys word << 13 | i in LDS, packs the segment heads with the shared
 * block rank, a head's lane walks its segment, one lane adds the norm), no upload, ONE download of the 8-byte head, one host wait.
 * Synchronous on the context stream.  Integer arithmetic decides every position, there is no floating-point atomic and no tree
 * reduction: the same inputs give the same bytes on every call.  The workspace belongs to the context and only grows.  The worst
 * case, every keypoint on one word, is a serial sum of n terms in one lane; it is accepted (DESIGN 9.20 has its time). */
int ms_bow_vector(ms_ctx *ctx, const int32_t *word, const double *weight, int n, int vocab_words, int cap,
                  int32_t *words, double *values, int32_t *counts);
/* the twin is named _validate: the set of ms_*_check functions is closed at 22 (tests/test_map_checks_corpus.py records them) */
int ms_bow_vector_validate(const int32_t *word, const double *weight, int n, int vocab_words, int cap,
                           const int32_t *words, const double *values, const int32_t *counts, char *why, size_t why_bytes);
/* BowIndex::add (bow_index.cpp:44-48) for a keyframe whose descent lies on the DEVICE (word_dev / weight_dev [n], n <=
 * MS_COVIS_MAX_STRIDE; ms_keyframe_admit_words hands them out): a duplicate id is refused on the host before any device work; room for
 * the bound of n words is reserved at the pool top by the code path of ms_bow_db_add (compaction, growth); the launch of ms_bow_vector
 * on the database's context packs the vector straight into the segment; the 8-byte head comes down in one synchronisation and only
 * then is the entry committed, with the cells of its real length.  No upload but the 24-byte entry row.  *n_words (may be NULL) = the
 * entry's length.  MS_ERR_INVALID, database unchanged (a following query is bit-identical to one before the call), when n_bad > 0,
 * for a duplicate id, a negative n, a missing array; MS_ERR_CAPACITY for n beyond the cap.  n_words = 0 is an entry like
 * ms_bow_db_add's n = 0.  Synchronous. */
int ms_bow_db_add_words(ms_bow_db *db, int32_t map_id, int32_t kf_id, const int32_t *word_dev, const double *weight_dev, int n,
                        int32_t *n_words);
/* Downloads a live entry's vector (what keyframe.shared->bowVec held, e.g. for serialization) into HOST words_host / values_host
 * [cap]; *n = its length.  MS_ERR_INVALID when (map_id, kf_id) is not live; MS_ERR_CAPACITY with the length in *n when cap is too
 * small (nothing is written).  Synchronous. */
int ms_bow_db_entry(ms_bow_db *db, int32_t map_id, int32_t kf_id, int cap, int32_t *words_host, double *values_host, int *n);

/* ---- N4: loop-closure RANSAC behind LoopRansac::ransacSolve (loop_ransac.cpp:8-314) --------------------------------------
 * Camera stand-in: tracker::Camera lives in the parent project, outside the reference tree, so the reprojection of
 * reprojectToImage (keyframe.cpp:340-356) is restated for a PINHOLE camera only (other models are not supported):
 *   p_c = A * p + t;  visible iff p_c.z > 0 and (u, v) lies in [0, width) x [0, height), u = fx * (p_c.x / p_c.z) + cx,
 *   v = fy * (p_c.y / p_c.z) + cy, all in double.  Comparisons with NaN are false, so a non-finite hypothesis sees nothing. */
typedef struct { double fx, fy, cx, cy; int32_t width, height; } ms_pinhole;

#define MS_RANSAC_SIM3 0                 /* LoopRansac::DoF::SIM3: computeSim3, Horn's quaternion method (:112-196) */
#define MS_RANSAC_ZROT 1                 /* LoopRansac::DoF::ZROT: computeRotZ, rotation about z only (:277-314) */
#define MS_LOOP_RANSAC_MAX_MATCHES (1 << 20)    /* per problem */
#define MS_LOOP_RANSAC_MAX_ITER (1 << 20)       /* per problem (the packed best key needs n_iter < 2^32) */
#define MS_LOOP_RANSAC_MAX_PROBLEMS 65535       /* per call */

/* One LoopRansac object (loop_ransac.cpp:8-45) and its ransacSolve arguments.  All pointers are HOST pointers. */
typedef struct {
    int32_t n_matches;                   /* matchCount */
    const double *pts1, *pts2;           /* [n*3] commonPtsInKeyframe1/2: the matched map points in each keyframe's camera frame */
    const float *thr1, *thr2;            /* [n] chiSqSigmaSq1/2 = CHI_SQ_2D * levelSigmaSq[octave], a float product (CHI_SQ_2D = 9.21034f) */
    ms_pinhole cam1, cam2;               /* the keyframes' cameras (width, height >= 1) */
    int32_t n_iter;                      /* max_num_iter, >= 0 */
    const int32_t *samples;              /* [n_iter*3] the triplet of each iteration: distinct indices in [0, n) (create_random_array(3, 0, n-1));
                                            not read (may be NULL) when the early return applies */
    int32_t dof;                         /* MS_RANSAC_SIM3 or MS_RANSAC_ZROT */
    int32_t fix_scale;                   /* loopClosureRansacFixScale */
    int32_t min_inliers;                 /* loopClosureRansacMinInliers, >= 0 */
} ms_loop_ransac_problem;

typedef struct {
    int32_t solution_ok;                 /* solutionOk */
    int32_t best_inlier_count;           /* bestInlierCount */
    int32_t best_iter;                   /* the earliest iteration with the most inliers; -1 when none scored above 0 (or the early return applied) */
    double R12[9];                       /* bestR12, row-major; bestT12; bestScale12.  Zero when best_iter = -1 (the reference leaves them unassigned) */
    double t12[3];
    float scale12;
} ms_loop_ransac_result;

/* LoopRansac::ransacSolve (loop_ransac.cpp:47-110) for n problems in one chain of launches on the context stream; synchronous.
 *   early return (:52-54): n_matches < 3 or n_matches < min_inliers -> solution_ok = 0, count 0, best_iter -1, no samples read.
 *   iteration i: the hypothesis (R21, t21, s21) of samples[3i..3i+2]; s21 = (float)(numer / denom); with fix_scale s21 = 1 while t21
 *     keeps the translation of the unfixed scale (:85-86); s12 = 1 / s21 in float, R12 = R21^T, t12 = -s12 * R12 * t21 (:88-91).
 *   inliers (:198-229): both own-image projections (identity pose) and both cross projections visible, and both squared pixel errors,
 *     in double, < their float thresholds.  The best is the earliest iteration with the largest count (:98); solution_ok = count >= min_inliers.
 * union_inliers[p] (optional, [n_matches] bytes): the reference's bestInliers -- its inlier vector is never cleared between iterations (:64, :202),
 *   so it is the UNION of the inlier sets of iterations 0 .. best_iter, the mask loop_closer.cpp:239-243 selects matches with.  All 0 when best_iter = -1.
 * best_inliers[p] (optional, [n_matches] bytes): the inlier set of the best hypothesis alone.
 * hyp_inliers[p] (optional, [n_iter] int32): every iteration's inlier count.
 * A coincident or collinear triplet gives a non-finite or arbitrary hypothesis; non-finite ones score 0, never an error.
 * MS_ERR_INVALID (nothing written) for a sample outside [0, n_matches), a triplet with a repeated index, a bad dof / camera / count;
 * MS_ERR_CAPACITY beyond the MS_LOOP_RANSAC_MAX_* caps.  One upload and one download per call; the workspace belongs to the context and only
 * grows, so calls no larger than an earlier one allocate nothing (ms_debug_host_allocs). */
int ms_loop_ransac(ms_ctx *ctx, const ms_loop_ransac_problem *problems, int n, ms_loop_ransac_result *results,
                   uint8_t *const *union_inliers, uint8_t *const *best_inliers, int32_t *const *hyp_inliers);

/* ---- N5: the Sim3 refinement behind OptimizeSim3Transform (optimize_transform.cpp:63-155) ---------------------------------
 * g2o is outside the reference tree; tests/sim3_opt_ref.py restates the solve and is this entry point's specification.
 * The unknown is one g2o::Sim3 S12 = (r, t, s), S.map(p) = s * (r * p) + t.  Match i gives two edges with focal lengths 1 and
 * principal points 0 (:89-97), proj(y) = (y.x / y.z, y.y / y.z) a plain division without a visibility test:
 *   edge 12 (EdgeSim3ProjectXYZ, :118-127)         e = obs1 - proj(S12.map(p2))
 *   edge 21 (EdgeInverseSim3ProjectXYZ, :133-142)  e = obs2 - proj(S12^-1.map(p1))
 * Information levelSigmaSq[octave] * I2: the reference multiplies by levelSigmaSq, NOT by its inverse (:122, :137); that is kept.
 * RobustKernelHuber on chi2 = info * |e|^2 (:124-126, :139-141).  Update S <- Sim3::exp(dx) * S, dx = (omega, upsilon, sigma), dx[6] = 0
 * under fix_scale (:87).  Levenberg-Marquardt as g2o's OptimizationAlgorithmLevenberg runs it (the schedule of ms_ba_solve), 7 x 7
 * Cholesky.  The Jacobian is the analytic derivative of that update; g2o differentiates these two edges numerically. */
#define MS_SIM3_OPT_MAX_MATCHES (1 << 20)       /* per problem */
#define MS_SIM3_OPT_MAX_PROBLEMS 65535          /* per call */

/* One OptimizeSim3Transform call.  All pointers are HOST pointers. */
typedef struct {
    int32_t n_matches;                   /* matches.size() (:101) */
    const double *pts1, *pts2;           /* [n*3] kf1.poseCW * mp1.position, kf2.poseCW * mp2.position: the fixed vertices (getMpVertex, :44-59) */
    const double *obs1, *obs2;           /* [n*2] bearing.xy / bearing.z of the observing keypoints (:116, :131) */
    const float *info1, *info2;          /* [n] settings.levelSigmaSq.at(octave) (:122, :137) */
    double huber_delta;                  /* (double)(float)sqrt(loopClosureInlierThreshold) (:72-73, :125); <= 0: no robust kernel */
    int32_t fix_scale;                   /* loopClosureRansacFixScale -> VertexSim3Expmap::_fix_scale (:74, :87) */
    int32_t max_iters;                   /* optimizer.optimize(20) (:146), >= 0 */
    double R12[9];                       /* the initial transform12 (:85): Sim3(bestR12, bestT12, bestScale12) of loop_closer.cpp:273-276, */
    double t12[3];                       /* R12 row-major -- what ms_loop_ransac_result holds, its float scale12 widened */
    double scale12;
} ms_sim3_opt_problem;

typedef struct {
    double R12[9];                       /* the refined transform12 (:151), row-major rotation, never re-orthonormalised */
    double t12[3];
    double scale12;                      /* bit-identical to the input under fix_scale */
    double chi2_init, chi2_final;        /* activeRobustChi2 before / at the returned state (as ms_ba_result: chi2_initial, chi2_final) */
    double lambda;                       /* final_lambda */
    int32_t iters;                       /* LM iterations run (iterations) */
    int32_t trials_total;                /* damped solves, including rejected ones (trials) */
    int32_t stop_reason;                 /* 1 if g2o's Terminate condition ended the run (stopped_early) */
    int32_t reserved;                    /* 0 */
} ms_sim3_opt_result;

/* OptimizeSim3Transform (optimize_transform.cpp:63-155) for n independent problems: one launch on the context stream, one workgroup per
 * problem; synchronous.  The reference's return value is matches.size() (:153-154); its inlier check is a TODO (:148) and is not invented.
 *   n_matches = 0 or max_iters = 0: the estimate comes back unchanged with iters = 0 (no match: chi2 0).
 *   Non-finite input: every trial is rejected, the initial estimate comes back bit for bit with a non-finite chi2, no error.
 * chi2_per_edge (optional; chi2_per_edge[p] optional): [2 * n_matches] info * |e|^2 at the returned state, edge 12 of match i at 2 i,
 *   edge 21 at 2 i + 1; through the Huber kernel they sum to chi2_final.
 * The same input gives the same bits on every call and at every position of a batch (fixed reduction order, no float atomics).
 * MS_ERR_INVALID (nothing written) for a negative count, max_iters < 0, a non-finite huber_delta or a missing array with n_matches > 0;
 * MS_ERR_CAPACITY beyond the MS_SIM3_OPT_MAX_* caps.  One upload and one download per call; the workspace belongs to the context and
 * only grows, so calls no larger than an earlier one allocate nothing (ms_debug_host_allocs). */
int ms_sim3_optimize(ms_ctx *ctx, const ms_sim3_opt_problem *problems, int n, ms_sim3_opt_result *results, double *const *chi2_per_edge);

/* FeatureSearch (feature_search.{hpp,cpp}): the keyframe's keypoints sorted by y.  Host helper; std::stable_sort, so points
 * with equal y keep index order (the reference's std::sort leaves that order unspecified).  sorted_idx[p] = keypoint index. */
int ms_feature_search_sort(const float *x, const float *y, int n, float *sorted_x, float *sorted_y, int32_t *sorted_idx);

/* getFeaturesAround + the candidate scan of searchByProjection / replaceDuplication / findMatchesTranformedMps in one launch
 * (feature_search.cpp:33-48 + keyframe_matcher.cpp:349-378, :479-494, :600-623): query i = (projected position, search radius,
 * map-point descriptor, optional octave window [min, max] as in :611).  Candidates are the keypoints with
 * y in [qy - r, qy + r] and dx*dx + dy*dy < r*r (float32), in sorted order; t_skip / t_octave are indexed by KEYPOINT index, as are
 * the returned best / second indices.  Outputs as ms_hamming_candidates; n_candidates[i] = size of the reference's output vector
 * (before skip / octave filtering), may be NULL.  All pointers are device memory. */
int ms_projection_candidates(ms_ctx *ctx, const float *sorted_x, const float *sorted_y, const int32_t *sorted_idx, int n_kp,
                             const uint32_t *t_desc, const int32_t *t_octave, const uint8_t *t_skip,
                             const float *q_x, const float *q_y, const float *q_radius, const int32_t *q_min_octave, const int32_t *q_max_octave,
                             const uint32_t *q_desc, int nq,
                             int32_t *best_idx, uint16_t *best_dist, uint16_t *second_dist, int32_t *best_octave, int32_t *second_octave,
                             int32_t *second_idx, int32_t *n_candidates);

/* The same two scans returning, per query, the FOUR best candidates in the order of (distance, position in the scan) instead of (best, second):
 * top_idx / top_octave [nq*4] (keypoint index / its octave, -1 where the list is shorter), top_dist [nq*4] (256 there), n_scored [nq] = candidates
 * that were scored (inside the radius, not skipped, inside the octave window).  searchByProjection binds keypoints while it walks its map points
 * (keyframe_matcher.cpp:356-360,:388-389): with the list a host replay finds the best and second best among the keypoints still free without going
 * back to the device -- exact whenever two list entries are still free or n_scored <= 4 (the list is the whole candidate set); otherwise that one
 * query is scored again against the current mask (rare: three of its four best must have been taken by earlier map points of the same call). */
int ms_hamming_candidates_topk(ms_ctx *ctx, const uint32_t *q_desc, int nq, const uint32_t *t_desc, const int32_t *cand_start, const int32_t *cand_idx,
                               const uint8_t *t_skip, const int32_t *t_octave, int32_t *top_idx, uint16_t *top_dist, int32_t *top_octave, int32_t *n_scored);
int ms_projection_topk(ms_ctx *ctx, const float *sorted_x, const float *sorted_y, const int32_t *sorted_idx, int n_kp,
                       const uint32_t *t_desc, const int32_t *t_octave, const uint8_t *t_skip,
                       const float *q_x, const float *q_y, const float *q_radius, const int32_t *q_min_octave, const int32_t *q_max_octave,
                       const uint32_t *q_desc, int nq, int32_t *top_idx, uint16_t *top_dist, int32_t *top_octave, int32_t *n_scored, int32_t *n_candidates);

/* ---- M3-M5 gates: the per-map-point loop in front of searchByProjection / replaceDuplication / findMatchesTranformedMps --------------
 * (keyframe_matcher.cpp:313-345, :442-471, :573-596; Keyframe::isInFrustum, keyframe.cpp:247-262, is the SEARCH gates without the radius).
 * One call gates a DEVICE-resident map-point table against n_views views and leaves, per view, the surviving points packed in walk order
 * as the query arrays of ms_projection_topk: no query array is built on the host or uploaded.  tests/project_gate_ref.py restates the
 * arithmetic and is this entry point's specification. */
#define MS_GATE_SEARCH 0   /* searchByProjection :313-345; isInFrustum with view_cos_limit */
#define MS_GATE_FUSE   1   /* replaceDuplication :442-471 */
#define MS_GATE_SIM3   2   /* findMatchesTranformedMps :573-596 */
#define MS_GATE_MAX_LEVELS 32
#define MS_GATE_MAX_VIEWS 4096
#define MS_GATE_MAX_ENTRIES (1 << 24)           /* n_entries stays BELOW this */
typedef struct {
    double R_cw[9], t_cw[3];   /* row-major; SIM3 mode: rotBAW / transBAW (may carry a scale) */
    ms_pinhole cam;
    float threshold;           /* SEARCH: threshold; FUSE / SIM3: margin */
    float view_cos_limit;      /* SEARCH only (0.5 in the reference) */
    int32_t mode;
    int32_t first, count;      /* this view's slice of mp_index */
} ms_gate_view;

/* Entry e in the slice [first, first + count) of view v is map point mp_index[e] seen from view v; slices must not overlap, entries in no
 * slice are not touched.  Gates in the reference's order, the first failing one gives the status:
 *   0 kept | 1 not visible (the ms_pinhole rule above, p_c = R p + t) | 2 viewing distance outside [min, max] (inclusive bounds)
 *   3 normal exactly zero (FUSE only, :460) | 4 viewing angle (SEARCH: cos < view_cos_limit, FUSE: cos < 0.5; SIM3 has none)
 * Per entry (device arrays [n_entries], any may be NULL): x, y = the reprojection narrowed to float (0 at status 1); dist = the viewing
 * distance as predictScaleLevel receives it (0 at status 1); level = predictScaleLevel (map_point.cpp:174-183), radius = the search radius
 * (-1 and 0 unless kept).  The conversion the reference leaves undefined is pinned: a quotient of +inf gives level n_levels - 1, NaN gives 0.
 * Per view, packed at offset views[v].first in entry order (device arrays [n_entries], q_desc [n_entries * 8]; any may be NULL): kept_entry
 * = the entry's position in mp_index, q_* = the arguments of ms_projection_topk for nq = n_kept[v] (the octave window is [level - 1, level]
 * in SIM3 mode, :611, and -0x7fffffff .. 0x7fffffff otherwise).  mp_desc / q_desc must be 16-byte aligned.
 * scale_factors [n_levels] as ms_scale_factors gives them; scale_factor = orbScaleFactor (positive, not 1).
 * The same input gives the same bits on every call and at every position of a batch; three launches whatever n_views is.  Synchronous: one
 * upload, one download (n_kept).  MS_ERR_INVALID (nothing written) for a bad mode, an index outside [0, n_mp) inside a slice, a slice outside
 * [0, n_entries), overlapping slices, a camera with width or height < 1, n_levels < 1, a scale_factor that is not positive and finite or is 1;
 * MS_ERR_CAPACITY beyond the MS_GATE_MAX_* caps.  n_entries = 0 and empty views are fine (n_kept = 0).  The workspace belongs to the context
 * and only grows, so calls no larger than an earlier one allocate nothing (ms_debug_host_allocs). */
int ms_project_gate(ms_ctx *ctx,
    /* map-point table, DEVICE */
    const double *mp_pos, const float *mp_norm, const float *mp_min_dist,
    const float *mp_max_dist, const uint32_t *mp_desc, int n_mp,
    /* HOST */
    const int32_t *mp_index, int n_entries, const ms_gate_view *views, int n_views,
    const float *scale_factors, int n_levels, float scale_factor,
    /* per entry, DEVICE, [n_entries] (any may be NULL) */
    uint8_t *status, float *x, float *y, float *dist, int32_t *level, float *radius,
    /* compacted per view at offset views[v].first, DEVICE */
    int32_t *kept_entry, float *q_x, float *q_y, float *q_radius,
    int32_t *q_min_octave, int32_t *q_max_octave, uint32_t *q_desc,
    /* HOST [n_views] */
    int32_t *n_kept);

/* ---- the writers of the map-point table --------------------------------------------------------------------------------
 * ms_map_refresh: MapPoint::updateDescriptor and MapPoint::updateDistanceAndNorm (map_point.cpp:75-116, :158-172) for chosen rows of the table
 * ms_project_gate reads, written where the table lies -- what mapper_helpers.cpp:1062-1077 runs for the map points of a new keyframe.
 * Entry r refreshes table row rows[r] from its observations obs_start[r] .. obs_start[r + 1], listed in the reference's iteration order
 * (ascending KfId; the first one is getFirstObservation()): obs_kf = the observing keyframe's slot in kf_pose ([n_kf * 12] doubles, rows 0-2
 * of poseCW, row-major), obs_desc = the observing keypoint's descriptor in desc_pool ([n_pool * 8]) or -1 for a keyframe without descriptors
 * (:80), first_octave[r] = the octave of the first observation's keypoint (:168).
 *   normal   = float(sum over the list, left to right, of (c - p).normalized() in float64) / float(n), c = -R^T t summed left to right; the
 *              squared norm is x^2 + (y^2 + z^2), a zero vector stays as it is
 *   max dist = float(|c_0 - p|) * sf[octave], min dist = (float(|c_0 - p|) * sf[octave]) / sf[n_levels - 1], in float32
 *   descriptor = the list's median-Hamming medoid (ms_descriptor_medoid on the observations that have a descriptor)
 * every operation rounded once, in one order: the result does not depend on the launch shape.  desc_pool == NULL or obs_desc == NULL skips
 * the descriptor half.  medoid (HOST, [n_rows], may be NULL): the chosen observation's position in the row's list, -1 when no observation has a
 * descriptor (the row keeps its descriptor, :86), -2 when more than MS_MEDOID_MAX_OBS have one (the row keeps its descriptor; normal and
 * distances are refreshed all the same).  Synchronous: one upload, five launches (two without descriptors), at most one download; the
 * workspace belongs to the context and only grows.  mp_desc and desc_pool are 16-byte aligned.
 * MS_ERR_INVALID, with nothing written and before any device call: a row, slot or pool index out of range, a row listed twice, obs_start not
 * starting at 0 or decreasing, an empty list (the reference asserts), an octave outside [0, n_levels), a missing array.  n_rows = 0 is fine.
 * ms_map_refresh_check is that validation alone (no context, no device; `why` receives the message). */
int ms_map_refresh(ms_ctx *ctx,
    /* map-point table, DEVICE: mp_pos is read, the others are written */
    const double *mp_pos, float *mp_norm, float *mp_min_dist, float *mp_max_dist, uint32_t *mp_desc, int n_mp,
    /* DEVICE */
    const double *kf_pose, int n_kf, const uint32_t *desc_pool /* may be NULL */, int n_pool,
    /* HOST */
    const int32_t *rows, int n_rows, const int32_t *obs_start, const int32_t *obs_kf, const int32_t *obs_desc /* may be NULL */,
    const int32_t *first_octave, const float *scale_factors, int n_levels,
    /* HOST [n_rows], may be NULL */
    int32_t *medoid);
int ms_map_refresh_check(const double *mp_pos, const float *mp_norm, const float *mp_min_dist, const float *mp_max_dist, const uint32_t *mp_desc,
                         int n_mp, const double *kf_pose, int n_kf, const uint32_t *desc_pool, int n_pool, const int32_t *rows, int n_rows,
                         const int32_t *obs_start, const int32_t *obs_kf, const int32_t *obs_desc, const int32_t *first_octave,
                         const float *scale_factors, int n_levels, char *why, size_t why_bytes);

/* ms_loop_correct: the pose correction and map-point transfer of LoopCloser::correctLoop (loop_closer.cpp:398-503) on the pose table and the
 * map-point positions, both DEVICE and updated in place.  T = the Sim3 of :405 as 8 HOST doubles: unit quaternion w, x, y, z, translation,
 * scale.  Keyframe entry i corrects pose kf_slot[i]: pose <- sim3ToSe3(se3ToSim3(pose) * Tl) with Tl = T where kf_rigid[i] (:427) and
 * interpolateSim3(identity, T, kf_lambda[i]) otherwise (:458-463: Eigen's slerp with its linear branch for |d| >= 1 - eps and the sign flip
 * for d < 0, linear translation and scale; the scale is dropped by sim3ToSe3).  Point entry j moves row mp_row[j] with its reference keyframe,
 * entry mp_ref[j] of kf_slot (the localMapPoints value): p <- (corrected^-1 * previous).map(p), both with scale 1 (:500-503).  The Sim3
 * algebra is mi355slam::Sim3's (host/mi355slam/optimize_transform.hpp), operation for operation.  Two launches, synchronous, deterministic.
 * MS_ERR_INVALID, with nothing written and before any device call: a slot, row or reference out of range, a slot or row listed twice, a
 * lambda that is read and is not in [0, 1], a T that is not finite, a missing array.  ms_loop_correct_check is that validation alone. */
int ms_loop_correct(ms_ctx *ctx, double *kf_pose, int n_kf, double *mp_pos, int n_mp,
    /* HOST */
    const double *T, const int32_t *kf_slot, const uint8_t *kf_rigid, const double *kf_lambda, int n_corr,
    const int32_t *mp_row, const int32_t *mp_ref, int n_pts);
int ms_loop_correct_check(const double *kf_pose, int n_kf, const double *mp_pos, int n_mp, const double *T, const int32_t *kf_slot,
                          const uint8_t *kf_rigid, const double *kf_lambda, int n_corr, const int32_t *mp_row, const int32_t *mp_ref, int n_pts,
                          char *why, size_t why_bytes);

/* ---- set queries over the keyframe table -------------------------------------------------------------------------------
 * kf_mp (DEVICE, int32 [n_kf * stride], row-major): entry (k, j) = the map-point table row bound to keypoint j of the keyframe in slot k
 * (Keyframe::mapPoints), -1 for none; a removed keyframe's slot is all -1.  An entry r is VALID iff (uint32)r < n_mp; the kernels make that
 * comparison before any access that uses r, and every other value counts as "none".  mp_flags (DEVICE, uint8 [n_mp], may be NULL when no
 * query asks for flags): the caller's encoding of MapPoint::status, bit 0 = TRIANGULATED, bit 1 = neither NOT_TRIANGULATED nor BAD.
 *
 * ms_covisibility: Keyframe::getNeighbors (keyframe.cpp:192-230) for n_q queries in one call.  S(q) = the valid entries r of slot q.slot
 * with (mp_flags[r] & require) == require (require = 1: triangulatedOnly; 0: no flags read).
 *   count[q * n_kf + k]  = the number of valid entries of slot k, with multiplicity, that lie in S(q) -- under the reference's invariant (a
 *                          keyframe lists a map point at most once) the value of the `covisibilities` map, k = slot included
 *   neighbour rule       k != slot and (k == force_a or k == force_b or (count >= 1 and count >= min_covis)); force_a / force_b =
 *                          previousKfId / nextKfId as slots, -1 for none (the reference seeds them with minCovisibilities and only adds)
 *   neighbours           the neighbour slots of q, ascending (the std::map walk), packed at neighbours + q * n_kf; what lies behind
 *                          n_neighbours[q] of them is unspecified
 * Four launches whatever n_q is (clear, mark, count, compact), one upload, one download; synchronous on the context stream.  The marks (one
 * bitmap of n_mp bits per query, in the context's grow-only workspace) are cleared on every call.  Atomics only OR bits into bitmap words; the
 * packed order comes from ballot prefix sums in slot order, so the same query gives the same bits at any batch position.
 * MS_ERR_INVALID, with nothing written and before any device call: a slot outside [0, n_kf), a forced slot outside [-1, n_kf), require != 0
 * with mp_flags == NULL, stride < 1, a negative count, a missing array.  MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps.  n_q = 0 and
 * n_mp = 0 are fine.  ms_covisibility_check is the validation alone (no context, no device; `why` receives the message). */
#define MS_COVIS_MAX_KF 65536
#define MS_COVIS_MAX_STRIDE 8192
#define MS_COVIS_MAX_QUERIES 4096               /* queries of ms_covisibility, problems of ms_map_point_union */
#define MS_COVIS_MAX_MP (1 << 24)               /* n_mp stays BELOW this */
#define MS_LOOP_MAX_CANDIDATES 4096             /* candidates of ms_loop_pairs and ms_loop_sim3_lists */
#define MS_UNION_MAX_ENTRIES (1 << 20)          /* the problems' list slices together */
typedef struct {
    int32_t slot, force_a, force_b, min_covis;
    uint8_t require;
} ms_covis_query;
int ms_covisibility(ms_ctx *ctx,
    /* DEVICE */
    const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags /* may be NULL */, int n_mp,
    /* HOST */
    const ms_covis_query *queries, int n_q,
    /* DEVICE [n_q * n_kf] each; count may be NULL */
    int32_t *count, int32_t *neighbours,
    /* HOST [n_q] */
    int32_t *n_neighbours);
int ms_covisibility_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, int n_mp, const ms_covis_query *queries, int n_q,
                          const int32_t *neighbours, const int32_t *n_neighbours, char *why, size_t why_bytes);

/* ms_map_point_union: the ordered union of the map points of a list of keyframes -- localMps of matchLocalMapPoints (mapper_helpers.cpp:
 * 241-261), adjacentMapPointsSet of deduplicateMapPoints (:337-345), loopMapPoints of searchAndDeduplicate (loop_closer.cpp:569-584) and
 * localMapPoints of correctLoop (:418-433, :465-469).  Problem u unites the valid entries of the slots kf_list[first .. first + count) in
 * the caller's order (a slot may repeat), drops rows with (mp_flags[r] & require) != require and rows that are a valid entry of
 * exclude_slot (-1 for none: !mp.observations.count(currentKeyframe.id)).  Packed at u * n_mp in ASCENDING ROW ORDER (the std::set /
 * std::map walk): rows, and owner = the smallest position p of the problem's list whose slot lists the row (the emplace-if-absent of
 * loop_closer.cpp:430-432; the list position, not the slot) -- mp_row / mp_ref of ms_loop_correct, mp_index of ms_project_gate.
 * Six launches whatever n_u is (fill, mark, exclude, count, offsets, pack), one upload, one download; synchronous.  The marks (one int32 per
 * row and problem in the context's workspace) are overwritten on every call; atomics only take the minimum of positions.
 * MS_ERR_INVALID, with nothing written and before any device call: a slice outside kf_list, a listed slot outside [0, n_kf), an exclude slot
 * outside [-1, n_kf), require != 0 with mp_flags == NULL, stride < 1, a negative count, a missing array.  MS_ERR_CAPACITY beyond the caps
 * above.  n_u = 0, n_mp = 0 and empty lists are fine (n_rows = 0).  ms_map_point_union_check is the validation alone. */
typedef struct {
    int32_t first, count, exclude_slot;
    uint8_t require;
} ms_union_problem;
int ms_map_point_union(ms_ctx *ctx,
    /* DEVICE */
    const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags /* may be NULL */, int n_mp,
    /* HOST */
    const int32_t *kf_list, int n_list, const ms_union_problem *problems, int n_u,
    /* DEVICE [n_u * n_mp] each; owner may be NULL */
    int32_t *rows, int32_t *owner,
    /* HOST [n_u] */
    int32_t *n_rows);
int ms_map_point_union_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, int n_mp, const int32_t *kf_list, int n_list,
                             const ms_union_problem *problems, int n_u, const int32_t *rows, const int32_t *n_rows, char *why, size_t why_bytes);

/* ---- observation counts and culling on the keyframe table ---------------------------------------------------------------
 * What cullMapPoints (mapper_helpers.cpp:349-373) and cullKeyframes (:433-482) read of a map point is mp.observations.size() and
 * getFirstObservation(); on the device that is the transpose of kf_mp.  kf_mp, mp_flags and the validity rule are those of 9.6.  New:
 *   mp_live (DEVICE, uint8 [n_mp])  non-zero = the row holds a map point of mapDB.mapPoints (a free row and a point whose observations
 *                                    are all gone both count zero observations; ms_triangulate overwrites mp_flags, so no flag bit says it)
 *   kf_id   (HOST, int32 [n_kf])    the slot's KfId, -1 for an empty slot, distinct where >= 0
 *   kf_t    (HOST, double [n_kf])   Keyframe::t
 *
 * ms_observation_count:
 *   n_obs[r]       the number of valid entries equal to r over the slots with kf_id >= 0, with multiplicity (observations.size() under
 *                  the reference's invariant that a keyframe lists a map point at most once)
 *   first_slot[r]  the slot with the smallest kf_id among the slots that list r (getFirstObservation, map_point.cpp:45-63); last_slot[r]
 *                  the one with the largest (getLastObservation); -1 when n_obs[r] == 0
 * Three launches whatever the sizes (fill, count, finish); integer atomics only (add on the counts; min / max on the slot's position in
 * KfId order), so the same table gives the same bits on every call.  Synchronous on the context stream: one upload, no download.
 * MS_ERR_INVALID, with nothing written and before any device call: stride < 1, a negative size, a missing table or kf_id, a non-negative
 * kf_id listed twice.  MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps. */
int ms_observation_count(ms_ctx *ctx,
    /* DEVICE */
    const int32_t *kf_mp, int n_kf, int stride, int n_mp,
    /* HOST */
    const int32_t *kf_id,
    /* DEVICE [n_mp], each may be NULL */
    int32_t *n_obs, int32_t *first_slot, int32_t *last_slot);

/* ms_map_cull: cullMapPoints, then cullKeyframes, on the tables in place.
 * Pass 1, when cull_points != 0: with the counts and first observations of ms_observation_count, a LIVE row r is removed iff
 *   reason 1   n_obs[r] == 0 (:359), or
 *   reason 2   r is not a valid entry of current_slot, and (double)(int32)(kf_t[current_slot] - kf_t[first_slot[r]]) > min_age (the cast
 *              truncates toward zero, the reference's `const int obsAge`), and (mp_flags[r] & 1) == 0 (:365-367).
 * Removal is MapDB::removeMapPoint (mapdb.cpp:161-174): mp_live[r] = 0, mp_flags[r] = 0 when flags are given, n_obs[r] = 0, and every
 * entry of kf_mp equal to r becomes -1.  A row that is not live is never removed; its entries count like any other.
 * Pass 2: `cand` (slots; the adjacent keyframes) is sorted by descending kf_id on the host (:445) and the candidates with cand_keep[i] != 0
 * are dropped (the first keyframe and the keyframes of loop-closure edges, :453-464).  ONE workgroup walks the rest in that order.  For a
 * candidate, nMapPoints = its valid entries, nCritical = those with n_obs[row] <= min_obs_for_ba, n_obs being the current value: after
 * pass 1 and after every removal made earlier in the walk.  If nCritical < nMapPoints * max_critical_ratio the slot is removed
 * (removeKeyframe, :375-431): n_obs[row] -= 1 per valid entry, a live row that reaches 0 is removed as above (reason 3, orphaned), the
 * whole slot becomes -1 and cand_removed[i] = 1 (i = the caller's position in cand; 0 for every other candidate).
 * Arithmetic: ratio_float32 == 0: (double)nCritical < (double)nMapPoints * max_critical_ratio; ratio_float32 != 0:
 * (float)nCritical < (float)nMapPoints * (float)max_critical_ratio, the product rounded once to float32 -- what C++ does for a float
 * parameter.  min_age is compared in float64 against the truncated int: exact for an int, float or double parameter below 2^24.
 * removed_rows / removed_why (DEVICE [n_mp]): the removed rows of both passes in ascending row order and their reasons at the same
 * positions; what lies behind n_removed_rows of them is unspecified.  n_obs (DEVICE [n_mp], may be NULL): the counts after both passes.
 * Eight launches whatever n_mp, n_kf and n_cand are (fill, count, points, keyframes, sweep, block counts, offsets, pack; `points` is left
 * out for cull_points == 0); synchronous: one upload, one download (cand_removed and the two counts).  Integer atomics only; the same
 * input gives the same bits on every call; the workspace belongs to the context and only grows.
 * Left to the caller, who derives them from cand_removed and the downloaded removed_rows: the previousKfId / nextKfId links, the
 * `uncertainty` accumulation, re-pointing referenceKeyframe, trackIdToMapPoint and bowIndex->remove.
 * MS_ERR_INVALID, with nothing written and before any device call: current_slot or a candidate outside [0, n_kf); a candidate listed
 * twice or equal to current_slot; kf_id < 0 at current_slot or at a candidate; a non-negative kf_id listed twice; kf_t of a slot with
 * kf_id >= 0 not finite, or its difference to kf_t[current_slot] outside int32 (the reference's cast is undefined there); min_age or
 * max_critical_ratio not finite; min_obs_for_ba < 0; stride < 1; a negative size; a missing array; mp_flags == NULL with cull_points != 0.
 * MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps (n_cand: MS_COVIS_MAX_QUERIES).  n_cand = 0, n_mp = 0 and cull_points = 0 are fine.
 * ms_map_cull_check is the validation alone (no context, no device; `why` receives the message). */
typedef struct {
    int32_t current_slot;          /* currentKeyframe: exempts its rows from the age rule; never a candidate */
    int32_t cull_points;           /* 0 skips the cullMapPoints pass */
    double  min_age;               /* minMapPointCullingAge */
    int32_t min_obs_for_ba;        /* minObservationsForBA */
    double  max_critical_ratio;    /* keyframeCullMaxCriticalRatio */
    int32_t ratio_float32;         /* the ratio test in float32 (a float parameter) instead of float64 */
} ms_cull_settings;
int ms_map_cull(ms_ctx *ctx,
    /* DEVICE, updated in place; mp_flags may be NULL iff cull_points == 0 */
    int32_t *kf_mp, int n_kf, int stride, uint8_t *mp_flags, uint8_t *mp_live, int n_mp,
    /* HOST */
    const int32_t *kf_id, const double *kf_t, const int32_t *cand, const uint8_t *cand_keep /* may be NULL */, int n_cand,
    const ms_cull_settings *settings,
    /* DEVICE [n_mp]; n_obs and removed_why may be NULL */
    int32_t *n_obs, int32_t *removed_rows, uint8_t *removed_why,
    /* HOST: [n_cand], one, one */
    uint8_t *cand_removed, int32_t *n_removed_rows, int32_t *n_removed_kf);
int ms_map_cull_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, int n_mp,
                      const int32_t *kf_id, const double *kf_t, const int32_t *cand, const uint8_t *cand_keep, int n_cand,
                      const ms_cull_settings *settings, const int32_t *removed_rows, const uint8_t *cand_removed,
                      const int32_t *n_removed_rows, const int32_t *n_removed_kf, char *why, size_t why_bytes);

/* ---- the map-point triangulator -----------------------------------------------------------------------------------------
 * ms_triangulate: triangulateMapPoint (mapper_helpers.cpp:600-722; MS_TRI_TME, MS_TRI_MIDPOINT) or triangulateMapPointFirstLastObs
 * (:724-812; MS_TRI_FIRST_LAST) for chosen rows of the map-point table, positions and status flags written where ms_project_gate,
 * ms_map_refresh and ms_covisibility read them -- the re-triangulation of LoopCloser::correctLoop (loop_closer.cpp:508-523),
 * createNewMapPoints (:308), the pass after local BA (:1083-1090) and matchTrackedFeatures (:90).  Entry r re-triangulates row rows[r] from
 * its observations obs_start[r] .. obs_start[r + 1], listed in the reference's iteration order (ascending KfId): obs_kf = the observing
 * keyframe's slot in kf_pose / kf_cam / kf_focal, obs_x / obs_y / obs_octave = the keypoint's pixel and octave, obs_depth = its
 * keyPointDepth (NULL: no depth anywhere).  was_triangulated[r] = status != NOT_TRIANGULATED on entry (:607); kf_focal = getFocalLength.
 * tests/triangulate_ref.py restates the arithmetic and is this entry point's specification: the camera is the ms_pinhole stand-in
 * (normalizePixel = ((x - cx) / fx, (y - cy) / fy), always true; bearing = its unit vector; reproject = the rule above narrowed to float32),
 * and the three Theia solvers, which are outside the reference tree, are pinned there (N-view: smallest eigenvector of sum C^T C; two views:
 * Lindstrom's niter2, then DLT; midpoint: the 3x3 normal equations), with one cyclic-Jacobi eigen-solve and one summation order.
 * Written for a listed row, exactly when the reference writes them: mp_flags[row] (when given; the 9.6 encoding, TRIANGULATED = 3, UNSURE = 2,
 * NOT_TRIANGULATED = 0 -- the status is reset at entry, so every listed row gets one) and mp_pos[row] (on success; on the depth branch of
 * :622 and at :746 / :776 also when a later check fails).  Rows not listed are not touched.
 * HOST outputs, [n_rows], each may be NULL: status (0 NOT_TRIANGULATED, 1 UNSURE, 2 TRIANGULATED), reason = the first gate that stopped the
 * point (0 none | 1 fewer than two observations | 2 triangulation angle | 3 solver failed | 4 negative depth | 5 reprojection error |
 * 6 fewer than two passing observations, FIRST_LAST | 7 dense-stereo skip, :748), n_pass = FIRST_LAST's nNew.  The trailing updateDescriptor
 * (:811) is ms_map_refresh's.
 * Any number of observations per point (rounds of 16 per point); at most MS_TRI_MAX_OBS observations and MS_TRI_MAX_ROWS rows per call
 * (MS_ERR_CAPACITY beyond).  The same input gives the same bits on every call and at every position of a batch.  Two launches whatever
 * n_rows is; synchronous: one upload, at most one download; the workspace belongs to the context and only grows (ms_debug_host_allocs).
 * MS_ERR_INVALID, with nothing written and before any device call: a row or slot out of range, a row listed twice, obs_start not starting
 * at 0 or decreasing, an octave outside [0, n_levels), an observing camera with width or height < 1 or fx / fy not positive and finite, a
 * bad mode, n_levels outside [1, MS_TRI_MAX_LEVELS], a setting that is not finite, a missing array.  n_rows = 0 and empty observation
 * lists are fine (reason 1).  ms_triangulate_check is that validation alone (no context, no device; `why` receives the message). */
#define MS_TRI_TME        0   /* TriangulationMethod::TME: theia::Triangulate for two observations, TriangulateNView for more */
#define MS_TRI_MIDPOINT   1   /* TriangulationMethod::MIDPOINT: theia::TriangulateMidpoint */
#define MS_TRI_FIRST_LAST 2   /* triangulateMapPointFirstLastObs */
#define MS_TRI_MAX_LEVELS 32
#define MS_TRI_MAX_ROWS (1 << 24)
#define MS_TRI_MAX_OBS (1 << 22)                /* observations of all rows of one call together */
typedef struct {
    const float *level_sigma_sq;         /* HOST [n_levels], StaticSettings::levelSigmaSq; the reference level is n_levels / 2 */
    int32_t n_levels;
    double min_angle_two_obs, min_angle_multiple_obs;    /* degrees: minTriangulationAngleTwoObs / MultipleObs */
    float rel_reprojection_threshold;    /* relativeReprojectionErrorThreshold */
    int32_t dense_stereo_depth;          /* tracker.computeDenseStereoDepth (FIRST_LAST, :748) */
} ms_tri_settings;
int ms_triangulate(ms_ctx *ctx,
    /* DEVICE: mp_pos [n_mp * 3] read and written, mp_flags [n_mp] written (may be NULL), kf_pose [n_kf * 12] */
    double *mp_pos, uint8_t *mp_flags, int n_mp, const double *kf_pose, int n_kf,
    /* HOST, per keyframe slot */
    const ms_pinhole *kf_cam, const int32_t *kf_focal,
    /* HOST, per entry */
    const int32_t *rows, const uint8_t *was_triangulated, int n_rows, const int32_t *obs_start,
    /* HOST, per observation */
    const int32_t *obs_kf, const float *obs_x, const float *obs_y, const int32_t *obs_octave, const float *obs_depth /* may be NULL */,
    const ms_tri_settings *settings, int mode,
    /* HOST [n_rows], each may be NULL */
    uint8_t *status, uint8_t *reason, int32_t *n_pass);
int ms_triangulate_check(const double *mp_pos, int n_mp, const double *kf_pose, int n_kf, const ms_pinhole *kf_cam, const int32_t *kf_focal,
                         const int32_t *rows, const uint8_t *was_triangulated, int n_rows, const int32_t *obs_start, const int32_t *obs_kf,
                         const float *obs_x, const float *obs_y, const int32_t *obs_octave, const ms_tri_settings *settings, int mode,
                         char *why, size_t why_bytes);

/* ---- observation lists on the device -------------------------------------------------------------------------------------
 * ms_observation_lists: the transpose of kf_mp for chosen rows -- MapPoint::observations (`std::map<KfId, KpId>`) of each, as CSR lists in
 * DEVICE memory, with the observing keypoints' table entries gathered next to them, in the form ms_map_refresh and ms_triangulate take
 * their host lists.  kf_mp, n_mp, kf_id and mp_flags are those of 9.6 / 9.8.  New:
 *   kp_x, kp_y, kp_depth (DEVICE float [n_kf * stride]), kp_octave (DEVICE int32 [n_kf * stride])   the keypoint table, parallel to kf_mp;
 *                                     each may be NULL when the outputs that read it are NULL
 *   kf_desc_base (HOST int32 [n_kf])  the index of keypoint 0 of the slot in desc_pool, -1 for a keyframe without descriptors
 *                                     (map_point.cpp:80); may be NULL when obs_desc is
 * The selection: MS_OBS_FROM_ROWS takes rows_in (DEVICE [n_in]; e.g. the output of ms_map_point_union, or removed_rows) in the given order,
 * skips entries outside [0, n_mp) and keeps a row at its first occurrence; MS_OBS_FROM_SLOT takes the valid entries of `slot` in ascending
 * keypoint order, each row at its first occurrence (the loops of mapper_helpers.cpp:1062 / :1085).  The filter drops selected rows:
 * MS_OBS_REFRESH keeps (mp_flags[r] & 2) != 0 (:1066), MS_OBS_RETRIANGULATE keeps (mp_flags[r] & 1) == 0 || n_obs[r] >= 2 (:1088).
 * drop_empty != 0 leaves out rows without observations (ms_map_refresh rejects an empty list).
 * Outputs (DEVICE, the caller's: rows, first_octave, was_triangulated, n_obs_row hold cap_rows, obs_start cap_rows + 1, the obs_* arrays
 * cap_obs; all but rows and obs_start may be NULL):
 *   rows [n_rows], obs_start [n_rows + 1], n_obs_row [n_rows]   the kept rows, the start and the length of each list
 *   obs_kf, obs_kp [n_obs]            the observing slot and the keypoint index j in it
 *   obs_x, obs_y, obs_octave, obs_depth [n_obs]   kp_*[slot * stride + j]
 *   obs_desc [n_obs]                  kf_desc_base[slot] + j, or -1 when the base is negative
 *   first_octave [n_rows]             the octave of the row's first observation, 0 for an empty list
 *   was_triangulated [n_rows]         (mp_flags[row] & 2) != 0 at the time of the call (:607); needs mp_flags
 * Observations come from the slots with kf_id >= 0 only, in ascending kf_id; entries of one slot that name the same row are all kept, in
 * ascending j (the multiplicity convention of ms_observation_count).  n_rows / n_obs (HOST) receive the counts.
 * Ten launches whatever the sizes; synchronous: one upload (the slot order by kf_id, kf_desc_base), one download (the two counts and the
 * violation counter); the lists never cross the bus.  Integer atomics only; entries wait behind an atomic cursor and every row's segment is
 * then put in (kf_id position, j) order -- inside a wave up to 64 observations, by a workgroup through LDS up to 1024, from global memory
 * beyond (correct up to n_kf * stride, quadratic in the length) -- so the same input gives the same bits on every call and at any capacity.
 * MS_ERR_INVALID, with nothing written and before any device call: slot outside [0, n_kf) or with kf_id < 0, a non-negative kf_id listed
 * twice, a flag filter (or was_triangulated) without mp_flags, stride < 1, a negative size, a missing array, a bad source or filter.
 * MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps (n_in: 1 << 24), and when n_rows > cap_rows or n_obs > cap_obs: nothing is written past
 * either capacity (the arrays' contents are unspecified then) and the needed counts are returned, so the caller can regrow and call again.
 * MS_ERR_INVALID after the device pass when n_levels > 0 and a gathered octave lies outside [0, n_levels): the lists are complete, the
 * offending octaves are stored clamped into the range.  n_levels = 0 gathers octaves as they are.
 * n_in = 0, n_mp = 0 and a slot without valid entries are fine and return zero counts and obs_start = {0} (for n_in = 0 and n_mp = 0 without a kernel launch).
 * ms_observation_lists_check is the validation alone (no context, no device; `why` receives the message). */
#define MS_OBS_FROM_ROWS      0
#define MS_OBS_FROM_SLOT      1
#define MS_OBS_ALL            0
#define MS_OBS_REFRESH        1
#define MS_OBS_RETRIANGULATE  2
typedef struct {
    int32_t source;                /* MS_OBS_FROM_ROWS | MS_OBS_FROM_SLOT */
    int32_t filter;                /* MS_OBS_ALL | MS_OBS_REFRESH | MS_OBS_RETRIANGULATE */
    int32_t drop_empty;
    int32_t slot;                  /* MS_OBS_FROM_SLOT */
    const int32_t *rows_in;        /* MS_OBS_FROM_ROWS: DEVICE [n_in] */
    int32_t n_in;
} ms_obs_select;
typedef struct {
    int32_t *rows, *obs_start, *n_obs_row, *first_octave;
    uint8_t *was_triangulated;
    int32_t *obs_kf, *obs_kp, *obs_octave, *obs_desc;
    float *obs_x, *obs_y, *obs_depth;
} ms_obs_lists;
int ms_observation_lists(ms_ctx *ctx,
    /* DEVICE */
    const int32_t *kf_mp, int n_kf, int stride, int n_mp,
    /* HOST */
    const int32_t *kf_id,
    /* DEVICE; see above for which may be NULL */
    const uint8_t *mp_flags, const float *kp_x, const float *kp_y, const int32_t *kp_octave, const float *kp_depth,
    /* HOST */
    const int32_t *kf_desc_base, const ms_obs_select *select, int n_levels,
    /* HOST struct of DEVICE pointers, and their capacities */
    const ms_obs_lists *lists, int cap_rows, int cap_obs,
    /* HOST */
    int32_t *n_rows, int32_t *n_obs);
int ms_observation_lists_check(const int32_t *kf_mp, int n_kf, int stride, int n_mp, const int32_t *kf_id, const uint8_t *mp_flags,
                               const float *kp_x, const float *kp_y, const int32_t *kp_octave, const float *kp_depth,
                               const int32_t *kf_desc_base, const ms_obs_select *select, int n_levels, const ms_obs_lists *lists,
                               int cap_rows, int cap_obs, const int32_t *n_rows, const int32_t *n_obs, char *why, size_t why_bytes);

/* ms_triangulate_lists / ms_map_refresh_lists: ms_triangulate (9.7) and ms_map_refresh (9.5) with the observation lists read from DEVICE
 * memory where ms_observation_lists left them: the same kernels, the same arithmetic and the same bits as the host-list entry points given
 * the same lists, and no list upload -- only the per-slot (kf_cam, kf_focal) and per-level (level_sigma_sq, scale_factors) HOST arrays are.
 * n_rows / n_obs are the counts ms_observation_lists returned.  ms_triangulate_lists reads rows, was_triangulated, obs_start, obs_kf, obs_x,
 * obs_y, obs_octave and obs_depth (NULL: no depth anywhere); ms_map_refresh_lists reads rows, obs_start, obs_kf, first_octave and obs_desc
 * (NULL, or desc_pool NULL: the descriptors are left alone).
 * Validation covers the HOST arguments only (sizes, settings, mode, pointers; MS_ERR_CAPACITY beyond MS_TRI_MAX_ROWS / MS_TRI_MAX_OBS).  The
 * lists are valid by construction when they come from ms_observation_lists -- built with drop_empty != 0 and the same n_levels for
 * ms_map_refresh_lists, with n_pool covering kf_desc_base[slot] + stride; the cameras of the observing slots must be those
 * ms_triangulate_check accepts.  Lists from anywhere else are the caller's responsibility: nothing on the device checks them again.
 * ms_map_refresh_lists builds the rows' descriptor lists (the observations with obs_desc != -1) on the device: a count per row, a scan that
 * also gives the total and the longest list (downloaded: the medoid kernel's LDS is sized by it), a pack; `medoid` (HOST [n_rows], may be
 * NULL) keeps its meaning, the position in the row's list or -1 / -2, and is mapped from the position among the descriptors by a kernel.
 * promote_min_obs > 0 adds the status promotion of mapper_helpers.cpp:1072-1076 to the end of the geometry kernel:
 * mp_flags[row] = list length >= promote_min_obs ? 3 (TRIANGULATED) : 2 (UNSURE); with 0 mp_flags is not touched and may be NULL. */
int ms_triangulate_lists(ms_ctx *ctx,
    /* DEVICE, as ms_triangulate */
    double *mp_pos, uint8_t *mp_flags, int n_mp, const double *kf_pose, int n_kf,
    /* HOST, per keyframe slot */
    const ms_pinhole *kf_cam, const int32_t *kf_focal,
    /* HOST struct of DEVICE pointers */
    const ms_obs_lists *lists, int n_rows, int n_obs,
    const ms_tri_settings *settings, int mode,
    /* HOST [n_rows], each may be NULL */
    uint8_t *status, uint8_t *reason, int32_t *n_pass);
int ms_map_refresh_lists(ms_ctx *ctx,
    /* DEVICE, as ms_map_refresh */
    const double *mp_pos, float *mp_norm, float *mp_min_dist, float *mp_max_dist, uint32_t *mp_desc, int n_mp,
    const double *kf_pose, int n_kf, const uint32_t *desc_pool, int n_pool,
    /* HOST struct of DEVICE pointers */
    const ms_obs_lists *lists, int n_rows, int n_obs,
    /* HOST */
    const float *scale_factors, int n_levels, int promote_min_obs,
    /* DEVICE [n_mp], written for promote_min_obs > 0 */
    uint8_t *mp_flags,
    /* HOST [n_rows] or NULL */
    int32_t *medoid);

/* ---- matchTrackedFeatures on the device map tables -----------------------------------------------------------------------
 * ms_match_tracked: the walk of mapper_helpers.cpp:76-141 over the keypoints of the current frame, whose keyframe slot is frame->slot.
 * The tables are those of 9.6 / 9.8 / 9.9 (kf_mp, mp_flags, mp_live, the map-point table, the keypoint table, desc_pool).  New:
 *   mp_track  (DEVICE int32 [n_mp])     MapPoint::trackId, -1 for none
 *   track_row (DEVICE int32 [n_track])  trackIdToMapPoint as a window: entry t - frame->track_base = the row of track t, -1 for absent
 *   kp_track  (HOST int32 [n_kp])       keyPointToTrackId, negative for none; n_kp <= stride
 *   new_rows  (HOST int32 [n_new])      the rows offered to new map points: the k-th created point in keypoint order takes new_rows[k]
 * A track t is PRESENT iff r = track_row[t - track_base] has (uint32)r < n_mp, mp_live[r] != 0 and mp_track[r] == t: a row that
 * ms_map_cull removed or that was given to another point counts as erased (trackIdToMapPoint.erase, mapdb.cpp:166-173) without anybody
 * touching track_row.  outcome (DEVICE uint8 [n_kp]), decided in the reference's order:
 *   0 no track | 1 created (:126-139: absent and desc_base >= 0) | 2 just tracked (:85-90: present and (mp_flags[r] & 1) == 0) |
 *   3 bound after isInFrustum and checkReprojectionError (:96-116) | 4 outside the frustum | 5 reprojection error |
 *   6 absent and the frame has no descriptors (nothing happens)
 * The gates are the SEARCH gates of 9.4 (statuses 1, 2, 4; view_cos_limit) and checkReprojectionError of 9.7, bit for bit.
 * Written: outcomes 2 and 3: kf_mp[slot * stride + j] = r.  Outcome 1 with r = new_rows[k]: that entry, mp_live[r] = 1, mp_flags[r] = 0,
 * mp_track[r] = t, track_row[t - track_base] = r, mp_desc[r] = desc_pool[desc_base + j] (updateDescriptor of one observation); mp_pos and
 * the rest of the row are left alone.  Packed in keypoint order (DEVICE, each may be NULL): created_rows / created_kp [n_new],
 * tracked_rows (outcome 2) and checked_rows (outcome 3) [n_kp].  counts (HOST [5]): created, just tracked, checked, frustum failures,
 * reprojection failures -- the reference's debug counters.
 * One launch: ONE workgroup of 256 lanes walks the keypoints in trips of 256 and decides and counts everything (phase A, which writes
 * nothing but `outcome`); behind a barrier it writes the tables and the lists (phase B), unless phase A counted a violation:
 * MS_ERR_INVALID with the tables untouched for a bound keypoint (outcome 1, 2, 3) whose kf_mp entry is already valid (keyframe.cpp:275), a
 * used new_rows entry that is live, the octave of a keypoint with a track outside [0, n_levels).  (Two keypoints cannot resolve to one
 * row: present tracks have mp_track[r] == t and kp_track holds an id once.)  MS_ERR_CAPACITY when the frame creates more than n_new
 * points: nothing but `outcome` is written and counts[0] is the needed number, so the caller can call again.
 * Synchronous: one upload, one download; the workspace belongs to the context and only grows.
 * MS_ERR_INVALID, with nothing written and before any device call: slot outside [0, n_kf); a track id listed twice or outside
 * [track_base, track_base + n_track); new_rows out of range or listed twice; n_kp > stride; level_sigma_sq, rel_reprojection_threshold or
 * view_cos_limit not finite; n_levels outside [1, MS_TRI_MAX_LEVELS]; a camera ms_triangulate_check rejects; desc_base >= 0 with
 * desc_base + n_kp > n_pool; descriptor arrays not 16-byte aligned; stride < 1; a negative size; a missing array.  MS_ERR_CAPACITY beyond
 * the MS_COVIS_MAX_* caps and MS_TRACKED_MAX_WINDOW.  n_kp = 0 is fine.
 *
 * ms_match_tracked_finish: after ms_observation_lists (MS_OBS_FROM_ROWS over tracked_rows) and ms_triangulate_lists (MS_TRI_FIRST_LAST)
 * on those lists.  (a) For every listed row with mp_flags == 2 (UNSURE: exactly two observations, :810) the updateDescriptor of :811:
 * mp_desc[row] = the descriptor of the FIRST observation with obs_desc != -1, nothing when there is none -- the reference's median rule
 * (map_point.cpp:101-113) reads index (unsigned)(0.5 * (n - 1)) = 0 of each descriptor's sorted distances, which is 0 for both, and keeps
 * the first under a strict `<`.  Skipped when desc_pool or lists->obs_desc is NULL.  (b) refresh_rows (DEVICE [cap_refresh]) = the listed
 * rows with mp_flags & 1 in list order, then, when append_checked != 0, checked_rows [n_checked]; n_refresh (HOST) = their number.
 * One launch in the same trip shape; one download.  MS_ERR_CAPACITY when cap_refresh < n_rows + the appended rows or a count exceeds
 * MS_COVIS_MAX_STRIDE.  The *_check twins are the validation alone (no context, no device; `why` receives the message). */
#define MS_TRACKED_MAX_WINDOW (1 << 24)         /* n_track */
typedef struct {
    int32_t slot;                        /* the current frame's keyframe slot */
    double pose[12];                     /* rows 0-2 of its poseCW, row-major */
    ms_pinhole cam;
    int32_t focal;                       /* getFocalLength */
    int32_t desc_base;                   /* index of keypoint 0 in desc_pool; negative: !hasFeatureDescriptors() */
    int32_t track_base;                  /* the track id of track_row[0] */
    const float *level_sigma_sq;         /* HOST [n_levels] */
    int32_t n_levels;
    float rel_reprojection_threshold;    /* relativeReprojectionErrorThreshold */
    float view_cos_limit;                /* isInFrustum's viewAngleLimitCos: 0.5 in the reference */
} ms_tracked_frame;
int ms_match_tracked(ms_ctx *ctx,
    /* DEVICE tables, updated in place */
    int32_t *kf_mp, int n_kf, int stride, uint8_t *mp_flags, uint8_t *mp_live,
    const double *mp_pos, const float *mp_norm, const float *mp_min_dist, const float *mp_max_dist, uint32_t *mp_desc, int32_t *mp_track, int n_mp,
    const float *kp_x, const float *kp_y, const int32_t *kp_octave, const uint32_t *desc_pool, int n_pool,
    int32_t *track_row, int n_track,
    /* HOST */
    const ms_tracked_frame *frame, const int32_t *kp_track, int n_kp, const int32_t *new_rows, int n_new,
    /* DEVICE; all but outcome may be NULL */
    uint8_t *outcome, int32_t *created_rows, int32_t *created_kp, int32_t *tracked_rows, int32_t *checked_rows,
    /* HOST [5] */
    int32_t *counts);
int ms_match_tracked_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live,
    const double *mp_pos, const float *mp_norm, const float *mp_min_dist, const float *mp_max_dist, const uint32_t *mp_desc, const int32_t *mp_track, int n_mp,
    const float *kp_x, const float *kp_y, const int32_t *kp_octave, const uint32_t *desc_pool, int n_pool,
    const int32_t *track_row, int n_track,
    const ms_tracked_frame *frame, const int32_t *kp_track, int n_kp, const int32_t *new_rows, int n_new,
    const uint8_t *outcome, const int32_t *counts, char *why, size_t why_bytes);
int ms_match_tracked_finish(ms_ctx *ctx,
    /* HOST struct of DEVICE pointers (rows, obs_start, obs_desc are read), the count ms_observation_lists returned */
    const ms_obs_lists *lists, int n_rows,
    /* DEVICE */
    const uint8_t *mp_flags, const uint32_t *desc_pool, uint32_t *mp_desc, int n_mp,
    const int32_t *checked_rows, int n_checked, int append_checked,
    int32_t *refresh_rows, int cap_refresh,
    /* HOST */
    int32_t *n_refresh);
int ms_match_tracked_finish_check(const ms_obs_lists *lists, int n_rows, const uint8_t *mp_flags, const uint32_t *desc_pool, const uint32_t *mp_desc,
    int n_mp, const int32_t *checked_rows, int n_checked, int append_checked, const int32_t *refresh_rows, int cap_refresh,
    const int32_t *n_refresh, char *why, size_t why_bytes);

/* ---- fusing duplicate map points on the device map tables ------------------------------------------------------------------
 * ms_map_fuse: the walk of replaceDuplication (keyframe_matcher.cpp:424-526) behind its gates and its descriptor search, on the tables of
 * 9.6 / 9.8 / 9.11 in place: kf_mp, mp_flags (the 9.6 encoding), mp_live, n_obs (DEVICE int32 [n_mp], in / out: the caller passes what
 * ms_observation_count gave and the walk keeps it current) and, both or neither, mp_track / track_row with track_base and n_track.
 * mp_index (HOST [n_entries]) is the array given to ms_project_gate; views[v] = {slot, first, count} are the gate's slices plus the walked
 * keyframe's slot; n_kept (HOST [n_views]) and kept_entry / top_idx / top_dist (DEVICE, packed per view at views[v].first) are what
 * ms_project_gate (MS_GATE_FUSE) and ms_projection_topk left.  The candidate of kept query q is top_idx[4q] when it is >= 0 and
 * top_dist[4q] <= max_dist (50 in the reference), else none; an entry the gate dropped has none.
 * The graph filters of :429-440 are part of the walk: the caller gates every valid row of its list without pre-filtering, which is legal
 * because replaceDuplication changes no position, normal, distance or descriptor, and a filter is a `continue` without side effects.
 * Views are walked in order, the entries of a view in slice order.  Entry e, row m = mp_index[e], K = views[v].slot; the first rule that
 * matches the CURRENT state of the tables gives outcome[e]:
 *   1  mp_live[m] == 0 (:429: erased earlier in this call, or before it)                       nothing
 *   2  m is a valid entry of slot K (:434)                                                     nothing
 *   3  (mp_flags[m] & 2) == 0 (:438)                                                           nothing
 *   0  no candidate                                                                            nothing
 *   4  candidate k, kf_mp[K][k] not valid (:502-505)                                           kf_mp[K][k] = m, n_obs[m] += 1
 *   5  x = kf_mp[K][k], n_obs[m] < n_obs[x] and (mp_flags[x] & 2) == 0 (:511-514)              n_obs[x] -= 1, kf_mp[K][k] = m, n_obs[m] += 1
 *   6  the same comparison, any other x (:516)                                                 replace(loser m, winner x)
 *   7  n_obs[m] >= n_obs[x] (:520)                                                             replace(loser x, winner m)
 * replace(l, w) = MapPoint::replaceWith (map_point.cpp:118-156): in every slot s that lists l at keypoint p, kf_mp[s][p] = -1 when w is a
 * valid entry of s before this replace, else kf_mp[s][p] = w and n_obs[w] += 1.  Then mp_live[l] = 0, mp_flags[l] = 0, n_obs[l] = 0 (the
 * state ms_map_cull leaves).  With track tables and t = mp_track[l] != -1: when mp_track[w] == -1, mp_track[w] = t and, for t inside the
 * window, track_row[t - track_base] = w; otherwise nothing (l is no longer live, so 9.11's PRESENT rule reads its track as erased).
 * mp_track[l] stays.
 * Per entry (DEVICE [n_entries], each may be NULL): outcome; kp = the candidate keypoint for codes 4-7, else -1; other = x for codes 5-7,
 * else -1.  Every entry of [0, n_entries) gets the defaults 0 / -1 / -1 first, also the entries of no slice and of views behind an early
 * stop (n_views = 0 writes nothing on the device).  In walk order (DEVICE [n_entries], each may be NULL): erased_rows = the losers, erased_into = their winners.  HOST: n_erased,
 * counts[8] (one per code, over the views walked), views_done.  Left to the caller, who derives them from erased_rows / erased_into and the
 * per-entry outputs: keyPointToTrackId.erase (:142-144), the host MapPoint objects, fusedCount (the entries with codes 4-7).
 * source_slot >= 0 (deduplicateMapPoints reads currentKeyframe.mapPoints live, mapper_helpers.cpp:331-334): when a replace in view v wrote
 * a new valid row into slot source_slot, the walk finishes view v and stops with views_done = v + 1; the caller reads that slot back,
 * rebuilds and gates the remaining views and calls again.  Inside one view the list cannot gain a row that matters: the loser of a code 6
 * is the entry itself, a code 7 turns a later entry into a dead row (code 1).  source_slot = -1 walks every view (searchAndDeduplicate's
 * std::set is a copy).
 * Three launches whatever n_views and n_entries are (fill; scatter the candidates and run the pre-pass; ONE workgroup of 1024 lanes walks:
 * the slice in trips of 1024 entries, the entries with a candidate compacted and stepped through in order, a replace as one pass of the
 * workgroup's 16 waves over the slots).  Integer work; atomics only as adds (and one exchange to zero) on n_obs; the same input gives the
 * same bits on every call.  Synchronous: one upload, one download; the workspace belongs to the context and only grows.
 * MS_ERR_INVALID from the pre-pass, with the tables untouched (the per-entry outputs hold their defaults): a valid entry of a walked slot
 * whose row is not live (mapDB.mapPoints.at would throw at :507), a kept_entry outside its view's slice, a top_idx[4q] outside
 * [-1, stride).  The walk preserves "the valid entries of every slot are live".
 * MS_ERR_INVALID, with nothing written and before any device call: a slot, row or slice out of range; overlapping slices; a row listed twice
 * within a view; n_kept[v] outside [0, count]; max_dist outside [0, 256]; source_slot outside [-1, n_kf); one track table without the
 * other; stride < 1; a negative size; a missing array.  MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps, MS_GATE_MAX_VIEWS,
 * MS_GATE_MAX_ENTRIES (n_entries stays below it) and MS_TRACKED_MAX_WINDOW.  n_entries = 0, n_views = 0 and empty views are fine.
 * Not checked: the reference's invariant that a slot lists a row at most once.  Under its violation the result is unspecified; every index
 * is still compared against n_mp and stride before it is used.
 *
 * ms_map_replace_pairs: the "merge moved map points" loop of loop_closer.cpp:531-546 with the same replace.  pairs (HOST [n_pairs][2]) =
 * (first, second) in order; outcome (HOST uint8 [n_pairs]): 0 replaced (loser first, winner second) | 1 equal (:534) | 2 skipped because
 * first or second was the first row of a pair replaced earlier (:537-541; the rule depends on the list alone and is applied on the host).
 * Chains (a -> b, then b -> c) run in order.  erased_rows / erased_into (DEVICE [n_pairs], each may be NULL): the replaced pairs in order;
 * n_erased (HOST) their number.  Two launches and one clear (check that every listed row is live; ONE workgroup walks the pairs).
 * MS_ERR_INVALID with the tables untouched for a listed row that is not live; before any device call for a row out of range and the table
 * conditions above; MS_ERR_CAPACITY for n_pairs >= MS_GATE_MAX_ENTRIES.  n_pairs = 0 is fine.
 * The *_check twins are the host validation alone (no context, no device; `why` receives the message). */
typedef struct {
    int32_t slot;                        /* the walked keyframe */
    int32_t first, count;                /* its slice of mp_index: the ms_gate_view's */
} ms_fuse_view;
int ms_map_fuse(ms_ctx *ctx,
    /* DEVICE tables, updated in place; mp_track / track_row both or neither */
    int32_t *kf_mp, int n_kf, int stride, uint8_t *mp_flags, uint8_t *mp_live, int32_t *n_obs, int n_mp,
    int32_t *mp_track, int32_t *track_row, int track_base, int n_track,
    /* DEVICE, read */
    const int32_t *kept_entry, const int32_t *top_idx, const uint16_t *top_dist,
    /* HOST */
    const int32_t *mp_index, int n_entries, const ms_fuse_view *views, const int32_t *n_kept, int n_views, int max_dist, int source_slot,
    /* DEVICE [n_entries], each may be NULL */
    uint8_t *outcome, int32_t *kp, int32_t *other, int32_t *erased_rows, int32_t *erased_into,
    /* HOST: one, [8], one */
    int32_t *n_erased, int32_t *counts, int32_t *views_done);
int ms_map_fuse_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const int32_t *n_obs, int n_mp,
    const int32_t *mp_track, const int32_t *track_row, int track_base, int n_track,
    const int32_t *kept_entry, const int32_t *top_idx, const uint16_t *top_dist,
    const int32_t *mp_index, int n_entries, const ms_fuse_view *views, const int32_t *n_kept, int n_views, int max_dist, int source_slot,
    const int32_t *n_erased, const int32_t *counts, const int32_t *views_done, char *why, size_t why_bytes);
int ms_map_replace_pairs(ms_ctx *ctx,
    /* DEVICE tables, updated in place */
    int32_t *kf_mp, int n_kf, int stride, uint8_t *mp_flags, uint8_t *mp_live, int32_t *n_obs, int n_mp,
    int32_t *mp_track, int32_t *track_row, int track_base, int n_track,
    /* HOST */
    const int32_t *pairs, int n_pairs, uint8_t *outcome,
    /* DEVICE [n_pairs], each may be NULL */
    int32_t *erased_rows, int32_t *erased_into,
    /* HOST */
    int32_t *n_erased);
int ms_map_replace_pairs_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const int32_t *n_obs, int n_mp,
    const int32_t *mp_track, const int32_t *track_row, int track_base, int n_track,
    const int32_t *pairs, int n_pairs, const uint8_t *outcome, const int32_t *n_erased, char *why, size_t why_bytes);

/* ---- createNewMapPoints on the device map tables -------------------------------------------------------------------------
 * The loop body of mapper_helpers.cpp:271-318 for one adjacent keyframe, between ms_match_triangulation and the next adjacent.  The tables
 * are those of 9.6 / 9.8 / 9.9 / 9.11.  cur = the slot of the current keyframe (kf1 of the matcher), adj = the adjacent one's.
 *
 * ms_create_points_lists: matched (DEVICE int32 [n_kp1], what ms_match_triangulation wrote for the pair: -1 none, else a keypoint of adj)
 * is walked in ascending keypoint index of cur (the order of :282-290).  The i-th match (j, m = matched[j]) takes the provisional row
 * new_rows[i] (HOST [n_new]) and becomes entry i of `lists` (:293-301): rows[i] = new_rows[i], was_triangulated[i] = 0, obs_start[i] = 2i,
 * n_obs_row[i] = 2, obs_start[n_matches] = 2 n_matches; the two observations (cur, j) and (adj, m) in ascending kf_id of their slots
 * (MapPoint::observations is a std::map<KfId, KpId>), each with obs_kf, obs_kp, obs_x, obs_y, obs_octave, obs_depth and obs_desc =
 * kf_desc_base[slot] + keypoint (-1 for a negative base) as ms_observation_lists gathers them; first_octave[i] = the first one's octave.
 * match_kp1 / match_kp2 (DEVICE [cap_rows], each may be NULL) = j / m.  n_matches goes to the HOST.  The lists are a valid input of
 * ms_triangulate_lists (n_rows = n_matches, n_obs = 2 n_matches; MS_TRI_TME or MS_TRI_MIDPOINT), which writes mp_pos and mp_flags of the
 * provisional rows (:308).  No table is written here: a provisional row stays mp_live = 0.  All of `lists` but rows and obs_start may be
 * NULL, and the keypoint-table array or kf_desc_base an output reads may be NULL when that output is.
 * One launch: ONE workgroup of 256 lanes walks the keypoints in trips of 256, decides and counts (phase A, which writes nothing) and writes
 * behind a barrier (phase B), unless phase A counted a violation: MS_ERR_INVALID with nothing written for a matched[j] outside
 * [0, n_kp2) other than -1, a keypoint of adj named twice, a matched keypoint of either slot whose kf_mp entry is already valid
 * (keyframe.cpp:275), a used new_rows entry that is live and, for n_levels > 0, a matched keypoint's octave outside [0, n_levels) (no
 * clamped copy is written; n_levels = 0 gathers octaves as they are).  MS_ERR_CAPACITY when n_matches > n_new, > cap_rows or 2 n_matches >
 * cap_obs: nothing is written and n_matches is the needed count, so the caller can call again.
 * Synchronous: one upload (new_rows), one download (the count and the violation counters); the workspace belongs to the context and only grows.
 * MS_ERR_INVALID, with nothing written and before any device call: cur or adj outside [0, n_kf) or with kf_id < 0 (or the same kf_id);
 * cur == adj; new_rows out of range or listed twice; n_kp1 or n_kp2 > stride; n_levels outside [0, MS_TRI_MAX_LEVELS]; stride < 1; a
 * negative size; a missing array.  MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps.  n_kp1 = 0 returns n_matches = 0 without a launch (the
 * lists are not touched); a matched array of -1 returns 0 and obs_start = {0}.
 *
 * ms_create_points_bind: after ms_triangulate_lists.  For every entry i with mp_flags[rows[i]] != 0 (:309; two observations give UNSURE = 2
 * or NOT_TRIANGULATED = 0, :629-636): kf_mp[cur][match_kp1[i]] = kf_mp[adj][match_kp2[i]] = rows[i] (:310-311), mp_live[row] = 1,
 * mp_desc[row] = the pool descriptor of the FIRST observation with obs_desc != -1 (updateDescriptor of two observations, the rule of
 * ms_match_tracked_finish; skipped when desc_pool or lists->obs_desc is NULL), n_obs[row] = 2 and mp_track[row] = -1 (DEVICE int32 [n_mp],
 * each may be NULL), usable1[match_kp1[i]] = 0 and usable2[match_kp2[i]] = 0 (the DEVICE `usable` masks of the two ms_match_frame, each
 * may be NULL).  A failed entry writes nothing: its row stays mp_live = 0 and mp_flags = 0 and free, its keypoints stay unbound and usable,
 * so they are offered to the next adjacent keyframe; the position ms_triangulate_lists may have left in the row means nothing.
 * Packed in match order (DEVICE [n_matches], each may be NULL): created_rows, created_kp1, created_kp2; n_created goes to the HOST.
 * One launch in the same trip shape, one download.  The lists are read where they lie; every row (n_mp), keypoint (n_kp1, n_kp2) and
 * descriptor index (n_pool) is compared with its table first, and MS_ERR_INVALID with nothing written is returned for one outside.
 * MS_ERR_INVALID before any device call: cur, adj as above; n_kp1 or n_kp2 > stride; descriptor arrays not 16-byte aligned; stride < 1; a
 * negative size; a missing array.  MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps (n_matches: MS_COVIS_MAX_STRIDE).  n_matches = 0 is fine.
 *
 * ms_unbound_mask: usable[s][j] = !((uint32)kf_mp[slots[s] * stride + j] < n_mp) for j < n_kp[s], for n_slots slots in one launch -- the
 * M2 mask of ms_match_frame (keyframe_matcher.cpp:205-221) taken from the table.  slots, n_kp (HOST int32 [n_slots]); usable (HOST
 * [n_slots] of DEVICE uint8 pointers, [n_kp[s]] each).  MS_ERR_INVALID for a slot outside [0, n_kf), n_kp[s] outside [0, stride], a
 * missing array; MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps (n_slots: MS_COVIS_MAX_QUERIES).
 *
 * All three give the same bits on every call and at every capacity: integer work, one LDS atomicOr per match in ms_create_points_lists
 * and no other atomic.  The *_check twins are the host validation alone (no context, no device; `why` receives the message). */
int ms_create_points_lists(ms_ctx *ctx,
    /* DEVICE tables, read */
    const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, int n_mp,
    /* HOST [n_kf] */
    const int32_t *kf_id,
    /* DEVICE keypoint table; see above for which may be NULL */
    const float *kp_x, const float *kp_y, const int32_t *kp_octave, const float *kp_depth,
    /* HOST [n_kf], may be NULL when lists->obs_desc is */
    const int32_t *kf_desc_base,
    int cur, int adj,
    /* DEVICE [n_kp1]; n_kp1 / n_kp2 = the keypoints of cur / adj */
    const int32_t *matched, int n_kp1, int n_kp2,
    /* HOST */
    const int32_t *new_rows, int n_new, int n_levels,
    /* HOST struct of DEVICE pointers, and their capacities */
    const ms_obs_lists *lists, int cap_rows, int cap_obs,
    /* DEVICE [cap_rows], each may be NULL */
    int32_t *match_kp1, int32_t *match_kp2,
    /* HOST */
    int32_t *n_matches);
int ms_create_points_lists_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, int n_mp, const int32_t *kf_id,
    const float *kp_x, const float *kp_y, const int32_t *kp_octave, const float *kp_depth, const int32_t *kf_desc_base, int cur, int adj,
    const int32_t *matched, int n_kp1, int n_kp2, const int32_t *new_rows, int n_new, int n_levels,
    const ms_obs_lists *lists, int cap_rows, int cap_obs, const int32_t *match_kp1, const int32_t *match_kp2,
    const int32_t *n_matches, char *why, size_t why_bytes);
int ms_create_points_bind(ms_ctx *ctx,
    /* DEVICE tables, updated in place (mp_flags is read); n_obs and mp_track may be NULL */
    int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, uint8_t *mp_live, uint32_t *mp_desc, int32_t *n_obs, int32_t *mp_track, int n_mp,
    const uint32_t *desc_pool, int n_pool,
    int cur, int adj,
    /* HOST struct of DEVICE pointers (rows, obs_desc are read); DEVICE [n_matches], what ms_create_points_lists left */
    const ms_obs_lists *lists, const int32_t *match_kp1, const int32_t *match_kp2, int n_matches,
    /* the keypoints of cur / adj; DEVICE masks of the two frames [n_kp1] / [n_kp2], each may be NULL */
    int n_kp1, int n_kp2, uint8_t *usable1, uint8_t *usable2,
    /* DEVICE [n_matches], each may be NULL */
    int32_t *created_rows, int32_t *created_kp1, int32_t *created_kp2,
    /* HOST */
    int32_t *n_created);
int ms_create_points_bind_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const uint32_t *mp_desc,
    const int32_t *n_obs, const int32_t *mp_track, int n_mp, const uint32_t *desc_pool, int n_pool, int cur, int adj,
    const ms_obs_lists *lists, const int32_t *match_kp1, const int32_t *match_kp2, int n_matches,
    int n_kp1, int n_kp2, const uint8_t *usable1, const uint8_t *usable2, const int32_t *created_rows, const int32_t *created_kp1, const int32_t *created_kp2,
    const int32_t *n_created, char *why, size_t why_bytes);
int ms_unbound_mask(ms_ctx *ctx, const int32_t *kf_mp, int n_kf, int stride, int n_mp,
    /* HOST [n_slots]: the slots, their keypoint counts, their DEVICE masks */
    const int32_t *slots, const int32_t *n_kp, uint8_t *const *usable, int n_slots);
int ms_unbound_mask_check(const int32_t *kf_mp, int n_kf, int stride, int n_mp, const int32_t *slots, const int32_t *n_kp,
    uint8_t *const *usable, int n_slots, char *why, size_t why_bytes);

/* ---- matchLocalMapPoints on the device map tables -------------------------------------------------------------------------
 * The walk of searchByProjection (keyframe_matcher.cpp:349-389) behind ms_project_gate (MS_GATE_SEARCH) and ms_projection_topk, with both
 * addObservations (:388-389) written where the tables lie.  tests/search_bind_ref.py restates it twice and is its specification.
 *
 * ms_bound_mask: skip[j] = ((uint32)kf_mp[slot * stride + j] < n_mp) for j < n_kp -- the keypoints of the slot that carry a map point
 * (:358; a valid entry of the tables always has n_obs >= 1, so the reference's second condition is implied).  One launch on a DEVICE uint8
 * array, in stream order: it is the t_skip of ms_projection_topk, and the complement of ms_unbound_mask for one slot.
 *
 * ms_search_bind: kept_entry, q_*, top_*, n_scored are what ms_project_gate and ms_projection_topk left for ONE view, given as the scoring got
 * them (element 0 = the view's first kept query; kept_entry holds positions of mp_index, inside [first, first + count)); skip is the mask that
 * scoring used; sorted_x .. t_octave, n_kp are the keyframe as the scoring got it; mp_index (HOST) is the gate's array, of which entries
 * [first, first + count) are read; slot = K, the keyframe's slot.  q_min_octave and q_max_octave may each be NULL (no window on that side).
 * Walk the kept queries q = 0 .. n_kept - 1 in order, e = kept_entry[q], m = mp_index[e], `taken` = the keypoints bound earlier in this call:
 *   an empty list (top_idx[4q] < 0) is outcome 0 and top_dist[4q] > 100 is outcome 1 without looking further (every candidate is at least that far);
 *   else best and second = the first two entries of top_idx[4q ..] that are >= 0 and not taken, with their top_dist and top_octave;
 *   fewer than two and n_scored[q] > 4: the radius query of ms_projection_topk again (same float32 arithmetic), over the keypoints not in skip,
 *     not taken and inside the octave window; best and second = the two smallest by (distance, position in the sorted array);
 *   no best -> 0; bestDist > 100 -> 1; bestLevel == bestLevel2 && bestDist > 0.8 * bestDist2 (float64) -> 2; else bind: kf_mp[K][best] = m,
 *     n_obs[m] += 1, match_kp[e - first] = best, best is taken, usable[best] = 0: outcome 3 from the list, 4 after a rescan.  A rescan that
 *     binds nothing reports 0, 1 or 2 with bit 3 set (8, 9, 10).
 * Outputs: match_kp (DEVICE int32 [count], per ENTRY of the slice, -1 for none), outcome (DEVICE uint8 [count], per kept QUERY; entries from
 * n_kept on are 0), usable (DEVICE uint8 [n_kp], K's matcher mask, cleared at each bound keypoint as ms_create_points_bind does) -- each may be
 * NULL; n_matched and counts[6] (HOST): counts[c] for c < 5 = the queries with outcome & 7 == c, counts[5] = the rescans.
 * A pre-pass on the device counts violations: a kept_entry outside the slice; a top_idx outside [-1, n_kp) or marked by skip; skip[j]
 * disagreeing with kf_mp[K][j]; a row m that is not live, that K already lists, or that two kept queries name.  Any of them returns
 * MS_ERR_INVALID with kf_mp and n_obs bit-identical (match_kp and outcome hold their defaults).  MS_ERR_INVALID before any device call: slot
 * outside [0, n_kf); n_kp > stride; n_kept > count; an mp_index of the slice outside [0, n_mp); descriptors not 16-byte aligned; stride < 1; a
 * negative size; a missing array.  MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps and for a slice that ends at or beyond MS_GATE_MAX_ENTRIES.
 * n_kept = 0 and count = 0 are fine.  Four launches, one upload (the slice of mp_index), one download; synchronous.  The same input gives the
 * same bits on every call; the workspace belongs to the context and only grows (ms_debug_host_allocs).  The *_check twins are the host
 * validation alone (no context, no device; `why` receives the message). */
int ms_bound_mask(ms_ctx *ctx, const int32_t *kf_mp, int n_kf, int stride, int n_mp, int slot, int n_kp,
    /* DEVICE [n_kp] */
    uint8_t *skip);
int ms_bound_mask_check(const int32_t *kf_mp, int n_kf, int stride, int n_mp, int slot, int n_kp, const uint8_t *skip, char *why, size_t why_bytes);
int ms_search_bind(ms_ctx *ctx,
    /* DEVICE tables: kf_mp and n_obs are updated in place, mp_live is read */
    int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, int32_t *n_obs, int n_mp,
    /* DEVICE, one view's lists where the gate and the scoring left them, and the mask that scoring used */
    const int32_t *kept_entry, const float *q_x, const float *q_y, const float *q_radius, const int32_t *q_min_octave, const int32_t *q_max_octave,
    const uint32_t *q_desc, const int32_t *top_idx, const uint16_t *top_dist, const int32_t *top_octave, const int32_t *n_scored, const uint8_t *skip,
    /* DEVICE, the keyframe */
    const float *sorted_x, const float *sorted_y, const int32_t *sorted_idx, const uint32_t *t_desc, const int32_t *t_octave, int n_kp,
    /* HOST */
    const int32_t *mp_index, int first, int count, int n_kept, int slot,
    /* DEVICE, each may be NULL */
    int32_t *match_kp, uint8_t *outcome, uint8_t *usable,
    /* HOST */
    int32_t *n_matched, int32_t *counts);
int ms_search_bind_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const int32_t *n_obs, int n_mp,
    const int32_t *kept_entry, const float *q_x, const float *q_y, const float *q_radius, const int32_t *q_min_octave, const int32_t *q_max_octave,
    const uint32_t *q_desc, const int32_t *top_idx, const uint16_t *top_dist, const int32_t *top_octave, const int32_t *n_scored, const uint8_t *skip,
    const float *sorted_x, const float *sorted_y, const int32_t *sorted_idx, const uint32_t *t_desc, const int32_t *t_octave, int n_kp,
    const int32_t *mp_index, int first, int count, int n_kept, int slot, const int32_t *n_matched, const int32_t *counts, char *why, size_t why_bytes);

/* ---- the local BA window on the device map tables ------------------------------------------------------------------------
 * The two steps of localBundleAdjust (bundle_adjuster.cpp:141-394) around the solve that walk MapPoint::observations and Keyframe::mapPoints:
 * building the graph's vertices and projection edges (:245-290) and writing the result back (:376-390, or :326-331 when the neighbourhood
 * stage is skipped).  kf_mp, mp_flags, n_obs, mp_pos, kf_pose and the validity rule are those of 9.5 - 9.8; tests/ba_window_ref.py restates
 * both steps and is their specification.
 *
 * ms_ba_window_lists: `lists` (n_rows, n_obs) is what ms_observation_lists left for the rows of an ms_map_point_union over the local slots
 * with require = 1 (localMapPoints: ascending row, TRIANGULATED only; every observation of each, ascending KfId); rows, obs_start, obs_kf,
 * obs_kp, obs_x, obs_y and obs_octave are read.  local_slot (HOST [n_local]) = the local keyframes in POSE ORDER: the caller sorts them by
 * descending KfId, the std::set<KfId, std::greater<>> walk of :245; distinct slots, each holding a keyframe.  current_index = the position
 * of the current keyframe in local_slot.  kf_cam / kf_focal (HOST, per slot) as ms_triangulate takes them; level_sigma_sq (HOST [n_levels]).
 * HOST outputs, the arrays of an ms_ba_problem (the caller's: pose holds n_local * 7, point cap_point * 3, the obs_* arrays cap_edge entries):
 *   pose [n_local * 7]   matrixToPose(poseCW) = g2o::SE3Quat(R, t) of kf_pose[local_slot[k]]: Eigen's quaternion of a rotation matrix (its
 *                        four branches in its operation order), then normalizeRotation (flipped to w >= 0, divided by its norm); qx, qy,
 *                        qz, qw, tx, ty, tz
 *   point [n_rows * 3]   mp_pos[rows[p]], bit for bit; a row without a kept observation is a point like any other
 *   per kept observation, in list order (rows ascending, inside a row ascending KfId, then keypoint: the order of :259-290):
 *   obs_point            the position p of the row in `rows`;   obs_pose   the position k of the observing slot in local_slot
 *   obs_uv               ((x - cx) / fx, (y - cy) / fy) of the float32 pixel in float64: bearing.xy / bearing.z of the ms_pinhole stand-in (:52)
 *   obs_info             (double)focal * (double)focal / (double)level_sigma_sq[octave] (:51)
 * An observation from a slot that is not in local_slot is dropped (:275).  n_edge = the kept observations; n_current = those with obs_pose ==
 * current_index (nCurrentFrameMapPoints of :219, which the thresholds of :236 and :326 read).
 * DEVICE outputs, kept for ms_ba_window_apply: window->edge_slot / edge_kp / edge_point ([cap_edge] each) = the table entry (slot, keypoint)
 * and the point index of every edge.
 * One thread per listed observation; keep / drop from a per-slot pose index (int32 [n_kf], -1 for a slot that is not local) that is uploaded
 * with the cameras; ranks and offsets from the shared block rank / offsets scan.  One clear of the result head and four launches whatever the sizes (count,
 * offsets, pack, vertices), one upload, one download: the host outputs lie side by side in the context's workspace and come down in one copy through the
 * context's pinned block.  Synchronous on the context stream.  Integer arithmetic decides every position, there is no atomic, and the float64
 * expressions are evaluated as written without contraction: the same input gives the same bits on every call and at any capacity.
 * MS_ERR_INVALID, with nothing written and before any device call: a local slot out of range or listed twice, current_index outside
 * [0, n_local), a local slot's camera with fx or fy not positive and finite (or cx, cy not finite), n_levels outside [1, MS_TRI_MAX_LEVELS],
 * a level_sigma_sq that is not positive and finite, a negative size, a missing array, observations without a row.  MS_ERR_CAPACITY when
 * n_rows > cap_point or n_edge > cap_edge: nothing is written to the caller's arrays or to `window`, and n_edge / n_current are returned, so
 * the caller regrows and calls again (n_edge <= n_obs always); also beyond MS_COVIS_MAX_KF / MS_COVIS_MAX_MP / MS_TRI_MAX_ROWS / MS_TRI_MAX_OBS.
 * n_rows = 0 is fine: poses only, n_edge = 0.  The lists are valid by construction when they come from ms_observation_lists (built with
 * n_levels); a row outside [0, n_mp) gives a zero point and an octave outside [0, n_levels) reads the nearest level.
 *
 * ms_ba_window_apply: the solver's answer into the tables, in place.  HOST inputs, the arrays ms_ba_download returned: pose [n_pose * 7] with
 * n_pose >= n_local (the fixed extra vertex of stage 2 is ignored), point [n_rows * 3], chi2 [n_edge] (NULL for MS_BA_APPLY_NEIGHBOR).  The
 * window: `window` and n_edge as ms_ba_window_lists left them, rows (DEVICE [n_rows]: lists->rows), local_slot, current_index.
 * MS_BA_APPLY_LOCAL (:376-390): every edge with chi2 > 5.991 (float64, strict; a NaN keeps the edge) is erased in both directions:
 * kf_mp[edge_slot * stride + edge_kp] = -1 and n_obs[row] -= 1.  Then every row that lost at least one observation and whose n_obs is now
 * <= 2 gets mp_flags = 2, UNSURE (the reference tests after each erase; the count only falls, so the test on the final count is the same);
 * a row that lost nothing keeps its flags whatever its count.  Then mp_pos[rows[p]] = point[p] for every point, and kf_pose[local_slot[k]] =
 * rows 0-2 of to_homogeneous_matrix() for every k < n_local: Eigen's toRotationMatrix of the quaternion as given, t copied.
 * MS_BA_APPLY_NEIGHBOR (:326-331): the positions, and the pose of local_slot[current_index] alone; kf_mp, mp_flags and n_obs (each may be
 * NULL) keep their bits.
 * n_obs holds the whole-map counts, as ms_observation_count gives them and the chain keeps them current.  The tables must not change between
 * the two calls: an edge whose table entry no longer names its row is skipped and counted (n_stale), and a non-zero count returns
 * MS_ERR_INVALID AFTER the pass, every other effect in place, as the octave rule of ms_observation_lists does.
 * HOST outputs: n_erased and erased_edge [n_erased], the erased edges' indices, ascending.  The application derives
 * keyPointToTrackId.erase (keyframe.cpp:285) and its host copies from them; the matcher's "no map point" masks of the touched slots are the
 * caller's to renew with ms_unbound_mask.  MS_ERR_CAPACITY when n_erased > cap_erased: NOTHING is written, to no table, and n_erased is the
 * needed count (n_erased <= n_edge always).
 * LOCAL: one clear and four launches whatever the sizes (count, offsets, erase, vertices); NEIGHBOR: one launch.  One upload, one download;
 * synchronous.  The only atomic is the integer decrement of n_obs: the same input gives the same bits on every call.
 * MS_ERR_INVALID before any device call: a bad mode, n_pose < n_local, local_slot / current_index as above, stride < 1, a negative size, a
 * missing array.  The *_check twins are the host validation alone (no context, no device; `why` receives the message). */
#define MS_BA_APPLY_LOCAL    0   /* BaStats::Ba::LOCAL: both stages ran */
#define MS_BA_APPLY_NEIGHBOR 1   /* BaStats::Ba::NEIGHBOR: the neighbourhood stage was skipped */
typedef struct {
    int32_t *edge_slot, *edge_kp, *edge_point;   /* DEVICE [cap_edge] each */
} ms_ba_window_dev;
int ms_ba_window_lists(ms_ctx *ctx,
    /* DEVICE tables, read */
    const double *kf_pose, int n_kf, const double *mp_pos, int n_mp,
    /* HOST struct of DEVICE pointers, and the counts ms_observation_lists returned */
    const ms_obs_lists *lists, int n_rows, int n_obs,
    /* HOST */
    const int32_t *local_slot, int n_local, int current_index, const ms_pinhole *kf_cam, const int32_t *kf_focal,
    const float *level_sigma_sq, int n_levels,
    /* HOST outputs and their capacities */
    double *pose, double *point, int32_t *obs_point, int32_t *obs_pose, double *obs_uv, double *obs_info, int cap_point, int cap_edge,
    /* HOST struct of DEVICE pointers, written */
    const ms_ba_window_dev *window,
    /* HOST */
    int32_t *n_edge, int32_t *n_current);
int ms_ba_window_lists_check(const double *kf_pose, int n_kf, const double *mp_pos, int n_mp, const ms_obs_lists *lists, int n_rows, int n_obs,
    const int32_t *local_slot, int n_local, int current_index, const ms_pinhole *kf_cam, const int32_t *kf_focal,
    const float *level_sigma_sq, int n_levels, const double *pose, const double *point, const int32_t *obs_point, const int32_t *obs_pose,
    const double *obs_uv, const double *obs_info, int cap_point, int cap_edge, const ms_ba_window_dev *window,
    const int32_t *n_edge, const int32_t *n_current, char *why, size_t why_bytes);
int ms_ba_window_apply(ms_ctx *ctx,
    /* DEVICE tables, updated in place; kf_mp, mp_flags and n_obs may be NULL for MS_BA_APPLY_NEIGHBOR */
    int32_t *kf_mp, int n_kf, int stride, double *mp_pos, uint8_t *mp_flags, int32_t *n_obs, int n_mp, double *kf_pose,
    /* HOST, what ms_ba_download returned */
    const double *pose, int n_pose, const double *point, const double *chi2,
    /* the window: HOST struct of DEVICE pointers, DEVICE rows, HOST local_slot */
    const ms_ba_window_dev *window, int n_edge, const int32_t *rows, int n_rows, const int32_t *local_slot, int n_local, int current_index,
    int mode,
    /* HOST */
    int32_t *erased_edge, int cap_erased, int32_t *n_erased, int32_t *n_stale);
int ms_ba_window_apply_check(const int32_t *kf_mp, int n_kf, int stride, const double *mp_pos, const uint8_t *mp_flags, const int32_t *n_obs, int n_mp,
    const double *kf_pose, const double *pose, int n_pose, const double *point, const double *chi2,
    const ms_ba_window_dev *window, int n_edge, const int32_t *rows, int n_rows, const int32_t *local_slot, int n_local, int current_index,
    int mode, const int32_t *erased_edge, int cap_erased, const int32_t *n_erased, const int32_t *n_stale, char *why, size_t why_bytes);

/* ---- the loop closer's candidates on the device map tables -----------------------------------------------------------------
 * The three pieces of LoopCloser::tryLoopClosure (loop_closer.cpp:126-378) between its batched solvers (ms_match_loop_closure, ms_loop_ransac,
 * matchMapPointsSim3 on table rows, ms_sim3_optimize) that read MapDB::mapPoints, MapPoint::observations and Keyframe::mapPoints.  kf_mp,
 * mp_flags, mp_live, mp_pos, kf_pose and the keypoint table kp_x / kp_y / kp_octave ([n_kf * stride], parallel to kf_mp) are those of
 * 9.5 - 9.9: row r is PRESENT iff (uint32)r < n_mp and mp_live[r] != 0 (mp_live == NULL: every row is live); bit 0 of mp_flags is
 * TRIANGULATED; kf_pose [n_kf * 12] = rows 0-2 of poseCW, row-major 3 x 4.  tests/loop_chain_ref.py restates all three and is their
 * specification.  The camera-frame point of row r in slot k is, in float64 and evaluated as written (no contraction),
 *   x_i = ((R[i][0] * p0 + R[i][1] * p1) + R[i][2] * p2) + t_i        R, t = kf_pose[k], p = mp_pos[r]
 *
 * ms_loop_usable_mask (keyframe_matcher.cpp:79-84, :94-96; :568-571): for n_slots slots in one launch, with r = kf_mp[slots[s] * stride + k]
 * for k < n_kp[s]:   usable[s][k] = 1 iff r is present and (require_triangulated[s] == 0 or mp_flags[r] & 1), else 0;
 *                    tri_row[s][k] = r iff r is present and mp_flags[r] & 1, else -1.
 * usable is the M1 mask of ms_match_frame: the current keyframe's with require = requireTringulationForLoopClosures, a candidate's with
 * require = 1 (:95); tri_row is the mps1 / mps2 argument of the table form of matchMapPointsSim3.  slots, n_kp, require_triangulated: HOST
 * int32 [n_slots]; usable: HOST [n_slots] of DEVICE uint8 [n_kp[s]]; tri_row: HOST [n_slots] of DEVICE int32 [n_kp[s]], the array or any
 * entry may be NULL.  Errors and caps are those of ms_unbound_mask; in addition mp_flags == NULL is MS_ERR_INVALID when any require is set
 * or any tri_row is asked for.  One upload, one launch, synchronous.
 *
 * ms_loop_pairs (loop_closer.cpp:203-213, loop_ransac.cpp:17-41): the RANSAC problems of all candidates in one call.  cur / n_kp_cur = the
 * current keyframe's slot and keypoints; cand_slot, n_kp_cand (HOST [n_cand]); matched (HOST [n_cand] of DEVICE int32 [n_kp_cur]) = what
 * ms_match_loop_closure wrote for the pair (cur, candidate c); level_sigma_sq (HOST [n_levels]).  For candidate c, keypoint i = 0 ..
 * n_kp_cur - 1 in ascending order yields a pair iff m = matched[c][i] >= 0, r1 = kf_mp[cur][i] is present, r2 = kf_mp[cand_slot[c]][m] is
 * present and r1 != r2.  HOST outputs, CSR over candidates through pair_start [n_cand + 1], cap_pairs entries each:
 *   kp1, kp2, row1, row2   i, m, r1, r2
 *   pts1, pts2 [3 each]    poseCW(cur) * mp_pos[r1], poseCW(cand) * mp_pos[r2] (commonPtsInKeyframe1 / 2)
 *   thr1, thr2             the float product 9.21034f * level_sigma_sq[octave], octave = kp_octave at (cur, i) / (cand, m): on consistent
 *                          tables the keypoints observations.at(kf.id) names (chiSqSigmaSq1 / 2)
 *   cur_pose [12], cand_pose [n_cand * 12]   the poses as read, for the accept gates of :279-338;   n_pairs   the total
 * They are the arrays of ms_loop_ransac_problem.  Three launches whatever n_cand is: a count pass (ONE workgroup per candidate walks the
 * keypoints in trips of 256 and writes nothing but counts), the offsets scan over the candidates (a second trip beyond 256 candidates),
 * the pack pass.  MS_ERR_INVALID with nothing written when the count pass met a matched value outside [-1, n_kp_cand[c]) or a kept pair's
 * octave outside [0, n_levels).  MS_ERR_CAPACITY when n_pairs > cap_pairs: nothing is written to the arrays or the poses, and n_pairs and
 * pair_start hold the needed sizes.  MS_ERR_INVALID before any device call: a slot outside [0, n_kf), cur among the candidates, a
 * candidate listed twice, a keypoint count outside [0, stride], n_levels outside [1, MS_TRI_MAX_LEVELS], a level_sigma_sq that is not
 * positive and finite, stride < 1, a negative size, a missing array.  MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps and
 * MS_LOOP_MAX_CANDIDATES.  n_cand = 0 and n_kp_cur = 0 return n_pairs = 0 and pair_start = {0} without a launch (the poses are not
 * written); a candidate with n_kp_cand = 0 or a matched array of -1 has no pair.
 *
 * ms_loop_sim3_lists (optimize_transform.cpp:44-59, :101-142): the arrays of ms_sim3_opt_problem for the final match lists (the inlier
 * pairs plus what matchMapPointsSim3 appended), given as keypoint pairs kp1 / kp2 (HOST) in CSR over candidates, match_start [n_cand + 1];
 * entry e of candidate c names the rows kf_mp[cur][kp1[e]] and kf_mp[cand_slot[c]][kp2[e]].  kf_cam (HOST, per slot) as
 * ms_ba_window_lists takes it.  HOST outputs, aligned with the lists:
 *   pts1, pts2 [3 each]   as in ms_loop_pairs;   row1, row2   the rows
 *   obs1, obs2 [2 each]   ((x - cx) / fx, (y - cy) / fy) of the float32 pixel in float64, the obs_uv rule of ms_ba_window_lists
 *   info1, info2          level_sigma_sq[octave] (the reference multiplies by it, :122, :137; that is kept)
 * One launch, one thread per entry.  MS_ERR_INVALID with nothing written for a keypoint outside its keyframe (n_kp_cur, n_kp_cand), an
 * entry whose row is not present, an octave outside the levels (all three found on the device), a camera with fx or fy not positive and
 * finite (or cx, cy not finite), a match_start that does not start at 0 or descends, and the cases of ms_loop_pairs.  MS_ERR_CAPACITY
 * beyond the table caps, MS_LOOP_MAX_CANDIDATES, and for a candidate's list longer than the stride.  No match: no launch.
 *
 * All three: the same input gives the same bits on every call, at every capacity and at every position of a batch (integer arithmetic
 * decides every position, the compaction keeps keypoint order, the only atomics are integer violation counters); the number of launches
 * does not depend on n_cand; synchronous on the context stream with one upload and one download through the context's pinned block; the
 * workspace belongs to the context and only grows (ms_debug_host_allocs).  The *_check twins are the host validation alone (no context,
 * no device; `why` receives the message, prefixed "loop mask: ", "loop pairs: ", "loop sim3 lists: "). */
int ms_loop_usable_mask(ms_ctx *ctx,
    /* DEVICE tables, read; mp_live may be NULL */
    const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, int n_mp,
    /* HOST [n_slots]: the slots, their keypoint counts, their require flags, their DEVICE masks and row arrays */
    const int32_t *slots, const int32_t *n_kp, const int32_t *require_triangulated, uint8_t *const *usable, int32_t *const *tri_row, int n_slots);
int ms_loop_usable_mask_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, int n_mp,
    const int32_t *slots, const int32_t *n_kp, const int32_t *require_triangulated, uint8_t *const *usable, int32_t *const *tri_row, int n_slots,
    char *why, size_t why_bytes);
int ms_loop_pairs(ms_ctx *ctx,
    /* DEVICE tables, read; mp_live may be NULL */
    const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const double *mp_pos, int n_mp, const double *kf_pose, const int32_t *kp_octave,
    /* HOST; matched [n_cand] of DEVICE int32 [n_kp_cur] */
    int cur, int n_kp_cur, const int32_t *cand_slot, const int32_t *n_kp_cand, const int32_t *const *matched, int n_cand,
    const float *level_sigma_sq, int n_levels,
    /* HOST outputs and their capacity */
    int cap_pairs, int32_t *pair_start, int32_t *kp1, int32_t *kp2, int32_t *row1, int32_t *row2, double *pts1, double *pts2, float *thr1, float *thr2,
    double *cur_pose, double *cand_pose, int32_t *n_pairs);
int ms_loop_pairs_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const double *mp_pos, int n_mp, const double *kf_pose, const int32_t *kp_octave,
    int cur, int n_kp_cur, const int32_t *cand_slot, const int32_t *n_kp_cand, const int32_t *const *matched, int n_cand,
    const float *level_sigma_sq, int n_levels,
    int cap_pairs, const int32_t *pair_start, const int32_t *kp1, const int32_t *kp2, const int32_t *row1, const int32_t *row2, const double *pts1, const double *pts2, const float *thr1, const float *thr2,
    const double *cur_pose, const double *cand_pose, const int32_t *n_pairs, char *why, size_t why_bytes);
int ms_loop_sim3_lists(ms_ctx *ctx,
    /* DEVICE tables, read; mp_live may be NULL */
    const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const double *mp_pos, int n_mp, const double *kf_pose,
    const float *kp_x, const float *kp_y, const int32_t *kp_octave,
    /* HOST */
    int cur, int n_kp_cur, const int32_t *cand_slot, const int32_t *n_kp_cand, int n_cand, const ms_pinhole *kf_cam,
    const float *level_sigma_sq, int n_levels, const int32_t *kp1, const int32_t *kp2, const int32_t *match_start,
    /* HOST outputs [match_start[n_cand]] */
    double *pts1, double *pts2, double *obs1, double *obs2, float *info1, float *info2, int32_t *row1, int32_t *row2);
int ms_loop_sim3_lists_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_live, const double *mp_pos, int n_mp, const double *kf_pose,
    const float *kp_x, const float *kp_y, const int32_t *kp_octave,
    int cur, int n_kp_cur, const int32_t *cand_slot, const int32_t *n_kp_cand, int n_cand, const ms_pinhole *kf_cam,
    const float *level_sigma_sq, int n_levels, const int32_t *kp1, const int32_t *kp2, const int32_t *match_start,
    const double *pts1, const double *pts2, const double *obs1, const double *obs2, const float *info1, const float *info2, const int32_t *row1, const int32_t *row2,
    char *why, size_t why_bytes);

/* Rotation-consistency histogram (openvslam/match_angle_checker.h:60-134), host arithmetic: 30 bins of
 * cvRound(delta/30), everything outside the 3 fullest bins is invalid (ties between bins go to the lower bin).
 * Writes the ids of invalid entries (bin order, then insertion order) and returns their count. */
int ms_angle_check(const float *delta_angle, const int32_t *ids, int n, int32_t *invalid_ids);

/* Bag-of-words buckets of one keyframe in CSR form (DBoW2::FeatureVector is an ordered std::map
 * node id -> keypoint indices; keyframe_matcher.cpp:65-76).  Arrays are DEVICE pointers. */
typedef struct {
    int32_t n_nodes;
    const int32_t *node_id;      /* [n_nodes] strictly ascending */
    const int32_t *node_start;   /* [n_nodes+1] */
    const int32_t *kp_idx;       /* [node_start[n_nodes]] */
} ms_bow;

/* One keyframe's matching inputs (device pointers). */
typedef struct {
    int32_t n;                   /* keypoints */
    const uint32_t *desc;        /* [n*8] */
    const float *angle;          /* [n] degrees */
    const int32_t *octave;       /* [n] (M2 only) */
    const double *bearing;       /* [n*3] KeyPoint::bearing (M2 only) */
    const uint8_t *usable;       /* [n] M1: has a (triangulated) map point (keyframe_matcher.cpp:79-84,:94-96);
                                        M2: has NO map point (keyframe_matcher.cpp:205-221) */
    ms_bow bow;
} ms_match_frame;

/* matchForLoopClosures (keyframe_matcher.hpp:33-40, keyframe_matcher.cpp:50-158): exact greedy
 * semantics (targets consumed in BoW-node / keypoint order), rotation histogram included.
 * Batched: pair p matches kf1[p] against kf2[p]; matched[p] is a device array [kf1[p].n] (-1 = none);
 * n_matches [n_pairs] device.  `pairs1/pairs2` are HOST arrays of structs holding device pointers. */
int ms_match_loop_closure(ms_ctx *ctx, const ms_match_frame *pairs1, const ms_match_frame *pairs2, int n_pairs,
                          float lowe_ratio, int check_orientation, int32_t *const *matched, int32_t *n_matches);

/* Execution path of the two greedy matchers: 0 (default) = one wavefront per shared vocabulary node, all nodes and pairs side by side
 * (valid because a DBoW2 FeatureVector names each keypoint in exactly one node, so the greedy order only matters inside a node; a pair
 * whose node lists break that property is detected on the device and redone sequentially); 1 = one wavefront per pair walking the
 * nodes in order; 2 = as 0, but ONE workgroup walks the whole work list of large nodes (a test setting: it makes a workgroup reuse its
 * staging memory across nodes).  All give the reference's result bit for bit. */
int ms_match_set_path(ms_ctx *ctx, int path);

/* matchForTriangulationDBoW (keyframe_matcher.hpp:53, keyframe_matcher.cpp:160-293).
 * E12 [n_pairs*9] device, row-major essential matrices (create_E_21, essential_solver.cc:157-162);
 * scale_factors [levels] device; residual_deg_thr = epipolarCheckThresholdDegrees. */
int ms_match_triangulation(ms_ctx *ctx, const ms_match_frame *pairs1, const ms_match_frame *pairs2, int n_pairs,
                           const double *E12, const float *scale_factors, float residual_deg_thr,
                           int check_orientation, int32_t *const *matched, int32_t *n_matches);

/* ---------------------------------------------------------------------------------------------
 * Bundle adjustment -- replaces the g2o optimisation inside localBundleAdjust / poseBundleAdjust /
 * globalBundleAdjust (bundle_adjuster.hpp:30-51; bundle_adjuster.cpp:149-154, :322-323, :372-373,
 * :482-483, :577-578): EdgeSE3ProjectXYZ + EdgeSE3Expmap residuals, Huber kernel, Levenberg-Marquardt.
 * The host wrapper builds the problem exactly as bundle_adjuster.cpp:156-319 builds the g2o graph.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_pose, n_point, n_obs, n_pose_edge;
    const double *pose;          /* [n_pose*7]  qx,qy,qz,qw,tx,ty,tz  world->camera (g2o::SE3Quat of poseCW, :250) */
    const uint8_t *pose_fixed;   /* [n_pose]    vertex->setFixed (:252, :351) */
    const double *point;         /* [n_point*3] MapPoint::position (:266) */
    const uint8_t *point_fixed;  /* [n_point] or NULL (pose-only BA fixes every point, :465) */
    const int32_t *obs_pose;     /* [n_obs] index of the keyframe vertex of each EdgeSE3ProjectXYZ */
    const int32_t *obs_point;    /* [n_obs] index of its map-point vertex */
    const double *obs_uv;        /* [n_obs*2] measurement bearing.xy / bearing.z (:52) */
    const double *obs_info;      /* [n_obs]   information = focal^2 / levelSigmaSq[octave] times I2 (:51-53) */
    double huber_delta;          /* sqrt(5.991) (:56); <= 0 disables the robust kernel (every projection edge quadratic, as with a delta no chi2 reaches) */
    const int32_t *edge_i;       /* [n_pose_edge] EdgeSE3Expmap vertex 0 (:76, :99, :355) */
    const int32_t *edge_j;       /* [n_pose_edge] vertex 1 */
    const double *edge_meas;     /* [n_pose_edge*7] measurement SE3 */
    const double *edge_info;     /* [n_pose_edge*36] 6x6 information W, row-major, (rotation, translation) order: chi2 = e^T W e, b = -J^T (W e),
                                    H = J^T W J with W as given (rows of W meet the left factor); the factorisation reads H's lower triangle.  A symmetric
                                    W is what g2o expects; a non-symmetric one is taken literally by all three kernels, neither transposed nor symmetrised */
    int32_t max_iters;           /* optimizer.optimize(iterations) */
} ms_ba_problem;                 /* all pointers are HOST memory, read during ms_ba_create only.  Poses may lie anywhere in the world and carry either quaternion
                                    sign.  Small shapes SOLVE, they are not rejected: n_obs == 0 and n_point == 0 (a pure pose graph, as globalBundleAdjust builds
                                    on a fresh map), n_pose_edge == 0, a free point with one observation or none (it stays where it is: its step is 0), a free
                                    pose without observations and edges (returned bit for bit when its quaternion is normalised with w >= 0, as a solver leaves
                                    it), an edge between two fixed poses or an observation of a fixed point from a fixed pose (constants of the chi2), repeated
                                    edges and observations (they count as often as they are listed).  No cheirality test: a point behind a camera is an edge
                                    like any other, as in g2o */

typedef struct {
    int32_t iterations;          /* LM iterations run */
    int32_t trials;              /* damped solves, including rejected ones */
    int32_t stopped_early;       /* 1 if g2o's Terminate condition ended the run */
    double final_lambda;
    double chi2_initial, chi2_final;   /* activeRobustChi2 before / after */
    double phase_cycles[8];            /* shader cycles of the problem's first workgroup: chi2 eval, linearise, Schur, Cholesky+back-subst,
                                          points+update, total, then inside the fused Schur pass: tile init, wait for the slowest wave
                                          (record-based path: Hinv / Y / S init, the same + rhs) */
} ms_ba_result;

typedef struct ms_ba ms_ba;

/* Upload `n` independent problems (different sizes allowed) and build their index structures.  The handle's device memory is ONE block;
 * ms_ba_destroy hands it back to the context (up to four blocks, 1 GiB in total: a block that would push the kept total past that --
 * a global-BA sized handle -- is freed instead), and the next ms_ba_create on that context takes the smallest kept block that is large
 * enough and at most 8 times the request instead of allocating: a window per keyframe (create, solve, download, destroy) allocates nothing
 * after warm-up, and a small window never sits on a large block.  If the device is out of memory the kept blocks are freed and the
 * allocation is tried once more.  Kept blocks are released by ms_ctx_destroy.
 * Two shapes are recognised here and solved by kernels of their own (same LM schedule, same arithmetic per edge; results agree with the general
 * kernel to rounding): every problem has ONE free pose and only fixed points, <= 8 SE3 edges at the free pose -- poseBundleAdjust, bundle_adjuster.cpp:396-491;
 * every problem has ONE free pose and at least one free point, <= 8 SE3 edges at the free pose -- stage 1 of localBundleAdjust,
 * bundle_adjuster.cpp:251-252,:322-333 (for this one ms_ba_set_team picks the team of the special kernel: 0 = automatic, up to 8 workgroups).
 * Environment switches for comparisons: MS_BA_NO_POSE_KERNEL=1 / MS_BA_NO_ONE_POSE_KERNEL=1 keep the general kernel. */
int ms_ba_create(ms_ctx *ctx, const ms_ba_problem *problems, int n, ms_ba **out);
void ms_ba_destroy(ms_ba *ba);
/* Run the full LM schedule of every problem from its initial estimates, one workgroup per problem,
 * entirely on the device; asynchronous on the context stream, repeatable. */
/* Workgroups (CUs) that share ONE problem in the next ms_ba_solve: 0 = automatic (by problem size, and only while
 * problems x workgroups fits the chip: a batch of >= #CUs problems always runs one workgroup per problem), 1 = the whole
 * Levenberg-Marquardt loop in one workgroup, up to 64.  Results agree to rounding: a team adds its sums with LDS and global fp64
 * atomics, in no fixed order (run-to-run differences stay below 1e-9 on poses and points; the reference's own order is
 * unspecified).  The index structures are built at create time for the regime the automatic rule will pick; forcing the other one
 * afterwards (a team on a handle created for a chip-filling batch, or one workgroup on a single window's handle) is correct but
 * slower.  A single local-BA window is ~10x faster with a team (1.7 ms against 21 ms for the 50-keyframe window of the bench). */
int ms_ba_set_team(ms_ba *ba, int workgroups_per_problem);
/* Of a team, the workgroups that share the distributed Cholesky factorisation of a system with more than 176 free poses
 * (0 = automatic: one per 16 row tiles a panel touches, so a banded trajectory is factored by one workgroup without team barriers
 * and a densely coupled map by many).  Has no effect on smaller systems. */
int ms_ba_set_factor_team(ms_ba *ba, int workgroups);
int ms_ba_solve(ms_ba *ba);
/* Chains two solves on the device: the state `src`'s last solve left (poses, points) becomes the INITIAL state of `dst`'s problems --
 * the step between stage 1 and stage 2 of localBundleAdjust (bundle_adjuster.cpp:335-373: same vertices, every keyframe unfixed, one more
 * edge against a fixed copy of the just-optimised pose) without a download / upload in between.  Both handles hold the same number of
 * problems on the same context; problem i of dst has the points of problem i of src and at least its poses; each pose dst has beyond
 * them takes the value of src's pose extra_pose_src[i] (HOST array, one entry per problem; may be NULL when the pose counts agree).
 * Asynchronous on the context stream, ordered after src's solve. */
int ms_ba_copy_state(ms_ba *dst, const ms_ba *src, const int32_t *extra_pose_src);
/* Team launches (more than one workgroup per problem) synchronise their workgroups with spin barriers, which need every workgroup
 * of the launch resident: problems x team <= CUs is enforced per launch, and the team launches of one process are admitted per device
 * so that their workgroups together fit the CUs (a launch waits, on the device, for as many older ones of other contexts as it takes),
 * so two contexts -- the front end's poseBundleAdjust beside the back
 * end's localBundleAdjust, mapper.cpp:379-390 vs :268-269 -- may solve at the same time.  If a barrier still gives up (no progress
 * for ~1 s: CUs held by another PROCESS), ms_ba_download repeats the solve with one workgroup per problem before it returns;
 * ms_ba_team_fallbacks counts those repeats.  Before the FIRST problem of a team launch is handed out every problem's marker is looked at, so
 * no result of a launch that is going to be repeated is ever returned.  A barrier gives up after 2 s WITHOUT PROGRESS (arrival counter and
 * the team's heartbeat both still), not after a fixed number of polls: a long single-workgroup phase is not mistaken for a lost team.
 *
 * Process-wide state: team launches are admitted per DEVICE across all contexts of the process (the sum of their workgroups must fit the CUs,
 * or two half-resident teams would wait for each other).  That list -- one event per running team launch, guarded by a mutex -- is the one
 * piece of global mutable state in the library; its events live until the process ends.  An event query that fails with anything but "not
 * ready" retires the entry, is counted (ms_ba_admission_errors) and its text is kept for ms_last_error of the context that saw it.  ms_ba_debug_fail_team_barriers(ba, 1) makes every team barrier of the following
 * launches give up at once (test hook for that path). */
int ms_ba_team_fallbacks(const ms_ba *ba);
/* Event-query failures the team admission list has seen in this process (0 in a healthy run; see above). */
int ms_ba_admission_errors(void);
int ms_ba_debug_fail_team_barriers(ms_ba *ba, int on);
/* Allocations the library has made so far on the host or the device (handle objects, growth of its host scratch, device blocks, pinned staging, events), process-wide.
 * The per-keyframe path -- ms_ba_create / solve / download / destroy of windows of a steady size -- leaves it unchanged after warm-up (the reference mallocs
 * per vertex and edge, bundle_adjuster.cpp:55,73,247,265,279).  tests/host_shim_smoke.cpp holds 20 consecutive windows against it. */
long long ms_debug_host_allocs(void);
/* Test hook: the first `first_trials` damped trials of the following solves count as rejected whatever their gain (state restored, lambda *= nu, nu *= 2): ten of them
 * in one iteration drive g2o's Terminate path (OptimizationAlgorithmLevenberg, _maxTrialsAfterFailure = 10) deterministically.  Every solver honours it: the general
 * one (k_ba_lm), the pose-only one (poseBundleAdjust) and the one-pose one (stage 1 of localBundleAdjust).  0 switches it off; a new handle starts at 0. */
int ms_ba_debug_force_reject(ms_ba *ba, int first_trials);
/* Results of problem i (synchronises): poses [n_pose*7], points [n_point*3], per-observation chi2
 * (what the outlier rule chi2 > 5.991 of :376-388 reads).  They are evaluated at the state that is RETURNED, i.e. the last accepted one.  g2o's edge->chi2() is the
 * error of the last computeActiveErrors(): when optimize() ends on rejected trials (Terminate after ten failures in a row, or a trial without gain) the vertices
 * are restored but the edges keep the rejected trial's errors, and bundle_adjuster.cpp:378 reads those.  The two differ by the last rejected step -- after ten
 * rejections lambda has grown by 2^55, so by about 2^-55 of a Gauss-Newton step; oracle/ba.c restates g2o's value under flag bit 1, and
 * tests/test_gpu_ba.py::test_ten_rejected_trials_terminate_like_the_oracle holds the two against each other.  Any output pointer may be NULL.  The status is read first: on
 * MS_ERR_NUMERIC (non-finite state) none of the caller's arrays is written (res, when given, is filled). */
int ms_ba_download(ms_ba *ba, int i, double *pose, double *point, double *chi2_per_obs, ms_ba_result *res);
/* create + solve + download + destroy for one problem. */
int ms_ba_solve_host(ms_ctx *ctx, const ms_ba_problem *problem, double *pose_out, double *point_out,
                     double *chi2_per_obs, ms_ba_result *res);

/* ---- poseBundleAdjust on the device map tables ---------------------------------------------------------------------------
 * poseBundleAdjust (bundle_adjuster.cpp:396-491) runs on every frame that is not a keyframe (mapper_helpers.cpp:1043-1050), behind
 * ms_match_tracked.  kf_mp, mp_flags, mp_live, mp_pos, kf_pose and the keypoint table kp_x / kp_y / kp_octave are those of 9.5 - 9.9: row r
 * is PRESENT iff (uint32)r < n_mp and mp_live[r] != 0 (mp_live == NULL: every row is live); bit 0 of mp_flags is TRIANGULATED.
 * tests/pose_tables_ref.py restates the gather and the apply and is their specification.
 *
 * ms_pose_tables_create: a persistent handle, created once per context and used for every frame.  It owns a pose-only solver handle with two
 * poses, up to cap_obs fixed points / observations and one SE3 edge, whose device input arrays are written by a kernel, never uploaded;
 * level_sigma_sq (HOST float [n_levels]) goes to the device once, here.  MS_ERR_INVALID for cap_obs outside [0, MS_COVIS_MAX_STRIDE],
 * n_levels outside [1, MS_TRI_MAX_LEVELS], a level_sigma_sq that is not positive and finite.
 *
 * ms_pose_tables_solve, frame f (HOST):
 *   Gather (:403-407, :453-480).  For keypoint j = 0 .. n_kp - 1 in ascending order, r = kf_mp[slot * stride + j] yields one observation iff r
 *   is PRESENT and mp_flags[r] & 1.  Observation k, the k-th kept keypoint: point[k] = mp_pos[r] bit for bit; obs_point[k] = k; obs_pose[k] =
 *   0; obs_uv and obs_info by the expressions of ms_ba_window_lists (the float32 pixel in float64, (x - cx) / fx; (double)focal *
 *   (double)focal / (double)level_sigma_sq[octave]), through the same device code.  Pose 0 = matrixToPose(kf_pose[slot]), free; pose 1 =
 *   matrixToPose(kf_pose[prev_slot]), fixed; both by the four-branch conversion ms_ba_window_lists documents.  The one SE3 edge is
 *   makeOdometryEdge(kf, prev): vertex 0 = pose 0, vertex 1 = pose 1, edge_meas / edge_info as INTEGRATION.md 4 fills them.
 *   n_triangulated = the number kept.
 *   Solve: the pose-only kernel of ms_ba_solve, unchanged, on that problem with max_iters and huber_delta; a frame the apply is not going to
 *   write (below) is evaluated once and not iterated on.
 *   Apply (:485-489).  Iff n_triangulated >= min_visible and the solve ended in a finite state, kf_pose[slot] = rows 0-2 of the returned
 *   pose's matrix by the conversion of ms_ba_window_apply, on the device, and out->ran = 1.  Otherwise kf_pose keeps its bits and out->ran = 0
 *   (the reference's `return false`, :410-412).  The decision is the apply kernel's: the host learns the count only with the results.  No
 *   other table is written.
 * out (HOST): ran; n_triangulated; pose [7] = pose 0 as the solver returned it (as gathered when ran = 0); result, the solver's ms_ba_result
 * (of the single evaluation when the frame was not iterated on).  chi2 (HOST [cap_obs], may be NULL) receives the chi2 per observation in
 * gather order, n_triangulated values, when ran = 1.
 * Per call: NO host-to-device copy (f travels as kernel arguments); three launches whatever the sizes -- the gather (ONE workgroup of 256
 * lanes walks the keypoints in trips of 256; order-preserving compaction through the shared block rank, the count carried across trips;
 * the descriptor's n_obs / n_point are written on the device), the solver, the apply (which also writes the small result record) -- ONE
 * device-to-host copy of that record through the context's pinned block and ONE polite host wait for the handle's event.  Synchronous on
 * the context stream.  Nothing is allocated after the first call of a handle (ms_debug_host_allocs).  Integer arithmetic decides every
 * position and there is no atomic: the same tables give the same bits on every call, and the same bits as ms_ba_solve_host on the restated
 * problem.
 * prev_slot == -1 (:430-432): ran = 0, n_triangulated = 0 and MS_OK before any device call.  MS_ERR_INVALID before any device call: slot
 * outside [0, n_kf), prev_slot outside [-1, n_kf) or equal to slot, n_kp > stride, stride < 1, a negative size, a missing array, a camera
 * ms_triangulate_check rejects, a non-finite edge_meas / edge_info / huber_delta, max_iters < 0.  MS_ERR_CAPACITY beyond the MS_COVIS_MAX_*
 * caps.  After the gather, with kf_pose untouched and n_triangulated returned: MS_ERR_INVALID when a KEPT keypoint's octave lies outside
 * [0, n_levels) (the rule of ms_match_tracked; a dropped keypoint's octave is never read); MS_ERR_CAPACITY when n_triangulated > cap_obs.
 * MS_ERR_NUMERIC, kf_pose untouched and out->pose not written, when the solve ended in a non-finite state (as ms_ba_download).
 *
 * ms_pose_tables_problem: a diagnostic for tests and probes, not on the per-frame path: the arrays the last gather wrote, HOST outputs, any
 * may be NULL: pose [2 * 7], point [n * 3], obs_point [n], obs_pose [n], obs_uv [n * 2], obs_info [n]; n = its count (0 before the first
 * call and after one that returned early or with an error).
 * ms_pose_tables_solve_check is the host validation of ms_pose_tables_solve alone (no context, no device; `why` receives the message). */
typedef struct ms_pose_tables ms_pose_tables;
typedef struct {
    int32_t slot, prev_slot;             /* the frame's keyframe slot; its previous keyframe's, -1 for none */
    int32_t n_kp;                        /* the frame's keypoints, <= stride */
    ms_pinhole cam;
    int32_t focal;                       /* getFocalLength */
    double edge_meas[7];                 /* makeOdometryEdge(kf, prev): the measurement SE3, qx, qy, qz, qw, tx, ty, tz */
    double edge_info[36];                /* its 6 x 6 information, row-major */
    int32_t min_visible;                 /* minVisibleMapPointsInCurrentFrameBA */
    int32_t max_iters;                   /* poseBAIterations */
    double huber_delta;                  /* as ms_ba_problem's */
} ms_pose_tables_frame;
typedef struct {
    int32_t ran;                         /* the reference's return value */
    int32_t n_triangulated;
    double pose[7];
    ms_ba_result result;
} ms_pose_tables_out;
int ms_pose_tables_create(ms_ctx *ctx, int cap_obs, const float *level_sigma_sq, int n_levels, ms_pose_tables **out);
void ms_pose_tables_destroy(ms_pose_tables *h);
int ms_pose_tables_solve(ms_pose_tables *h,
    /* DEVICE tables, read; mp_live may be NULL */
    const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const double *mp_pos, int n_mp,
    const float *kp_x, const float *kp_y, const int32_t *kp_octave,
    /* DEVICE, updated in place */
    double *kf_pose,
    /* HOST */
    const ms_pose_tables_frame *frame, ms_pose_tables_out *out, double *chi2);
int ms_pose_tables_solve_check(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live, const double *mp_pos, int n_mp,
    const float *kp_x, const float *kp_y, const int32_t *kp_octave, const double *kf_pose,
    const ms_pose_tables_frame *frame, const ms_pose_tables_out *out, char *why, size_t why_bytes);
int ms_pose_tables_problem(ms_pose_tables *h, double *pose, double *point, int32_t *obs_point, int32_t *obs_pose, double *obs_uv, double *obs_info, int32_t *n);

/* ---- the end of a frame on the device map tables --------------------------------------------------------------------------
 * What the mapper does with every frame after the pose adjustment: setPointCloudOutput (mapper_helpers.cpp:484-497, called at :1219-1221),
 * the frame's result point cloud, and removeKeyframe (:375-431) for a frame that did not become a keyframe (:1223-1226) or for keyframes that
 * dropped out of the odometry pose trail (:1172-1183).  The tables are those of 9.5 - 9.17: row r is PRESENT iff (uint32)r < n_mp and
 * mp_live[r] != 0 (mp_live == NULL: every row is live); bit 0 of mp_flags is TRIANGULATED; a VALID entry is (uint32)r < n_mp (9.6).
 * tests/frame_finish_ref.py restates the call and is its specification.
 *
 * Cloud (:484-497), the state BEFORE any removal of this call.  For keypoint j = 0 .. n_kp - 1 in ascending order, r = kf_mp[cloud_slot *
 * stride + j] is kept iff r is PRESENT and mp_flags[r] & 1 -- ms_pose_tables_solve's gather predicate and order.  The k-th kept keypoint
 * gives cloud_row[k] = r, cloud_kp[k] = j, cloud_track[k] = mp_track[r] (-1 with mp_track == NULL) and cloud_pos[3k ..] = mp_pos[r] bit for
 * bit.  counts[0] = the number kept.  cloud_slot == -1: no cloud, counts[0] = 0.
 *
 * Removal (:375-431), the table part, for the slots of remove_slots in list order.  A REMAINING slot has kf_id >= 0 and is not in the list.
 * For every row r a removed slot lists (valid entries), remain[r] = the number of valid entries equal to r in the remaining slots, with
 * multiplicity (ms_observation_count's definition; a stale entry of a slot with kf_id < 0 does not count).  A LIVE row with remain[r] == 0 is
 * removed as MapDB::removeMapPoint does, the way ms_map_cull does it: mp_live[r] = 0, mp_flags[r] = 0.  A row that is not live is never
 * reported; its entries are erased like any other.  Every one of the `stride` entries of every removed slot becomes -1.  With n_obs != NULL,
 * n_obs[r] = remain[r] for every row a removed slot lists (0 for a removed row); other rows are untouched, and the incoming n_obs is never
 * read (ms_match_tracked leaves it stale).  removed_rows holds each removed row once, in first-claim order: the order of remove_slots, then
 * keypoint index.  counts[1] = the number of removed rows, counts[2] = the number of valid entries erased.
 * Left to the caller, as for ms_map_cull: the previous / next links, `uncertainty`, referenceKeyframe, bowIndex->remove and kf_id[slot] = -1;
 * track_row needs no write (the presence rule of 9.11).
 *
 * MS_ERR_INVALID, nothing written, before any device call: cloud_slot outside [-1, n_kf) or with kf_id < 0; n_kp outside [0, stride]; a removed
 * slot out of range, listed twice or with kf_id < 0; a non-negative kf_id listed twice; mp_live == NULL with n_remove > 0; stride < 1, a
 * negative size, a missing array.  MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps (n_remove: MS_COVIS_MAX_QUERIES), and when more rows are
 * removed than cap_removed: then every table keeps its bits, counts holds the needed numbers and the cloud outputs are valid -- every verdict
 * is taken before a table is written (the rule of ms_ba_window_apply).  n_remove == 0, cloud_slot == -1, n_mp == 0 and n_kp == 0 are fine.
 * Per call: one upload block (the per-slot list positions and the list; none with n_remove == 0), at most six launches whatever the sizes (one
 * with n_remove == 0, none when no cloud is wanted either), no host wait between them, ONE download (counts, cloud, removed rows) through the
 * context's pinned block.  The cloud is launched first and so sees the tables before the removal.  Integer arithmetic decides every position
 * and every atomic is an integer min or add: the same tables give the same bytes on every call.  Nothing is allocated after warm-up.
 * ms_frame_finish_validate is the host validation alone (no context, no device; `why` receives the message). */
typedef struct {
    int32_t cloud_slot;      /* slot whose point cloud is wanted, -1 for none */
    int32_t n_kp;            /* its keypoints, <= stride (pose_tables' rule) */
} ms_frame_finish_args;
int ms_frame_finish(ms_ctx *ctx,
    /* DEVICE tables, updated in place; mp_live may be NULL iff n_remove == 0; mp_track, n_obs may be NULL */
    int32_t *kf_mp, int n_kf, int stride, uint8_t *mp_flags, uint8_t *mp_live,
    const double *mp_pos, const int32_t *mp_track, int32_t *n_obs, int n_mp,
    /* HOST */
    const int32_t *kf_id, const int32_t *remove_slots, int n_remove, const ms_frame_finish_args *args,
    /* HOST outputs: cloud_* [n_kp] (each may be NULL), removed_rows [cap_removed], counts [3] */
    int32_t *cloud_row, int32_t *cloud_kp, int32_t *cloud_track, double *cloud_pos,
    int32_t *removed_rows, int cap_removed, int32_t *counts);
/* the twin is named _validate: the set of ms_*_check functions is closed at 22 (tests/test_map_checks_corpus.py records them) */
int ms_frame_finish_validate(const int32_t *kf_mp, int n_kf, int stride, const uint8_t *mp_flags, const uint8_t *mp_live,
    const double *mp_pos, const int32_t *mp_track, const int32_t *n_obs, int n_mp,
    const int32_t *kf_id, const int32_t *remove_slots, int n_remove, const ms_frame_finish_args *args,
    const int32_t *cloud_row, const int32_t *cloud_kp, const int32_t *cloud_track, const double *cloud_pos,
    const int32_t *removed_rows, int cap_removed, const int32_t *counts, char *why, size_t why_bytes);

/* ---- a new keyframe from the extractor's output to the map tables ----------------------------------------------------------
 * Keyframe::addFullFeatures / processKeyPoints (keyframe.cpp:34-116, called at mapper_helpers.cpp:1186-1203) without the host in between:
 * ms_keyframe_admit puts frame `frame` of a DEVICE ms_keypoints view (ms_orb_device_view, or any SoA of device arrays, as ms_keypoints_pack
 * accepts) into slot `slot` of the tables of 9.4 - 9.18 and completes the DEVICE arrays of an ms_match_frame and of FeatureSearch::create.
 * n = view->count[frame] is read ON THE DEVICE; the host learns it with the results.  tests/keyframe_admit_ref.py restates the call and is
 * its specification.
 *
 * Written for j < n:
 *   keypoint table, entry slot * stride + j: kp_x, kp_y, kp_octave copied bit for bit; entries j >= n keep their bytes
 *   kp_depth (keyframe.cpp:55-64): depth = -1; with view->track_id[j] >= 0 and track_ids given, depth = track_depth[i], i the LAST index with
 *     track_ids[i] == the id (trackIdToIndex[id] = idx overwrites); then, iff depth < 0 as written (a NaN stays), the sample of depth_image at
 *     (__float2int_rn(x), __float2int_rn(y)) -- the rounding of the valid mask in ms_orb_set_valid_mask -- or -1 outside the image or with no
 *     image.  The image is a stand-in for frame->getDepth, which belongs to the external image class, as the valid mask stands in for
 *     tracker::Camera::isValidPixel
 *   desc_pool[(desc_base + j) * 8 ..]: the descriptor
 *   out->desc, angle, octave copied; out->bearing = the unit vector of ((x - cx) / fx, (y - cy) / fy, 1) in float64 without contraction, the
 *     stand-in of 9.7 (one device function, shared with ms_triangulate); out->usable[j] = 1, what ms_unbound_mask gives for the cleared row
 *   out->sorted_x / sorted_y / sorted_idx: FeatureSearch::create by ms_feature_search_sort's rule.  The position of j is the number of k with
 *     y[k] < y[j] || (y[k] == y[j] && k < j): integer ranks, no atomics
 *   out->node_id / node_start / kp_idx with a vocabulary: the descent of ms_bow_transform on the view's descriptors where they lie, then the
 *     keypoints with weight > 0 (DBoW2's rule) ranked by (node, index) -- the ms_bow of a FeatureVector.  Without a vocabulary n_nodes = 0.
 * Written per slot: kf_mp[slot * stride + j] = -1 for ALL stride entries; kf_pose[slot] = pose (it travels as a kernel argument).
 * HOST outputs (ms_admit_host, the struct and each member may be NULL; each array holds cap_kp elements), one download through the context's
 * pinned block: kp_track = keyPointTrackIds, what ms_match_tracked takes next; word, weight of the descent (-1 and 0 without a vocabulary)
 * for the host's BowVector, whose floating-point sums stay in feature order on the host; sorted_x, sorted_y, sorted_idx, octave, desc: the
 * host copies a keyframe record keeps.  counts (HOST [3]) = n, n_nodes, the keypoints in the node lists.
 *
 * Every verdict is taken before any write: a first pass counts into the head of the block that goes down, and the writing kernels return at
 * once when it is non-zero.  MS_ERR_CAPACITY with the needed n in counts[0] when n > stride, n > cap_kp or desc_base + n > n_pool.
 * MS_ERR_INVALID for n outside [0, view->capacity], a non-finite x or y among the first n (ranks would collide), a VALID entry
 * ((uint32)r < n_mp, ms_match_tracked's rule) already in the slot's row, a tracked keypoint whose id is not in track_ids when track_ids is
 * given (the reference's .at throws).  In every such case each table and frame array keeps its bytes.  Before any device call
 * (ms_keyframe_admit_validate, the host validation alone: no context, no device; `why` receives the message): MS_ERR_INVALID for slot, frame
 * or desc_base out of range, descriptor arrays that are not 16-byte aligned, stride < 1, a non-finite pose or camera, a depth image without
 * a size, a missing array; MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps (n_tracks, cap_kp and view->capacity: MS_COVIS_MAX_STRIDE).
 * FOUR launches whatever the sizes (descent and head; verdicts; ranks and every write; node lists), at most one upload block (the track
 * lists; none without them), ONE download, one host wait.  Synchronous on the context stream, behind ms_orb_extract.  The workspace belongs
 * to the context and only grows: nothing is allocated after warm-up (ms_debug_host_allocs).  The same inputs give the same bytes on every
 * call.  The BowVector itself is not built here: ms_bow_db_add takes host arrays, so a caller either takes word / weight down and sums on the
 * host, or leaves them NULL and hands the descent to ms_bow_db_add_words where it lies (ms_keyframe_admit_words).
 * Not covered: colours (getPixel), reuse of pool space when keyframes leave.  The keypoints of a frame that carries tracker features only
 * (addTrackerFeatures) come in through ms_frame_admit. */
typedef struct {
    int32_t slot;                        /* the keyframe's slot in kf_mp, the keypoint table and kf_pose */
    int32_t desc_base;                   /* index of keypoint 0 in desc_pool */
    double pose[12];                     /* rows 0-2 of poseCW, row-major */
    ms_pinhole cam;
    int32_t levels_up;                   /* of the descent (4 in the reference); read with a vocabulary only */
    const ms_bow_vocab *vocab;           /* may be NULL */
    const int32_t *track_ids;            /* HOST [n_tracks] the tracker features' ids, may be NULL */
    const float *track_depth;            /* HOST [n_tracks] their depth */
    int32_t n_tracks;
    const float *depth_image;            /* DEVICE float32, may be NULL */
    int32_t depth_width, depth_height, depth_stride;     /* row stride in elements */
} ms_admit_args;
typedef struct {                         /* DEVICE arrays of one keyframe */
    int32_t cap_kp;
    uint32_t *desc;                      /* [cap * 8] */
    float *angle;                        /* [cap] */
    int32_t *octave;                     /* [cap] */
    double *bearing;                     /* [cap * 3] */
    uint8_t *usable;                     /* [cap] */
    float *sorted_x, *sorted_y;          /* [cap] */
    int32_t *sorted_idx;                 /* [cap] */
    int32_t *node_id;                    /* [cap] */
    int32_t *node_start;                 /* [cap + 1] */
    int32_t *kp_idx;                     /* [cap] */
} ms_admit_frame;
typedef struct {                         /* HOST outputs, [cap_kp] each, each may be NULL */
    int32_t *kp_track;
    int32_t *word;
    double *weight;
    float *sorted_x, *sorted_y;
    int32_t *sorted_idx;
    int32_t *octave;
    uint32_t *desc;                      /* [cap_kp * 8] */
} ms_admit_host;
int ms_keyframe_admit(ms_ctx *ctx,
    /* HOST struct of DEVICE arrays */
    const ms_keypoints *view, int frame,
    /* DEVICE tables, updated in place */
    int32_t *kf_mp, int n_kf, int stride, int n_mp,
    float *kp_x, float *kp_y, int32_t *kp_octave, float *kp_depth,
    uint32_t *desc_pool, int n_pool, double *kf_pose,
    /* HOST */
    const ms_admit_args *args, const ms_admit_frame *out, const ms_admit_host *host, int32_t *counts);
/* the twin is named _validate: the set of ms_*_check functions is closed at 22 (tests/test_map_checks_corpus.py records them) */
int ms_keyframe_admit_validate(const ms_keypoints *view, int frame,
    const int32_t *kf_mp, int n_kf, int stride, int n_mp,
    const float *kp_x, const float *kp_y, const int32_t *kp_octave, const float *kp_depth,
    const uint32_t *desc_pool, int n_pool, const double *kf_pose,
    const ms_admit_args *args, const ms_admit_frame *out, const ms_admit_host *host, const int32_t *counts, char *why, size_t why_bytes);
/* The descent of the context's latest successful ms_keyframe_admit where it lies: *word (int32) / *weight (float64) are
 * DEVICE arrays of that call's workspace, *n = its n (without a vocabulary word = -1, weight = 0).  The pointers are valid until the
 * next ms_keyframe_admit on that context.  What ms_bow_db_add_words takes: a caller that uses it passes NULL for the admission's host
 * word / weight.  MS_ERR_INVALID (NULL, NULL, 0) before the first admit and after an admit that returned an error. */
int ms_keyframe_admit_words(ms_ctx *ctx, const int32_t **word, const double **weight, int32_t *n);

/* ---- the partial map copy for the front end on the device map tables -------------------------------------------------------
 * copyMap (mapper.cpp:281-326) with copyPartialMapToFrontend: MapDB(mapDB, activeKeyframes) (mapdb.cpp:116-159) and MapPoint(mp,
 * activeKeyframes) (map_point.cpp:22-43).  ms_map_extract gathers the ACTIVE keyframes of a SOURCE set of tables (9.4 - 9.19) into a
 * DESTINATION set, compacted; the source is never written.  tests/map_extract_ref.py restates the call and is its specification.
 *
 * PRESENT and VALID as in 9.18: (uint32)r < n_mp is valid; valid and mp_live[r] != 0 (src->mp_live == NULL: every row is live) is present.
 * `active` [n_active] (HOST) lists source slots; destination slot i is active[i] (the caller passes ascending KfId, the std::set's order; any
 * order is taken).  A source row is ACTIVE iff some entry of an active slot names it and it is present.  Active rows are numbered
 * 0 .. n_rows - 1 in ascending source-row order (the walk of std::set<MpId> activeMapPoints): row_src[d] = the source row of destination
 * row d, row_dst[r] = d, or -1 for a row that is not active.
 * Destination row d < n_rows: mp_pos, mp_norm, mp_min_dist, mp_max_dist, mp_desc, mp_flags and mp_track copied bit for bit; mp_live = 1;
 *   n_obs[d] = the number of valid entries equal to the row in the active slots, with multiplicity (ms_observation_count's definition: the
 *   size of the observation map after map_point.cpp:32-36).  Rows [n_rows, dst->n_mp): mp_live = 0, mp_flags = 0, mp_track = -1, n_obs = 0;
 *   their other fields keep their bytes.
 * Destination slot i < n_active: entry j = row_dst[r] for a present r, else -1 (an entry that is -1, out of range, or valid but not live:
 *   the reference's mapPoints.at would throw on the last kind; here it is dropped and counted).  kp_x, kp_y, kp_octave, kp_depth (all
 *   `stride` entries) and the 12 doubles of kf_pose copied bit for bit.  Slots [n_active, dst->n_kf): every entry -1, the keypoint arrays
 *   0; their poses keep their bytes.  These are empty slots a frame can be admitted into.
 * Tracks (mapdb.cpp:141-145 under the presence rule of 9.11): dst track_row[t] = row_dst[r] where the source has track_row[t] = r, r
 *   present, mp_track[r] == track_base + t and r active; otherwise -1.  Both sides share track_base and n_track.
 * Pool: the n_kp[i] descriptors at desc_base[active[i]] go to dst_desc_base[i], the running sum of the n_kp of the active slots with
 *   desc_base >= 0, in list order; dst_desc_base[i] = -1 for a slot with desc_base < 0, and for every slot without a pool.
 * counts [5]: n_rows, entries kept, valid entries dropped because their row is not live, tracks kept, descriptors copied.
 * Left to the caller, as for ms_map_cull and ms_frame_finish: the previous / next links, referenceKeyframe (map_point.cpp:38-42), the
 * scalar members of mapdb.cpp:150-158, bowIndex and the per-slot host records.  Ordering between contexts is the caller's: the source
 * tables must be quiescent while the call runs (the reference's frontendMapMutex).  The call runs on the stream of `ctx`.
 *
 * Optional arrays: mp_live (source only), mp_track, the four keypoint arrays (all or none), kf_pose, track_row (requires mp_track),
 * desc_pool -- each on both sides or on neither; n_obs, row_src, row_dst of the destination may each be NULL.
 * MS_ERR_INVALID, nothing written, before any device call: an active slot out of range, listed twice or with kf_id < 0; a non-negative
 * kf_id listed twice; n_active > dst->n_kf; n_kp[i] outside [0, stride]; a pool slice outside src->pool_size; the sum of the slices beyond
 * dst->pool_size; track_row without mp_track; an optional array on one side only or only some of the keypoint arrays; a destination pointer
 * equal to its source pointer; descriptor arrays that are not 16-byte aligned; stride < 1, a negative size, a missing array.  MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps (both table
 * sizes; n_track: MS_TRACKED_MAX_WINDOW), and when n_rows > dst->n_mp: then no DEVICE array of the destination
 * is written, while both HOST outputs are: counts holds the needed numbers (all five) and dst_desc_base the pool offsets, neither of which
 * depends on the row capacity -- every verdict is taken before a table is written (the rule of ms_ba_window_apply and ms_frame_finish).
 * n_active == 0 is fine: an empty destination.
 * Per call: one upload block (the list, the keypoint counts, the pool offsets of both sides), at most NINE launches whatever the sizes
 * (fill, mark, count, offsets, place, rows, slots, tracks, pool; the last two only with their arrays), no host wait between them, ONE
 * download (counts) through the context's pinned block.  Every position is a prefix count and every atomic is an integer add: the same
 * tables give the same bytes on every call.  Nothing is allocated after warm-up.
 * ms_map_extract_validate is the host validation alone (no context, no device; `why` receives the message). */
typedef struct {                         /* DEVICE arrays of the source, never written */
    const int32_t *kf_mp;                /* [n_kf * stride] */
    const uint8_t *mp_flags, *mp_live;   /* [n_mp]; mp_live may be NULL */
    const double *mp_pos;                /* [n_mp * 3] */
    const float *mp_norm;                /* [n_mp * 3] */
    const float *mp_min_dist, *mp_max_dist;
    const uint32_t *mp_desc;             /* [n_mp * 8] */
    const int32_t *mp_track;             /* [n_mp], may be NULL */
    const float *kp_x, *kp_y;            /* [n_kf * stride], all four or none */
    const int32_t *kp_octave;
    const float *kp_depth;
    const double *kf_pose;               /* [n_kf * 12], may be NULL */
    const int32_t *track_row;            /* [n_track], may be NULL */
    const uint32_t *desc_pool;           /* [pool_size * 8], may be NULL */
    int32_t n_kf, stride, n_mp, track_base, n_track, pool_size;
} ms_map_extract_src;
typedef struct {                         /* DEVICE arrays of the destination; stride, track_base and n_track are the source's */
    int32_t *kf_mp;                      /* [n_kf * stride] */
    uint8_t *mp_flags, *mp_live;         /* [n_mp] */
    double *mp_pos;
    float *mp_norm;
    float *mp_min_dist, *mp_max_dist;
    uint32_t *mp_desc;
    int32_t *mp_track;
    float *kp_x, *kp_y;
    int32_t *kp_octave;
    float *kp_depth;
    double *kf_pose;
    int32_t *track_row;
    uint32_t *desc_pool;
    int32_t *n_obs;                      /* [n_mp], may be NULL */
    int32_t *row_src;                    /* [n_mp], may be NULL */
    int32_t *row_dst;                    /* [src->n_mp], may be NULL */
    int32_t n_kf, n_mp, pool_size;       /* slots >= n_active, row capacity, pool capacity in descriptors */
} ms_map_extract_dst;
int ms_map_extract(ms_ctx *ctx,
    /* HOST structs of DEVICE arrays */
    const ms_map_extract_src *src, const ms_map_extract_dst *dst,
    /* HOST: kf_id [src->n_kf], active [n_active]; with a pool desc_base [src->n_kf] and n_kp [n_active] */
    const int32_t *kf_id, const int32_t *active, int n_active, const int32_t *desc_base, const int32_t *n_kp,
    /* HOST outputs: dst_desc_base [n_active], counts [5] */
    int32_t *dst_desc_base, int32_t *counts);
/* the twin is named _validate: the set of ms_*_check functions is closed at 22 (tests/test_map_checks_corpus.py records them) */
int ms_map_extract_validate(const ms_map_extract_src *src, const ms_map_extract_dst *dst,
    const int32_t *kf_id, const int32_t *active, int n_active, const int32_t *desc_base, const int32_t *n_kp,
    const int32_t *dst_desc_base, const int32_t *counts, char *why, size_t why_bytes);

/* ---- a frame of tracker features to the map tables --------------------------------------------------------------------------
 * Keyframe::addTrackerFeatures / processKeyPoints (keyframe.cpp:34-69, :118-133, called at mapper_helpers.cpp:1196) without table rows going
 * up piece by piece: the arrival of a frame that did not go through the extractor -- every front-end frame (isBackend is false,
 * mapper_helpers.cpp:1186-1197) and every back-end frame that is no keyframe.  ms_frame_admit puts the HOST list of tracker features
 * (points[0].x, points[0].y, id, depth) into slot `slot` of the tables of 9.4 - 9.21; after it the frame is ms_match_tracked,
 * ms_pose_tables_solve and ms_frame_finish with no table upload in between.  tests/frame_admit_ref.py restates the call and is its
 * specification.
 *
 * Kept: feature i is KEPT iff (keep == NULL || keep[i] != 0) and the mask rule holds.  keep is the host's evaluation of
 * tracker::Camera::isValidPixel (keyframe.cpp:122), the exact form.  The mask rule: valid_mask == NULL, or the rounded position
 * (__float2int_rn(x), __float2int_rn(y)) lies inside the raster and its byte is non-zero (ms_orb_set_valid_mask's rule; a position outside the
 * raster is invalid).  Keypoint k is the k-th kept feature in ascending i; n_kp, the number kept, is decided ON THE DEVICE.
 * Written for k < n_kp, at entry slot * stride + k: kp_x, kp_y = the feature's bits; kp_octave = 0 (keyframe.cpp:127); kp_depth
 *   (keyframe.cpp:57-64) = depth[i] of the feature itself, or, iff that is < 0 as written (a NaN stays), the sample of depth_image at the
 *   rounded position -- ms_keyframe_admit's expression, the image being the same stand-in for frame->getDepth -- or -1 outside the image or
 *   with no image.  Entries k >= n_kp of the keypoint table keep their bytes.
 * Written per slot: kf_mp[slot * stride + j] = -1 for ALL stride entries; kf_pose[slot] = pose (it travels as a kernel argument).
 * HOST outputs, one download through the context's pinned block: kp_track[k] = id[i], what ms_match_tracked takes as kp_track next;
 * kp_feature[k] = i.  counts (HOST [4]) = n_kp, the features dropped by keep, those dropped by the mask alone, the kept features whose
 * depth was taken from the image (depth[i] < 0 and the rounded position inside a given image).
 * One deliberate deviation: keyframe.cpp:129 binds the id to KpId(i), the FEATURE index, so that after a dropped feature every later id sits
 * on the wrong keypoint or on none; this call binds the k-th kept feature's id and depth to keypoint k.  Equal whenever nothing is dropped
 * (DESIGN section 3).
 *
 * Every verdict is taken before any write (the rule of ms_keyframe_admit and ms_ba_window_apply): MS_ERR_CAPACITY with the needed n_kp in
 * counts[0] when n_kp > stride or n_kp > cap_kp; MS_ERR_INVALID when the slot's row already holds a VALID entry ((uint32)r < n_mp,
 * keyframe.cpp:275).  In both cases every table keeps its bytes.  Before any device call (ms_frame_admit_validate, the host validation
 * alone: no context, no device; `why` receives the message): MS_ERR_INVALID for a slot out of range, a non-finite x or y, an id < 0 (it
 * would read as "no track" downstream), an id listed twice (ms_match_tracked refuses such a frame; the reference lets the last feature win,
 * keyframe.cpp:51-53), a non-finite pose, an image or a mask without a size, stride < 1, a negative size, a missing array;
 * MS_ERR_CAPACITY beyond the MS_COVIS_MAX_* caps (n_tracks and cap_kp: MS_COVIS_MAX_STRIDE; an image or a mask of 2^31 elements or more).
 * n_tracks == 0 is fine: the row is cleared and the pose is written.
 * TWO launches whatever the sizes (ranks and verdicts in one workgroup; every write), at most one upload block (the features, through the
 * context's staging; none with n_tracks == 0), ONE download, one host wait behind the last launch.  The workspace belongs to the context
 * and only grows: nothing is allocated after warm-up (ms_debug_host_allocs).  No atomics; positions are prefix counts: the same inputs
 * give the same bytes on every call.
 * Not covered: colours (getPixel), a device-resident kp_track for ms_match_tracked, several frames per call. */
typedef struct {
    int32_t slot;                        /* the frame's slot in kf_mp, the keypoint table and kf_pose */
    double pose[12];                     /* rows 0-2 of poseCW, row-major (insertNewKeyframeCandidate's result: the host computes it) */
    const float *depth_image;            /* DEVICE float32, may be NULL: the stand-in for frame->getDepth, as in ms_keyframe_admit */
    int32_t depth_width, depth_height, depth_stride;     /* row stride in elements */
    const uint8_t *valid_mask;           /* DEVICE bytes, 0 = invalid, may be NULL: the raster stand-in for isValidPixel */
    int32_t mask_width, mask_height, mask_stride;        /* row stride in bytes */
} ms_frame_admit_args;
int ms_frame_admit(ms_ctx *ctx,
    /* DEVICE tables, updated in place */
    int32_t *kf_mp, int n_kf, int stride, int n_mp,
    float *kp_x, float *kp_y, int32_t *kp_octave, float *kp_depth, double *kf_pose,
    /* HOST: the tracker features [n_tracks]; keep may be NULL */
    const float *x, const float *y, const int32_t *id, const float *depth, const uint8_t *keep, int n_tracks,
    const ms_frame_admit_args *args,
    /* HOST outputs, [cap_kp] each, each may be NULL; counts [4] */
    int32_t *kp_track, int32_t *kp_feature, int cap_kp, int32_t *counts);
/* the twin is named _validate: the set of ms_*_check functions is closed at 22 (tests/test_map_checks_corpus.py records them) */
int ms_frame_admit_validate(const int32_t *kf_mp, int n_kf, int stride, int n_mp,
    const float *kp_x, const float *kp_y, const int32_t *kp_octave, const float *kp_depth, const double *kf_pose,
    const float *x, const float *y, const int32_t *id, const float *depth, const uint8_t *keep, int n_tracks,
    const ms_frame_admit_args *args,
    const int32_t *kp_track, const int32_t *kp_feature, int cap_kp, const int32_t *counts, char *why, size_t why_bytes);

/* ---- the viewer map and the point-cloud record on the device map tables ------------------------------------------------------
 * The last two steps of addKeyframeCommonInner, the only ones that hand the map to someone outside the mapper: publishMapForViewer
 * (mapper_helpers.cpp:814-879, called at :1117 and :1129) and updatePointCloudRecording (:881-909, called at :1125, the recorder behind
 * pointCloudSavePath).  Both walk every MapPoint once per keyframe; ms_map_publish is that walk as one pass over the rows of the tables of
 * 9.5 - 9.22, and the record comes down as the CHANGES since the last call.  tests/map_publish_ref.py restates the call and is its
 * specification.  Row r is PRESENT iff (uint32)r < n_mp and mp_live[r] != 0; an entry is VALID iff (uint32)r < n_mp; bits 0-1 of mp_flags are
 * 3 = TRIANGULATED, 2 = UNSURE, 0 = NOT_TRIANGULATED.  MapPointStatus::BAD cannot be seen in a map: map_point.cpp:154 sets it on the line
 * before the erase, so no present row carries it.
 *
 * View (:823-839), with MS_PUBLISH_VIEW.  Row r is PUBLISHED iff it is PRESENT and mp_flags[r] & 3 (:830).  The k-th published row in
 * ascending row order -- row order stands in for the std::map<MpId> walk, as in ms_map_point_union -- gives pub_row[k] = r; pub_pos[3k ..] =
 * (float)mp_pos[r], round to nearest even (cast<float>()); pub_norm[3k ..] = mp_norm[r] bit for bit; pub_color[3k ..] = (float)c / 255.0f, a
 * float division per channel (0 with mp_color == NULL); pub_status[k] = int(MapPointStatus): 0 when bit 0 is set, 2 otherwise; pub_bits[k]
 * bit 0 = localMap: r is among the VALID entries of local_rows (workspaceBA.localMpIds as rows, e.g. the rows of the last
 * ms_ba_window_lists; any order, repeats allowed, an entry that is not VALID is ignored); bit 1 = nowVisible: r is a VALID entry among all
 * `stride` entries of current_slot (visibleIds, :823-826).
 *
 * Record (:881-909), with MS_PUBLISH_RECORD, on the caller's record state rec_pos (float [3 n_mp]) / rec_state (uint8 [n_mp]: 0 never
 * recorded, 1 recorded, 2 removed), DEVICE arrays that start as zero bytes and that the caller extends with zeros when n_mp grows.  n_obs are
 * the whole-map counts of ms_observation_count, which the chain keeps current.  For every row in ascending order, p = (float)mp_pos[r]:
 *   1. PRESENT, n_obs[r] >= min_record_obs, state 0 or 2: event NEW (1) with p and the normal; state = 1, rec_pos = p.  (State 2 on a present
 *      row: the table reused the row for a new map point.  The reference never reuses an id; on tables that never reuse rows this is never taken.)
 *   2. PRESENT, n_obs[r] >= min_record_obs, state 1: if rec_pos differs from p as Eigen's != compares -- by float value per component, so
 *      -0.0f equals 0.0f and a NaN always differs -- event MOVED (2) with p and the normal, rec_pos = p; otherwise nothing.
 *   3. PRESENT with fewer observations: nothing, whatever its state (:889).
 *   4. not PRESENT, state 1: event REMOVED (3) with position 0, 0, 0 (:902-907) and a zero normal; state = 2, rec_pos keeps its bytes.
 * Events come out in ascending row order as ev_row, ev_kind, ev_pos[3], ev_norm[3]: the reference's two loops write disjoint records, so one
 * ordered stream carries the same information.
 *
 * Keyframes (:854): for i < n_list, pose_wc[16 i ..] = the rigid inverse of kf_pose[kf_list[i]] as a row-major 4 x 4 float matrix: R^T | -R^T t
 * in float64, -((R0j*t0 + R1j*t1) + R2j*t2) with no contraction, then cast to float; the last row is 0 0 0 1.  The reference takes Eigen's
 * general 4 x 4 inverse; for rigid poses the float results agree to one unit in the last place.
 *
 * counts (HOST [8]) = n_pub, n_ev, the NEW, MOVED and REMOVED events, the published rows with localMap, those with nowVisible, the present
 * rows skipped as NOT_TRIANGULATED.  Every verdict is taken before any write (the rule of ms_frame_finish and ms_ba_window_apply):
 * MS_ERR_CAPACITY when n_pub > cap_pub or n_ev > cap_ev; then no output array is written, rec_pos and rec_state keep their bytes, and counts
 * holds the needed numbers.  Nothing behind n_pub / n_ev is written.  Before any device call (ms_map_publish_validate, the host validation
 * alone: no context, no device; `why` receives the message): MS_ERR_INVALID for `what` outside 1 .. 3, current_slot outside [-1, n_kf), a
 * kf_list slot out of range or listed twice, min_record_obs < 0, stride < 1, a negative size or capacity, a missing array for the chosen
 * `what` (n_obs / rec_* with RECORD, an output array with a non-zero capacity, local_rows with n_local > 0); MS_ERR_CAPACITY beyond the
 * MS_COVIS_MAX_* caps (n_local: below MS_COVIS_MAX_MP; n_list: MS_COVIS_MAX_KF).  n_mp == 0, n_list == 0, n_local == 0 and current_slot ==
 * -1 are fine; with n_mp == 0 and n_list == 0 nothing is launched.
 * FIVE launches whatever the sizes (clear the two mark bitmaps and write pose_wc; mark, the only atomics ORing bits into bitmap words; count
 * per workgroup; one workgroup's block_offsets over both streams with the verdict and the head; pack, recomputing the predicates), no host
 * wait between them; at most one upload block (kf_list); TWO downloads through the context's pinned block: the head with pose_wc, then
 * exactly the bytes that n_pub and n_ev name (none when both are 0).  That is one copy more than ms_frame_finish: the caps are the size of
 * the map and the answer usually is not, so one download sized by the caps would move the whole map for a handful of events.  Integer
 * arithmetic decides every position: the same tables give the same bytes on every call, at any capacity.  The workspace only grows;
 * nothing is allocated after warm-up (ms_debug_host_allocs). */
#define MS_PUBLISH_VIEW 1
#define MS_PUBLISH_RECORD 2
typedef struct {
    int32_t what;                        /* MS_PUBLISH_VIEW | MS_PUBLISH_RECORD; 0 is invalid */
    int32_t current_slot;                /* the slot with the largest KfId (mapDB.keyframes.rbegin()), -1 for none */
    int32_t min_record_obs;              /* the 4 of :889 */
} ms_map_publish_args;
int ms_map_publish(ms_ctx *ctx,
    /* DEVICE tables, read; n_obs may be NULL without MS_PUBLISH_RECORD, mp_color may be NULL */
    const double *mp_pos, const float *mp_norm, const uint8_t *mp_flags, const uint8_t *mp_live,
    const int32_t *n_obs, const uint8_t *mp_color, int n_mp,
    const int32_t *kf_mp, int n_kf, int stride, const double *kf_pose,
    const int32_t *local_rows, int n_local,
    /* DEVICE, updated in place: the record state; each may be NULL without MS_PUBLISH_RECORD */
    float *rec_pos, uint8_t *rec_state,
    /* HOST */
    const ms_map_publish_args *args, const int32_t *kf_list, int n_list,
    /* HOST outputs: pub_* [cap_pub], ev_* [cap_ev], pose_wc [16 n_list], counts [8] */
    int32_t *pub_row, float *pub_pos, float *pub_norm, float *pub_color, uint8_t *pub_status, uint8_t *pub_bits, int cap_pub,
    int32_t *ev_row, uint8_t *ev_kind, float *ev_pos, float *ev_norm, int cap_ev,
    float *pose_wc, int32_t *counts);
/* the twin is named _validate: the set of ms_*_check functions is closed at 22 (tests/test_map_checks_corpus.py records them) */
int ms_map_publish_validate(const double *mp_pos, const float *mp_norm, const uint8_t *mp_flags, const uint8_t *mp_live,
    const int32_t *n_obs, const uint8_t *mp_color, int n_mp,
    const int32_t *kf_mp, int n_kf, int stride, const double *kf_pose,
    const int32_t *local_rows, int n_local,
    const float *rec_pos, const uint8_t *rec_state,
    const ms_map_publish_args *args, const int32_t *kf_list, int n_list,
    const int32_t *pub_row, const float *pub_pos, const float *pub_norm, const float *pub_color, const uint8_t *pub_status, const uint8_t *pub_bits, int cap_pub,
    const int32_t *ev_row, const uint8_t *ev_kind, const float *ev_pos, const float *ev_norm, int cap_ev,
    const float *pose_wc, const int32_t *counts, char *why, size_t why_bytes);

#ifdef __cplusplus
}
#endif
#endif /* MI355SLAM_H */
