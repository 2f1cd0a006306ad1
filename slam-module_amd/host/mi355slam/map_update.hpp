// map_update.hpp -- the operations of the host mirror on the device-resident map (map_tables.hpp), with their argument and result structs:
// loop correction (correctLoop), triangulation (triangulateMapPoints), covisibility (getNeighbors, computeAdjacentKeyframes, localMapPoints),
// culling (observationCounts, cullMap), the observation-list passes (updateMapPoints, retriangulateCurrent), matchTrackedFeatures and the
// fusing of duplicate map points (deduplicateMapPoints, searchAndDeduplicate, mergeMatchedMapPoints), matchLocalMapPoints, createNewMapPoints and the local
// bundle adjustment whose window is gathered from the tables and written back into them (localBundleAdjustOnTables), the per-frame pose
// adjustment (poseBundleAdjustOnTables), the end of a frame (finishFrame, removeKeyframes), the arrival of a frame of tracker features
// (admitTrackerFrame, with makeKeyframeDecision in front of it), the arrival of a keyframe from the extractor's device output (admitKeyframe)
// and the map copy for the front end (extractMap, copyMapToFrontend), and the map as it leaves the mapper (publishMapForViewer,
// updatePointCloudRecording).
// Results come back through Context::workspace and Context::download; nothing here owns device memory but the two row maps of a MapExtract
// and the record state of a DeviceMapPointRecords.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <functional>
#include <limits>
#include <map>
#include <stdexcept>
#include "bow_index.hpp"
#include "bundle_adjuster.hpp"
#include "keyframe_matcher.hpp"
#include "map_tables.hpp"
#include "optimize_transform.hpp"

namespace mi355slam {

// The keyframes LoopCloser::correctLoop moves (loop_closer.cpp:420-470), as slots of DeviceKeyframePoses: rigid = a member of
// rigidlyTransformedKfIds (:427, T itself), otherwise lambda = (t - t0) / (t1 - t0) of :458.
struct LoopCorrections {
    std::vector<std::int32_t> slot;
    std::vector<std::uint8_t> rigid;
    std::vector<double> lambda;
};
// localMapPoints (:418, :429-433, :465-469) as table rows: row[j] moves with the keyframe at position reference[j] of LoopCorrections::slot.
struct LoopPoints {
    std::vector<std::int32_t> row, reference;
};
// What DeviceMapPoints::refresh takes for the moved points (:504-505).
struct RefreshArgs {
    std::vector<std::int32_t> rows;
    std::vector<std::vector<MapObservation>> observations;
    std::vector<std::int32_t> firstOctave;
    const DeviceDescriptorPool *pool = nullptr;
};

// LoopCloser::correctLoop from the pose correction to the refresh of the moved map points (loop_closer.cpp:398-506) on the device tables:
// ms_loop_correct (poses, then points), then DeviceMapPoints::refresh of refreshArgs.rows.  T = the Sim3 of :405.  Re-triangulation (:508-523)
// stays with the caller.  Returns refresh's medoids.
inline std::vector<int> correctLoop(Context &ctx, DeviceMapPoints &points, DeviceKeyframePoses &poses, const Sim3 &T, const LoopCorrections &corrections,
                                    const LoopPoints &moved, const RefreshArgs &refreshArgs, const StaticSettings &settings) {
    if (corrections.rigid.size() != corrections.slot.size() || corrections.lambda.size() != corrections.slot.size() || moved.reference.size() != moved.row.size())
        throw std::invalid_argument("correctLoop: the correction lists have different lengths");
    const double t8[8] = {T.q[0], T.q[1], T.q[2], T.q[3], T.t[0], T.t[1], T.t[2], T.s};
    ctx.check(ms_loop_correct(ctx.get(), poses.pose(), (int)poses.size(), points.mutablePosition(), (int)points.size(), t8, corrections.slot.data(),
                              corrections.rigid.data(), corrections.lambda.data(), (int)corrections.slot.size(), moved.row.data(), moved.reference.data(),
                              (int)moved.row.size()), "ms_loop_correct");
    return points.refresh(ctx, poses, refreshArgs.rows, refreshArgs.observations, refreshArgs.firstOctave, settings, refreshArgs.pool);
}

// ---- the map-point triangulator (ms_triangulate) ------------------------------------------------------------------------------------
// TriangulationMethod of mapper_helpers.hpp plus the first / last variant (triangulateMapPointFirstLastObs).
enum class TriangulationMethod { TME = MS_TRI_TME, MIDPOINT = MS_TRI_MIDPOINT, FIRST_LAST = MS_TRI_FIRST_LAST };
namespace detail {
inline ms_tri_settings tri_settings(const StaticSettings &settings) {
    const Parameters &p = settings.parameters;
    return ms_tri_settings{settings.levelSigmaSq.data(), (std::int32_t)settings.levelSigmaSq.size(), p.minTriangulationAngleTwoObs, p.minTriangulationAngleMultipleObs,
                           p.relativeReprojectionErrorThreshold, p.computeDenseStereoDepth ? 1 : 0};
}
}  // namespace detail
// The map points to triangulate and MapPoint::observations of each, flattened in the reference's iteration order (ascending KfId):
// row r's observations are [obsStart[r], obsStart[r + 1]); obsKf = the keyframe's slot, obsX / obsY / obsOctave = kp.pt and kp.octave,
// obsDepth = keyPointDepth (empty: no depth anywhere); wasTriangulated = status != NOT_TRIANGULATED on entry (mapper_helpers.cpp:607).
struct TriangulateArgs {
    std::vector<std::int32_t> rows;
    std::vector<std::uint8_t> wasTriangulated;
    std::vector<std::int32_t> obsStart, obsKf, obsOctave;
    std::vector<float> obsX, obsY, obsDepth;
};
// Per entry of TriangulateArgs::rows: status (0 NOT_TRIANGULATED, 1 UNSURE, 2 TRIANGULATED), the first gate that stopped the point (the reason
// codes of ms_triangulate) and nNew of triangulateMapPointFirstLastObs.
struct TriangulateResult {
    std::vector<std::uint8_t> status, reason;
    std::vector<std::int32_t> passCount;
};

// triangulateMapPoint / triangulateMapPointFirstLastObs (mapper_helpers.cpp:600-812) for args.rows, on the device: positions are written into
// `points`, the status flags (DeviceMapPointFlags encoding) into `flags` when given; slots.camera / slots.focalLength per slot of `poses`.  The
// debug counters of loop_closer.cpp:516-521 follow from the result and the entry state: `failed` = the entry status was TRIANGULATED and
// status != 2; `changed` (a comparison of position values in the reference) = the position was written: status != 0, or the depth branch of
// :621 ran (not wasTriangulated, a positive depth, reason != 1).
inline TriangulateResult triangulateMapPoints(Context &ctx, DeviceMapPoints &points, DeviceMapPointFlags *flags, const DeviceKeyframePoses &poses,
                                              const KeyframeSlots &slots, const TriangulateArgs &args, const StaticSettings &settings, TriangulationMethod method) {
    const std::size_t n = args.rows.size();
    if (args.wasTriangulated.size() != n || args.obsStart.size() != n + 1) throw std::invalid_argument("triangulateMapPoints: one flag and one list per row");
    const std::size_t nObs = (std::size_t)std::max<std::int32_t>(args.obsStart.back(), 0);
    if (args.obsKf.size() < nObs || args.obsOctave.size() < nObs || args.obsX.size() < nObs || args.obsY.size() < nObs || (!args.obsDepth.empty() && args.obsDepth.size() < nObs))
        throw std::invalid_argument("triangulateMapPoints: the observation arrays are shorter than obsStart says");
    if (slots.camera.size() != poses.size() || slots.focalLength.size() != poses.size()) throw std::invalid_argument("triangulateMapPoints: one camera per keyframe slot");
    if (flags && flags->size() < points.size()) throw std::invalid_argument("triangulateMapPoints: fewer flags than map points");
    const ms_tri_settings s = detail::tri_settings(settings);
    TriangulateResult out;
    out.status.assign(n, 0); out.reason.assign(n, 0); out.passCount.assign(n, 0);
    ctx.check(ms_triangulate(ctx.get(), points.mutablePosition(), flags ? flags->mutableFlags() : nullptr, (int)points.size(), poses.pose(), (int)poses.size(),
                             slots.camera.data(), slots.focalLength.data(), args.rows.data(), args.wasTriangulated.data(), (int)n, args.obsStart.data(), args.obsKf.data(),
                             args.obsX.data(), args.obsY.data(), args.obsOctave.data(), args.obsDepth.empty() ? nullptr : args.obsDepth.data(), &s, (int)method,
                             out.status.data(), out.reason.data(), out.passCount.data()), "ms_triangulate");
    return out;
}

// ---- set queries over the map graph (ms_covisibility, ms_map_point_union) ---------------------------------------------------------
// One call of Keyframe::getNeighbors (keyframe.cpp:192-230): the keyframe's slot, its previousKfId / nextKfId as slots (-1 for none).
struct NeighborQuery {
    std::int32_t slot = 0, previous = -1, next = -1;
    int minCovisibilities = 1;
    bool triangulatedOnly = false;
};

// getNeighbors for every query in one device call: per query the neighbour slots, ascending (the order of the reference's std::map walk).
inline std::vector<std::vector<std::int32_t>> getNeighbors(Context &ctx, const DeviceKeyframeMapPoints &keyframes, const DeviceMapPointFlags *flags,
                                                           const std::vector<NeighborQuery> &queries) {
    std::vector<std::vector<std::int32_t>> out(queries.size());
    if (queries.empty()) return out;
    if (flags && flags->size() < keyframes.mapPointCount()) throw std::invalid_argument("getNeighbors: fewer flags than map points");
    std::vector<ms_covis_query> q(queries.size());
    for (std::size_t i = 0; i < queries.size(); ++i)
        q[i] = ms_covis_query{queries[i].slot, queries[i].previous, queries[i].next, (std::int32_t)queries[i].minCovisibilities,
                              (std::uint8_t)(queries[i].triangulatedOnly ? DeviceMapPointFlags::TRIANGULATED : 0)};
    const std::size_t nKf = keyframes.size(), bytes = 4 * queries.size() * nKf;
    std::int32_t *packed = reinterpret_cast<std::int32_t *>(ctx.workspace(bytes));
    std::vector<std::int32_t> n(queries.size(), 0);
    ctx.check(ms_covisibility(ctx.get(), keyframes.table(), (int)nKf, (int)keyframes.stride(), flags ? flags->flags() : nullptr, (int)keyframes.mapPointCount(), q.data(),
                              (int)q.size(), nullptr, packed, n.data()), "ms_covisibility");
    std::vector<std::int32_t> host(queries.size() * nKf);
    ctx.check(ms_dev_download(ctx.get(), host.data(), packed, bytes), "ms_dev_download");
    for (std::size_t i = 0; i < queries.size(); ++i) out[i].assign(host.begin() + i * nKf, host.begin() + i * nKf + n[i]);
    return out;
}

// computeAdjacentKeyframes (mapper_helpers.cpp:144-229): the getNeighbors calls of every second keyframe of the chain behind `current`
// (:160-176) are ONE ms_covisibility call; the chain walks from the parents and the squared-distance sort (:178-216) stay on the host, on the
// links and camera centres of M.slots.  Writes nothing.
inline std::vector<std::int32_t> computeAdjacentKeyframes(Context &ctx, MapTables M, std::int32_t current, int minCovisibilities, int maxKeyframes) {
    M.require("computeAdjacentKeyframes", M.LINKS | M.CENTRES);
    const KeyframeSlots &chain = M.slots;
    const std::size_t nKf = M.keyframes.size();
    auto inTable = [&](std::int32_t s) { return s >= 0 && (std::size_t)s < nKf; };
    if (!inTable(current)) throw std::invalid_argument("computeAdjacentKeyframes: current keyframe outside the table");
    std::vector<char> adjacentSet(nKf, 0);          // std::set<KfId> over slots: walked in ascending order below
    std::vector<NeighborQuery> queries;
    int i = 0;
    for (std::int32_t backwards = current; backwards != -1; backwards = chain.previous[backwards]) {
        if (!inTable(backwards)) throw std::invalid_argument("computeAdjacentKeyframes: a link leaves the table");
        adjacentSet[backwards] = 1;
        if (i % 2 == 0) queries.push_back({backwards, chain.previous[backwards], chain.next[backwards], minCovisibilities, false});
        if (++i >= maxKeyframes) break;
    }
    std::vector<char> parents(nKf, 0);
    for (const std::vector<std::int32_t> &nb : getNeighbors(ctx, M.keyframes, M.flags, queries))
        for (std::int32_t k : nb) parents[k] = 1;
    for (std::size_t parent = 0; parent < parents.size(); ++parent) {
        if (!parents[parent]) continue;
        for (const std::vector<std::int32_t> *link : {&chain.previous, &chain.next}) {
            i = 0;
            for (std::int32_t at = (std::int32_t)parent; at != -1; at = (*link)[at]) {
                if (!inTable(at)) throw std::invalid_argument("computeAdjacentKeyframes: a link leaves the table");
                adjacentSet[at] = 1;
                if (++i >= maxKeyframes / 2) break;
            }
        }
    }
    adjacentSet[current] = 0;
    std::vector<std::int32_t> adjacent;
    for (std::size_t k = 0; k < adjacentSet.size(); ++k) if (adjacentSet[k]) adjacent.push_back((std::int32_t)k);
    const std::array<double, 3> &c = chain.cameraCenter[current];
    auto dist2 = [&](std::int32_t k) {                       // squaredNorm of a 3-vector, Eigen's unrolled redux: x^2 + (y^2 + z^2)
        const std::array<double, 3> &p = chain.cameraCenter[k];
        const double x = p[0] - c[0], y = p[1] - c[1], z = p[2] - c[2];
        return x * x + (y * y + z * z);
    };
    std::sort(adjacent.begin(), adjacent.end(), [&](std::int32_t a, std::int32_t b) { return dist2(a) < dist2(b); });
    if ((int)adjacent.size() > maxKeyframes) adjacent.erase(adjacent.begin() + maxKeyframes, adjacent.end());
    return adjacent;
}

// The ordered union of the map points of a list of keyframes: rows ascending (the std::set / std::map walk) and, for each, the first
// position of the list whose keyframe lists it (localMapPoints.emplace of loop_closer.cpp:430-432) -- LoopPoints as it stands.
//   matchLocalMapPoints (mapper_helpers.cpp:241-261)   localMapPoints(ctx, keyframes, &flags, adjacentSlots, currentSlot, DeviceMapPointFlags::USABLE).row
//                                                      is GateView::indices of the SEARCH view that matchLocalMapPoints (below) gates, scores
//                                                      and binds on the device (searchByProjectionOnTables)
//   deduplicateMapPoints (:337-345), searchAndDeduplicate (loop_closer.cpp:569-584)   exclude = -1, require = 0
//   correctLoop (:418-433, :465-469)                   slots = LoopCorrections::slot; the result is its LoopPoints
inline LoopPoints localMapPoints(Context &ctx, const DeviceKeyframeMapPoints &keyframes, const DeviceMapPointFlags *flags, const std::vector<std::int32_t> &slots,
                                 std::int32_t excludeSlot = -1, std::uint8_t require = 0, bool withOwner = true) {
    LoopPoints out;
    const std::size_t nMp = keyframes.mapPointCount();
    if (flags && flags->size() < nMp) throw std::invalid_argument("localMapPoints: fewer flags than map points");
    const ms_union_problem problem{0, (std::int32_t)slots.size(), excludeSlot, require};
    std::int32_t *rows = reinterpret_cast<std::int32_t *>(ctx.workspace(8 * nMp + 256)), *owner = rows + (nMp + 63) / 64 * 64;
    std::int32_t n = 0;
    ctx.check(ms_map_point_union(ctx.get(), keyframes.table(), (int)keyframes.size(), (int)keyframes.stride(), flags ? flags->flags() : nullptr, (int)nMp, slots.data(),
                                 (int)slots.size(), &problem, 1, rows, withOwner ? owner : nullptr, &n), "ms_map_point_union");
    out.row = ctx.download(rows, (std::size_t)n);
    if (withOwner) out.reference = ctx.download(owner, (std::size_t)n);
    return out;
}

// ---- observation counts and culling on the map tables (ms_observation_count, ms_map_cull) -----------------------------------------
// Per table row: mp.observations.size(), getFirstObservation() and getLastObservation() as slots (-1 for a row nobody observes).
struct ObservationCounts {
    std::vector<std::int32_t> count, first, last;
};

// The transpose of the keyframe table, computed where it lies: what the status promotion of mapper_helpers.cpp:1072 and the row selection of
// :1088 read, without a std::map of observations per point on the host.  kfIds: per slot the KfId, -1 for an empty slot.
inline ObservationCounts observationCounts(Context &ctx, const DeviceKeyframeMapPoints &keyframes, const std::vector<std::int32_t> &kfIds) {
    if (kfIds.size() != keyframes.size()) throw std::invalid_argument("observationCounts: one KfId per slot");
    const std::size_t nMp = keyframes.mapPointCount(), pitch = (nMp + 63) / 64 * 64;
    std::int32_t *dev = reinterpret_cast<std::int32_t *>(ctx.workspace(12 * pitch + 256));
    ctx.check(ms_observation_count(ctx.get(), keyframes.table(), (int)keyframes.size(), (int)keyframes.stride(), (int)nMp, kfIds.data(), dev, dev + pitch, dev + 2 * pitch),
              "ms_observation_count");
    ObservationCounts out;
    out.count = ctx.download(dev, nMp); out.first = ctx.download(dev + pitch, nMp); out.last = ctx.download(dev + 2 * pitch, nMp);
    return out;
}

// The three ParametersSlam fields the culling step reads.  Their types are not in the reference tree: ratioFloat32 says whether
// keyframeCullMaxCriticalRatio is a float there (the product of :476 is then rounded to float32); see INTEGRATION.md.
struct CullSettings {
    double minMapPointCullingAge = 0.0;
    int minObservationsForBA = 0;
    double keyframeCullMaxCriticalRatio = 0.0;
    bool cullPoints = true;             // false: cullKeyframes alone
    bool ratioFloat32 = false;
};

// What the host side of the map still has to do after a cull: the removed rows (ascending) with the reason of each (1 no observation left,
// 2 aged and not triangulated, 3 orphaned by a removed keyframe) -- trackIdToMapPoint.erase and the host copies of those points -- and the
// removed keyframes as slots, in the order of removal (descending KfId) -- bowIndex->remove, the `uncertainty` accumulation onto the next
// keyframe and re-pointing referenceKeyframe to the previous one (mapper_helpers.cpp:384, :408-426), with the links as they were before.
struct CullResult {
    std::vector<std::int32_t> removedRows;
    std::vector<std::uint8_t> removedWhy;
    std::vector<std::int32_t> removedKeyframes, removedPrevious, removedNext;
};

// cullMapPoints + cullKeyframes (mapper_helpers.cpp:1095-1096) in ONE device call on the tables in place: writes M.keyframes, M.flags and
// M.live.  `current` and adjacentKfIds / loopClosureKeyframes are slots; a candidate without a previous keyframe (:453) or named by a
// loop-closure edge (:455-464) is kept.  The previous / next links of M.slots are relinked as removeKeyframe does (:414-420) and a removed
// slot's id becomes -1.
inline CullResult cullMap(Context &ctx, MapTables M, std::int32_t current, const std::vector<std::int32_t> &adjacentKfIds, const std::vector<std::int32_t> &loopClosureKeyframes,
                          const CullSettings &settings) {
    M.require("cullMap", M.LIVE | M.LINKS | M.IDS | M.TIMES | (settings.cullPoints ? M.FLAGS : 0u));
    KeyframeSlots &chain = M.slots;
    const std::size_t nKf = M.keyframes.size(), nMp = M.keyframes.mapPointCount();
    std::vector<std::uint8_t> keep(adjacentKfIds.size(), 0), removed(adjacentKfIds.size(), 0);
    for (std::size_t i = 0; i < adjacentKfIds.size(); ++i) {
        const std::int32_t k = adjacentKfIds[i];
        if (k < 0 || (std::size_t)k >= nKf) throw std::invalid_argument("cullMap: adjacent keyframe outside the table");
        keep[i] = chain.previous[k] < 0 || std::find(loopClosureKeyframes.begin(), loopClosureKeyframes.end(), k) != loopClosureKeyframes.end();
    }
    const ms_cull_settings s{current, settings.cullPoints ? 1 : 0, settings.minMapPointCullingAge, (std::int32_t)settings.minObservationsForBA,
                             settings.keyframeCullMaxCriticalRatio, settings.ratioFloat32 ? 1 : 0};
    const std::size_t pitch = (nMp + 63) / 64 * 64;
    std::int32_t *rows = reinterpret_cast<std::int32_t *>(ctx.workspace(5 * pitch + 256));
    std::uint8_t *why = reinterpret_cast<std::uint8_t *>(rows + pitch);
    std::int32_t nRows = 0, nKfs = 0;
    ctx.check(ms_map_cull(ctx.get(), M.keyframes.mutableTable(), (int)nKf, (int)M.keyframes.stride(), M.flags ? M.flags->mutableFlags() : nullptr, M.live->mutableLive(), (int)nMp,
                          chain.id.data(), chain.t.data(), adjacentKfIds.data(), keep.data(), (int)adjacentKfIds.size(), &s, nullptr, rows, why, removed.data(), &nRows, &nKfs), "ms_map_cull");
    CullResult out;
    out.removedRows = ctx.download(rows, (std::size_t)nRows); out.removedWhy = ctx.download(why, (std::size_t)nRows);
    for (std::size_t i = 0; i < adjacentKfIds.size(); ++i) if (removed[i]) out.removedKeyframes.push_back(adjacentKfIds[i]);
    std::sort(out.removedKeyframes.begin(), out.removedKeyframes.end(), [&](std::int32_t a, std::int32_t b) { return chain.id[a] > chain.id[b]; });
    for (std::int32_t k : out.removedKeyframes) {            // :414-420, in the order of removal
        const std::int32_t prev = chain.previous[k], next = chain.next[k];
        out.removedPrevious.push_back(prev); out.removedNext.push_back(next);
        if (next != -1) chain.previous[next] = prev;
        if (prev != -1) chain.next[prev] = next;
        chain.previous[k] = chain.next[k] = -1;
        chain.id[k] = -1;
    }
    return out;
}

// ---- the passes over device observation lists (DeviceObservationLists, ms_map_refresh_lists, ms_triangulate_lists) -------------------
// The map-point update of a new keyframe, mapper_helpers.cpp:1062-1077, without a per-point host structure: the observation lists of the
// current keyframe's usable map points (status neither NOT_TRIANGULATED nor BAD, :1066) are built on the device, then updateDescriptor +
// updateDistanceAndNorm (:1069-1070) and the status promotion of :1072-1076 run on them where they lie: writes M.points and M.flags->  M.pool
// may be null (descriptors stay).  Returns the number of refreshed map points; M.lists holds them afterwards.
inline std::size_t updateMapPoints(Context &ctx, MapTables M, std::int32_t currentSlot, int minObservationsForBA, const StaticSettings &settings) {
    M.require("updateMapPoints", M.POINTS | M.FLAGS | M.LISTS | M.KEYPOINTS | M.POSES | M.IDS);
    ObservationSelection sel;
    sel.slot = currentSlot; sel.filter = MS_OBS_REFRESH; sel.dropEmpty = true;
    const int levels = (int)settings.scaleFactors.size();
    M.lists->build(M, M.pool != nullptr, sel, levels);
    const ms_obs_lists l = M.lists->lists();
    ctx.check(ms_map_refresh_lists(ctx.get(), M.points->position(), M.points->mutableNorm(), M.points->mutableMinDistance(), M.points->mutableMaxDistance(),
                                   M.points->mutableDescriptor(), (int)M.points->size(), M.poses->pose(), (int)M.poses->size(), M.poolDescriptor(), M.poolSize(), &l,
                                   (int)M.lists->rowCount(), (int)M.lists->observationCount(), settings.scaleFactors.data(), levels, std::max(minObservationsForBA, 1),
                                   M.flags->mutableFlags(), nullptr), "ms_map_refresh_lists");
    return M.lists->rowCount();
}

// The re-triangulation after local BA, mapper_helpers.cpp:1085-1092: the current keyframe's map points that are not TRIANGULATED or have at
// least two observations (:1088), triangulated from device lists: writes M.points and M.flags->  The per-point results come back as from
// triangulateMapPoints, in the order of the keyframe's keypoints.
inline TriangulateResult retriangulateCurrent(Context &ctx, MapTables M, std::int32_t currentSlot, const StaticSettings &settings, TriangulationMethod method) {
    M.require("retriangulateCurrent", M.POINTS | M.FLAGS | M.LISTS | M.KEYPOINTS | M.POSES | M.IDS | M.CAMERAS | M.FOCALS);
    ObservationSelection sel;
    sel.slot = currentSlot; sel.filter = MS_OBS_RETRIANGULATE;
    M.lists->build(M, false, sel, (int)settings.levelSigmaSq.size());
    const ms_tri_settings s = detail::tri_settings(settings);
    const std::size_t n = M.lists->rowCount();
    TriangulateResult out;
    out.status.assign(n, 0); out.reason.assign(n, 0); out.passCount.assign(n, 0);
    const ms_obs_lists l = M.lists->lists();
    ctx.check(ms_triangulate_lists(ctx.get(), M.points->mutablePosition(), M.flags->mutableFlags(), (int)M.points->size(), M.poses->pose(), (int)M.poses->size(),
                                   M.slots.camera.data(), M.slots.focalLength.data(), &l, (int)n, (int)M.lists->observationCount(), &s, (int)method, out.status.data(),
                                   out.reason.data(), out.passCount.data()), "ms_triangulate_lists");
    return out;
}

// ---- matchTrackedFeatures on the device tables (ms_match_tracked, ms_match_tracked_finish) ----------------------------------------------
// The current frame as matchTrackedFeatures reads it: its keyframe slot (the keypoints are in DeviceKeypointTable, the pose in
// DeviceKeyframePoses; poseCW is the same pose on the host) and keyPointToTrackId per keypoint, -1 for none.
struct TrackedFrame {
    std::int32_t slot = 0;
    DeviceKeyframePoses::Pose poseCW{};
    std::vector<std::int32_t> keyPointToTrackId;
};
// Per keypoint the outcome (0 no track | 1 created | 2 just tracked | 3 bound after isInFrustum and checkReprojectionError | 4 outside the
// frustum | 5 reprojection error | 6 absent track, no descriptors), the rows of the created map points with their keypoints (in keypoint
// order: what nextMpId, the host MapPoint objects and their colours are derived from), the reference's debug counters, and FIRST_LAST's
// result per just-tracked point.
struct MatchTrackedResult {
    std::vector<std::uint8_t> outcome;
    std::vector<std::int32_t> createdRows, createdKeyPoints;
    std::size_t newPoints = 0, justTriangulated = 0, checked = 0, frustumFail = 0, reproFail = 0, success = 0;
    TriangulateResult firstLast;
};

// matchTrackedFeatures (mapper_helpers.cpp:67-142) for one frame on the device tables, nothing per keypoint on the host:
//   ms_match_tracked (the walk: bind, gate, create) -> ms_observation_lists of the just-tracked rows -> ms_triangulate_lists FIRST_LAST (:90)
//   -> ms_match_tracked_finish (the descriptor of the points that are now UNSURE, :811; the rows of :121) -> the refresh of :121-124: one pass
//   when the frame has descriptors, otherwise the just-tracked TRIANGULATED rows with the descriptor half and the checked rows without it.
// freeRows: table rows the caller offers to new map points, at least as many as the frame can create (the k-th created point takes the
// k-th); M.pool must hold the frame's descriptors at descBase[slot] when that is >= 0.  Writes M.keyframes, M.points, M.flags, M.live and
// M.tracks; M.lists is scratch and holds the last refresh's rows.
inline MatchTrackedResult matchTrackedFeatures(Context &ctx, MapTables M, const TrackedFrame &frame, const std::vector<std::int32_t> &freeRows, const StaticSettings &settings,
                                               float viewAngleLimitCos = 0.5f) {
    const std::size_t nKf = M.keyframes.size(), nMp = M.keyframes.mapPointCount(), nKp = frame.keyPointToTrackId.size(), nNew = freeRows.size();
    if (frame.slot < 0 || (std::size_t)frame.slot >= nKf) throw std::invalid_argument("matchTrackedFeatures: slot outside the table");
    M.require("matchTrackedFeatures", M.POINTS | M.FLAGS | M.LISTS | M.LIVE | M.TRACKS | M.KEYPOINTS | M.POSES | M.CAMERAS | M.FOCALS | M.IDS | M.DESC_BASES);
    DeviceObservationLists &lists = *M.lists;
    DeviceMapPoints &points = *M.points;
    const bool hasDescriptors = M.slots.descBase[frame.slot] >= 0;
    if (hasDescriptors && !M.pool) throw std::invalid_argument("matchTrackedFeatures: the frame has descriptors and there is no pool");
    for (std::int32_t t : frame.keyPointToTrackId) if (t >= 0) M.tracks->ensureTrack(t);
    const int levels = (int)settings.levelSigmaSq.size();
    ms_tracked_frame f{};
    f.slot = frame.slot;
    std::copy(frame.poseCW.begin(), frame.poseCW.end(), f.pose);
    f.cam = M.slots.camera[frame.slot]; f.focal = M.slots.focalLength[frame.slot];
    f.desc_base = M.slots.descBase[frame.slot]; f.track_base = M.tracks->trackBase();
    f.level_sigma_sq = settings.levelSigmaSq.data(); f.n_levels = levels;
    f.rel_reprojection_threshold = settings.parameters.relativeReprojectionErrorThreshold; f.view_cos_limit = viewAngleLimitCos;
    // device scratch: created rows | created keypoints | just-tracked rows | checked rows | refresh rows | outcomes
    const std::size_t pitchKp = detail::padded(nKp), pitchNew = detail::padded(nNew);
    std::int32_t *createdRows = reinterpret_cast<std::int32_t *>(ctx.workspace(4 * (2 * pitchNew + 4 * pitchKp) + pitchKp + 256));
    std::int32_t *createdKp = createdRows + pitchNew, *trackedRows = createdKp + pitchNew, *checkedRows = trackedRows + pitchKp, *refreshRows = checkedRows + pitchKp;
    std::uint8_t *outcome = reinterpret_cast<std::uint8_t *>(refreshRows + 2 * pitchKp);
    std::int32_t counts[5] = {0, 0, 0, 0, 0};
    ctx.check(ms_match_tracked(ctx.get(), M.keyframes.mutableTable(), (int)nKf, (int)M.keyframes.stride(), M.flags->mutableFlags(), M.live->mutableLive(), points.position(),
                               points.norm(), points.minDistance(), points.maxDistance(), points.mutableDescriptor(), M.tracks->mpTrack(), (int)nMp, M.keypoints->x(), M.keypoints->y(),
                               M.keypoints->octave(), M.poolDescriptor(), M.poolSize(), M.tracks->trackRow(), (int)M.tracks->window(), &f, frame.keyPointToTrackId.data(), (int)nKp,
                               freeRows.data(), (int)nNew, outcome, createdRows, createdKp, trackedRows, checkedRows, counts), "ms_match_tracked");
    MatchTrackedResult out;
    out.newPoints = (std::size_t)counts[0]; out.justTriangulated = (std::size_t)counts[1]; out.checked = (std::size_t)counts[2];
    out.frustumFail = (std::size_t)counts[3]; out.reproFail = (std::size_t)counts[4];
    out.outcome = ctx.download(outcome, nKp);
    out.createdRows = ctx.download(createdRows, out.newPoints); out.createdKeyPoints = ctx.download(createdKp, out.newPoints);
    auto listsOf = [&](const std::int32_t *rows, std::size_t n, bool dropEmpty) {
        ObservationSelection sel;
        sel.deviceRows = rows; sel.rowCount = n; sel.dropEmpty = dropEmpty;
        lists.build(M, M.pool != nullptr, sel, levels);
    };
    std::size_t nTracked = 0;
    if (out.justTriangulated) {                              // :90
        listsOf(trackedRows, out.justTriangulated, false);
        nTracked = lists.rowCount();
        const ms_tri_settings s = detail::tri_settings(settings);
        out.firstLast.status.assign(nTracked, 0); out.firstLast.reason.assign(nTracked, 0); out.firstLast.passCount.assign(nTracked, 0);
        const ms_obs_lists l = lists.lists();
        ctx.check(ms_triangulate_lists(ctx.get(), points.mutablePosition(), M.flags->mutableFlags(), (int)nMp, M.poses->pose(), (int)nKf, M.slots.camera.data(),
                                       M.slots.focalLength.data(), &l, (int)nTracked, (int)lists.observationCount(), &s, MS_TRI_FIRST_LAST, out.firstLast.status.data(),
                                       out.firstLast.reason.data(), out.firstLast.passCount.data()), "ms_triangulate_lists");
    }
    const ms_obs_lists l = lists.lists(M.pool != nullptr);
    std::int32_t nRefresh = 0;
    ctx.check(ms_match_tracked_finish(ctx.get(), &l, (int)nTracked, M.flags->flags(), M.poolDescriptor(), points.mutableDescriptor(), (int)nMp, checkedRows, (int)out.checked,
                                      hasDescriptors ? 1 : 0, refreshRows, (int)(2 * pitchKp), &nRefresh), "ms_match_tracked_finish");
    auto refresh = [&](const std::int32_t *rows, std::size_t n, bool descriptors) {                      // :121-124
        if (n == 0) return;
        listsOf(rows, n, true);
        const ms_obs_lists r = lists.lists();
        ctx.check(ms_map_refresh_lists(ctx.get(), points.position(), points.mutableNorm(), points.mutableMinDistance(), points.mutableMaxDistance(), points.mutableDescriptor(),
                                       (int)nMp, M.poses->pose(), (int)nKf, descriptors ? M.poolDescriptor() : nullptr, descriptors ? M.poolSize() : 0, &r, (int)lists.rowCount(),
                                       (int)lists.observationCount(), settings.scaleFactors.data(), (int)settings.scaleFactors.size(), 0, nullptr, nullptr), "ms_map_refresh_lists");
    };
    refresh(refreshRows, (std::size_t)nRefresh, true);
    if (!hasDescriptors) refresh(checkedRows, out.checked, false);
    out.success = (std::size_t)nRefresh + (hasDescriptors ? 0 : out.checked);
    return out;
}

// ---- createNewMapPoints on the device tables (ms_create_points_lists, ms_create_points_bind, ms_unbound_mask) --------------------------
// The `usable` masks of the triangulation matcher ("the keypoint has no map point", keyframe_matcher.cpp:205-221) of the listed slots, written
// from the keyframe table in one launch into M.slots.frames[slot], the DeviceKeyframe of that slot.
inline void unboundMasks(Context &ctx, MapTables M, const std::vector<std::int32_t> &slots) {
    const std::vector<DeviceKeyframe *> &frames = M.slots.frames;
    std::vector<std::int32_t> counts;
    std::vector<std::uint8_t *> masks;
    for (std::int32_t s : slots) {
        if (s < 0 || (std::size_t)s >= frames.size() || !frames[s]) throw std::invalid_argument("unboundMasks: no frame for slot " + std::to_string(s));
        counts.push_back((std::int32_t)frames[s]->keyPointCount());
        masks.push_back(frames[s]->mutableUsable());
    }
    ctx.check(ms_unbound_mask(ctx.get(), M.keyframes.table(), (int)M.keyframes.size(), (int)M.keyframes.stride(), (int)M.keyframes.mapPointCount(), slots.data(), counts.data(),
                              masks.data(), (int)slots.size()), "ms_unbound_mask");
}

// What one adjacent keyframe gave: per match (ascending keypoint of the current keyframe) the provisional row, the two keypoints and the
// triangulator's status / reason; the created points packed in the same order -- what nextMpId, the host MapPoint objects and their colours
// are derived from.  skipped = the slot was the current keyframe's (mapper_helpers.cpp:281).
struct CreatedPoints {
    std::int32_t slot = -1;
    bool skipped = false;
    std::vector<std::int32_t> rows, keyPoints1, keyPoints2;
    std::vector<std::uint8_t> status, reason;
    std::vector<std::int32_t> createdRows, createdKeyPoints1, createdKeyPoints2;
};

// createNewMapPoints (mapper_helpers.cpp:271-318) for the keyframe in currentSlot, nothing per match on the host.  Per adjacent slot, in the
// given order:  create_E_21 -> ms_match_triangulation -> ms_create_points_lists -> ms_triangulate_lists (TME or MIDPOINT, :308) ->
// ms_create_points_bind.  M.slots.frames[slot] = the slot's DeviceKeyframe, whose `usable` mask says "no map point" (unboundMasks) and is kept
// current by the bind step, so the next adjacent's matcher sees this adjacent's binds.  freeRows: free table rows, at least as many as one
// adjacent can match; an adjacent takes the first ones and hands back those whose triangulation failed.  Writes M.keyframes, M.points, M.flags,
// M.live and, where given, M.observationCount and M.tracks' mp_track (2 and -1 for a created row); M.lists is scratch.
// hostPoses: the poses DeviceKeyframePoses holds (downloaded when null).
inline std::vector<CreatedPoints> createNewMapPoints(Context &ctx, MapTables M, std::int32_t currentSlot, const std::vector<std::int32_t> &adjacentSlots,
                                                     const std::vector<std::int32_t> &freeRows, const StaticSettings &settings, TriangulationMethod method,
                                                     const std::vector<DeviceKeyframePoses::Pose> *hostPoses = nullptr) {
    const std::size_t nKf = M.keyframes.size(), nMp = M.keyframes.mapPointCount();
    if (currentSlot < 0 || (std::size_t)currentSlot >= nKf) throw std::invalid_argument("createNewMapPoints: slot outside the table");
    M.require("createNewMapPoints", M.POINTS | M.FLAGS | M.LISTS | M.LIVE | M.KEYPOINTS | M.POSES | M.CAMERAS | M.FOCALS | M.IDS | M.DESC_BASES | M.FRAMES);
    DeviceObservationLists &lists = *M.lists;
    const std::vector<DeviceKeyframe *> &frames = M.slots.frames;
    const bool pool = M.pool != nullptr;
    if (method == TriangulationMethod::FIRST_LAST) throw std::invalid_argument("createNewMapPoints: TME or MIDPOINT");
    if (!frames[currentSlot]) throw std::invalid_argument("createNewMapPoints: no frame for the current slot");
    const std::vector<DeviceKeyframePoses::Pose> downloaded = hostPoses ? std::vector<DeviceKeyframePoses::Pose>() : M.poses->download();
    const std::vector<DeviceKeyframePoses::Pose> &P = hostPoses ? *hostPoses : downloaded;
    if (P.size() != nKf) throw std::invalid_argument("createNewMapPoints: one host pose per slot");
    auto rotation = [](const DeviceKeyframePoses::Pose &p, double R[9], double t[3]) {
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) R[3 * i + j] = p[4 * i + j]; t[i] = p[4 * i + 3]; }
    };
    DeviceKeyframe &kf1 = *frames[currentSlot];
    const std::size_t n1 = kf1.keyPointCount();
    const int levels = (int)settings.levelSigmaSq.size();
    const ms_tri_settings s = detail::tri_settings(settings);
    // device scratch: E and the scale factors | match count | matched | the matches' keypoints | the created points
    const std::size_t pitch = detail::padded(n1), oS = 128, oCount = oS + detail::pad16(4 * settings.scaleFactors.size()) + 64, oInts = oCount + 64;
    unsigned char *ws = ctx.workspace(oInts + 4 * 6 * pitch);
    std::int32_t *matched = reinterpret_cast<std::int32_t *>(ws + oInts), *kp1 = matched + pitch, *kp2 = kp1 + pitch, *createdRows = kp2 + pitch,
                 *createdKp1 = createdRows + pitch, *createdKp2 = createdKp1 + pitch;
    std::vector<std::int32_t> free = freeRows;
    std::vector<CreatedPoints> out;
    for (std::int32_t adj : adjacentSlots) {
        CreatedPoints r;
        r.slot = adj;
        if (adj == currentSlot) {                            // :281
            r.skipped = true;
            out.push_back(std::move(r));
            continue;
        }
        if (adj < 0 || (std::size_t)adj >= nKf || !frames[adj]) throw std::invalid_argument("createNewMapPoints: no frame for slot " + std::to_string(adj));
        DeviceKeyframe &kf2 = *frames[adj];
        double R1[9], t1[3], R2[9], t2[3], E[9];
        rotation(P[currentSlot], R1, t1); rotation(P[adj], R2, t2);
        create_E_21(R2, t2, R1, t1, E);                      // keyframe_matcher.cpp:171-175
        std::vector<unsigned char> &st = ctx.staging();
        st.assign(oCount, 0);
        std::memcpy(st.data(), E, 72);
        std::memcpy(st.data() + oS, settings.scaleFactors.data(), 4 * settings.scaleFactors.size());
        ctx.check(ms_dev_upload(ctx.get(), ws, st.data(), st.size()), "ms_dev_upload");
        const ms_match_frame f1 = kf1.frame(), f2 = kf2.frame();
        ctx.check(ms_match_triangulation(ctx.get(), &f1, &f2, 1, reinterpret_cast<const double *>(ws), reinterpret_cast<const float *>(ws + oS),
                                         settings.parameters.epipolarCheckThresholdDegrees, 1, &matched, reinterpret_cast<std::int32_t *>(ws + oCount)), "ms_match_triangulation");
        std::int32_t nMatches = 0;
        for (int attempt = 0;; ++attempt) {
            const ms_obs_lists l = lists.lists(pool);
            const int rc = ms_create_points_lists(ctx.get(), M.keyframes.table(), (int)nKf, (int)M.keyframes.stride(), M.live->live(), (int)nMp, M.slots.id.data(), M.keypoints->x(),
                                                  M.keypoints->y(), M.keypoints->octave(), M.keypoints->depth(), pool ? M.slots.descBase.data() : nullptr, currentSlot, adj, matched,
                                                  (int)n1, (int)kf2.keyPointCount(), free.data(), (int)free.size(), levels, &l, (int)lists.rowCapacity(), (int)lists.observationCapacity(),
                                                  kp1, kp2, &nMatches);
            if (rc == MS_ERR_CAPACITY && attempt == 0 && (std::size_t)nMatches <= free.size() &&
                ((std::size_t)nMatches > lists.rowCapacity() || 2 * (std::size_t)nMatches > lists.observationCapacity())) {
                lists.ensure((std::size_t)nMatches, 2 * (std::size_t)nMatches);      // the needed count came back: once is enough
                continue;
            }
            ctx.check(rc, "ms_create_points_lists");
            break;
        }
        const std::size_t n = (std::size_t)nMatches;
        lists.setCounts(n, 2 * n, pool);
        r.rows.assign(free.begin(), free.begin() + (std::ptrdiff_t)n);
        r.keyPoints1 = ctx.download(kp1, n); r.keyPoints2 = ctx.download(kp2, n);
        r.status.assign(n, 0); r.reason.assign(n, 0);
        const ms_obs_lists l = lists.lists(pool);
        ctx.check(ms_triangulate_lists(ctx.get(), M.points->mutablePosition(), M.flags->mutableFlags(), (int)nMp, M.poses->pose(), (int)nKf, M.slots.camera.data(),
                                       M.slots.focalLength.data(), &l, (int)n, (int)(2 * n), &s, (int)method, r.status.data(), r.reason.data(), nullptr), "ms_triangulate_lists");      // :308
        std::int32_t nCreated = 0;
        ctx.check(ms_create_points_bind(ctx.get(), M.keyframes.mutableTable(), (int)nKf, (int)M.keyframes.stride(), M.flags->flags(), M.live->mutableLive(),
                                        M.points->mutableDescriptor(), M.observationCount, M.trackWindow().mpTrack, (int)nMp, M.poolDescriptor(), M.poolSize(), currentSlot, adj, &l, kp1,
                                        kp2, (int)n, (int)n1, (int)kf2.keyPointCount(), kf1.mutableUsable(), kf2.mutableUsable(), createdRows, createdKp1, createdKp2, &nCreated),
                  "ms_create_points_bind");      // :309-316
        r.createdRows = ctx.download(createdRows, (std::size_t)nCreated);
        r.createdKeyPoints1 = ctx.download(createdKp1, (std::size_t)nCreated); r.createdKeyPoints2 = ctx.download(createdKp2, (std::size_t)nCreated);
        std::vector<std::int32_t> left;                      // the rows of the failed matches go back to the front, in order
        left.reserve(free.size());
        std::size_t c = 0;
        for (std::size_t i = 0; i < free.size(); ++i) {
            if (i < n && c < r.createdRows.size() && r.createdRows[c] == free[i]) { ++c; continue; }
            left.push_back(free[i]);
        }
        free.swap(left);
        out.push_back(std::move(r));
    }
    return out;
}

// ---- local bundle adjustment on the device tables (ms_ba_window_lists, ms_ba_window_apply) ---------------------------------------------
// The EdgeSE3Expmap edges of a window (the odometry chain of bundle_adjuster.cpp:296-311 and the loop closures of :314-319): they read odometry
// data that no table holds, so the caller fills edgeI / edgeJ / edgeMeas / edgeInfo of the window, given the local keyframes' slots in pose
// order (descending KfId; vertex k of the window is localSlots[k]).
using PoseEdgeBuilder = std::function<void(const std::vector<std::int32_t> &localSlots, BaWindow &window)>;

// What localBundleAdjustOnTables did: which stage ended it (NONE: one of the early-outs of :235-240, nothing solved and nothing written),
// the local keyframes' slots in pose order, localMapPoints as table rows (the reference's return value, :393) and the erased observations in
// edge order -- what keyPointToTrackId.erase (keyframe.cpp:285) and the host copies are derived from.
struct LocalBaOnTables {
    BaStats::Ba stage = BaStats::Ba::NONE;
    BaOutcome outcome;
    std::vector<std::int32_t> localSlots, localRows;
    std::size_t currentFrameMapPoints = 0, edgeCount = 0;
    struct Erased { std::int32_t edge, slot, keyPoint, row; };
    std::vector<Erased> erased;
};

namespace detail {
// localKeyframes of :177-193 as slots, descending KfId: the current keyframe, the adjacent ones and the seven newest of the map (the loop
// inserts, then breaks at i > 5)
inline std::vector<std::int32_t> local_keyframes(const std::vector<std::int32_t> &kfIds, std::int32_t currentSlot, const std::vector<std::int32_t> &adjacentSlots) {
    const std::size_t nKf = kfIds.size();
    std::vector<char> local(nKf, 0);
    auto insert = [&](std::int32_t s) {
        if (s < 0 || (std::size_t)s >= nKf || kfIds[s] < 0) throw std::invalid_argument("localBundleAdjustOnTables: slot " + std::to_string(s) + " holds no keyframe");
        local[s] = 1;
    };
    insert(currentSlot);
    for (std::int32_t s : adjacentSlots) insert(s);
    std::vector<std::int32_t> byId;
    for (std::size_t s = 0; s < nKf; ++s) if (kfIds[s] >= 0) byId.push_back((std::int32_t)s);
    std::sort(byId.begin(), byId.end(), [&](std::int32_t a, std::int32_t b) { return kfIds[a] > kfIds[b]; });
    for (std::size_t i = 0; i < byId.size() && i < 7; ++i) local[byId[i]] = 1;
    std::vector<std::int32_t> out;
    for (std::int32_t s : byId) if (local[s]) out.push_back(s);
    return out;
}
}  // namespace detail

// localBundleAdjust (bundle_adjuster.cpp:141-394) for the keyframe in currentSlot with nothing walked on the host: the local keyframes
// (:177-193), ms_map_point_union -> ms_observation_lists -> ms_ba_window_lists for the window (:214-290), the early-outs of :235-240, the
// existing two-stage localBundleAdjust on the gathered window, then ms_ba_window_apply in the mode the stage dictates (:326-331 or :376-390).
// adjacentSlots = computeAdjacentKeyframes(minCovisibilities 15, problemMaxSize) as slots; M.slots.id = the KfId per slot, -1 for an empty one.
// M.observationCount: the whole-map counts the chain keeps current (observationCountsOnDevice).  Writes M.keyframes, M.points, M.flags, M.poses
// and M.observationCount; M.lists is scratch and holds the window's lists afterwards.  The mirror's localBundleAdjust reports the outliers, not
// their chi2, so the apply step is handed +inf for an outlier and 0 otherwise.  With M.slots.frames filled, the "no map point" masks of the slots that lost
// an observation are renewed with unboundMasks.
inline LocalBaOnTables localBundleAdjustOnTables(Context &ctx, MapTables M, std::int32_t currentSlot, const std::vector<std::int32_t> &adjacentSlots, const PoseEdgeBuilder &edges,
                                                 int problemMaxSize, const Parameters &parameters, const StaticSettings &settings, WorkspaceBA *workspace = nullptr) {
    M.require("localBundleAdjustOnTables", M.POINTS | M.FLAGS | M.LISTS | M.KEYPOINTS | M.POSES | M.COUNTS | M.CAMERAS | M.FOCALS | M.IDS);
    const std::size_t nKf = M.keyframes.size(), nMp = M.keyframes.mapPointCount();
    DeviceObservationLists &lists = *M.lists;
    LocalBaOnTables out;
    out.localSlots = detail::local_keyframes(M.slots.id, currentSlot, adjacentSlots);
    const std::vector<std::int32_t> &local = out.localSlots;
    const std::int32_t current = (std::int32_t)(std::find(local.begin(), local.end(), currentSlot) - local.begin());
    // localMapPoints and their observations, on the device
    std::int32_t *unionRows = reinterpret_cast<std::int32_t *>(ctx.workspace(4 * nMp + 256));
    const ms_union_problem problem{0, (std::int32_t)local.size(), -1, DeviceMapPointFlags::TRIANGULATED};
    std::int32_t nUnion = 0;
    ctx.check(ms_map_point_union(ctx.get(), M.keyframes.table(), (int)nKf, (int)M.keyframes.stride(), M.flags->flags(), (int)nMp, local.data(), (int)local.size(), &problem, 1, unionRows, nullptr,
                                 &nUnion), "ms_map_point_union");
    ObservationSelection sel;
    sel.deviceRows = unionRows; sel.rowCount = (std::size_t)nUnion;
    const int levels = (int)settings.levelSigmaSq.size();
    lists.build(M, false, sel, levels);
    const std::size_t nRows = lists.rowCount(), nObs = lists.observationCount();
    const ms_obs_lists l = lists.lists();
    out.localRows = lists.download(l.rows, nRows);
    // the window: the edge arrays stay on the device for the apply step
    const std::size_t pitch = detail::padded(nObs);
    std::int32_t *edgeArrays = reinterpret_cast<std::int32_t *>(ctx.workspace(12 * pitch));
    const ms_ba_window_dev window{edgeArrays, edgeArrays + pitch, edgeArrays + 2 * pitch};
    BaWindow w;
    w.poses.resize(local.size()); w.points.resize(nRows); w.obsPose.resize(nObs); w.obsPoint.resize(nObs); w.obsUv.resize(nObs); w.obsInfo.resize(nObs);
    std::int32_t nEdge = 0, nCurrent = 0;
    ctx.check(ms_ba_window_lists(ctx.get(), M.poses->pose(), (int)nKf, M.points->position(), (int)nMp, &l, (int)nRows, (int)nObs, local.data(), (int)local.size(), current,
                                 M.slots.camera.data(), M.slots.focalLength.data(), settings.levelSigmaSq.data(), levels, w.poses[0].data(), nRows ? w.points[0].data() : nullptr,
                                 w.obsPoint.data(), w.obsPose.data(), nObs ? w.obsUv[0].data() : nullptr, w.obsInfo.data(), (int)nRows, (int)nObs, &window, &nEdge, &nCurrent),
              "ms_ba_window_lists");
    out.currentFrameMapPoints = (std::size_t)nCurrent; out.edgeCount = (std::size_t)nEdge;
    if (local.empty() || (unsigned)nCurrent < parameters.minVisibleMapPointsInCurrentFrameBA || local.size() < parameters.minKeyframesInBA) return out;      // :235-240
    w.obsPose.resize((std::size_t)nEdge); w.obsPoint.resize((std::size_t)nEdge); w.obsUv.resize((std::size_t)nEdge); w.obsInfo.resize((std::size_t)nEdge);
    w.currentKeyframe = current;
    if (edges) edges(local, w);
    const bool neighbourhood = !((unsigned)nCurrent < parameters.minVisibleMapPointsInNeighborhoodBA);         // :326
    out.outcome = localBundleAdjust(ctx, w, problemMaxSize, parameters, neighbourhood, workspace);
    out.stage = neighbourhood ? BaStats::Ba::LOCAL : BaStats::Ba::NEIGHBOR;
    std::vector<double> chi2;
    if (neighbourhood) {
        chi2.resize((std::size_t)nEdge);
        for (std::size_t e = 0; e < chi2.size(); ++e) chi2[e] = out.outcome.outlier[e] ? std::numeric_limits<double>::infinity() : 0.0;
    }
    std::vector<std::int32_t> erased((std::size_t)nEdge + 1);
    std::int32_t nErased = 0, nStale = 0;
    ctx.check(ms_ba_window_apply(ctx.get(), M.keyframes.mutableTable(), (int)nKf, (int)M.keyframes.stride(), M.points->mutablePosition(), M.flags->mutableFlags(), M.observationCount,
                                 (int)nMp, M.poses->pose(), w.poses[0].data(), (int)w.poses.size(), nRows ? w.points[0].data() : nullptr, neighbourhood ? chi2.data() : nullptr, &window, nEdge,
                                 l.rows, (int)nRows, local.data(), (int)local.size(), current, neighbourhood ? MS_BA_APPLY_LOCAL : MS_BA_APPLY_NEIGHBOR, erased.data(), nEdge,
                                 &nErased, &nStale), "ms_ba_window_apply");
    if (nErased > 0) {
        const std::vector<std::int32_t> keyPoints = ctx.download(window.edge_kp, (std::size_t)nEdge);
        std::vector<std::int32_t> touched;
        for (std::int32_t i = 0; i < nErased; ++i) {
            const std::int32_t e = erased[(std::size_t)i], slot = local[(std::size_t)w.obsPose[(std::size_t)e]];
            out.erased.push_back({e, slot, keyPoints[(std::size_t)e], out.localRows[(std::size_t)w.obsPoint[(std::size_t)e]]});
            if (std::find(touched.begin(), touched.end(), slot) == touched.end()) touched.push_back(slot);
        }
        if (!M.slots.frames.empty()) unboundMasks(ctx, M, touched);
    }
    return out;
}

// ---- poseBundleAdjust on the device tables (ms_pose_tables_solve) ----------------------------------------------------------------------
// makeOdometryEdge(keyframe, previous) (bundle_adjuster.cpp:65-112): it reads odometry data that no table holds, so the caller fills it as
// it fills edgeMeas / edgeInfo of a BaWindow.  Vertex 0 = the frame, vertex 1 = its previous keyframe.
struct PoseOdometryEdge {
    std::array<double, 7> measurement{{0, 0, 0, 1, 0, 0, 0}};
    std::array<double, 36> information{};
};

// The persistent handle of poseBundleAdjustOnTables: one per context, for frames of up to maxMapPoints triangulated map points.
class DevicePoseAdjuster {
public:
    DevicePoseAdjuster(Context &ctx, std::size_t maxMapPoints, const StaticSettings &settings) {
        ctx.check(ms_pose_tables_create(ctx.get(), (int)maxMapPoints, settings.levelSigmaSq.data(), (int)settings.levelSigmaSq.size(), &h_), "ms_pose_tables_create");
    }
    ~DevicePoseAdjuster() { ms_pose_tables_destroy(h_); }
    DevicePoseAdjuster(const DevicePoseAdjuster &) = delete;
    DevicePoseAdjuster &operator=(const DevicePoseAdjuster &) = delete;
    ms_pose_tables *get() const { return h_; }
    ms_pose_tables_out last{};               // what the last poseBundleAdjustOnTables on this handle returned
private:
    ms_pose_tables *h_ = nullptr;
};

// poseBundleAdjust (bundle_adjuster.cpp:396-491) for the frame in `slot` with nothing walked on the host: the frame's TRIANGULATED map points
// are gathered from the tables, solved and the pose written back into `poses` on the device.  Returns the reference's bool: false, with
// nothing written, for a frame with fewer than minVisibleMapPointsInCurrentFrameBA such points (:410-412) or without a previous keyframe
// (prevSlot = -1, :430-432).  M.live may be null (every row holds a map point).  Writes M.poses alone.  keyPointCount defaults to the stride:
// the entries behind a keyframe's keypoints are -1 (DeviceKeyframeMapPoints::update pads them).
inline bool poseBundleAdjustOnTables(Context &ctx, MapTables M, DevicePoseAdjuster &handle, std::int32_t slot, std::int32_t prevSlot, const PoseOdometryEdge &odometryEdge,
                                     const Parameters &parameters, const StaticSettings &settings, std::size_t keyPointCount = ~(std::size_t)0) {
    detail::TraceRange range("poseBundleAdjust");                             // mapper_helpers.cpp:1044
    M.require("poseBundleAdjustOnTables", M.POINTS | M.FLAGS | M.KEYPOINTS | M.POSES | M.CAMERAS | M.FOCALS);
    const std::size_t nKf = M.keyframes.size(), nMp = M.keyframes.mapPointCount();
    if (slot < 0 || (std::size_t)slot >= nKf) throw std::invalid_argument("poseBundleAdjustOnTables: slot " + std::to_string(slot) + " outside the table");
    (void)settings;                                                            // (its level sigmas went to the device with the handle)
    ms_pose_tables_frame f{};
    f.slot = slot; f.prev_slot = prevSlot;
    f.n_kp = (std::int32_t)std::min(keyPointCount, M.keyframes.stride());
    f.cam = M.slots.camera[(std::size_t)slot]; f.focal = M.slots.focalLength[(std::size_t)slot];
    std::copy(odometryEdge.measurement.begin(), odometryEdge.measurement.end(), f.edge_meas);
    std::copy(odometryEdge.information.begin(), odometryEdge.information.end(), f.edge_info);
    f.min_visible = (std::int32_t)parameters.minVisibleMapPointsInCurrentFrameBA;
    f.max_iters = (std::int32_t)parameters.poseBAIterations;
    f.huber_delta = std::sqrt(CHI2_THRESHOLD);                                 // rk->setDelta(std::sqrt(CHI2_THRESHOLD)) (:56), as detail::as_problem
    ctx.check(ms_pose_tables_solve(handle.get(), M.keyframes.table(), (int)nKf, (int)M.keyframes.stride(), M.flags->flags(), M.live ? M.live->live() : nullptr, M.points->position(),
                                   (int)nMp, M.keypoints->x(), M.keypoints->y(), M.keypoints->octave(), M.poses->pose(), &f, &handle.last, nullptr), "ms_pose_tables_solve");
    return handle.last.ran != 0;
}

// ---- the end of a frame on the device tables (ms_frame_finish) ---------------------------------------------------------------------------
// The frame's result point cloud (setPointCloudOutput, mapper_helpers.cpp:484-497: table row, keypoint, trackId, position of every keypoint
// whose map point is TRIANGULATED, in keypoint order) and what the host side of the map still has to do after removeKeyframe (:375-431):
// the removed map points in first-claim order -- trackIdToMapPoint.erase and the host copies -- and the removed keyframes' links as they
// were before -- bowIndex->remove, the `uncertainty` accumulation onto the next keyframe, re-pointing referenceKeyframe to the previous one.
struct FrameFinish {
    std::vector<std::int32_t> cloudRows, cloudKeyPoints, cloudTracks;
    std::vector<double> cloudPositions;
    std::vector<std::int32_t> removedRows, removedPrevious, removedNext;
    std::size_t erasedObservations = 0;
};

namespace detail {
// ONE ms_frame_finish call: the cloud of cloudSlot (-1: none), then the removal of `slots`.  Writes M.keyframes, M.flags, M.live and, when given,
// M.observationCount; relinks M.slots.previous / next in list order and empties the removed slots' ids, as cullMap does.
inline FrameFinish finish_frame(Context &ctx, MapTables &M, const char *who, std::int32_t cloudSlot, std::size_t nKeyPoints, const std::vector<std::int32_t> &slots,
                                const std::vector<std::int32_t> &loopClosureKeyframes) {
    M.require(who, M.POINTS | M.FLAGS | M.LIVE | M.LINKS | M.IDS);
    KeyframeSlots &chain = M.slots;
    const std::size_t nKf = M.keyframes.size(), nMp = M.keyframes.mapPointCount(), stride = M.keyframes.stride();
    for (std::int32_t k : slots) {
        if (k < 0 || (std::size_t)k >= nKf) throw std::invalid_argument(std::string(who) + ": slot " + std::to_string(k) + " outside the table");
        if (chain.previous[k] < 0) throw std::invalid_argument(std::string(who) + ": slot " + std::to_string(k) + " has no previous keyframe (cannot delete the first keyframe)");      // :392
        if (std::find(loopClosureKeyframes.begin(), loopClosureKeyframes.end(), k) != loopClosureKeyframes.end())
            throw std::invalid_argument(std::string(who) + ": slot " + std::to_string(k) + " is named by a loop-closure edge");                                                  // :382-385
    }
    const ms_frame_finish_args args{cloudSlot, (std::int32_t)std::min(nKeyPoints, stride)};
    const std::size_t nCloud = cloudSlot >= 0 ? (std::size_t)args.n_kp : 0, cap = std::min(nMp, slots.size() * stride);
    FrameFinish out;
    out.cloudRows.resize(nCloud); out.cloudKeyPoints.resize(nCloud); out.cloudTracks.resize(nCloud); out.cloudPositions.resize(3 * nCloud); out.removedRows.resize(cap);
    std::int32_t counts[3] = {0, 0, 0};
    ctx.check(ms_frame_finish(ctx.get(), M.keyframes.mutableTable(), (int)nKf, (int)stride, M.flags->mutableFlags(), M.live->mutableLive(), M.points->position(),
                              M.tracks ? M.tracks->mpTrack() : nullptr, M.observationCount, (int)nMp, chain.id.data(), slots.data(), (int)slots.size(), &args,
                              out.cloudRows.data(), out.cloudKeyPoints.data(), out.cloudTracks.data(), out.cloudPositions.data(), out.removedRows.data(), (int)cap, counts),
              "ms_frame_finish");
    out.cloudRows.resize((std::size_t)counts[0]); out.cloudKeyPoints.resize((std::size_t)counts[0]); out.cloudTracks.resize((std::size_t)counts[0]);
    out.cloudPositions.resize(3 * (std::size_t)counts[0]); out.removedRows.resize((std::size_t)counts[1]);
    out.erasedObservations = (std::size_t)counts[2];
    for (std::int32_t k : slots) {                           // :414-420, in list order
        const std::int32_t prev = chain.previous[k], next = chain.next[k];
        out.removedPrevious.push_back(prev); out.removedNext.push_back(next);
        if (next != -1) chain.previous[next] = prev;
        if (prev != -1) chain.next[prev] = next;
        chain.previous[k] = chain.next[k] = -1;
        chain.id[k] = -1;
    }
    return out;
}
}  // namespace detail

// The end of addKeyframe, mapper_helpers.cpp:1216-1230, for the frame in `slot`: its point cloud from the tables as they are, then, iff it did
// not become a keyframe, removeKeyframe (:375-431) on the tables -- one device call, nothing of the map walked on the host.  Throws
// std::invalid_argument before any device call when the frame is to be removed and has no previous keyframe (:392) or is named by a
// loop-closure edge (loopClosureKeyframes: slots, :382-385).  M.tracks may be null (cloudTracks = -1), M.observationCount is kept current when given.
inline FrameFinish finishFrame(Context &ctx, MapTables M, std::int32_t slot, std::size_t nKeyPoints, bool keyframeDecision, const std::vector<std::int32_t> &loopClosureKeyframes) {
    const std::vector<std::int32_t> slots = keyframeDecision ? std::vector<std::int32_t>{} : std::vector<std::int32_t>{slot};
    return detail::finish_frame(ctx, M, "finishFrame", slot, nKeyPoints, slots, loopClosureKeyframes);
}

// removeKeyframe (:375-431) for a list of keyframes, in list order: the keyframes that dropped out of the odometry pose trail (:1172-1183).
// One device call; no cloud.  The same two refusals as finishFrame, for every slot of the list, before any device call.
inline FrameFinish removeKeyframes(Context &ctx, MapTables M, const std::vector<std::int32_t> &slots, const std::vector<std::int32_t> &loopClosureKeyframes) {
    return detail::finish_frame(ctx, M, "removeKeyframes", -1, 0, slots, loopClosureKeyframes);
}

// ---- a frame of tracker features to the device tables (ms_frame_admit) ------------------------------------------------------------------
// makeKeyframeDecision (mapper_helpers.cpp:28-65) on what the host already holds: the two times, the two origPoseCameraCenter()s, the previous
// keyframe's keyPointToTrackId values and the current tracker features' ids.  It stays on the host on purpose: in the back end it decides
// whether the extractor runs at all, and it is a set lookup over a few hundred ids.  The comparison types are the reference's: maxCovis is a
// float product and the test is <=.
struct KeyframeDecisionParameters {
    double keyframeDecisionMinIntervalSeconds = 0.0;
    double keyframeDecisionDistanceThreshold = 0.0;
    float keyframeDecisionCovisibilityRatio = 0.0f;
};
inline bool makeKeyframeDecision(bool hasPreviousKeyframe, double currentT, double previousT, const std::array<double, 3> &currentCenter, const std::array<double, 3> &previousCenter,
                                 const std::vector<std::int32_t> &previousTrackIds, const std::vector<std::int32_t> &currentTrackIds, const KeyframeDecisionParameters &parameters) {
    if (!hasPreviousKeyframe) return true;                   // :34
    const double age = currentT - previousT;
    if (age < parameters.keyframeDecisionMinIntervalSeconds) return false;      // :38
    double sq = 0.0;
    for (int j = 0; j < 3; ++j) sq += (currentCenter[j] - previousCenter[j]) * (currentCenter[j] - previousCenter[j]);
    if (std::sqrt(sq) > parameters.keyframeDecisionDistanceThreshold) return true;      // :40-44
    std::vector<std::int32_t> previous(previousTrackIds);    // the std::set of :49-51 as a sorted vector
    std::sort(previous.begin(), previous.end());
    int prevCovisibilities = 0;
    unsigned nTracks = 0;
    for (std::int32_t id : currentTrackIds) {                // :55-58
        ++nTracks;
        if (std::binary_search(previous.begin(), previous.end(), id)) ++prevCovisibilities;
    }
    const float maxCovis = static_cast<float>(nTracks) * parameters.keyframeDecisionCovisibilityRatio;      // :61
    return prevCovisibilities <= maxCovis;                   // :62: the int converts to float
}

// What addKeyframeCommonOuter knows of a frame that carries tracker features only (mapper_helpers.cpp:1196): its KfId and time, poseCW
// (insertNewKeyframeCandidate's result), the pinhole stand-in of its camera, the tracker features (points[0], id, depth of
// mapperInput.trackerFeatures), optionally the host's camera.isValidPixel per feature, a DEVICE depth image standing in for frame->getDepth
// (float32, rows depthStride elements apart) and a DEVICE valid mask (bytes, rows maskStride apart).
struct TrackerFrameAdmission {
    std::int32_t id = -1;
    double t = 0.0;
    DeviceKeyframePoses::Pose poseCW{};
    ms_pinhole camera{};
    std::int32_t focalLength = 0;
    std::vector<float> x, y, depth;
    std::vector<std::int32_t> trackIds;
    std::vector<std::uint8_t> validPixel;                    // empty: every feature passes
    const float *depthImage = nullptr;
    std::int32_t depthWidth = 0, depthHeight = 0, depthStride = 0;
    const std::uint8_t *validMask = nullptr;
    std::int32_t maskWidth = 0, maskHeight = 0, maskStride = 0;
};

struct AdmittedTrackerFrame {
    std::size_t keyPoints = 0, droppedByValidPixel = 0, droppedByMask = 0, depthsFromImage = 0;
    std::vector<std::int32_t> keyPointTrackIds;              // what matchTrackedFeatures takes next
    std::vector<std::int32_t> keyPointFeature;               // the tracker feature behind each keypoint
};

// Keyframe::addTrackerFeatures and processKeyPoints (keyframe.cpp:34-69, :118-133) for one frame into `slot`: ONE device call, no table row
// uploaded.  Writes M.keyframes (the slot's row = -1), M.keypoints and M.poses; fills the slot's record: id, t, previous / next (the frame
// follows `previousSlot`, -1 for the first, mapdb.cpp:84-87), cameraCenter, camera, focalLength, descBase = -1 (the frame has no descriptors)
// and frames = nullptr.  The k-th KEPT feature becomes keypoint k with its own id and depth (the reference keys keyPointToTrackId by the
// feature index, keyframe.cpp:129).  The refusals of the mirror come before the call as std::invalid_argument; a refusal of
// the call throws and leaves the tables and the record as they were.
inline AdmittedTrackerFrame admitTrackerFrame(Context &ctx, MapTables M, std::int32_t slot, std::int32_t previousSlot, const TrackerFrameAdmission &frame) {
    M.require("admitTrackerFrame", M.KEYPOINTS | M.POSES | M.IDS | M.TIMES | M.LINKS | M.CENTRES | M.CAMERAS | M.FOCALS | M.DESC_BASES | M.FRAMES);
    const std::size_t nKf = M.keyframes.size(), n = frame.x.size();
    if (slot < 0 || (std::size_t)slot >= nKf || previousSlot < -1 || (std::size_t)(previousSlot + 1) > nKf || previousSlot == slot)
        throw std::invalid_argument("admitTrackerFrame: slot " + std::to_string(slot) + " or previous slot " + std::to_string(previousSlot) + " outside the table");
    KeyframeSlots &S = M.slots;
    if (S.id[slot] >= 0) throw std::invalid_argument("admitTrackerFrame: slot " + std::to_string(slot) + " holds keyframe " + std::to_string(S.id[slot]));
    if (previousSlot >= 0 && S.id[previousSlot] < 0) throw std::invalid_argument("admitTrackerFrame: previous slot " + std::to_string(previousSlot) + " is empty");
    if (frame.id < 0) throw std::invalid_argument("admitTrackerFrame: KfId " + std::to_string(frame.id));
    if (frame.y.size() != n || frame.depth.size() != n || frame.trackIds.size() != n || (!frame.validPixel.empty() && frame.validPixel.size() != n))
        throw std::invalid_argument("admitTrackerFrame: one y, depth and id (and validPixel) per tracker feature");
    ms_frame_admit_args args{};
    args.slot = slot;
    std::copy(frame.poseCW.begin(), frame.poseCW.end(), args.pose);
    args.depth_image = frame.depthImage; args.depth_width = frame.depthWidth; args.depth_height = frame.depthHeight; args.depth_stride = frame.depthStride;
    args.valid_mask = frame.validMask; args.mask_width = frame.maskWidth; args.mask_height = frame.maskHeight; args.mask_stride = frame.maskStride;
    AdmittedTrackerFrame out;
    const std::size_t cap = std::min(n, M.keyframes.stride());
    out.keyPointTrackIds.resize(cap); out.keyPointFeature.resize(cap);
    std::int32_t counts[4] = {0, 0, 0, 0};
    ctx.check(ms_frame_admit(ctx.get(), M.keyframes.mutableTable(), (int)nKf, (int)M.keyframes.stride(), (int)M.keyframes.mapPointCount(), M.keypoints->mutableX(),
                             M.keypoints->mutableY(), M.keypoints->mutableOctave(), M.keypoints->mutableDepth(), M.poses->pose(), frame.x.data(), frame.y.data(),
                             frame.trackIds.data(), frame.depth.data(), frame.validPixel.empty() ? nullptr : frame.validPixel.data(), (int)n, &args, out.keyPointTrackIds.data(),
                             out.keyPointFeature.data(), (int)cap, counts), "ms_frame_admit");
    out.keyPoints = (std::size_t)counts[0]; out.droppedByValidPixel = (std::size_t)counts[1]; out.droppedByMask = (std::size_t)counts[2];
    out.depthsFromImage = (std::size_t)counts[3];
    out.keyPointTrackIds.resize(out.keyPoints); out.keyPointFeature.resize(out.keyPoints);
    S.id[slot] = frame.id; S.t[slot] = frame.t;
    S.previous[slot] = previousSlot; S.next[slot] = -1;      // keyframe.cpp:82-83, then mapdb.cpp:84-87
    if (previousSlot >= 0) S.next[previousSlot] = slot;
    const auto &P = frame.poseCW;                            // cameraCenter() = -R^T t
    for (int j = 0; j < 3; ++j) S.cameraCenter[slot][j] = -(P[j] * P[3] + P[4 + j] * P[7] + P[8 + j] * P[11]);
    S.camera[slot] = frame.camera; S.focalLength[slot] = frame.focalLength;
    S.descBase[slot] = -1; S.frames[slot] = nullptr;
    return out;
}

// ---- a new keyframe from the extractor's output to the device tables (ms_keyframe_admit) ---------------------------------------------------
// What addKeyframeCommonOuter knows of the frame that becomes a keyframe (mapper_helpers.cpp:1186-1203): its KfId and time, poseCW, the
// pinhole stand-in of its camera, the tracker features' ids and depths (mapperInput.trackerFeatures) and, optionally, a DEVICE depth image
// standing in for frame->getDepth (float32, rows depthStride elements apart).
struct KeyframeAdmission {
    std::int32_t id = -1;
    double t = 0.0;
    DeviceKeyframePoses::Pose poseCW{};
    ms_pinhole camera{};
    std::int32_t focalLength = 0;
    std::vector<std::int32_t> trackIds;
    std::vector<float> trackDepths;
    bool hasTrackerFeatures = false;         // false: nobody is looked up, every depth comes from the image or is -1
    const float *depthImage = nullptr;
    std::int32_t depthWidth = 0, depthHeight = 0, depthStride = 0;
};

struct AdmittedKeyframe {
    std::size_t keyPoints = 0;
    std::vector<std::int32_t> keyPointTrackIds;              // what matchTrackedFeatures takes next
    BowVector bowVector;                                     // for BowIndex::add; empty without a BowIndex
};

// Keyframe::addFullFeatures (keyframe.cpp:95-116) and BowIndex::transform for frame `frame` of a device keypoint view (the extractor's
// ms_orb_device_view), into `slot`: ONE device call, nothing of the frame is downloaded but the 64 bytes per keypoint the host keeps.  Writes
// M.keyframes (the slot's row = -1), M.keypoints, M.poses, M.pool (reserve()) and M.slots.frames[slot], which must be a DeviceKeyframe(ctx, capacity);
// fills the slot's record: id, t, previous / next (the new keyframe follows `previousSlot`, -1 for the first), cameraCenter, camera, focalLength,
// descBase.  A refusal of the call throws and leaves the tables, the pool's fill and the record as they were.
inline AdmittedKeyframe admitKeyframe(Context &ctx, MapTables M, const ms_keypoints &view, int frame, std::int32_t slot, std::int32_t previousSlot,
                                      const KeyframeAdmission &kf, BowIndex *bowIndex) {
    M.require("admitKeyframe", M.KEYPOINTS | M.POSES | M.IDS | M.TIMES | M.LINKS | M.CENTRES | M.CAMERAS | M.FOCALS | M.DESC_BASES | M.FRAMES);
    const std::size_t nKf = M.keyframes.size();
    if (!M.pool) throw std::invalid_argument("admitKeyframe: no descriptor pool");
    if (slot < 0 || (std::size_t)slot >= nKf || previousSlot < -1 || (std::size_t)(previousSlot + 1) > nKf || previousSlot == slot)
        throw std::invalid_argument("admitKeyframe: slot " + std::to_string(slot) + " or previous slot " + std::to_string(previousSlot) + " outside the table");
    KeyframeSlots &S = M.slots;
    if (S.id[slot] >= 0) throw std::invalid_argument("admitKeyframe: slot " + std::to_string(slot) + " holds keyframe " + std::to_string(S.id[slot]));
    DeviceKeyframe *dk = S.frames[slot];
    if (!dk || dk->capacity() == 0) throw std::invalid_argument("admitKeyframe: slot " + std::to_string(slot) + " has no DeviceKeyframe with a capacity");
    if (kf.trackIds.size() != kf.trackDepths.size()) throw std::invalid_argument("admitKeyframe: one depth per tracker feature");
    // the device learns n; the pool hands out what the frame arrays could hold at most and gets the rest back
    const std::size_t room = std::min({dk->capacity(), M.keyframes.stride(), (std::size_t)std::max(view.capacity, 0), M.pool->size() - M.pool->used()});
    const std::size_t base = M.pool->reserve(room);
    static const std::int32_t noId = 0;                      // a non-null pointer for an empty list: "no tracker features" is the flag's to say
    static const float noDepth = 0.f;
    ms_admit_args args{};
    args.slot = slot; args.desc_base = (std::int32_t)base;
    std::copy(kf.poseCW.begin(), kf.poseCW.end(), args.pose);
    args.cam = kf.camera;
    args.levels_up = 4;                                      // bow_index.cpp:85
    args.vocab = bowIndex ? bowIndex->vocabulary() : nullptr;
    if (kf.hasTrackerFeatures) { args.track_ids = kf.trackIds.empty() ? &noId : kf.trackIds.data(); args.track_depth = kf.trackDepths.empty() ? &noDepth : kf.trackDepths.data(); }
    args.n_tracks = (std::int32_t)kf.trackIds.size();
    args.depth_image = kf.depthImage; args.depth_width = kf.depthWidth; args.depth_height = kf.depthHeight; args.depth_stride = kf.depthStride;
    AdmittedKeyframe out;
    std::vector<std::int32_t> word(dk->capacity());
    std::vector<double> weight(dk->capacity());
    out.keyPointTrackIds.resize(dk->capacity());
    const ms_admit_frame arrays = dk->admitFrame();
    const ms_admit_host host = dk->admitHost(out.keyPointTrackIds.data(), word.data(), weight.data());
    std::int32_t counts[3] = {0, 0, 0};
    const int rc = ms_keyframe_admit(ctx.get(), &view, frame, M.keyframes.mutableTable(), (int)nKf, (int)M.keyframes.stride(), (int)M.keyframes.mapPointCount(), M.keypoints->mutableX(),
                                     M.keypoints->mutableY(), M.keypoints->mutableOctave(), M.keypoints->mutableDepth(), M.pool->mutableDescriptor(), (int)(base + room),
                                     M.poses->pose(), &args, &arrays, &host, counts);
    if (rc != MS_OK) { M.pool->release(room); ctx.check(rc, "ms_keyframe_admit"); }
    const std::size_t n = (std::size_t)counts[0];
    M.pool->release(room - n);                               // the tail of the reservation nobody wrote
    dk->admitted(counts);
    out.keyPoints = n;
    out.keyPointTrackIds.resize(n); word.resize(n); weight.resize(n);
    if (bowIndex) BowIndex::assembleVector(word, weight, out.bowVector);
    S.id[slot] = kf.id; S.t[slot] = kf.t;
    S.previous[slot] = previousSlot; S.next[slot] = -1;      // keyframe.cpp:82-83, then the chain of addKeyframeCommonOuter
    if (previousSlot >= 0) S.next[previousSlot] = slot;
    const auto &P = kf.poseCW;                               // cameraCenter() = -R^T t
    for (int j = 0; j < 3; ++j) S.cameraCenter[slot][j] = -(P[j] * P[3] + P[4 + j] * P[7] + P[8 + j] * P[11]);
    S.camera[slot] = kf.camera; S.focalLength[slot] = kf.focalLength;
    S.descBase[slot] = (std::int32_t)base;
    return out;
}

// ---- fusing duplicate map points on the device tables (ms_map_fuse, ms_map_replace_pairs) ----------------------------------------------
// The fuse steps update M.keyframes, M.flags, M.live, M.observationCount (mp.observations.size() of every row as ms_observation_count leaves
// it, observationCountsOnDevice; the walk keeps it current, so one count serves a whole new-keyframe chain) and, when given, M.tracks.
// One keyframe as replaceDuplication reads it: its slot, its matcher features, poseCW (p_c = R p + t, row-major) and camera.
struct FuseKeyframe {
    std::int32_t slot = 0;
    const DeviceKeyframe *features = nullptr;
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    ms_pinhole camera{};
};
// The erased rows with their winners in the order of erasure -- what the caller's keyPointToTrackId.erase, its host MapPoint objects and
// trackIdToMapPoint bookkeeping are derived from -- the entries per outcome code of ms_map_fuse, fusedCount (codes 4-7) and how often
// direction 1 of deduplicateMapPoints gated again after an early stop.
struct FuseResult {
    std::vector<std::int32_t> erasedRows, erasedInto;
    std::array<std::int32_t, 8> counts{};
    unsigned fusedCount = 0, regates = 0;
};

// mp.observations.size() of every row, written into M.observationCount
inline void observationCountsOnDevice(Context &ctx, MapTables M) {
    M.require("observationCountsOnDevice", M.COUNTS | M.IDS);
    ctx.check(ms_observation_count(ctx.get(), M.keyframes.table(), (int)M.keyframes.size(), (int)M.keyframes.stride(), (int)M.keyframes.mapPointCount(), M.slots.id.data(),
                                   M.observationCount, nullptr, nullptr), "ms_observation_count");
}

namespace detail {
constexpr unsigned FUSE_PARTS = MapTables::FLAGS | MapTables::LIVE | MapTables::COUNTS;      // what every fuse step needs of the view

// replaceDuplication of `rows` against each of `keyframes`, in order, as ONE gate call, one scoring launch per keyframe and ONE ms_map_fuse
// on the lists where they lie.  Returns views_done.
inline std::size_t fuse_batch(Context &ctx, MapTables M, const FuseKeyframe *keyframes, std::size_t n, const std::vector<std::int32_t> &rows,
                              float margin, std::int32_t sourceSlot, const StaticSettings &settings, FuseResult &out) {
    std::vector<GateView> views(n);
    std::vector<const DeviceKeyframe *> kfs(n);
    for (std::size_t v = 0; v < n; ++v) {
        std::copy(keyframes[v].R, keyframes[v].R + 9, views[v].R); std::copy(keyframes[v].t, keyframes[v].t + 3, views[v].t);
        views[v].camera = keyframes[v].camera; views[v].threshold = margin; views[v].mode = MS_GATE_FUSE; views[v].indices = rows;
        kfs[v] = keyframes[v].features;
    }
    const DeviceGatedLists g = gate_and_score_device(ctx, *M.points, views, kfs, settings, 8);
    std::vector<ms_fuse_view> fv(n);
    for (std::size_t v = 0; v < n; ++v) fv[v] = ms_fuse_view{keyframes[v].slot, g.first[v], g.count[v]};
    const std::size_t ne = g.index.size();
    std::int32_t *erasedRows = reinterpret_cast<std::int32_t *>(g.extra), *erasedInto = erasedRows + ne;
    std::int32_t nErased = 0, counts[8] = {0}, viewsDone = 0;
    const MapTables::TrackWindow tw = M.trackWindow();
    ctx.check(ms_map_fuse(ctx.get(), M.keyframes.mutableTable(), (int)M.keyframes.size(), (int)M.keyframes.stride(), M.flags->mutableFlags(), M.live->mutableLive(), M.observationCount,
                          (int)M.keyframes.mapPointCount(), tw.mpTrack, tw.trackRow, tw.base, tw.window, g.keptEntry, g.topIdx, g.topDist, g.index.data(), (int)ne, fv.data(),
                          g.nKept.data(), (int)n, (int)HAMMING_DIST_THR_LOW, sourceSlot, nullptr, nullptr, nullptr, erasedRows, erasedInto, &nErased, counts, &viewsDone),
              "ms_map_fuse");
    const std::vector<std::int32_t> rowsDown = ctx.download(erasedRows, (std::size_t)nErased), intoDown = ctx.download(erasedInto, (std::size_t)nErased);
    out.erasedRows.insert(out.erasedRows.end(), rowsDown.begin(), rowsDown.end());
    out.erasedInto.insert(out.erasedInto.end(), intoDown.begin(), intoDown.end());
    for (int c = 0; c < 8; ++c) { out.counts[c] += counts[c]; if (c >= 4) out.fusedCount += (unsigned)counts[c]; }
    return (std::size_t)viewsDone;
}
}  // namespace detail

// deduplicateMapPoints (mapper_helpers.cpp:320-347) on the device tables; nothing of the map graph is on the host between its steps.
//   direction 1 (:330-334)  the current keyframe's valid rows, in keypoint order, against ALL remaining adjacent keyframes in one gate + score
//                           batch and one ms_map_fuse with source_slot = current.  The reference reads currentKeyframe.mapPoints live: when a
//                           replace put a new row into that slot the walk stops behind the view, the slot is read back (one row of kf_mp)
//                           and the rest is gated again.  A row an earlier view of a batch erased ends as outcome 1 in the later ones.
//   the union (:337-345)    ms_map_point_union over the adjacent slots as the tables are then, rows ascending
//   direction 2 (:346)      one view: the union against the current keyframe
// margin = getFocalLength(currentKeyframe) * relativeReprojectionErrorThreshold (:328), computed by the caller.  The graph filters of
// keyframe_matcher.cpp:429-440 run inside the walk, so every valid row is gated.
inline FuseResult deduplicateMapPoints(Context &ctx, MapTables M, const FuseKeyframe &current, const std::vector<FuseKeyframe> &adjacent, float margin, const StaticSettings &settings) {
    M.require("deduplicateMapPoints", detail::FUSE_PARTS | M.POINTS);
    const std::size_t nMp = M.keyframes.mapPointCount(), stride = M.keyframes.stride();
    if (current.slot < 0 || (std::size_t)current.slot >= M.keyframes.size()) throw std::invalid_argument("deduplicateMapPoints: current keyframe outside the table");
    FuseResult out;
    std::vector<std::int32_t> rows, adjacentSlots;
    for (std::size_t done = 0; done < adjacent.size();) {
        const std::vector<std::int32_t> slotRow = ctx.download(M.keyframes.table() + (std::size_t)current.slot * stride, stride);
        rows.clear();
        for (std::int32_t r : slotRow) if (r >= 0 && (std::size_t)r < nMp) rows.push_back(r);
        if (rows.empty()) break;
        if (done) ++out.regates;
        done += detail::fuse_batch(ctx, M, adjacent.data() + done, adjacent.size() - done, rows, margin, current.slot, settings, out);
    }
    for (const FuseKeyframe &k : adjacent) adjacentSlots.push_back(k.slot);
    rows = localMapPoints(ctx, M.keyframes, nullptr, adjacentSlots, -1, 0, false).row;
    if (!rows.empty()) detail::fuse_batch(ctx, M, &current, 1, rows, margin, -1, settings, out);
    return out;
}

// searchAndDeduplicate (loop_closer.cpp:567-591): loopMapPoints = the usable rows (neither BAD nor NOT_TRIANGULATED, :575-578) of the
// candidate keyframe's neighbours (slots; the caller's getNeighbors), a std::set and therefore a copy: every rigidly transformed keyframe
// is walked against the same list (source_slot = -1), margin 4.
inline FuseResult searchAndDeduplicate(Context &ctx, MapTables M, const std::vector<std::int32_t> &neighbourSlots, const std::vector<FuseKeyframe> &rigidlyTransformed,
                                       const StaticSettings &settings) {
    M.require("searchAndDeduplicate", detail::FUSE_PARTS | M.POINTS);
    FuseResult out;
    const std::vector<std::int32_t> rows = localMapPoints(ctx, M.keyframes, M.flags, neighbourSlots, -1, DeviceMapPointFlags::USABLE, false).row;
    if (!rows.empty() && !rigidlyTransformed.empty()) detail::fuse_batch(ctx, M, rigidlyTransformed.data(), rigidlyTransformed.size(), rows, 4.0f, -1, settings, out);
    return out;
}

// ---- matchLocalMapPoints on the device tables (ms_bound_mask, ms_search_bind) ----------------------------------------------------------
// matchLocalMapPoints (mapper_helpers.cpp:231-269) for the keyframe `current`: the usable rows of the adjacent keyframes that the current one
// does not list yet (:241-261; they come down once, as the gate takes its rows from the host), then ONE MS_GATE_SEARCH view with
// viewAngleLimitCos 0.5 (:304) and searchByProjection with the walk and both addObservations on the tables (searchByProjectionOnTables): the
// top-4 lists and the query arrays stay on the device, and neither the current keyframe's row of kf_mp nor n_obs is uploaded afterwards.
// M.observationCount stays current.  usable (optional) = current.features' DEVICE matcher mask (DeviceKeyframe::mutableUsable), cleared at each
// bound keypoint.  Returns at once on an empty list (:263).
inline SearchBindResult matchLocalMapPoints(Context &ctx, MapTables M, const FuseKeyframe &current, const std::vector<std::int32_t> &adjacentSlots, float threshold,
                                            const StaticSettings &settings, std::uint8_t *usable = nullptr, bool wantMatches = false) {
    M.require("matchLocalMapPoints", detail::FUSE_PARTS | M.POINTS);
    if (current.slot < 0 || (std::size_t)current.slot >= M.keyframes.size() || !current.features) throw std::invalid_argument("matchLocalMapPoints: current keyframe outside the table");
    GateView view;
    view.indices = localMapPoints(ctx, M.keyframes, M.flags, adjacentSlots, current.slot, DeviceMapPointFlags::USABLE, false).row;
    if (view.indices.empty()) return SearchBindResult{};
    std::copy(current.R, current.R + 9, view.R); std::copy(current.t, current.t + 3, view.t);
    view.camera = current.camera; view.threshold = threshold; view.cosLimit = 0.5f; view.mode = MS_GATE_SEARCH;
    return searchByProjectionOnTables(ctx, M, *current.features, view, current.slot, settings, usable, wantMatches);
}

// "Merge moved map points", loop_closer.cpp:531-546: loopClosure.mapPointMatches as (first, second) table rows, in order.  outcome per pair:
// 0 replaced (first by second) | 1 equal | 2 skipped by the `merged` rule.  counts stays zero; fusedCount = the replaced pairs.
inline FuseResult mergeMatchedMapPoints(Context &ctx, MapTables M, const std::vector<std::pair<std::int32_t, std::int32_t>> &matches, std::vector<std::uint8_t> *outcome = nullptr) {
    M.require("mergeMatchedMapPoints", detail::FUSE_PARTS);
    FuseResult out;
    const std::size_t n = matches.size();
    std::vector<std::int32_t> pairs(2 * n);
    for (std::size_t i = 0; i < n; ++i) { pairs[2 * i] = matches[i].first; pairs[2 * i + 1] = matches[i].second; }
    std::vector<std::uint8_t> oc(n, 0);
    std::int32_t *erasedRows = reinterpret_cast<std::int32_t *>(ctx.workspace(8 * n + 64)), *erasedInto = erasedRows + n, nErased = 0;
    const MapTables::TrackWindow tw = M.trackWindow();
    ctx.check(ms_map_replace_pairs(ctx.get(), M.keyframes.mutableTable(), (int)M.keyframes.size(), (int)M.keyframes.stride(), M.flags->mutableFlags(), M.live->mutableLive(),
                                   M.observationCount, (int)M.keyframes.mapPointCount(), tw.mpTrack, tw.trackRow, tw.base, tw.window, pairs.data(), (int)n, oc.data(), erasedRows, erasedInto,
                                   &nErased), "ms_map_replace_pairs");
    out.erasedRows = ctx.download(erasedRows, (std::size_t)nErased); out.erasedInto = ctx.download(erasedInto, (std::size_t)nErased);
    out.fusedCount = (unsigned)nErased;
    if (outcome) *outcome = oc;
    return out;
}

// ---- the partial map copy for the front end on the device tables (ms_map_extract) ---------------------------------------------------------
// What copyMap (mapper.cpp:281-326) hands the front end: the counts of the copy and, as DEVICE arrays this object owns, the source row of
// every destination row and the destination row of every source row (-1: not copied) -- what a caller translates its own row lists with.
struct MapExtract {
    std::size_t mapPoints = 0, observations = 0, droppedObservations = 0, tracks = 0, descriptors = 0;
    DeviceArray<std::int32_t> rowSource, rowDestination;
};

// MapDB(mapDB, activeKeyframes) (mapdb.cpp:116-159) from the tables `src` into the tables `dst`, compacted: ONE device call, nothing of either map
// walked on the host.  activeSlots = source slots in the order the destination gets them (ascending KfId, the std::set's order); destination slot i
// is activeSlots[i].  Reads src (never written); writes dst.keyframes, dst.points, dst.flags, dst.live, and dst.keypoints, dst.poses, dst.tracks,
// dst.pool (reserve()), dst.observationCount where both sides have them; fills dst.slots: id, t, cameraCenter, camera, focalLength and frames copied
// (the frames' matcher arrays are immutable and shared: the pointers are copied as they are, non-owning), previous / next translated to destination
// slots and cut where the neighbour is not active (mapdb.cpp:124-129), descBase from the call; the slots behind the active ones are emptied.
// The two row maps of the result are allocated by every call (MapExtract owns them): "nothing is allocated after warm-up" is the C entry point's
// property, not this function's; a caller that copies the map often and wants none keeps its own arrays and calls ms_map_extract.
// keyPointCounts (per SOURCE slot) stands in for frames[s]->keyPointCount() where a slot has no frame.  Left to the caller: referenceKeyframe
// (map_point.cpp:38-42), the scalar members of mapdb.cpp:150-158, bowIndex.  Throws std::invalid_argument before the device call for an active
// slot outside the table or empty, a destination with fewer slots than active keyframes, a different stride, a part present on one side only.
inline MapExtract extractMap(Context &ctx, MapTables src, const std::vector<std::int32_t> &activeSlots, MapTables dst, const std::vector<std::int32_t> &keyPointCounts = {}) {
    const unsigned perSlot = MapTables::IDS | MapTables::TIMES | MapTables::LINKS | MapTables::CENTRES | MapTables::CAMERAS | MapTables::FOCALS | MapTables::DESC_BASES | MapTables::FRAMES;
    src.require("extractMap", MapTables::POINTS | MapTables::FLAGS | perSlot);
    dst.require("extractMap (destination)", MapTables::POINTS | MapTables::FLAGS | MapTables::LIVE | perSlot);
    const std::size_t nKf = src.keyframes.size(), nActive = activeSlots.size(), stride = src.keyframes.stride();
    auto refuse = [](const std::string &what) { throw std::invalid_argument("extractMap: " + what); };
    if (dst.keyframes.stride() != stride) refuse("the destination's stride " + std::to_string(dst.keyframes.stride()) + " is not the source's " + std::to_string(stride));
    if (dst.keyframes.size() < nActive) refuse(std::to_string(nActive) + " active keyframes for a destination of " + std::to_string(dst.keyframes.size()) + " slots");
    for (std::int32_t s : activeSlots) {
        if (s < 0 || (std::size_t)s >= nKf) refuse("active slot " + std::to_string(s) + " outside the table");
        if (src.slots.id[s] < 0) refuse("active slot " + std::to_string(s) + " is empty");
    }
    if ((src.keypoints != nullptr) != (dst.keypoints != nullptr)) refuse("a keypoint table on one side only");
    if ((src.poses != nullptr) != (dst.poses != nullptr)) refuse("poses on one side only");
    if ((src.tracks != nullptr) != (dst.tracks != nullptr)) refuse("a track table on one side only");
    if ((src.pool != nullptr) != (dst.pool != nullptr)) refuse("a descriptor pool on one side only");
    if (src.tracks && (src.tracks->trackBase() != dst.tracks->trackBase() || src.tracks->window() != dst.tracks->window())) refuse("the track windows differ");
    if (!keyPointCounts.empty() && keyPointCounts.size() != nKf) refuse("one keypoint count per source slot");
    std::vector<std::int32_t> nKp(nActive, 0), where(nKf, -1);
    std::size_t total = 0;
    for (std::size_t i = 0; i < nActive; ++i) {
        const std::int32_t s = activeSlots[i];
        where[s] = (std::int32_t)i;
        if (!src.pool || src.slots.descBase[s] < 0) continue;
        if (!src.slots.frames[s] && keyPointCounts.empty()) refuse("active slot " + std::to_string(s) + " has descriptors, no frame and no keypoint count");
        nKp[i] = src.slots.frames[s] ? (std::int32_t)src.slots.frames[s]->keyPointCount() : keyPointCounts[s];
        total += (std::size_t)std::max(nKp[i], 0);
    }
    const std::size_t poolBase = dst.pool ? dst.pool->reserve(total) : 0;
    MapExtract out;
    out.rowSource = DeviceArray<std::int32_t>(ctx, dst.keyframes.mapPointCount());
    out.rowDestination = DeviceArray<std::int32_t>(ctx, src.keyframes.mapPointCount());
    const DeviceMapPoints &P = *src.points;
    DeviceMapPoints &Q = *dst.points;
    const ms_map_extract_src S{src.keyframes.table(), src.flags->flags(), src.live ? src.live->live() : nullptr, P.position(), P.norm(), P.minDistance(), P.maxDistance(), P.descriptor(),
                               src.tracks ? src.tracks->mpTrack() : nullptr, src.keypoints ? src.keypoints->x() : nullptr, src.keypoints ? src.keypoints->y() : nullptr,
                               src.keypoints ? src.keypoints->octave() : nullptr, src.keypoints ? src.keypoints->depth() : nullptr, src.poses ? src.poses->pose() : nullptr,
                               src.tracks ? src.tracks->trackRow() : nullptr, src.poolDescriptor(), (std::int32_t)nKf, (std::int32_t)stride, (std::int32_t)src.keyframes.mapPointCount(),
                               src.tracks ? src.tracks->trackBase() : 0, src.tracks ? (std::int32_t)src.tracks->window() : 0, src.poolSize()};
    const ms_map_extract_dst D{dst.keyframes.mutableTable(), dst.flags->mutableFlags(), dst.live->mutableLive(), Q.mutablePosition(), Q.mutableNorm(), Q.mutableMinDistance(),
                               Q.mutableMaxDistance(), Q.mutableDescriptor(), dst.tracks ? dst.tracks->mpTrack() : nullptr, dst.keypoints ? dst.keypoints->mutableX() : nullptr,
                               dst.keypoints ? dst.keypoints->mutableY() : nullptr, dst.keypoints ? dst.keypoints->mutableOctave() : nullptr,
                               dst.keypoints ? dst.keypoints->mutableDepth() : nullptr, dst.poses ? dst.poses->pose() : nullptr, dst.tracks ? dst.tracks->trackRow() : nullptr,
                               dst.pool ? dst.pool->mutableDescriptor() + 8 * poolBase : nullptr, dst.observationCount, out.rowSource.data(), out.rowDestination.data(),
                               (std::int32_t)dst.keyframes.size(), (std::int32_t)dst.keyframes.mapPointCount(), (std::int32_t)total};
    std::vector<std::int32_t> base(std::max<std::size_t>(nActive, 1), -1);
    std::int32_t counts[5] = {0, 0, 0, 0, 0};
    const int rc = ms_map_extract(ctx.get(), &S, &D, src.slots.id.data(), activeSlots.data(), (int)nActive, src.pool ? src.slots.descBase.data() : nullptr, src.pool ? nKp.data() : nullptr,
                                  base.data(), counts);
    if (rc != MS_OK) { if (dst.pool) dst.pool->release(total); ctx.check(rc, "ms_map_extract"); }
    out.mapPoints = (std::size_t)counts[0]; out.observations = (std::size_t)counts[1]; out.droppedObservations = (std::size_t)counts[2];
    out.tracks = (std::size_t)counts[3]; out.descriptors = (std::size_t)counts[4];
    const KeyframeSlots &A = src.slots;
    KeyframeSlots &B = dst.slots;
    auto translated = [&](std::int32_t s) { return s >= 0 && (std::size_t)s < nKf ? where[s] : -1; };      // mapdb.cpp:124-129
    for (std::size_t i = 0; i < dst.keyframes.size(); ++i) {
        const bool copied = i < nActive;
        const std::int32_t s = copied ? activeSlots[i] : 0;
        B.id[i] = copied ? A.id[s] : -1;
        B.previous[i] = copied ? translated(A.previous[s]) : -1;
        B.next[i] = copied ? translated(A.next[s]) : -1;
        B.descBase[i] = copied && base[i] >= 0 ? (std::int32_t)poolBase + base[i] : -1;
        B.frames[i] = copied ? A.frames[s] : nullptr;
        if (!copied) continue;
        B.t[i] = A.t[s]; B.cameraCenter[i] = A.cameraCenter[s]; B.camera[i] = A.camera[s]; B.focalLength[i] = A.focalLength[s];
    }
    return out;
}

// copyMap, mapper.cpp:281-310: with `partial` (copyPartialMapToFrontend) the keyframes of computeAdjacentKeyframes(latest, 5, adjacentSpaceSize)
// plus the latest one, by ascending KfId; otherwise, or without a latest keyframe (latestSlot == -1, :289-292), every keyframe of the back end's
// map (MapDB(mapDB), mapdb.cpp:98-114, through the same call).  Then extractMap.  Exchanging the front end's tables for the new ones under the
// reference's frontendMapMutex, and fastForward (:317-321), are the caller's.
inline MapExtract copyMapToFrontend(Context &ctx, MapTables backend, std::int32_t latestSlot, int adjacentSpaceSize, bool partial, MapTables frontend,
                                    const std::vector<std::int32_t> &keyPointCounts = {}) {
    backend.require("copyMapToFrontend", MapTables::IDS);
    std::vector<std::int32_t> active;
    if (partial && latestSlot != -1) {
        constexpr int minCovisibilities = 5;                 // :296
        active = computeAdjacentKeyframes(ctx, backend, latestSlot, minCovisibilities, adjacentSpaceSize);
        active.push_back(latestSlot);
    } else {
        for (std::size_t k = 0; k < backend.slots.id.size(); ++k) if (backend.slots.id[k] >= 0) active.push_back((std::int32_t)k);
    }
    for (std::int32_t s : active)
        if (s < 0 || (std::size_t)s >= backend.slots.id.size()) throw std::invalid_argument("copyMapToFrontend: slot " + std::to_string(s) + " outside the table");
    std::sort(active.begin(), active.end(), [&](std::int32_t a, std::int32_t b) { return backend.slots.id[a] < backend.slots.id[b]; });      // std::set<KfId>
    return extractMap(ctx, backend, active, frontend, keyPointCounts);
}

// ---- the viewer map and the point-cloud record on the device tables (ms_map_publish) ------------------------------------------------------
// The record state of updatePointCloudRecording on the device: the last recorded position and the state (0 never recorded, 1 recorded,
// 2 removed) of every table row.  It starts empty; grow() keeps what is there and puts zeros behind it, the caller's step when the map-point
// table grows.  It never shrinks.
class DeviceMapPointRecords {
public:
    explicit DeviceMapPointRecords(Context &ctx) : ctx_(&ctx) {}
    void grow(std::size_t rows) {
        if (rows <= n_) return;
        std::vector<float> pos = pos_.download();
        std::vector<std::uint8_t> state = state_.download();
        pos.resize(3 * rows, 0.0f); state.resize(rows, 0);
        pos_ = DeviceArray<float>(*ctx_, 3 * rows); state_ = DeviceArray<std::uint8_t>(*ctx_, rows);
        pos_.upload(0, 3 * rows, pos.data()); state_.upload(0, rows, state.data());
        n_ = rows;
    }
    std::size_t size() const { return n_; }
    float *position() { return pos_.data(); }
    std::uint8_t *state() { return state_.data(); }
    std::vector<std::uint8_t> downloadState() const { return state_.download(); }
private:
    Context *ctx_;
    std::size_t n_ = 0;
    DeviceArray<float> pos_;
    DeviceArray<std::uint8_t> state_;
};

// ViewerMapPoint / ViewerKeyframe (viewer_data_publisher.hpp) as the tables can fill them: `row` stands in for the MpId; origPoseWC and the
// stereo clouds stay with the caller, who holds them.
struct ViewerMapPoint {
    std::int32_t row = -1;
    std::array<float, 3> position{}, normal{}, color{};
    int status = 0;
    bool localMap = false, nowVisible = false;
};
struct ViewerKeyframe {
    std::int32_t id = -1;
    bool localMap = false, current = false;
    std::array<float, 16> poseWC{};                          // row-major 4 x 4
    std::vector<int> neighbors;                              // indices into ViewerMap::keyframes
};
struct ViewerMap {
    std::vector<ViewerMapPoint> mapPoints;
    std::vector<ViewerKeyframe> keyframes;                   // ascending KfId
};
// rows that lie on the device, e.g. workspaceBA.localMpIds as the last ms_ba_window_lists left them; any order, repeats allowed
struct DeviceRows {
    const std::int32_t *rows = nullptr;
    std::size_t count = 0;
};

// publishMapForViewer (mapper_helpers.cpp:814-879) from the tables: ONE ms_map_publish call for the map points and every keyframe's poseWC,
// ONE getNeighbors call over all keyframes for the neighbour indices (:862-872).  adjacentSlots is mapDB.adjacentKfIds as slots (:848-852).
// An empty map of keyframes gives an empty result (:820).  Colours are not a table of MapTables: they come out as 0.  Writes nothing.
inline ViewerMap publishMapForViewer(Context &ctx, MapTables M, const std::vector<std::int32_t> &adjacentSlots, DeviceRows localRows, int minNeighbourCovisibilities) {
    M.require("publishMapForViewer", M.POINTS | M.FLAGS | M.LIVE | M.POSES | M.IDS | M.LINKS);
    const std::size_t nKf = M.keyframes.size(), nMp = M.keyframes.mapPointCount();
    for (std::int32_t k : adjacentSlots)
        if (k < 0 || (std::size_t)k >= nKf) throw std::invalid_argument("publishMapForViewer: adjacent slot " + std::to_string(k) + " outside the table");
    if (localRows.count && !localRows.rows) throw std::invalid_argument("publishMapForViewer: local rows without an array");
    std::vector<std::int32_t> order;                         // mapDB.keyframes: the slots by ascending KfId
    for (std::size_t k = 0; k < nKf; ++k) if (M.slots.id[k] >= 0) order.push_back((std::int32_t)k);
    std::sort(order.begin(), order.end(), [&](std::int32_t a, std::int32_t b) { return M.slots.id[a] < M.slots.id[b]; });
    ViewerMap out;
    if (order.empty()) return out;
    const std::int32_t current = order.back();               // mapDB.keyframes.rbegin()
    const ms_map_publish_args args{MS_PUBLISH_VIEW, current, 0};
    std::vector<std::int32_t> row(nMp);
    std::vector<float> pos(3 * nMp), norm(3 * nMp), color(3 * nMp), poseWC(16 * order.size());
    std::vector<std::uint8_t> status(nMp), bits(nMp);
    std::int32_t counts[8] = {0};
    ctx.check(ms_map_publish(ctx.get(), M.points->position(), M.points->norm(), M.flags->flags(), M.live->live(), M.observationCount, nullptr, (int)nMp, M.keyframes.table(),
                             (int)nKf, (int)M.keyframes.stride(), M.poses->pose(), localRows.rows, (int)localRows.count, nullptr, nullptr, &args, order.data(),
                             (int)order.size(), row.data(), pos.data(), norm.data(), color.data(), status.data(), bits.data(), (int)nMp, nullptr, nullptr, nullptr, nullptr, 0,
                             poseWC.data(), counts), "ms_map_publish");
    out.mapPoints.resize((std::size_t)counts[0]);
    for (std::size_t k = 0; k < out.mapPoints.size(); ++k) {
        ViewerMapPoint &p = out.mapPoints[k];
        p.row = row[k]; p.status = status[k]; p.localMap = (bits[k] & 1) != 0; p.nowVisible = (bits[k] & 2) != 0;
        for (int a = 0; a < 3; ++a) { p.position[a] = pos[3 * k + a]; p.normal[a] = norm[3 * k + a]; p.color[a] = color[3 * k + a]; }
    }
    std::vector<int> inds(nKf, -1);                          // :841-846
    std::vector<NeighborQuery> queries(order.size());
    out.keyframes.resize(order.size());
    for (std::size_t i = 0; i < order.size(); ++i) {
        const std::int32_t k = order[i];
        inds[k] = (int)i;
        ViewerKeyframe &kf = out.keyframes[i];
        kf.id = M.slots.id[k];
        kf.localMap = std::find(adjacentSlots.begin(), adjacentSlots.end(), k) != adjacentSlots.end();
        kf.current = k == current;
        std::copy(poseWC.begin() + 16 * i, poseWC.begin() + 16 * (i + 1), kf.poseWC.begin());
        queries[i] = NeighborQuery{k, M.slots.previous[k], M.slots.next[k], minNeighbourCovisibilities, false};
    }
    const std::vector<std::vector<std::int32_t>> neighbours = getNeighbors(ctx, M.keyframes, M.flags, queries);
    for (std::size_t i = 0; i < order.size(); ++i) {
        for (std::int32_t k : neighbours[i]) out.keyframes[i].neighbors.push_back(inds.at((std::size_t)k));      // inds.at(kfId), :870
        std::sort(out.keyframes[i].neighbors.begin(), out.keyframes[i].neighbors.end());                          // the std::map walk: ascending KfId
    }
    return out;
}

// MapPointRecord as updatePointCloudRecording fills it (:892-906), keyed by table row.
struct MapPointRecord {
    struct Position { float t; std::array<float, 3> p; };
    std::vector<Position> positions;
    std::array<float, 3> normal{};
    bool removed = false;
};

// updatePointCloudRecording (mapper_helpers.cpp:881-909) from the tables: ONE ms_map_publish call brings down the CHANGES since the last call
// (new, moved and removed points), and they are applied to hostRecords as :892-906 does.  M.observationCount must be current
// (observationCountsOnDevice, or the chain that keeps it).  `records` grows to the table's rows.  A NEW event on a row that already has a record
// -- the table reused a removed row, which the reference's ids never do -- starts that row's record again.  Returns the number of events.
inline std::size_t updatePointCloudRecording(Context &ctx, MapTables M, DeviceMapPointRecords &records, float t, std::map<std::int32_t, MapPointRecord> &hostRecords,
                                             int minObservations = 4) {
    M.require("updatePointCloudRecording", M.POINTS | M.FLAGS | M.LIVE | M.COUNTS);
    const std::size_t nMp = M.keyframes.mapPointCount();      // the record reads no keyframe table: the call gets none
    if (minObservations < 0) throw std::invalid_argument("updatePointCloudRecording: minObservations < 0");
    records.grow(nMp);
    const ms_map_publish_args args{MS_PUBLISH_RECORD, -1, minObservations};
    std::vector<std::int32_t> row(nMp);
    std::vector<std::uint8_t> kind(nMp);
    std::vector<float> pos(3 * nMp), norm(3 * nMp);
    std::int32_t counts[8] = {0};
    ctx.check(ms_map_publish(ctx.get(), M.points->position(), M.points->norm(), M.flags->flags(), M.live->live(), M.observationCount, nullptr, (int)nMp, nullptr, 0,
                             (int)M.keyframes.stride(), nullptr, nullptr, 0, records.position(), records.state(), &args, nullptr, 0,
                             nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, row.data(), kind.data(), pos.data(), norm.data(), (int)nMp, nullptr, counts),
              "ms_map_publish");
    for (std::size_t k = 0; k < (std::size_t)counts[1]; ++k) {
        const std::array<float, 3> p{pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]}, n{norm[3 * k], norm[3 * k + 1], norm[3 * k + 2]};
        if (kind[k] == 1) {                                  // :892-894
            MapPointRecord r;
            r.positions.push_back({t, p}); r.normal = n;
            hostRecords[row[k]] = r;
        } else if (kind[k] == 2) {                           // :895-898
            MapPointRecord &r = hostRecords.at(row[k]);
            r.positions.push_back({t, p}); r.normal = n;
        } else {                                             // :902-907
            MapPointRecord &r = hostRecords.at(row[k]);
            r.removed = true;
            r.positions.push_back({t, p});
        }
    }
    return (std::size_t)counts[1];
}

}  // namespace mi355slam
