// map_tables_smoke.cpp -- MapTables::require (host/mi355slam/map_tables.hpp) as every map-table entry point of the host mirror uses it.
//   map_tables_smoke --no-gpu   the mirror compiles and links
//   map_tables_smoke --gpu      on the smallest tables that can still disagree (3 slots, stride 8, 9 map points, a pool of 4 descriptors):
//                               every call with exactly one thing wrong is turned away with std::invalid_argument("<function>: ...") and
//                               leaves kf_mp, the flags and the live bytes as they were uploaded; then one passing call per function.
// The cases are the std::invalid_argument conditions the entry points had before they took the view, one case per elementary condition
// (a vector too short, a table one row short, a required part null, a slot equal to the slot count):
//   DeviceObservationLists::build 5   retriangulateCurrent 2   matchTrackedFeatures 13   unboundMasks 2   createNewMapPoints 17
//   localBundleAdjustOnTables 9   poseBundleAdjustOnTables 9   cullMap 8   computeAdjacentKeyframes 5   observationCountsOnDevice 1
//   deduplicateMapPoints 5   searchAndDeduplicate 4   matchLocalMapPoints 6   mergeMatchedMapPoints 4   tryLoopClosureOnTables 9        = 99
// updateMapPoints and searchByProjectionOnTables had none of their own.  Two conditions are met only after device work and are not listed:
// a link that leaves the table in computeAdjacentKeyframes' walk from the parents, and a chain that does not reach the candidate in
// tryLoopClosureOnTables' accept gates.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>
#include "mi355slam/loop_closer.hpp"

using namespace mi355slam;

namespace {

constexpr int kKf = 3, kStride = 8, kMp = 9, kPool = 4, kCur = 2;
const ms_pinhole kCam{500.0, 500.0, 320.0, 240.0, 640, 480};

// three keyframes side by side looking down +z at eight points; row 8 is free
struct Scene {
    std::vector<DeviceKeyframePoses::Pose> pose;
    std::vector<DeviceMapPoints::Vec3d> position;
    std::vector<std::vector<std::int32_t>> kfMp;
    std::vector<KeyPointVector> keyPoints;
    std::vector<std::uint8_t> flags, live;
    std::vector<KeyPoint::Descriptor> pool;
    KeyframeSlots slots;
    Scene() {
        for (int r = 0; r < kMp; ++r) {
            position.push_back({0.2 * (r - 4), 0.1 * (r % 3 - 1), 4.0 + 0.1 * r});
            flags.push_back(r < 8 ? 3 : 0); live.push_back(r < 8 ? 1 : 0);
        }
        for (int i = 0; i < kPool; ++i) { KeyPoint::Descriptor d; d.fill(0x01010101u * (unsigned)(i + 1)); pool.push_back(d); }
        for (int k = 0; k < kKf; ++k) {
            pose.push_back({1, 0, 0, -0.1 * k, 0, 1, 0, 0, 0, 0, 1, 0});
            kfMp.push_back(std::vector<std::int32_t>(kStride, -1));
            KeyPointVector kps;
            for (int j = 0; j < kStride; ++j) {
                KeyPoint kp{};
                kp.pt.x = 10.0f + 30.0f * j; kp.pt.y = 20.0f;
                if (j < 4) {                                 // bound to row 2 k + j, at its projection
                    const int r = 2 * k + j;
                    kfMp[k][j] = r;
                    const double x = position[r][0] - 0.1 * k, y = position[r][1], z = position[r][2];
                    kp.pt.x = (float)(kCam.fx * x / z + kCam.cx); kp.pt.y = (float)(kCam.fy * y / z + kCam.cy);
                }
                const double bx = (kp.pt.x - kCam.cx) / kCam.fx, by = (kp.pt.y - kCam.cy) / kCam.fy, norm = std::sqrt(bx * bx + by * by + 1.0);
                kp.bearing = {bx / norm, by / norm, 1.0 / norm};
                kp.descriptor.fill(0x00010001u * (unsigned)(8 * k + j + 1));
                kps.push_back(kp);
            }
            keyPoints.push_back(kps);
            slots.id.push_back(10 + k); slots.t.push_back(k == kCur ? 10.0 : (double)k);
            slots.previous.push_back(k - 1); slots.next.push_back(k + 1 < kKf ? k + 1 : -1);
            slots.cameraCenter.push_back({0.1 * k, 0.0, 0.0});
            slots.camera.push_back(kCam); slots.focalLength.push_back(500);
            slots.descBase.push_back(k == 0 ? 0 : -1);       // slot 0's first four keypoints have their descriptors in the pool
        }
    }
};

// the tables of the scene, and beside each one that a check reads a twin that is one row (or one slot, or one column) off
struct Tables {
    Context &ctx;
    DeviceKeyframeMapPoints keyframes;
    DeviceMapPoints points, points8;
    DeviceMapPointFlags flags, flags8;
    DeviceMapPointLive live, live8;
    DeviceKeypointTable keypoints, keypoints2, keypointsWide;
    DeviceKeyframePoses poses, poses2;
    DeviceTrackTable tracks, tracks8;
    DeviceDescriptorPool pool;
    DeviceArray<std::int32_t> nObs;
    DeviceObservationLists lists;
    std::vector<std::unique_ptr<DeviceKeyframe>> frames;
    static DeviceMapPoints pointsOf(Context &c, const Scene &S, std::size_t n) {
        return DeviceMapPoints(c, std::vector<DeviceMapPoints::Vec3d>(S.position.begin(), S.position.begin() + (std::ptrdiff_t)n), std::vector<DeviceMapPoints::Vec3f>(n, {0, 0, 1}),
                               std::vector<float>(n, 0.1f), std::vector<float>(n, 100.0f), std::vector<KeyPoint::Descriptor>(n, S.pool[0]));
    }
    Tables(Context &c, Scene &S)
        : ctx(c), keyframes(c, kKf, kStride, kMp), points(pointsOf(c, S, kMp)), points8(pointsOf(c, S, kMp - 1)), flags(c, S.flags),
          flags8(c, std::vector<std::uint8_t>(kMp - 1, 3)), live(c, S.live), live8(c, std::vector<std::uint8_t>(kMp - 1, 1)), keypoints(c, kKf, kStride),
          keypoints2(c, kKf - 1, kStride), keypointsWide(c, kKf, kStride + 1), poses(c, S.pose), poses2(c, std::vector<DeviceKeyframePoses::Pose>(S.pose.begin(), S.pose.end() - 1)),
          tracks(c, kMp, 0, 16), tracks8(c, kMp - 1, 0, 16), pool(c, S.pool), nObs(c, kMp), lists(c, 4, 8) {
        for (int k = 0; k < kKf; ++k) {
            keyframes.update((std::size_t)k, S.kfMp[k]);
            std::vector<float> x, y;
            for (const KeyPoint &kp : S.keyPoints[k]) { x.push_back(kp.pt.x); y.push_back(kp.pt.y); }
            keypoints.update((std::size_t)k, x, y, std::vector<std::int32_t>(kStride, 0), {});
            KeyframeFeatures f;
            f.keyPoints = &S.keyPoints[k]; f.usable.assign(kStride, 1);
            frames.emplace_back(new DeviceKeyframe(c, f));
            S.slots.frames.push_back(frames.back().get());
        }
        nObs.fill(0);
    }
    MapTables view(KeyframeSlots &slots) {
        MapTables M{keyframes, slots};
        M.points = &points; M.flags = &flags; M.live = &live; M.keypoints = &keypoints; M.poses = &poses; M.tracks = &tracks; M.pool = &pool;
        M.observationCount = nObs.data(); M.lists = &lists;
        return M;
    }
};

int g_cases = 0, g_failed = 0;

using Mutate = std::function<void(MapTables &, KeyframeSlots &)>;
using Call = std::function<void(MapTables)>;

// `call` on the consistent view with `mutate` applied must throw std::invalid_argument whose text starts with "who: "
void reject(Tables &T, const Scene &S, const char *who, const char *what, const Mutate &mutate, const Call &call) {
    KeyframeSlots slots = S.slots;
    MapTables M = T.view(slots);
    mutate(M, slots);
    ++g_cases;
    try {
        call(M);
        std::printf("%s accepted %s\n", who, what);
    } catch (const std::invalid_argument &e) {
        const std::size_t n = std::strlen(who);
        if (std::strncmp(e.what(), who, n) == 0 && std::strncmp(e.what() + n, ": ", 2) == 0) return;
        std::printf("%s, %s: the message is \"%s\"\n", who, what, e.what());
    } catch (const std::exception &e) {
        std::printf("%s, %s: not std::invalid_argument but \"%s\"\n", who, what, e.what());
    }
    ++g_failed;
}

const Mutate kNothing = [](MapTables &, KeyframeSlots &) {};
#define SHORT(member) Mutate([](MapTables &, KeyframeSlots &s) { s.member.pop_back(); })
#define PART(statement) Mutate([&T](MapTables &M, KeyframeSlots &) { (void)T; statement; })

FuseKeyframe fuseKeyframe(const Scene &S, Tables &T, int k) {
    FuseKeyframe f;
    f.slot = k; f.features = T.frames[(std::size_t)k].get(); f.camera = kCam;
    f.t[0] = S.pose[(std::size_t)k][3];
    return f;
}

int gpu() {
    Context ctx(0);
    Parameters prm;
    const StaticSettings st(prm);
    Scene S;
    Tables T(ctx, S);
    const std::vector<std::int32_t> kfBefore = ctx.download(T.keyframes.table(), (std::size_t)kKf * kStride);
    const std::vector<std::uint8_t> flagsBefore = ctx.download(T.flags.flags(), (std::size_t)kMp), liveBefore = T.live.download();

    // the four groups of conditions most functions share
    const std::vector<std::pair<const char *, Mutate>> pointTables{{"points one row short", PART(M.points = &T.points8)}, {"flags one row short", PART(M.flags = &T.flags8)},
                                                                   {"live one row short", PART(M.live = &T.live8)}};
    const std::vector<std::pair<const char *, Mutate>> keypointTables{{"keypoints one slot short", PART(M.keypoints = &T.keypoints2)},
                                                                      {"keypoints one column wide", PART(M.keypoints = &T.keypointsWide)}};
    const std::pair<const char *, Mutate> cameras{"camera short", SHORT(camera)}, focals{"focal length short", SHORT(focalLength)}, ids{"id short", SHORT(id)},
        bases{"descriptor base short", SHORT(descBase)}, poses{"poses one slot short", PART(M.poses = &T.poses2)}, frames{"frames short", SHORT(frames)},
        tracks{"tracks one row short", PART(M.tracks = &T.tracks8)}, counts{"no observation counts", PART(M.observationCount = nullptr)};
    auto all = [&](const char *who, const std::vector<std::pair<const char *, Mutate>> &cases, const Call &call) {
        for (const auto &c : cases) reject(T, S, who, c.first, c.second, call);
    };

    ObservationSelection sel;
    sel.slot = kCur;
    const Call build = [&](MapTables M) { M.lists->build(M, true, sel, 0); };
    all("DeviceObservationLists::build", {ids, bases, keypointTables[0], keypointTables[1], pointTables[1]}, build);

    all("retriangulateCurrent", {cameras, focals}, [&](MapTables M) { retriangulateCurrent(ctx, M, kCur, st, TriangulationMethod::TME); });

    TrackedFrame frame;
    frame.slot = kCur; frame.poseCW = S.pose[kCur]; frame.keyPointToTrackId.assign(kStride, -1);
    const std::vector<std::int32_t> freeRows{8};
    const Call tracked = [&](MapTables M) { matchTrackedFeatures(ctx, M, frame, freeRows, st); };
    all("matchTrackedFeatures", {cameras, focals, ids, bases, poses, pointTables[0], pointTables[1], pointTables[2], tracks, keypointTables[0], keypointTables[1]}, tracked);
    TrackedFrame outside = frame;
    outside.slot = kKf;
    reject(T, S, "matchTrackedFeatures", "slot = slot count", kNothing, [&](MapTables M) { matchTrackedFeatures(ctx, M, outside, freeRows, st); });
    TrackedFrame described = frame;
    described.slot = 0;                                      // slot 0 has descriptors
    reject(T, S, "matchTrackedFeatures", "descriptors and no pool", PART(M.pool = nullptr), [&](MapTables M) { matchTrackedFeatures(ctx, M, described, freeRows, st); });

    reject(T, S, "unboundMasks", "slot = slot count", kNothing, [&](MapTables M) { unboundMasks(ctx, M, {0, kKf}); });
    reject(T, S, "unboundMasks", "a slot without a frame", Mutate([](MapTables &, KeyframeSlots &s) { s.frames[1] = nullptr; }), [&](MapTables M) { unboundMasks(ctx, M, {0, 1}); });

    const std::vector<DeviceKeyframePoses::Pose> shortPoses(S.pose.begin(), S.pose.end() - 1);
    auto create = [&](std::int32_t slot, std::vector<std::int32_t> adjacent, TriangulationMethod method, const std::vector<DeviceKeyframePoses::Pose> *hostPoses) {
        return Call([&ctx, &st, &freeRows, slot, adjacent, method, hostPoses](MapTables M) { createNewMapPoints(ctx, M, slot, adjacent, freeRows, st, method, hostPoses); });
    };
    const Call created = create(kCur, {0, 1}, TriangulationMethod::TME, &S.pose);
    all("createNewMapPoints", {cameras, focals, ids, bases, poses, frames, pointTables[0], pointTables[1], pointTables[2], keypointTables[0], keypointTables[1]}, created);
    reject(T, S, "createNewMapPoints", "slot = slot count", kNothing, create(kKf, {0, 1}, TriangulationMethod::TME, &S.pose));
    reject(T, S, "createNewMapPoints", "FIRST_LAST", kNothing, create(kCur, {0, 1}, TriangulationMethod::FIRST_LAST, &S.pose));
    reject(T, S, "createNewMapPoints", "no frame in the current slot", Mutate([](MapTables &, KeyframeSlots &s) { s.frames[kCur] = nullptr; }), created);
    reject(T, S, "createNewMapPoints", "host poses one slot short", kNothing, create(kCur, {0, 1}, TriangulationMethod::TME, &shortPoses));
    reject(T, S, "createNewMapPoints", "adjacent slot = slot count", kNothing, create(kCur, {kKf}, TriangulationMethod::TME, &S.pose));
    reject(T, S, "createNewMapPoints", "no frame in an adjacent slot", Mutate([](MapTables &, KeyframeSlots &s) { s.frames[0] = nullptr; }), created);

    Parameters early = prm;
    early.minVisibleMapPointsInCurrentFrameBA = 1000;        // the passing call stops at the early-out of :235-240
    auto localBa = [&](std::vector<std::int32_t> adjacent) {
        return Call([&ctx, &st, &early, adjacent](MapTables M) { localBundleAdjustOnTables(ctx, M, kCur, adjacent, PoseEdgeBuilder(), 20, early, st); });
    };
    all("localBundleAdjustOnTables", {ids, cameras, focals, poses, pointTables[0], pointTables[1], counts}, localBa({0, 1}));
    reject(T, S, "localBundleAdjustOnTables", "adjacent slot = slot count", kNothing, localBa({0, kKf}));
    reject(T, S, "localBundleAdjustOnTables", "an adjacent slot that is empty", Mutate([](MapTables &, KeyframeSlots &s) { s.id[1] = -1; }), localBa({0, 1}));

    DevicePoseAdjuster adjuster(ctx, 64, st);
    const PoseOdometryEdge edge;
    auto poseBa = [&](std::int32_t slot) { return Call([&, slot](MapTables M) { poseBundleAdjustOnTables(ctx, M, adjuster, slot, -1, edge, prm, st); }); };
    all("poseBundleAdjustOnTables", {cameras, focals, poses, keypointTables[0], keypointTables[1], pointTables[0], pointTables[1], pointTables[2]}, poseBa(kCur));
    reject(T, S, "poseBundleAdjustOnTables", "slot = slot count", kNothing, poseBa(kKf));

    CullSettings cs;
    cs.minMapPointCullingAge = 100.0; cs.minObservationsForBA = 2; cs.keyframeCullMaxCriticalRatio = 0.0;
    auto cull = [&](std::vector<std::int32_t> adjacent) { return Call([&ctx, &cs, adjacent](MapTables M) { cullMap(ctx, M, kCur, adjacent, {}, cs); }); };
    all("cullMap", {{"previous short", SHORT(previous)}, {"next short", SHORT(next)}, ids, {"time short", SHORT(t)}, pointTables[2], pointTables[1],
                    {"cullMapPoints without flags", PART(M.flags = nullptr)}}, cull({0}));
    reject(T, S, "cullMap", "adjacent slot = slot count", kNothing, cull({kKf}));

    auto adjacentOf = [&](std::int32_t current) { return Call([&ctx, current](MapTables M) { computeAdjacentKeyframes(ctx, M, current, 1, 20); }); };
    all("computeAdjacentKeyframes", {{"previous short", SHORT(previous)}, {"next short", SHORT(next)}, {"camera centre short", SHORT(cameraCenter)},
                                     {"a link = slot count", Mutate([](MapTables &, KeyframeSlots &s) { s.previous[kCur] = kKf; })}}, adjacentOf(kCur));
    reject(T, S, "computeAdjacentKeyframes", "current = slot count", kNothing, adjacentOf(kKf));

    const Call countsOnDevice = [&](MapTables M) { observationCountsOnDevice(ctx, M); };
    all("observationCountsOnDevice", {ids}, countsOnDevice);

    const std::vector<std::pair<const char *, Mutate>> fuseTables{pointTables[1], pointTables[2], tracks, counts};
    const FuseKeyframe current = fuseKeyframe(S, T, kCur);
    FuseKeyframe outsideKf = current, noFeatures = current;
    outsideKf.slot = kKf; noFeatures.features = nullptr;
    const std::vector<FuseKeyframe> adjacentKfs{fuseKeyframe(S, T, 0), fuseKeyframe(S, T, 1)};
    const Call dedup = [&](MapTables M) { deduplicateMapPoints(ctx, M, current, adjacentKfs, 5.0f, st); };
    all("deduplicateMapPoints", fuseTables, dedup);
    reject(T, S, "deduplicateMapPoints", "current slot = slot count", kNothing, [&](MapTables M) { deduplicateMapPoints(ctx, M, outsideKf, adjacentKfs, 5.0f, st); });
    const Call searchDedup = [&](MapTables M) { searchAndDeduplicate(ctx, M, {0, 1}, {current}, st); };
    all("searchAndDeduplicate", fuseTables, searchDedup);
    const Call matchLocal = [&](MapTables M) { matchLocalMapPoints(ctx, M, current, {0, 1}, 10.0f, st); };
    all("matchLocalMapPoints", fuseTables, matchLocal);
    reject(T, S, "matchLocalMapPoints", "current slot = slot count", kNothing, [&](MapTables M) { matchLocalMapPoints(ctx, M, outsideKf, {0, 1}, 10.0f, st); });
    reject(T, S, "matchLocalMapPoints", "no features", kNothing, [&](MapTables M) { matchLocalMapPoints(ctx, M, noFeatures, {0, 1}, 10.0f, st); });
    const Call merge = [&](MapTables M) { mergeMatchedMapPoints(ctx, M, {{0, 1}}); };
    all("mergeMatchedMapPoints", fuseTables, merge);

    auto closure = [&](std::int32_t cur, std::vector<std::int32_t> candidates) {
        return Call([&ctx, &st, cur, candidates](MapTables M) { tryLoopClosureOnTables(ctx, M, cur, candidates, {1}, -1.0, st); });
    };
    all("tryLoopClosureOnTables", {frames, cameras, {"time short", SHORT(t)}, ids, {"camera centre short", SHORT(cameraCenter)}, {"previous short", SHORT(previous)}}, closure(kCur, {}));
    reject(T, S, "tryLoopClosureOnTables", "current = slot count", kNothing, closure(kKf, {}));
    reject(T, S, "tryLoopClosureOnTables", "candidate = slot count", kNothing, closure(kCur, {kKf}));
    reject(T, S, "tryLoopClosureOnTables", "candidate = current", kNothing, closure(kCur, {kCur}));

    if (g_failed) { std::printf("%d of %d rejections failed\n", g_failed, g_cases); return 2; }
    if (ctx.download(T.keyframes.table(), (std::size_t)kKf * kStride) != kfBefore || ctx.download(T.flags.flags(), (std::size_t)kMp) != flagsBefore || T.live.download() != liveBefore) {
        std::printf("a rejected call wrote to the tables\n");
        return 3;
    }
    std::printf("rejections ok %d cases\n", g_cases);

    // ---- one passing call per function on the consistent tables, in the order of a new keyframe's chain; cullMap last
    KeyframeSlots slots = S.slots;
    const MapTables M = T.view(slots);
    int passed = 0;
    const std::vector<Call> calls{countsOnDevice, adjacentOf(kCur), [&](MapTables V) { updateMapPoints(ctx, V, kCur, 3, st); },
                                  [&](MapTables V) { retriangulateCurrent(ctx, V, kCur, st, TriangulationMethod::TME); }, tracked, [&](MapTables V) { unboundMasks(ctx, V, {0, 1, 2}); },
                                  create(kCur, {kCur}, TriangulationMethod::TME, &S.pose), localBa({0, 1}), poseBa(kCur), dedup, searchDedup, matchLocal,
                                  [&](MapTables V) {
                                      GateView view;
                                      view.camera = kCam; view.threshold = 10.0f; view.t[0] = S.pose[kCur][3]; view.indices = {0, 1};
                                      searchByProjectionOnTables(ctx, V, *T.frames[kCur], view, kCur, st);
                                  },
                                  merge, closure(kCur, {}), cull({0})};
    for (const Call &call : calls) {
        try {
            call(M);
            ++passed;
        } catch (const std::exception &e) {
            std::printf("passing call %d threw \"%s\"\n", passed, e.what());
            return 4;
        }
    }
    std::printf("passing calls ok %d functions\n", passed);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) { std::printf("link ok %d\n", (int)(sizeof(MapTables) > 0 && sizeof(KeyframeSlots) > 0)); return 0; }
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu();
    std::printf("usage: map_tables_smoke --no-gpu | --gpu\n");
    return 64;
}
