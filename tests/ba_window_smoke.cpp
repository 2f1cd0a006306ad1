// Compile + link check of the local-BA part of the host mirror (mi355slam/map_update.hpp: localBundleAdjustOnTables) against libmi355slam.so,
// and its run on one small map.
//   ba_window_smoke --no-gpu   the symbols link; a few calls of the two *_check twins; the mirror's local-keyframe set against a
//                              std::set<KfId, std::greater<>> restatement of bundle_adjuster.cpp:177-193 (no context, no device)
//   ba_window_smoke            localBundleAdjustOnTables on a seeded map against a restatement that keeps Keyframe::mapPoints and
//                              `std::map<KfId, KpId> observations` on the host: the local keyframes, localMapPoints, nCurrentFrameMapPoints,
//                              the three early-outs of :235-240 (nothing written), the NEIGHBOR stage (:326-331: the current pose and the
//                              positions only) and the LOCAL stage, whose erased observations, keyframe table, observation counts and
//                              flags must equal the loop of :376-388 run on the host maps with the outliers the solve reported.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <vector>
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

struct Rng {                             // a fixed sequence: the same map on every run
    std::uint64_t s = 0x9E3779B97F4A7C15ull;
    std::uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (std::uint32_t)(s >> 33); }
    double unit() { return next() / 2147483648.0; }
    int below(int n) { return (int)(next() % (std::uint32_t)n); }
};

// localKeyframes of bundle_adjuster.cpp:177-193 with the reference's containers
std::vector<std::int32_t> local_restated(const std::vector<std::int32_t> &kfId, std::int32_t current, const std::vector<std::int32_t> &adjacent) {
    std::map<int, std::int32_t> keyframes;                   // mapDB.keyframes: KfId -> slot
    for (std::size_t s = 0; s < kfId.size(); ++s) if (kfId[s] >= 0) keyframes[kfId[s]] = (std::int32_t)s;
    std::set<int, std::greater<int>> localKeyframes;
    localKeyframes.insert(kfId[current]);
    for (std::int32_t s : adjacent) localKeyframes.insert(kfId[s]);
    int i = 0;
    for (auto it = keyframes.rbegin(); it != keyframes.rend(); ++it, ++i) {
        localKeyframes.insert(it->first);
        if (i > 5) break;
    }
    std::vector<std::int32_t> out;
    for (int id : localKeyframes) out.push_back(keyframes[id]);
    return out;
}

int no_gpu() {
    char why[256] = {0};
    const auto *dev = reinterpret_cast<std::int32_t *>(0x1000);       // never dereferenced by the validation
    const auto *devd = reinterpret_cast<double *>(0x1000);
    const auto *devf = reinterpret_cast<float *>(0x1000);
    const auto *devb = reinterpret_cast<std::uint8_t *>(0x1000);
    ms_obs_lists l{};
    l.rows = l.obs_start = l.obs_kf = l.obs_kp = l.obs_octave = const_cast<std::int32_t *>(dev);
    l.obs_x = l.obs_y = const_cast<float *>(devf);
    const ms_ba_window_dev window{const_cast<std::int32_t *>(dev), const_cast<std::int32_t *>(dev), const_cast<std::int32_t *>(dev)};
    std::int32_t local[3] = {4, 0, 2}, focal[5] = {500, 500, 500, 500, 500}, nEdge = 0, nCurrent = 0;
    ms_pinhole cams[5];
    for (ms_pinhole &c : cams) c = ms_pinhole{500.0, 501.0, 320.0, 240.0, 640, 480};
    float sigma[3] = {1.f, 1.44f, 2.0736f};
    double pose[21], point[18], uv[28], info[14];
    std::int32_t op[14], ok[14];
    auto gather = [&](int current, int levels) {
        return ms_ba_window_lists_check(devd, 5, devd, 20, &l, 6, 14, local, 3, current, cams, focal, sigma, levels, pose, point, op, ok, uv, info, 6, 14, &window, &nEdge, &nCurrent,
                                        why, sizeof(why));
    };
    if (gather(0, 3) != MS_OK) { std::printf("a valid lists call was rejected: %s\n", why); return 1; }
    int cases = 0;
    cases += gather(3, 3) == MS_ERR_INVALID && why[0];                                    // current index outside the local keyframes
    cases += gather(0, 0) == MS_ERR_INVALID && why[0];                                    // no levels
    local[1] = 4;          cases += gather(0, 3) == MS_ERR_INVALID && why[0]; local[1] = 0;          // a local slot twice
    local[2] = 5;          cases += gather(0, 3) == MS_ERR_INVALID && why[0]; local[2] = 2;          // a local slot outside the table
    cams[2].fx = 0.0;      cases += gather(0, 3) == MS_ERR_INVALID && why[0]; cams[2].fx = 500.0;    // a local camera without a focal length
    sigma[1] = -1.f;       cases += gather(0, 3) == MS_ERR_INVALID && why[0]; sigma[1] = 1.44f;
    std::int32_t erased[14], nErased = 0, nStale = 0;
    auto apply = [&](int mode, int nPose, const double *chi2) {
        return ms_ba_window_apply_check(dev, 5, 8, devd, devb, dev, 20, devd, pose, nPose, point, chi2, &window, 14, dev, 6, local, 3, 0, mode, erased, 14, &nErased, &nStale, why,
                                        sizeof(why));
    };
    if (apply(MS_BA_APPLY_LOCAL, 4, info) != MS_OK || apply(MS_BA_APPLY_NEIGHBOR, 3, nullptr) != MS_OK) { std::printf("a valid apply call was rejected: %s\n", why); return 1; }
    cases += apply(2, 4, info) == MS_ERR_INVALID && why[0];                               // a bad mode
    cases += apply(MS_BA_APPLY_LOCAL, 2, info) == MS_ERR_INVALID && why[0];               // fewer poses than local keyframes
    cases += apply(MS_BA_APPLY_LOCAL, 4, nullptr) == MS_ERR_INVALID && why[0];            // LOCAL without chi2
    if (cases != 9) { std::printf("%d of 9 bad calls were rejected\n", cases); return 1; }
    // the local-keyframe set: fewer than seven keyframes, exactly seven, more; adjacent ones old and new; an empty slot in between
    int sets = 0;
    Rng rng;
    for (int n : {1, 3, 7, 8, 12, 30}) {
        for (int round = 0; round < 4; ++round) {
            std::vector<std::int32_t> kfId((std::size_t)n + 2, -1), ids;
            for (int i = 0; i < n; ++i) ids.push_back(3 * i + 1);
            for (int i = n - 1; i > 0; --i) std::swap(ids[(std::size_t)i], ids[(std::size_t)rng.below(i + 1)]);
            for (int i = 0; i < n; ++i) kfId[(std::size_t)(i + (i >= n / 2 ? 2 : 0))] = ids[(std::size_t)i];        // two empty slots in the middle
            std::vector<std::int32_t> occupied;
            for (std::size_t s = 0; s < kfId.size(); ++s) if (kfId[s] >= 0) occupied.push_back((std::int32_t)s);
            const std::int32_t current = occupied[(std::size_t)rng.below(n)];
            std::vector<std::int32_t> adjacent;
            for (int i = 0; i < round; ++i) adjacent.push_back(occupied[(std::size_t)rng.below(n)]);
            if (detail::local_keyframes(kfId, current, adjacent) != local_restated(kfId, current, adjacent)) { std::printf("local keyframes differ for %d keyframes\n", n); return 1; }
            ++sets;
        }
    }
    bool threw = false;
    try { detail::local_keyframes({4, -1, 7}, 1, {}); } catch (const std::invalid_argument &) { threw = true; }
    if (!threw) { std::printf("an empty current slot was accepted\n"); return 1; }
    std::printf("no-gpu ok %d cases, %d local-keyframe sets\n", cases, sets);
    return 0;
}

struct Map {
    static constexpr int nKf = 12, stride = 96, nMp = 260, current = 9, emptySlot = 4;
    std::vector<std::int32_t> kfId;
    std::vector<std::vector<std::int32_t>> mapPoints;        // Keyframe::mapPoints per slot
    std::vector<std::vector<float>> x, y;
    std::vector<std::vector<std::int32_t>> octave;
    std::vector<DeviceKeyframePoses::Pose> pose;
    KeyframeSlots cams;                      // camera and focalLength; the view's id is kfId above
    std::vector<DeviceMapPoints::Vec3d> position;
    std::vector<std::uint8_t> flags;
    std::vector<std::int32_t> adjacent;
    int outliers = 0;
};

Map make_map() {
    Map m;
    Rng rng;
    const int ids[Map::nKf] = {2, 5, 8, 11, -1, 14, 17, 20, 23, 32, 26, 29};            // slot 9 is the newest keyframe; slot 4 is empty
    const ms_pinhole cam{500.0, 502.0, 320.0, 240.0, 640, 480};
    m.mapPoints.assign(Map::nKf, {}); m.x.assign(Map::nKf, {}); m.y.assign(Map::nKf, {}); m.octave.assign(Map::nKf, {});
    auto centre = [](int k) { return 0.2 * (k < 9 ? k : (k == 9 ? 11 : k - 1)); };       // along x in KfId order
    for (int k = 0; k < Map::nKf; ++k) {
        m.kfId.push_back(ids[k]);
        m.pose.push_back({1, 0, 0, -centre(k) + 0.004 * rng.unit(), 0, 1, 0, 0.003 * rng.unit(), 0, 0, 1, 0.003 * rng.unit()});
        m.cams.camera.push_back(cam);
        m.cams.focalLength.push_back(500);
    }
    m.adjacent = {10, 11, 3};
    m.position.assign(Map::nMp, DeviceMapPoints::Vec3d{0, 0, 0});
    m.flags.assign(Map::nMp, 0);
    for (int r = 0; r < 200; ++r) {
        const DeviceMapPoints::Vec3d X{-1.0 + 4.0 * rng.unit(), -1.0 + 2.0 * rng.unit(), 4.0 + 5.0 * rng.unit()};
        m.position[(std::size_t)r] = {X[0] + 0.01 * (rng.unit() - 0.5), X[1] + 0.01 * (rng.unit() - 0.5), X[2] + 0.01 * (rng.unit() - 0.5)};
        m.flags[(std::size_t)r] = r % 7 == 3 ? 2 : (r % 11 == 5 ? 0 : 3);
        const int first = rng.below(Map::nKf), count = 2 + rng.below(6);
        for (int k = first; k < std::min(first + count, (int)Map::nKf); ++k) {
            if (k == Map::emptySlot || (int)m.mapPoints[(std::size_t)k].size() >= Map::stride - 4) continue;
            double u = 500.0 * (X[0] - centre(k)) / X[2] + 320.0 + 0.3 * (rng.unit() - 0.5), v = 502.0 * X[1] / X[2] + 240.0 + 0.3 * (rng.unit() - 0.5);
            if (m.flags[(std::size_t)r] == 3 && r % 13 == 0 && k >= 8) { u += 30.0; ++m.outliers; }      // gross outliers among the newest keyframes
            m.mapPoints[(std::size_t)k].push_back(r); m.x[(std::size_t)k].push_back((float)u); m.y[(std::size_t)k].push_back((float)v);
            m.octave[(std::size_t)k].push_back(rng.below(8));
        }
    }
    for (int k = 0; k < Map::nKf; ++k)                       // unbound keypoints in between
        for (int j = 0; j < 3; ++j) {
            const std::size_t at = (std::size_t)rng.below((int)m.mapPoints[(std::size_t)k].size() + 1);
            m.mapPoints[(std::size_t)k].insert(m.mapPoints[(std::size_t)k].begin() + (std::ptrdiff_t)at, -1);
            m.x[(std::size_t)k].insert(m.x[(std::size_t)k].begin() + (std::ptrdiff_t)at, 1.f); m.y[(std::size_t)k].insert(m.y[(std::size_t)k].begin() + (std::ptrdiff_t)at, 1.f);
            m.octave[(std::size_t)k].insert(m.octave[(std::size_t)k].begin() + (std::ptrdiff_t)at, 0);
        }
    return m;
}

// the tables of a map on the device
struct Tables {
    DeviceKeyframeMapPoints kf;
    DeviceMapPoints points;
    DeviceMapPointFlags flags;
    DeviceKeypointTable kp;
    DeviceKeyframePoses poses;
    DeviceArray<std::int32_t> nObs;
    KeyframeSlots slots;
    Tables(Context &ctx, const Map &m)
        : kf(ctx, Map::nKf, Map::stride, Map::nMp),
          points(ctx, m.position, std::vector<DeviceMapPoints::Vec3f>(Map::nMp, DeviceMapPoints::Vec3f{0, 0, 1}), std::vector<float>(Map::nMp, 0.f), std::vector<float>(Map::nMp, 0.f),
                 std::vector<KeyPoint::Descriptor>(Map::nMp, KeyPoint::Descriptor{})),
          flags(ctx, m.flags), kp(ctx, Map::nKf, Map::stride), poses(ctx, m.pose), nObs(ctx, Map::nMp), slots(m.cams) {
        slots.id = m.kfId;
        for (int k = 0; k < Map::nKf; ++k) {
            kf.update((std::size_t)k, m.mapPoints[(std::size_t)k]);
            kp.update((std::size_t)k, m.x[(std::size_t)k], m.y[(std::size_t)k], m.octave[(std::size_t)k], {});
        }
        observationCountsOnDevice(ctx, view(nullptr));
    }
    MapTables view(DeviceObservationLists *lists) {
        MapTables M{kf, slots};
        M.flags = &flags; M.points = &points; M.keypoints = &kp; M.poses = &poses; M.observationCount = nObs.data(); M.lists = lists;
        return M;
    }
};

struct Snapshot {
    std::vector<std::int32_t> kf, nObs;
    std::vector<std::uint8_t> flags;
    std::vector<double> position;
    std::vector<DeviceKeyframePoses::Pose> poses;
    bool operator==(const Snapshot &o) const {
        return kf == o.kf && nObs == o.nObs && flags == o.flags && poses == o.poses && position.size() == o.position.size() &&
               std::memcmp(position.data(), o.position.data(), 8 * position.size()) == 0;
    }
};

Snapshot snapshot(Context &ctx, Tables &t) {
    return Snapshot{ctx.download(t.kf.table(), (std::size_t)Map::nKf * Map::stride), t.nObs.download(), ctx.download(t.flags.flags(), (std::size_t)Map::nMp),
                    ctx.download(t.points.position(), 3 * (std::size_t)Map::nMp), t.poses.download()};
}

int fail(const char *what) { std::printf("FAILED: %s\n", what); return 1; }

int with_gpu() {
    Context ctx(0);
    const Map m = make_map();
    Parameters params;
    const StaticSettings settings(params);
    const PoseEdgeBuilder edges = [&](const std::vector<std::int32_t> &local, BaWindow &w) {      // the odometry chain of :296-311 between neighbours in pose order
        for (std::size_t k = 1; k < local.size(); ++k) {
            w.edgeI.push_back((std::int32_t)k - 1); w.edgeJ.push_back((std::int32_t)k);
            const auto &a = w.poses[k - 1], &b = w.poses[k];                                  // rotations are the identity here: the difference of the translations
            w.edgeMeas.push_back({0, 0, 0, 1, b[4] - a[4], b[5] - a[5], b[6] - a[6]});
            std::array<double, 36> info{};
            for (int i = 0; i < 6; ++i) info[(std::size_t)(7 * i)] = (i < 3 ? 100.0 * 100.0 : 50.0 * 50.0) * 2.6667;
            w.edgeInfo.push_back(info);
        }
    };
    // ---- the restatement: the reference's containers on the host
    const std::vector<std::int32_t> localWant = local_restated(m.kfId, Map::current, m.adjacent);
    std::map<int, std::map<int, std::vector<int>>> observations;       // MpId -> KfId -> keypoints
    for (int k = 0; k < Map::nKf; ++k)
        if (m.kfId[(std::size_t)k] >= 0)
            for (std::size_t j = 0; j < m.mapPoints[(std::size_t)k].size(); ++j)
                if (m.mapPoints[(std::size_t)k][j] >= 0) observations[m.mapPoints[(std::size_t)k][j]][m.kfId[(std::size_t)k]].push_back((int)j);
    std::set<int> localMapPoints;
    std::size_t nCurrentWant = 0;
    for (std::int32_t s : localWant)
        for (std::int32_t r : m.mapPoints[(std::size_t)s]) {
            if (r == -1 || m.flags[(std::size_t)r] != 3) continue;
            if (s == Map::current) ++nCurrentWant;
            localMapPoints.insert(r);
        }
    std::map<int, std::int32_t> slotOf;
    for (int k = 0; k < Map::nKf; ++k) if (m.kfId[(std::size_t)k] >= 0) slotOf[m.kfId[(std::size_t)k]] = k;
    struct Edge { std::int32_t slot, keyPoint, row; };
    std::vector<Edge> edgesWant;                             // mapPointEdges in the order of :259-290
    for (int r : localMapPoints)
        for (const auto &o : observations[r]) {
            if (std::find(localWant.begin(), localWant.end(), slotOf[o.first]) == localWant.end()) continue;
            for (int j : o.second) edgesWant.push_back({slotOf[o.first], j, r});
        }
    // ---- the early-outs: nothing solved, nothing written, localMapPoints still returned
    for (int which = 0; which < 2; ++which) {
        Tables t(ctx, m);
        DeviceObservationLists lists(ctx);
        const Snapshot before = snapshot(ctx, t);
        Parameters p = params;
        if (which == 0) p.minVisibleMapPointsInCurrentFrameBA = (unsigned)nCurrentWant + 1; else p.minKeyframesInBA = (unsigned)localWant.size() + 1;
        const LocalBaOnTables out = localBundleAdjustOnTables(ctx, t.view(&lists), Map::current, m.adjacent, edges, 20,
                                                              p, settings);
        if (out.stage != BaStats::Ba::NONE || out.outcome.ran) return fail("an early-out ran the solver");
        if (out.localSlots != localWant || out.localRows != std::vector<std::int32_t>(localMapPoints.begin(), localMapPoints.end())) return fail("early-out: local sets");
        if (!(snapshot(ctx, t) == before)) return fail("an early-out wrote to the tables");
        p = params;
        if (which == 0) p.minVisibleMapPointsInCurrentFrameBA = (unsigned)nCurrentWant; else p.minKeyframesInBA = (unsigned)localWant.size();       // at the threshold it runs
        if (localBundleAdjustOnTables(ctx, t.view(&lists), Map::current, m.adjacent, edges, 20, p, settings).stage !=
            BaStats::Ba::LOCAL)
            return fail("a window at the threshold did not run");
    }
    // ---- NEIGHBOR: the neighbourhood stage is skipped
    {
        Tables t(ctx, m);
        DeviceObservationLists lists(ctx);
        const Snapshot before = snapshot(ctx, t);
        Parameters p = params;
        p.minVisibleMapPointsInNeighborhoodBA = (unsigned)nCurrentWant + 1;
        WorkspaceBA workspace(true);
        const LocalBaOnTables out = localBundleAdjustOnTables(ctx, t.view(&lists), Map::current, m.adjacent, edges, 20,
                                                              p, settings, &workspace);
        const Snapshot after = snapshot(ctx, t);
        if (out.stage != BaStats::Ba::NEIGHBOR || !out.outcome.ran || workspace.baStats.frameCount(BaStats::Ba::NEIGHBOR) != 1 || !out.erased.empty()) return fail("NEIGHBOR stage");
        if (after.kf != before.kf || after.nObs != before.nObs || after.flags != before.flags) return fail("NEIGHBOR wrote to kf_mp, n_obs or the flags");
        for (int k = 0; k < Map::nKf; ++k)
            if ((after.poses[(std::size_t)k] != before.poses[(std::size_t)k]) != (k == Map::current)) return fail("NEIGHBOR: the current pose, and only it, moves");
        for (int r = 0; r < Map::nMp; ++r) {
            const bool same = std::memcmp(&after.position[3 * (std::size_t)r], &before.position[3 * (std::size_t)r], 24) == 0;
            if (!localMapPoints.count(r) && !same) return fail("NEIGHBOR moved a point outside the window");
        }
    }
    // ---- LOCAL
    Tables t(ctx, m);
    DeviceObservationLists lists(ctx);
    const Snapshot before = snapshot(ctx, t);
    WorkspaceBA workspace(true);
    const LocalBaOnTables out = localBundleAdjustOnTables(ctx, t.view(&lists), Map::current, m.adjacent, edges, 20, params,
                                                          settings, &workspace);
    const Snapshot after = snapshot(ctx, t);
    if (out.stage != BaStats::Ba::LOCAL || workspace.baStats.frameCount(BaStats::Ba::LOCAL) != 1) return fail("LOCAL stage");
    if (out.localSlots != localWant) return fail("local keyframes");
    if (out.localRows != std::vector<std::int32_t>(localMapPoints.begin(), localMapPoints.end())) return fail("localMapPoints");
    if (out.currentFrameMapPoints != nCurrentWant || out.edgeCount != edgesWant.size() || out.outcome.outlier.size() != edgesWant.size()) return fail("nCurrentFrameMapPoints or the edge count");
    // :376-388 on the host maps with the outliers the solve reported
    std::vector<std::vector<std::int32_t>> mapPoints = m.mapPoints;
    std::vector<std::uint8_t> flags = m.flags;
    std::vector<LocalBaOnTables::Erased> erasedWant;
    for (std::size_t e = 0; e < edgesWant.size(); ++e) {
        if (!out.outcome.outlier[e]) continue;
        const Edge &g = edgesWant[e];
        auto &obs = observations[g.row][m.kfId[(std::size_t)g.slot]];
        obs.erase(std::find(obs.begin(), obs.end(), g.keyPoint));
        if (obs.empty()) observations[g.row].erase(m.kfId[(std::size_t)g.slot]);
        mapPoints[(std::size_t)g.slot][(std::size_t)g.keyPoint] = -1;
        std::size_t left = 0;
        for (const auto &o : observations[g.row]) left += o.second.size();
        if (left <= 2) flags[(std::size_t)g.row] = 2;
        erasedWant.push_back({(std::int32_t)e, g.slot, g.keyPoint, g.row});
    }
    if (erasedWant.empty()) return fail("the scene's gross outliers were not found: nothing to hold the erase step against");
    if (out.erased.size() != erasedWant.size()) return fail("erased count");
    for (std::size_t i = 0; i < erasedWant.size(); ++i) {
        const auto &a = out.erased[i], &b = erasedWant[i];
        if (a.edge != b.edge || a.slot != b.slot || a.keyPoint != b.keyPoint || a.row != b.row) return fail("erased entries");
    }
    for (int k = 0; k < Map::nKf; ++k)
        for (int j = 0; j < Map::stride; ++j) {
            const std::int32_t want = (std::size_t)j < mapPoints[(std::size_t)k].size() ? mapPoints[(std::size_t)k][(std::size_t)j] : -1;
            if (after.kf[(std::size_t)k * Map::stride + (std::size_t)j] != want) return fail("kf_mp after the erase");
        }
    for (int r = 0; r < Map::nMp; ++r) {
        std::size_t n = 0;
        for (const auto &o : observations[r]) n += o.second.size();
        if ((std::size_t)after.nObs[(std::size_t)r] != n) return fail("n_obs after the erase");
        if (after.flags[(std::size_t)r] != flags[(std::size_t)r]) return fail("flags after the erase");
        const bool same = std::memcmp(&after.position[3 * (std::size_t)r], &before.position[3 * (std::size_t)r], 24) == 0;
        if (!localMapPoints.count(r) && !same) return fail("LOCAL moved a point outside the window");
    }
    for (int k = 0; k < Map::nKf; ++k) {
        const bool isLocal = std::find(localWant.begin(), localWant.end(), k) != localWant.end();
        if (!isLocal && after.poses[(std::size_t)k] != before.poses[(std::size_t)k]) return fail("LOCAL moved a keyframe outside the window");
        for (double v : after.poses[(std::size_t)k]) if (!std::isfinite(v)) return fail("a pose is not finite");
    }
    std::printf("localBundleAdjustOnTables ok: %zu local keyframes, %zu map points, %zu edges, %zu in the current frame, %zu erased of %d planted; early-outs and NEIGHBOR hold\n",
                localWant.size(), localMapPoints.size(), edgesWant.size(), nCurrentWant, erasedWant.size(), m.outliers);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_ba_window_lists, (const void *)&ms_ba_window_lists_check, (const void *)&ms_ba_window_apply,
                                   (const void *)&ms_ba_window_apply_check};
    std::printf("link ok %d\n", syms[0] && syms[1] && syms[2] && syms[3]);
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    try {
        return with_gpu();
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
}
