// Compile + link check of the matchTrackedFeatures part of the host mirror (mi355slam/map_tables.hpp and map_update.hpp: DeviceTrackTable,
// matchTrackedFeatures) against libmi355slam.so, and its run on one small map.
//   match_tracked_smoke --no-gpu   the symbols link; a few calls of ms_match_tracked_check / ms_match_tracked_finish_check (no context, no device)
//   match_tracked_smoke            mapper_helpers.cpp:67-142 twice on copies of one seeded map: through mi355slam::matchTrackedFeatures (nothing
//                                  per keypoint on the host), and through a sequential restatement that walks keyPointToTrackId and
//                                  trackIdToMapPoint in std::maps, evaluates isInFrustum and checkReprojectionError per keypoint on the host,
//                                  uploads the keyframe's row (DeviceKeyframeMapPoints::update) and hands host lists built from
//                                  `std::map<KfId, KpId> observations` to triangulateMapPoints (FIRST_LAST), updateDescriptors and
//                                  DeviceMapPoints::refresh.  Outcomes, counters and every table must agree bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>
#include "mi355slam/keyframe_matcher.hpp"       // updateDescriptors, the restatement's medoid
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

int no_gpu() {
    char why[256] = {0};
    const auto *dev = reinterpret_cast<std::int32_t *>(0x1000);       // never dereferenced by the validation
    const auto *devf = reinterpret_cast<float *>(0x1000);
    const auto *devd = reinterpret_cast<double *>(0x1000);
    const auto *devb = reinterpret_cast<std::uint8_t *>(0x1000);
    const auto *devu = reinterpret_cast<std::uint32_t *>(0x1000);
    const float sigma[4] = {1.f, 1.44f, 2.07f, 2.99f};
    ms_tracked_frame f{};
    f.slot = 1; f.pose[0] = f.pose[5] = f.pose[10] = 1.0;
    f.cam = ms_pinhole{500.0, 500.0, 320.0, 240.0, 640, 480}; f.focal = 500; f.desc_base = 0; f.track_base = 10;
    f.level_sigma_sq = sigma; f.n_levels = 4; f.rel_reprojection_threshold = 0.004f; f.view_cos_limit = 0.5f;
    std::int32_t kpTrack[4] = {10, -1, 12, 15}, newRows[2] = {3, 8}, counts[5];
    auto check = [&](int nKp, int nTrack) {
        return ms_match_tracked_check(dev, 2, 4, devb, devb, devd, devf, devf, devf, devu, dev, 9, devf, devf, dev, devu, 64, dev, nTrack, &f, kpTrack, nKp, newRows, 2,
                                      devb, counts, why, sizeof(why));
    };
    if (check(4, 6) != MS_OK) { std::printf("a valid call was rejected: %s\n", why); return 1; }
    int cases = 0;
    cases += check(5, 6) == MS_ERR_INVALID && why[0];                                    // n_kp > stride
    cases += check(4, 5) == MS_ERR_INVALID && why[0];                                    // track id 15 outside the window
    kpTrack[1] = 12;    cases += check(4, 6) == MS_ERR_INVALID && why[0]; kpTrack[1] = -1;          // a track id twice
    newRows[1] = 3;     cases += check(4, 6) == MS_ERR_INVALID && why[0]; newRows[1] = 8;           // a new row twice
    newRows[0] = 9;     cases += check(4, 6) == MS_ERR_INVALID && why[0]; newRows[0] = 3;           // a new row outside the table
    f.slot = 2;         cases += check(4, 6) == MS_ERR_INVALID && why[0]; f.slot = 1;
    f.view_cos_limit = NAN; cases += check(4, 6) == MS_ERR_INVALID && why[0]; f.view_cos_limit = 0.5f;
    cases += check(4, MS_TRACKED_MAX_WINDOW + 1) == MS_ERR_CAPACITY && why[0];
    ms_obs_lists l{};
    l.rows = const_cast<std::int32_t *>(dev); l.obs_start = const_cast<std::int32_t *>(dev);
    std::int32_t nRefresh = 0;
    if (ms_match_tracked_finish_check(&l, 3, devb, nullptr, nullptr, 9, dev, 2, 1, dev, 5, &nRefresh, why, sizeof(why)) != MS_OK) { std::printf("a valid finish was rejected: %s\n", why); return 1; }
    cases += ms_match_tracked_finish_check(&l, 3, devb, nullptr, nullptr, 9, dev, 2, 1, dev, 4, &nRefresh, why, sizeof(why)) == MS_ERR_CAPACITY && why[0];
    cases += ms_match_tracked_finish_check(&l, 3, nullptr, nullptr, nullptr, 9, dev, 2, 1, dev, 5, &nRefresh, why, sizeof(why)) == MS_ERR_INVALID && why[0];
    if (cases != 10) { std::printf("%d of 10 bad calls were rejected\n", cases); return 1; }
    std::printf("no-gpu ok %d cases\n", cases);
    return 0;
}

struct Rng {                             // a fixed sequence: the same map on every run
    std::uint64_t s = 0x9E3779B97F4A7C15ull;
    std::uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (std::uint32_t)(s >> 33); }
    double unit() { return next() / 2147483648.0; }
    int below(int n) { return (int)(next() % (std::uint32_t)n); }
};

struct Map {
    static constexpr int nKf = 10, stride = 320, nMp = 700, current = 9, noDescSlot = 3, nKp = 300, trackBase = 500, firstFree = 600;
    std::vector<std::vector<std::int32_t>> mapPoints;        // Keyframe::mapPoints per slot
    std::vector<std::int32_t> kfId, descBase;
    std::vector<std::vector<float>> x, y, depth;
    std::vector<std::vector<std::int32_t>> octave;
    std::vector<DeviceKeyframePoses::Pose> pose;
    KeyframeSlots cams;                      // camera and focalLength; the view's id and descBase are kfId and descBase above
    std::vector<DeviceMapPoints::Vec3d> position;
    std::vector<DeviceMapPoints::Vec3f> norm;
    std::vector<float> minDist, maxDist;
    std::vector<std::uint8_t> flags, live;
    std::vector<std::int32_t> mpTrack;                       // MapPoint::trackId per row
    std::map<std::int32_t, std::int32_t> staleTracks;        // track -> row entries the device window holds for rows that are culled or recycled
    std::vector<std::int32_t> keyPointToTrackId, freeRows;
    std::vector<KeyPoint::Descriptor> pool;
};

Map make_map(bool frameHasDescriptors) {
    Map m;
    Rng rng;
    const int K = Map::nKf;
    m.mapPoints.assign(K, {}); m.x.assign(K, {}); m.y.assign(K, {}); m.depth.assign(K, {}); m.octave.assign(K, {});
    for (int k = 0; k < K; ++k) {                            // cameras 0.15 apart along x, looking down +z
        m.pose.push_back({1, 0, 0, -0.15 * k, 0, 1, 0, 0.01 * (k % 3), 0, 0, 1, 0});
        m.cams.camera.push_back(ms_pinhole{500.0, 502.0, 320.0, 240.0, 640, 480});
        m.cams.focalLength.push_back(500);
        m.kfId.push_back(k == 2 ? 11 : (k == 5 ? 5 : 3 * k + 1));                     // id order is not slot order; the current frame holds the newest
        m.descBase.push_back(k == Map::noDescSlot || (k == Map::current && !frameHasDescriptors) ? -1 : k * Map::stride);
    }
    m.keyPointToTrackId.assign(Map::nKp, -1);
    m.x[Map::current].assign(Map::nKp, 0.f); m.y[Map::current].assign(Map::nKp, 0.f); m.depth[Map::current].assign(Map::nKp, -1.f);
    m.octave[Map::current].assign(Map::nKp, 0); m.mapPoints[Map::current].assign(Map::nKp, -1);
    for (int j = 0; j < Map::nKp; ++j) { m.x[Map::current][j] = (float)(640 * rng.unit()); m.y[Map::current][j] = (float)(480 * rng.unit()); m.octave[Map::current][j] = rng.below(8); }
    int nextTrack = Map::trackBase;
    for (int r = 0; r < Map::nMp; ++r) {
        const double cx = 0.15 * Map::current;
        const DeviceMapPoints::Vec3d X{cx + (rng.unit() - 0.5) * 3.0, (rng.unit() - 0.5) * 2.0, 4.0 + rng.unit() * 6.0};
        const double dx = cx - X[0], dy = -0.01 * (Map::current % 3) - X[1], dz = -X[2], d = std::sqrt(dx * dx + dy * dy + dz * dz);
        m.position.push_back(X);
        m.norm.push_back({(float)(dx / d), (float)(dy / d), (float)(dz / d)});
        m.minDist.push_back((float)(d / 3)); m.maxDist.push_back((float)(d * 1.5));
        m.flags.push_back(0); m.live.push_back(0); m.mpTrack.push_back(-1);
        if (r >= Map::firstFree) { m.freeRows.push_back(r); continue; }
        m.live[r] = 1;
        const int kind = r % 10;                             // 0-3 TRIANGULATED and fine | 4 behind | 5 pixel off | 6, 7 not triangulated | 8 culled | 9 recycled
        const int n = kind == 6 ? 1 : 2 + rng.below(4), k0 = rng.below(Map::current - n + 1);
        for (int k = k0; k < k0 + n; ++k) {                  // older keyframes that observe it
            if ((int)m.mapPoints[k].size() >= Map::stride) continue;
            const double xc = X[0] - 0.15 * k, yc = X[1] + 0.01 * (k % 3);
            m.mapPoints[k].push_back(r);
            m.x[k].push_back((float)(500.0 * xc / X[2] + 320.0 + 0.05 * rng.unit()));
            m.y[k].push_back((float)(502.0 * yc / X[2] + 240.0 + 0.05 * rng.unit()));
            m.depth[k].push_back(-1.0f);
            m.octave[k].push_back(rng.below(8));
        }
        m.flags[r] = kind == 6 ? 0 : (kind == 7 ? (rng.below(2) ? 2 : 0) : 3);
        m.mpTrack[r] = nextTrack++;
        if (r % 3) continue;                                 // every third point is tracked into the current frame, at keypoint 7 (r / 3) mod nKp (distinct)
        const int j = (7 * (r / 3)) % Map::nKp;
        m.keyPointToTrackId[j] = m.mpTrack[r];
        const double xc = X[0] - cx, yc = X[1] + 0.01 * (Map::current % 3);
        m.x[Map::current][j] = (float)(500.0 * xc / X[2] + 320.0 + 0.05 * rng.unit());
        m.y[Map::current][j] = (float)(502.0 * yc / X[2] + 240.0 + 0.05 * rng.unit()) + (kind == 5 || (kind == 7 && r % 40 == 7) ? 25.f : 0.f);
        if (kind == 4) m.position[r] = {2 * cx - X[0], X[1], -X[2]};
        if (kind == 8) { m.live[r] = 0; m.staleTracks[m.mpTrack[r]] = r; }
        if (kind == 9) { m.staleTracks[m.mpTrack[r]] = r; m.mpTrack[r] = nextTrack++; }
    }
    for (int j = 0; j < Map::nKp; j += 9)                    // tracks the map has never seen
        if (m.keyPointToTrackId[j] == -1) m.keyPointToTrackId[j] = nextTrack++;
    m.pool.resize((std::size_t)K * Map::stride);
    for (auto &d : m.pool) for (auto &w : d) w = rng.next() & 0x0F0F0F0Fu;
    return m;
}

struct Tables {
    DeviceMapPoints points;
    DeviceMapPointFlags flags;
    DeviceMapPointLive live;
    DeviceKeyframeMapPoints table;
    DeviceTrackTable tracks;
    Tables(Context &ctx, const Map &m)
        : points(ctx, m.position, m.norm, m.minDist, m.maxDist, std::vector<KeyPoint::Descriptor>(Map::nMp, KeyPoint::Descriptor{})), flags(ctx, m.flags), live(ctx, m.live),
          table(ctx, Map::nKf, Map::stride, Map::nMp), tracks(ctx, Map::nMp, Map::trackBase, 16) {       // a small window on purpose: it grows
        for (int k = 0; k < Map::nKf; ++k) table.update(k, m.mapPoints[k]);
        std::vector<std::int32_t> rows, ids;
        for (int r = 0; r < Map::nMp; ++r) if (m.mpTrack[r] >= 0) { rows.push_back(r); ids.push_back(m.mpTrack[r]); }
        for (const auto &kv : m.staleTracks) { rows.push_back(kv.second); ids.push_back(kv.first); }     // bound first, then taken back below: stale window entries
        tracks.bind(rows, ids);
        std::vector<std::int32_t> all(Map::nMp);
        for (int r = 0; r < Map::nMp; ++r) all[r] = m.mpTrack[r];
        ctx.check(ms_dev_upload(ctx.get(), tracks.mpTrack(), all.data(), 4 * all.size()), "ms_dev_upload");
    }
    std::vector<unsigned char> bytes(Context &ctx, std::size_t window) {      // every table, one after another
        const std::size_t n = Map::nMp, sizes[10] = {24 * n, 12 * n, 4 * n, 4 * n, 32 * n, n, n, 4 * (std::size_t)Map::nKf * Map::stride, 4 * n, 4 * window};
        const void *src[10] = {points.position(), points.norm(), points.minDistance(), points.maxDistance(), points.descriptor(), flags.flags(), live.live(), table.table(),
                               tracks.mpTrack(), tracks.trackRow()};
        std::vector<unsigned char> out;
        for (int i = 0; i < 10; ++i) {
            std::vector<unsigned char> part(sizes[i]);
            ctx.check(ms_dev_download(ctx.get(), part.data(), src[i], sizes[i]), "ms_dev_download");
            out.insert(out.end(), part.begin(), part.end());
        }
        return out;
    }
};

// Keyframe::isInFrustum (keyframe.cpp:247-262) with the pinhole stand-in, the reference's types
bool in_frustum(const DeviceKeyframePoses::Pose &P, const ms_pinhole &c, const DeviceMapPoints::Vec3d &X, const DeviceMapPoints::Vec3f &n, float minD, float maxD, float cosLimit,
                double &u, double &v) {
    const double pc[3] = {((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3], ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7], ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11]};
    u = c.fx * (pc[0] / pc[2]) + c.cx; v = c.fy * (pc[1] / pc[2]) + c.cy;
    if (!(pc[2] > 0.0 && u >= 0.0 && u < (double)c.width && v >= 0.0 && v < (double)c.height)) return false;
    float d[3];
    for (int j = 0; j < 3; ++j) d[j] = (float)(-((P[j] * P[3] + P[4 + j] * P[7]) + P[8 + j] * P[11]) - X[j]);
    const float dist = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (dist < minD || maxD < dist) return false;
    const float cosv = ((d[0] / dist) * n[0] + (d[1] / dist) * n[1]) + (d[2] / dist) * n[2];
    return !(cosv < cosLimit);
}

// checkReprojectionError (mapper_helpers.cpp:576-598) for a visible point at pixel (u, v)
bool reprojection_ok(double u, double v, float x, float y, int octave, int focal, const StaticSettings &s) {
    const float du = (float)u - x, dv = (float)v - y, sq = du * du + dv * dv;
    const double base = (double)((float)focal * s.parameters.relativeReprojectionErrorThreshold);
    const double sigma2 = (double)(s.levelSigmaSq[octave] / s.levelSigmaSq[s.levelSigmaSq.size() / 2]) * base * base;
    return (double)sq <= 5.991 * sigma2;
}

int run(bool frameHasDescriptors) {
    const Map m = make_map(frameHasDescriptors);
    Parameters p;
    StaticSettings settings(p);
    Context ctx(0);
    DeviceKeyframePoses poses(ctx, m.pose);
    DeviceDescriptorPool pool(ctx, m.pool);
    DeviceKeypointTable keypoints(ctx, Map::nKf, Map::stride);
    for (int k = 0; k < Map::nKf; ++k) keypoints.update(k, m.x[k], m.y[k], m.octave[k], m.depth[k]);
    TrackedFrame frame;
    frame.slot = Map::current; frame.poseCW = m.pose[Map::current]; frame.keyPointToTrackId = m.keyPointToTrackId;

    // ---- the device path
    Tables dev(ctx, m);
    DeviceObservationLists lists(ctx, 4, 8);
    KeyframeSlots slots = m.cams;
    slots.id = m.kfId; slots.descBase = m.descBase;
    MapTables tables{dev.table, slots};
    tables.flags = &dev.flags; tables.points = &dev.points; tables.live = &dev.live; tables.tracks = &dev.tracks; tables.keypoints = &keypoints; tables.poses = &poses; tables.pool = &pool; tables.lists = &lists;
    const MatchTrackedResult got = matchTrackedFeatures(ctx, tables, frame, m.freeRows, settings);

    // ---- the restatement: std::maps, one keypoint after the other
    Tables ref(ctx, m);
    for (std::int32_t t : m.keyPointToTrackId) if (t >= 0) ref.tracks.ensureTrack(t);
    std::map<std::int32_t, std::int32_t> keyPointToTrackId, trackIdToMapPoint, slotOfId;
    for (int j = 0; j < Map::nKp; ++j) if (m.keyPointToTrackId[j] >= 0) keyPointToTrackId[j] = m.keyPointToTrackId[j];
    for (int r = 0; r < Map::nMp; ++r) if (m.live[r] && m.mpTrack[r] >= 0) trackIdToMapPoint[m.mpTrack[r]] = r;       // culled and recycled rows were erased
    std::vector<std::map<std::int32_t, std::int32_t>> observations(Map::nMp);
    for (int k = 0; k < Map::nKf; ++k) {
        slotOfId[m.kfId[k]] = k;
        for (std::size_t j = 0; j < m.mapPoints[k].size(); ++j)
            if (m.mapPoints[k][j] != -1) observations[m.mapPoints[k][j]][m.kfId[k]] = (std::int32_t)j;
    }
    std::vector<std::uint8_t> outcome(Map::nKp, 0), status = m.flags, live = m.live;
    std::vector<std::int32_t> row = m.mapPoints[Map::current], tracked, checked, createdRows, createdKp, mpTrack = m.mpTrack;
    std::size_t frustumFail = 0, reproFail = 0;
    for (int v = 0; v < Map::nKp; ++v) {                     // :76-141 up to the binding
        if (!keyPointToTrackId.count(v)) continue;
        const std::int32_t t = keyPointToTrackId.at(v);
        if (trackIdToMapPoint.count(t)) {
            const std::int32_t r = trackIdToMapPoint.at(t);
            if (!(status[r] & DeviceMapPointFlags::TRIANGULATED)) { outcome[v] = 2; tracked.push_back(r); }
            else {
                double pu, pv;
                if (!in_frustum(m.pose[Map::current], m.cams.camera[Map::current], m.position[r], m.norm[r], m.minDist[r], m.maxDist[r], 0.5f, pu, pv)) { outcome[v] = 4; ++frustumFail; continue; }
                if (!reprojection_ok(pu, pv, m.x[Map::current][v], m.y[Map::current][v], m.octave[Map::current][v], m.cams.focalLength[Map::current], settings)) { outcome[v] = 5; ++reproFail; continue; }
                outcome[v] = 3; checked.push_back(r);
            }
            observations[r][m.kfId[Map::current]] = v;
            row[v] = r;
        } else if (frameHasDescriptors) {
            const std::int32_t r = m.freeRows.at(createdRows.size());
            outcome[v] = 1; createdRows.push_back(r); createdKp.push_back(v);
            observations[r][m.kfId[Map::current]] = v;
            row[v] = r; live[r] = 1; status[r] = 0; mpTrack[r] = t;
            trackIdToMapPoint[t] = r;
            ref.points.update(r, 1, nullptr, nullptr, nullptr, nullptr, &m.pool[(std::size_t)m.descBase[Map::current] + v]);
            ref.tracks.bind({r}, {t});
        } else {
            outcome[v] = 6;
        }
    }
    ref.table.update(Map::current, row);                     // kfTable.update
    ref.live.update(0, Map::nMp, live.data());
    ref.flags.update(0, Map::nMp, status.data());
    auto observationsOf = [&](std::int32_t r, std::vector<MapObservation> &obs, std::vector<KeyPoint::Descriptor> &desc) {
        for (const auto &kv : observations[r]) {
            const std::int32_t k = slotOfId.at(kv.first), d = m.descBase[k] < 0 ? -1 : m.descBase[k] + kv.second;
            obs.push_back(MapObservation{k, d});
            if (d >= 0) desc.push_back(m.pool[d]);
        }
    };
    TriangulateArgs args;                                    // :90 for every just-tracked point
    args.obsStart.push_back(0);
    for (std::int32_t r : tracked) {
        args.rows.push_back(r);
        args.wasTriangulated.push_back((status[r] & DeviceMapPointFlags::USABLE) != 0);
        for (const auto &kv : observations[r]) {
            const std::int32_t k = slotOfId.at(kv.first);
            args.obsKf.push_back(k); args.obsX.push_back(m.x[k][kv.second]); args.obsY.push_back(m.y[k][kv.second]);
            args.obsOctave.push_back(m.octave[k][kv.second]); args.obsDepth.push_back(m.depth[k][kv.second]);
        }
        args.obsStart.push_back((std::int32_t)args.obsKf.size());
    }
    const TriangulateResult tri = triangulateMapPoints(ctx, ref.points, &ref.flags, poses, m.cams, args, settings, TriangulationMethod::FIRST_LAST);
    std::size_t unsure = 0, promoted = 0;
    auto refresh = [&](const std::vector<std::int32_t> &rows, bool descriptors) {
        std::vector<std::vector<MapObservation>> obs;
        std::vector<std::int32_t> firstOctave;
        for (std::int32_t r : rows) {
            std::vector<KeyPoint::Descriptor> unused;
            obs.emplace_back();
            observationsOf(r, obs.back(), unused);
            const auto &first = *observations[r].begin();
            firstOctave.push_back(m.octave[slotOfId.at(first.first)][first.second]);
        }
        if (!rows.empty()) ref.points.refresh(ctx, poses, rows, obs, firstOctave, settings, descriptors ? &pool : nullptr);
    };
    std::vector<std::int32_t> refreshRows;
    for (std::size_t i = 0; i < tracked.size(); ++i) {
        if (tri.status[i] == 1) {                            // UNSURE: updateDescriptor of :811 alone, the general medoid
            std::vector<MapObservation> obs;
            std::vector<std::vector<KeyPoint::Descriptor>> desc(1);
            observationsOf(tracked[i], obs, desc[0]);
            const int best = updateDescriptors(ctx, desc)[0];
            if (best >= 0) ref.points.update(tracked[i], 1, nullptr, nullptr, nullptr, nullptr, &desc[0][best]);
            ++unsure;
        } else if (tri.status[i] == 2) { refreshRows.push_back(tracked[i]); ++promoted; }
    }
    refresh(refreshRows, true);                              // :811 and :121-124 of the just-tracked points
    refresh(checked, frameHasDescriptors);                   // :121-124 of the checked ones

    if (got.outcome != outcome) { std::printf("the outcomes differ\n"); return 3; }
    if (got.createdRows != createdRows || got.createdKeyPoints != createdKp) { std::printf("the created rows differ\n"); return 3; }
    if (got.justTriangulated != tracked.size() || got.checked != checked.size() || got.frustumFail != frustumFail || got.reproFail != reproFail || got.newPoints != createdRows.size() ||
        got.success != promoted + checked.size()) { std::printf("the counters differ\n"); return 4; }
    if (got.firstLast.status != tri.status || got.firstLast.reason != tri.reason || got.firstLast.passCount != tri.passCount) { std::printf("FIRST_LAST's results differ\n"); return 4; }
    if (dev.tracks.window() != ref.tracks.window()) { std::printf("the track windows differ\n"); return 5; }
    if (dev.bytes(ctx, dev.tracks.window()) != ref.bytes(ctx, ref.tracks.window())) { std::printf("the tables differ\n"); return 5; }
    const std::size_t created = createdRows.size(), absent = (std::size_t)std::count(outcome.begin(), outcome.end(), (std::uint8_t)6);
    if (tracked.size() < 5 || checked.size() < 5 || frustumFail < 3 || reproFail < 3 || unsure < 3 || promoted < 3 || (frameHasDescriptors ? created : absent) < 5) {
        std::printf("the map exercises too little (%zu %zu %zu %zu %zu %zu %zu %zu)\n", tracked.size(), checked.size(), frustumFail, reproFail, unsure, promoted, created, absent);
        return 6;
    }
    std::printf("matchTrackedFeatures ok descriptors %d: %zu created, %zu just tracked (%zu unsure, %zu triangulated), %zu checked, %zu + %zu rejected, %zu without descriptors, tables bit-equal\n",
                frameHasDescriptors ? 1 : 0, created, tracked.size(), unsure, promoted, checked.size(), frustumFail, reproFail, absent);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_match_tracked, (const void *)&ms_match_tracked_check, (const void *)&ms_match_tracked_finish,
                                   (const void *)&ms_match_tracked_finish_check};
    std::printf("link ok %d\n", syms[0] && syms[1] && syms[2] && syms[3]);
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    try {
        if (int rc = run(true)) return rc;
        return run(false);
    } catch (const std::exception &e) {
        std::printf("failed: %s\n", e.what());
        return 2;
    }
}
