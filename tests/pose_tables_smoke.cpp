// Compile + link check of poseBundleAdjustOnTables (mi355slam/map_update.hpp) against libmi355slam.so, and its run on one small map.
//   pose_tables_smoke --no-gpu   the symbols link; a few calls of ms_pose_tables_solve_check (no context, no device)
//   pose_tables_smoke            poseBundleAdjustOnTables on a seeded map against the mirror's own poseBundleAdjust on a BaWindow that the host
//                                builds from Keyframe::mapPoints and a map of MapPoints the way bundle_adjuster.cpp:403-480 does: the same
//                                pose bit for bit, the same solver counters, kf_pose[slot] = the matrix of that pose and nothing else written;
//                                and the reference's bool in both directions (too few points, no previous keyframe: false, nothing written).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
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

int fail(const char *what) { std::printf("FAILED: %s\n", what); return 1; }

int no_gpu() {
    char why[256] = {0};
    const auto *dev = reinterpret_cast<std::int32_t *>(0x1000);       // never dereferenced by the validation
    const auto *devd = reinterpret_cast<double *>(0x1000);
    const auto *devf = reinterpret_cast<float *>(0x1000);
    const auto *devb = reinterpret_cast<std::uint8_t *>(0x1000);
    ms_pose_tables_frame f{};
    f.slot = 1; f.prev_slot = 2; f.n_kp = 20; f.cam = ms_pinhole{500.0, 501.0, 320.0, 240.0, 640, 480}; f.focal = 500;
    f.edge_meas[3] = 1.0; f.min_visible = 10; f.max_iters = 10; f.huber_delta = 2.4477;
    ms_pose_tables_out out{};
    auto check = [&](int nKf, int stride) { return ms_pose_tables_solve_check(dev, nKf, stride, devb, nullptr, devd, 50, devf, devf, dev, devd, &f, &out, why, sizeof(why)); };
    int cases = 0;
    if (check(3, 32) != MS_OK) return fail("a valid call was turned away");
    ++cases;
    f.prev_slot = -1;
    if (check(3, 32) != MS_OK) return fail("a frame without a previous keyframe was turned away");
    ++cases;
    f.prev_slot = 1;
    if (check(3, 32) != MS_ERR_INVALID || !std::strstr(why, "its own previous keyframe")) return fail("slot == prev_slot passed");
    ++cases;
    f.prev_slot = 2; f.n_kp = 33;
    if (check(3, 32) != MS_ERR_INVALID || !std::strstr(why, "33 keypoints")) return fail("n_kp > stride passed");
    ++cases;
    f.n_kp = 20; f.edge_info[7] = std::nan("");
    if (check(3, 32) != MS_ERR_INVALID || !std::strstr(why, "edge_info[7]")) return fail("a NaN information passed");
    ++cases;
    f.edge_info[7] = 0.0;
    if (check(MS_COVIS_MAX_KF + 1, 32) != MS_ERR_CAPACITY) return fail("the slot cap");
    ++cases;
    std::printf("link ok %d\n", (int)(reinterpret_cast<void *>(&ms_pose_tables_solve) != nullptr && reinterpret_cast<void *>(&ms_pose_tables_create) != nullptr));
    std::printf("no-gpu ok %d cases\n", cases);
    return 0;
}

struct Map {
    static constexpr int nKf = 3, stride = 320, nMp = 300, frame = 1, prev = 2, nKp = 290;
    std::vector<std::vector<std::int32_t>> mapPoints;        // Keyframe::mapPoints per slot
    std::vector<std::vector<float>> x, y;
    std::vector<std::vector<std::int32_t>> octave;
    std::vector<DeviceKeyframePoses::Pose> pose;
    KeyframeSlots cams;                      // camera and focalLength
    std::vector<DeviceMapPoints::Vec3d> position;
    std::vector<std::uint8_t> flags, live;
    PoseOdometryEdge edge;
};

Map make_map() {
    Map m;
    Rng rng;
    const ms_pinhole cam{500.0, 502.0, 320.0, 240.0, 640, 480};
    const double centre[Map::nKf] = {0.0, 0.4, 0.2};         // the frame lies ahead of its previous keyframe
    m.mapPoints.assign(Map::nKf, {}); m.x.assign(Map::nKf, {}); m.y.assign(Map::nKf, {}); m.octave.assign(Map::nKf, {});
    for (int k = 0; k < Map::nKf; ++k) {
        const double off = k == Map::frame ? 0.05 : 0.002;   // the tracker's pose of the frame is 5 cm off
        m.pose.push_back({1, 0, 0, -centre[k] + off * rng.unit(), 0, 1, 0, off * rng.unit(), 0, 0, 1, off * rng.unit()});
        m.cams.camera.push_back(cam);
        m.cams.focalLength.push_back(501);
    }
    m.position.assign(Map::nMp, DeviceMapPoints::Vec3d{0, 0, 0});
    m.flags.assign(Map::nMp, 0); m.live.assign(Map::nMp, 1);
    std::vector<std::int32_t> rows;
    for (int r = 0; r < Map::nMp; ++r) rows.push_back(r);
    for (int r = Map::nMp - 1; r > 0; --r) std::swap(rows[(std::size_t)r], rows[(std::size_t)rng.below(r + 1)]);      // rows do not ascend with the keypoint
    std::size_t next = 0;
    for (int j = 0; j < Map::nKp; ++j) {
        const int kind = j % 9;                              // 0: unbound | 4: not live | 7: UNSURE | otherwise TRIANGULATED
        const DeviceMapPoints::Vec3d X{-1.5 + 4.0 * rng.unit(), -1.0 + 2.0 * rng.unit(), 4.0 + 5.0 * rng.unit()};
        const double u = 500.0 * (X[0] - centre[Map::frame]) / X[2] + 320.0 + 0.3 * (rng.unit() - 0.5), v = 502.0 * X[1] / X[2] + 240.0 + 0.3 * (rng.unit() - 0.5);
        std::int32_t r = -1;
        if (kind != 0) {
            r = rows[next++];
            m.position[(std::size_t)r] = {X[0] + 0.01 * (rng.unit() - 0.5), X[1] + 0.01 * (rng.unit() - 0.5), X[2] + 0.01 * (rng.unit() - 0.5)};
            m.flags[(std::size_t)r] = kind == 7 ? 2 : 3;
            m.live[(std::size_t)r] = kind == 4 ? 0 : 1;
            if (j % 2) { m.mapPoints[Map::prev].push_back(r); m.x[Map::prev].push_back((float)u + 20.f); m.y[Map::prev].push_back((float)v); m.octave[Map::prev].push_back(0); }
        }
        m.mapPoints[Map::frame].push_back(r); m.x[Map::frame].push_back((float)u); m.y[Map::frame].push_back((float)v);
        m.octave[Map::frame].push_back(rng.below(8));
    }
    // rotations are the identity here: poseDifference(previous, frame) is the difference of the true translations
    m.edge.measurement = {0, 0, 0, 1, -centre[Map::prev] + centre[Map::frame] + 0.002 * rng.unit(), 0.002 * rng.unit(), 0.002 * rng.unit()};
    for (int i = 0; i < 6; ++i) m.edge.information[(std::size_t)(7 * i)] = (i < 3 ? 100.0 * 100.0 : 50.0 * 50.0) * 2.6667;
    return m;
}

struct Tables {
    DeviceKeyframeMapPoints kf;
    DeviceMapPoints points;
    DeviceMapPointFlags flags;
    DeviceMapPointLive live;
    DeviceKeypointTable kp;
    DeviceKeyframePoses poses;
    KeyframeSlots slots;
    Tables(Context &ctx, const Map &m)
        : kf(ctx, Map::nKf, Map::stride, Map::nMp),
          points(ctx, m.position, std::vector<DeviceMapPoints::Vec3f>(Map::nMp, DeviceMapPoints::Vec3f{0, 0, 1}), std::vector<float>(Map::nMp, 0.f), std::vector<float>(Map::nMp, 0.f),
                 std::vector<KeyPoint::Descriptor>(Map::nMp, KeyPoint::Descriptor{})),
          flags(ctx, m.flags), live(ctx, m.live), kp(ctx, Map::nKf, Map::stride), poses(ctx, m.pose), slots(m.cams) {
        for (int k = 0; k < Map::nKf; ++k) {
            kf.update((std::size_t)k, m.mapPoints[(std::size_t)k]);
            kp.update((std::size_t)k, m.x[(std::size_t)k], m.y[(std::size_t)k], m.octave[(std::size_t)k], {});
        }
    }
    MapTables view() {
        MapTables M{kf, slots};
        M.flags = &flags; M.points = &points; M.live = &live; M.keypoints = &kp; M.poses = &poses;
        return M;
    }
};

struct Snapshot {
    std::vector<std::int32_t> kf;
    std::vector<std::uint8_t> flags, live;
    std::vector<double> position;
    std::vector<DeviceKeyframePoses::Pose> poses;
    bool same_but_poses(const Snapshot &o) const {
        return kf == o.kf && flags == o.flags && live == o.live && position.size() == o.position.size() && std::memcmp(position.data(), o.position.data(), 8 * position.size()) == 0;
    }
};

Snapshot snapshot(Context &ctx, Tables &t) {
    return Snapshot{ctx.download(t.kf.table(), (std::size_t)Map::nKf * Map::stride), ctx.download(t.flags.flags(), (std::size_t)Map::nMp), t.live.download(),
                    ctx.download(t.points.position(), 3 * (std::size_t)Map::nMp), t.poses.download()};
}

bool same_pose(const DeviceKeyframePoses::Pose &a, const DeviceKeyframePoses::Pose &b) { return std::memcmp(a.data(), b.data(), sizeof(a)) == 0; }

// rows 0-2 of to_homogeneous_matrix(): Eigen's toRotationMatrix of the quaternion as given (the conversion of ms_ba_window_apply)
DeviceKeyframePoses::Pose matrix_of(const double *s) {
    const double x = s[0], y = s[1], z = s[2], w = s[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    return {1.0 - (tyy + tzz), txy - twz, txz + twy, s[4], txy + twz, 1.0 - (txx + tzz), tyz - twx, s[5], txz - twy, tyz + twx, 1.0 - (txx + tyy), s[6]};
}

int with_gpu() {
    Context ctx(0);
    const Map m = make_map();
    Parameters params;
    params.poseBAIterations = 3;
    const StaticSettings settings(params);
    // ---- the restatement: poseBundleAdjust's walk over keyframe.mapPoints with a map of MapPoints on the host (:403-407, :453-480)
    struct MapPoint { std::uint8_t status; DeviceMapPoints::Vec3d position; };
    std::map<int, MapPoint> mapPoints;
    for (int r = 0; r < Map::nMp; ++r) if (m.live[(std::size_t)r]) mapPoints[r] = MapPoint{m.flags[(std::size_t)r], m.position[(std::size_t)r]};
    BaWindow w;
    const auto &P0 = m.pose[Map::frame], &P1 = m.pose[Map::prev];
    w.poses = {{0, 0, 0, 1, P0[3], P0[7], P0[11]}, {0, 0, 0, 1, P1[3], P1[7], P1[11]}};          // matrixToPose of an identity rotation
    w.currentKeyframe = 0;
    const ms_pinhole &cam = m.cams.camera[Map::frame];
    std::size_t triangulated = 0;
    for (std::size_t i = 0; i < m.mapPoints[Map::frame].size(); ++i) {
        const std::int32_t id = m.mapPoints[Map::frame][i];
        if (id == -1 || !mapPoints.count(id)) continue;      // a row that is not live holds no map point: its binding reads as erased
        const MapPoint &mp = mapPoints.at(id);
        if (!(mp.status & DeviceMapPointFlags::TRIANGULATED)) continue;
        ++triangulated;
        w.obsPose.push_back(0); w.obsPoint.push_back((std::int32_t)w.points.size());
        w.points.push_back(mp.position);
        w.obsUv.push_back({((double)m.x[Map::frame][i] - cam.cx) / cam.fx, ((double)m.y[Map::frame][i] - cam.cy) / cam.fy});
        const double focal = (double)m.cams.focalLength[Map::frame];
        w.obsInfo.push_back(focal * focal / (double)settings.levelSigmaSq[(std::size_t)m.octave[Map::frame][i]]);
    }
    w.edgeI = {0}; w.edgeJ = {1}; w.edgeMeas = {m.edge.measurement}; w.edgeInfo = {m.edge.information};
    if (triangulated < 150 || triangulated >= (std::size_t)Map::nKp - 60) return fail("the map does not mix kept and dropped keypoints");
    ms_ba_result want{};
    if (!poseBundleAdjust(ctx, w, (int)params.poseBAIterations, &want)) return fail("the mirror's poseBundleAdjust did not run");
    if (!(want.chi2_final < 0.5 * want.chi2_initial)) return fail("the host-built problem does not move the pose");
    // ---- the device path
    Tables t(ctx, m);
    DevicePoseAdjuster adjuster(ctx, 320, settings);
    const Snapshot before = snapshot(ctx, t);
    auto run = [&](std::int32_t prevSlot) {
        return poseBundleAdjustOnTables(ctx, t.view(), adjuster, Map::frame, prevSlot, m.edge, params, settings);
    };
    // false: one point too few, and no previous keyframe; nothing is written
    params.minVisibleMapPointsInCurrentFrameBA = (unsigned)triangulated + 1;
    if (run(Map::prev)) return fail("ran with one triangulated map point too few");
    if (adjuster.last.n_triangulated != (std::int32_t)triangulated) return fail("n_triangulated");
    params.minVisibleMapPointsInCurrentFrameBA = (unsigned)triangulated;
    if (run(-1)) return fail("ran without a previous keyframe");
    {
        const Snapshot s = snapshot(ctx, t);
        if (!s.same_but_poses(before) || s.poses != before.poses) return fail("a call that returned false wrote a table");
    }
    // true: at the threshold
    if (!run(Map::prev)) return fail("did not run at the threshold");
    const ms_pose_tables_out &got = adjuster.last;
    if (got.n_triangulated != (std::int32_t)triangulated) return fail("n_triangulated");
    if (std::memcmp(got.pose, w.poses[0].data(), 7 * sizeof(double)) != 0) return fail("the pose differs from poseBundleAdjust on the host-built window");
    if (got.result.iterations != want.iterations || got.result.trials != want.trials || got.result.stopped_early != want.stopped_early ||
        got.result.final_lambda != want.final_lambda || got.result.chi2_initial != want.chi2_initial || got.result.chi2_final != want.chi2_final)
        return fail("the solver counters differ from poseBundleAdjust on the host-built window");
    const Snapshot after = snapshot(ctx, t);
    if (!after.same_but_poses(before)) return fail("a table other than kf_pose was written");
    for (int k = 0; k < Map::nKf; ++k) {
        const DeviceKeyframePoses::Pose wantPose = k == Map::frame ? matrix_of(got.pose) : before.poses[(std::size_t)k];
        if (!same_pose(after.poses[(std::size_t)k], wantPose)) return fail("kf_pose");
    }
    if (same_pose(after.poses[Map::frame], before.poses[Map::frame])) return fail("the frame's pose did not move");
    // the whole stride instead of the frame's keypoint count gives the same problem: the entries behind the keypoints are -1
    t.poses.update(0, Map::nKf, before.poses.data());
    if (!poseBundleAdjustOnTables(ctx, t.view(), adjuster, Map::frame, Map::prev, m.edge, params, settings, (std::size_t)Map::nKp))
        return fail("did not run with the keypoint count given");
    if (std::memcmp(adjuster.last.pose, w.poses[0].data(), 7 * sizeof(double)) != 0) return fail("the pose with the keypoint count given");
    std::printf("poseBundleAdjustOnTables ok: %zu of %d keypoints, chi2 %.1f -> %.1f in %d iterations, both directions of the bool hold\n", triangulated, Map::nKp,
                want.chi2_initial, want.chi2_final, want.iterations);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    return with_gpu();
}
