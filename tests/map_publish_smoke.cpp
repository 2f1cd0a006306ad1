// Compile + link check of the two steps of the host mirror that hand the map to someone outside the mapper (publishMapForViewer and
// updatePointCloudRecording in mi355slam/map_update.hpp) against libmi355slam.so, and both against literal std::map / std::set restatements of
// mapper_helpers.cpp:814-909 on a hand-computed map of 3 keyframes and 12 points (tests/test_map_publish_smoke.py).
//   map_publish_smoke --no-gpu   the restatements against the hand-computed answers (no context, no device)
//   map_publish_smoke --gpu      the mirror against the restatements over three recording steps; the neighbour indices; the refusals
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

int fails = 0;
void expect(bool ok, const char *what) { if (!ok) { std::printf("FAILED: %s\n", what); ++fails; } }

constexpr int kSlots = 3, kStride = 6, kRows = 12;
enum Status { TRIANGULATED = 0, NOT_TRIANGULATED = 1, UNSURE = 2 };

// ---- the map as the reference holds it ------------------------------------------------------------------------------------------------------
struct Mp {
    int id;
    std::array<double, 3> position;
    std::array<float, 3> norm;
    int status;
    std::set<int> observations;                              // the observing KfIds
};
struct Map {
    std::map<int, Mp> mapPoints;
    std::map<int, std::vector<int>> keyframes;               // KfId -> Keyframe::mapPoints
    std::set<int> localMpIds;
};
struct Point { std::array<float, 3> position, normal; int status; bool localMap, nowVisible; int id; };

// mapper_helpers.cpp:823-839, statement by statement
std::vector<Point> restatedPublish(const Map &db) {
    const std::vector<int> &current = db.keyframes.rbegin()->second;
    std::set<int> visibleIds;
    for (int mpId : current) if (mpId != -1) visibleIds.insert(mpId);
    std::vector<Point> mps;
    for (const auto &idMp : db.mapPoints) {
        const Mp &mp = idMp.second;
        if (mp.status == NOT_TRIANGULATED) continue;
        mps.push_back(Point{{(float)mp.position[0], (float)mp.position[1], (float)mp.position[2]}, mp.norm, mp.status, db.localMpIds.count(mp.id) > 0,
                            visibleIds.count(mp.id) > 0, mp.id});
    }
    return mps;
}

// :881-909, statement by statement (4 -> minObservations)
void restatedRecording(float t, std::map<int, MapPointRecord> &records, const std::map<int, Mp> &mapPoints, std::size_t minObservations) {
    for (const auto &it : mapPoints) {
        const Mp &mp = it.second;
        if (mp.observations.size() < minObservations) continue;
        const std::array<float, 3> p{(float)mp.position[0], (float)mp.position[1], (float)mp.position[2]};
        if (!records.count(mp.id)) {
            MapPointRecord r;
            r.positions.push_back({t, p}); r.normal = mp.norm;
            records.insert({mp.id, r});
        } else if (records.at(mp.id).positions.back().p != p) {
            records.at(mp.id).positions.push_back({t, p});
            records.at(mp.id).normal = mp.norm;
        }
    }
    const std::array<float, 3> p0{0.0f, 0.0f, 0.0f};
    for (auto &it : records) {
        if (!it.second.removed && !mapPoints.count(it.first)) {
            it.second.removed = true;
            it.second.positions.push_back({t, p0});
        }
    }
}

bool sameRecords(const std::map<int, MapPointRecord> &a, const std::map<std::int32_t, MapPointRecord> &b) {
    if (a.size() != b.size()) return false;
    for (const auto &it : a) {
        const auto f = b.find(it.first);
        if (f == b.end() || f->second.removed != it.second.removed || f->second.normal != it.second.normal || f->second.positions.size() != it.second.positions.size()) return false;
        for (std::size_t i = 0; i < it.second.positions.size(); ++i)
            if (f->second.positions[i].t != it.second.positions[i].t || f->second.positions[i].p != it.second.positions[i].p) return false;
    }
    return true;
}

// the hand-computed map: KfIds 5, 9, 7 in slots 0, 1, 2 (the current keyframe, id 9, is slot 1); rows 0 - 8 are map points, 9 - 11 free
const int kKfId[kSlots] = {5, 9, 7};
const std::uint8_t kFlags[kRows] = {3, 3, 2, 0, 3, 2, 3, 0, 3, 3, 0, 0};      // row 9: a stale flag on a free row
Map handMap() {
    Map db;
    db.keyframes[5] = {0, 1, 2, 3, 4, 5};
    db.keyframes[9] = {0, 1, 2, 3, -1, 6};
    db.keyframes[7] = {0, 1, 2, 3, 4, 7};
    for (int r = 0; r < 9; ++r) {
        Mp mp{r, {r + 0.5, -1.0 * r, 0.25 * r + 1.0 / 3.0}, {(float)r, 1.0f, 2.0f}, kFlags[r] == 3 ? TRIANGULATED : kFlags[r] == 2 ? UNSURE : NOT_TRIANGULATED, {}};
        for (const auto &kf : db.keyframes) for (int e : kf.second) if (e == r) mp.observations.insert(kf.first);
        db.mapPoints[r] = mp;
    }
    db.localMpIds = {1, 4, 6};
    return db;
}

int no_gpu() {
    std::printf("link ok %d\n", ms_version() != nullptr);
    Map db = handMap();
    const std::vector<Point> mps = restatedPublish(db);
    // NOT_TRIANGULATED rows 3 and 7 are skipped; localMap 1, 4, 6; the current keyframe (id 9) sees 0, 1, 2, 3, 6
    const int ids[] = {0, 1, 2, 4, 5, 6, 8}, local[] = {0, 1, 0, 1, 0, 1, 0}, visible[] = {1, 1, 1, 0, 0, 1, 0}, status[] = {0, 0, 2, 0, 2, 0, 0};
    expect(mps.size() == 7, "seven published points");
    for (std::size_t k = 0; k < mps.size() && k < 7; ++k)
        expect(mps[k].id == ids[k] && mps[k].localMap == (local[k] != 0) && mps[k].nowVisible == (visible[k] != 0) && mps[k].status == status[k], "the hand-computed point vector");
    expect(mps[1].position == std::array<float, 3>({1.5f, -1.0f, (float)(0.25 + 1.0 / 3.0)}), "positions are cast once");
    std::map<int, MapPointRecord> records;
    restatedRecording(1.0f, records, db.mapPoints, 3);
    expect(records.size() == 4 && records.count(3) && !records.count(4), "rows 0 - 3 have three observations; the status does not matter");
    std::printf(fails ? "restatement FAILED\n" : "restatement ok\n");
    return fails ? 1 : 0;
}

// ---- the device side ----------------------------------------------------------------------------------------------------------------------
struct Device {
    Context &ctx;
    DeviceKeyframeMapPoints keyframes;
    DeviceMapPoints points;
    DeviceMapPointFlags flags;
    DeviceMapPointLive live;
    DeviceKeyframePoses poses;
    DeviceArray<std::int32_t> counts;
    KeyframeSlots slots;
    static std::vector<DeviceMapPoints::Vec3d> zeros3d() { return std::vector<DeviceMapPoints::Vec3d>(kRows, DeviceMapPoints::Vec3d{7.0, 7.0, 7.0}); }
    explicit Device(Context &c)
        : ctx(c), keyframes(c, kSlots, kStride, kRows),
          points(c, zeros3d(), std::vector<DeviceMapPoints::Vec3f>(kRows, DeviceMapPoints::Vec3f{-9.0f, -9.0f, -9.0f}), std::vector<float>(kRows, 0.0f), std::vector<float>(kRows, 0.0f),
                 std::vector<KeyPoint::Descriptor>(kRows, KeyPoint::Descriptor{})),
          flags(c, std::vector<std::uint8_t>(kFlags, kFlags + kRows)), live(c, std::vector<std::uint8_t>(kRows, 0)),
          poses(c, std::vector<DeviceKeyframePoses::Pose>(kSlots, DeviceKeyframePoses::Pose{0, -1, 0, 1.0, 1, 0, 0, 2.0, 0, 0, 1, 3.0})), counts(c, kRows) {
        slots.id.assign(kKfId, kKfId + kSlots);
        slots.previous = {-1, 2, 0}; slots.next = {2, -1, 1};      // 5 -> 7 -> 9 as slots 0 -> 2 -> 1
    }
    MapTables tables() {
        MapTables M{keyframes, slots};
        M.points = &points; M.flags = &flags; M.live = &live; M.poses = &poses; M.observationCount = counts.data();
        return M;
    }
    // the tables of a map state: row = MpId, the flags of live rows from the status, free rows keep kFlags
    void upload(const Map &db) {
        std::vector<std::uint8_t> f(kFlags, kFlags + kRows), l(kRows, 0);
        for (const auto &it : db.mapPoints) {
            const Mp &mp = it.second;
            f[mp.id] = mp.status == TRIANGULATED ? 3 : mp.status == UNSURE ? 2 : 0; l[mp.id] = 1;
            const DeviceMapPoints::Vec3d p = mp.position;
            const DeviceMapPoints::Vec3f n = mp.norm;
            points.update((std::size_t)mp.id, 1, &p, &n, nullptr, nullptr, nullptr);
        }
        flags.update(0, kRows, f.data()); live.update(0, kRows, l.data());
        for (int k = 0; k < kSlots; ++k) keyframes.update((std::size_t)k, db.keyframes.at(kKfId[k]));
        observationCountsOnDevice(ctx, tables());
    }
};

int gpu() {
    Context ctx(0);
    Device D(ctx);
    Map db = handMap();
    D.upload(db);
    MapTables M = D.tables();
    const std::vector<std::int32_t> localHost = {4, 1, 6, 6, -1, kRows, 1 << 30};     // any order, a repeat, entries that are not VALID
    DeviceArray<std::int32_t> local(ctx, localHost.size());
    local.upload(0, localHost.size(), localHost.data());

    // ---- the refusals, all before any device call
    int refused = 0;
    try { publishMapForViewer(ctx, M, {3}, DeviceRows{}, 1); } catch (const std::invalid_argument &) { ++refused; }
    try { publishMapForViewer(ctx, M, {}, DeviceRows{nullptr, 2}, 1); } catch (const std::invalid_argument &) { ++refused; }
    { MapTables N = M; N.poses = nullptr; try { publishMapForViewer(ctx, N, {}, DeviceRows{}, 1); } catch (const std::invalid_argument &) { ++refused; } }
    DeviceMapPointRecords records(ctx);
    std::map<std::int32_t, MapPointRecord> host;
    { MapTables N = M; N.observationCount = nullptr; try { updatePointCloudRecording(ctx, N, records, 0.0f, host, 3); } catch (const std::invalid_argument &) { ++refused; } }
    try { updatePointCloudRecording(ctx, M, records, 0.0f, host, -1); } catch (const std::invalid_argument &) { ++refused; }
    expect(refused == 5 && records.size() == 0 && host.empty(), "five refusals that leave everything");
    std::printf("refusals ok %d cases\n", refused);

    // ---- publishMapForViewer against the restatement
    const ViewerMap V = publishMapForViewer(ctx, M, {0}, DeviceRows{local.data(), local.size()}, 1);
    const std::vector<Point> want = restatedPublish(db);
    expect(V.mapPoints.size() == want.size(), "the number of published points");
    for (std::size_t k = 0; k < want.size() && k < V.mapPoints.size(); ++k) {
        const ViewerMapPoint &p = V.mapPoints[k];
        expect(p.row == want[k].id && p.position == want[k].position && p.normal == want[k].normal && p.status == want[k].status && p.localMap == want[k].localMap &&
               p.nowVisible == want[k].nowVisible && p.color == std::array<float, 3>({0.0f, 0.0f, 0.0f}), "a published point");
    }
    // the keyframes in ascending KfId: 5 (slot 0, adjacent), 7 (slot 2), 9 (slot 1, current); R = a quarter turn about z, t = (1, 2, 3): poseWC = R^T | (-2, 1, -3)
    expect(V.keyframes.size() == 3 && V.keyframes[0].id == 5 && V.keyframes[1].id == 7 && V.keyframes[2].id == 9, "ascending KfId");
    expect(V.keyframes[0].localMap && !V.keyframes[1].localMap && !V.keyframes[2].localMap && V.keyframes[2].current && !V.keyframes[0].current && !V.keyframes[1].current, "localMap, current");
    const std::array<float, 16> poseWC = {0, 1, 0, -2, -1, 0, 0, 1, 0, 0, 1, -3, 0, 0, 0, 1};
    for (const ViewerKeyframe &kf : V.keyframes) expect(kf.poseWC == poseWC, "poseWC");
    // the neighbour indices: getNeighbors per keyframe, through inds.at(kfId) (:862-872); every pair shares rows 0 - 3
    std::map<int, std::size_t> inds;
    for (std::size_t i = 0; i < V.keyframes.size(); ++i) inds.emplace(V.keyframes[i].id, i);
    const std::int32_t slotOf[3] = {0, 2, 1};
    for (std::size_t i = 0; i < 3; ++i) {
        const std::int32_t k = slotOf[i];
        const std::vector<std::vector<std::int32_t>> nb = getNeighbors(ctx, D.keyframes, &D.flags, {NeighborQuery{k, D.slots.previous[k], D.slots.next[k], 1, false}});
        std::vector<int> wantIdx;
        for (std::int32_t s : nb[0]) wantIdx.push_back((int)inds.at(kKfId[s]));
        std::sort(wantIdx.begin(), wantIdx.end());
        expect(V.keyframes[i].neighbors == wantIdx && wantIdx.size() == 2 && wantIdx[0] != (int)i && wantIdx[1] != (int)i, "neighbour indices");
    }
    std::printf("publishMapForViewer ok: %zu points, %zu keyframes\n", V.mapPoints.size(), V.keyframes.size());

    // ---- three recording steps
    std::map<int, MapPointRecord> wantRecords;
    std::size_t events[4];
    restatedRecording(1.0f, wantRecords, db.mapPoints, 3);
    events[0] = updatePointCloudRecording(ctx, M, records, 1.0f, host, 3);
    expect(events[0] == 4 && sameRecords(wantRecords, host) && records.size() == kRows, "step 1: rows 0 - 3 are new");
    // row 1 moves, row 2 is removed and row 9 takes its entries, row 4 moves with two observations
    db.mapPoints[1].position = {1.75, -1.0, 0.5};
    db.mapPoints[4].position = {40.0, 40.0, 40.0};
    db.mapPoints.erase(2);
    for (auto &kf : db.keyframes) for (int &e : kf.second) if (e == 2) e = 9;
    db.mapPoints[9] = Mp{9, {9.0, 9.5, -9.0}, {0.5f, 0.5f, 0.5f}, UNSURE, {5, 7, 9}};
    D.upload(db);
    restatedRecording(2.0f, wantRecords, db.mapPoints, 3);
    events[1] = updatePointCloudRecording(ctx, M, records, 2.0f, host, 3);
    expect(events[1] == 3 && sameRecords(wantRecords, host), "step 2: moved, removed, new");
    expect(host.at(2).removed && host.at(2).positions.back().p == std::array<float, 3>({0.0f, 0.0f, 0.0f}) && host.at(1).positions.size() == 2 && host.at(9).positions.size() == 1, "step 2 by hand");
    // nothing changes; then row 0 loses an observation and moves: still nothing
    events[2] = updatePointCloudRecording(ctx, M, records, 2.5f, host, 3);
    db.keyframes[5][0] = -1; db.mapPoints[0].observations.erase(5); db.mapPoints[0].position = {-1.0, -1.0, -1.0};
    D.upload(db);
    restatedRecording(3.0f, wantRecords, db.mapPoints, 3);
    events[3] = updatePointCloudRecording(ctx, M, records, 3.0f, host, 3);
    expect(events[2] == 0 && events[3] == 0 && sameRecords(wantRecords, host), "step 3: no event");
    expect(records.downloadState() == std::vector<std::uint8_t>({1, 1, 2, 1, 0, 0, 0, 0, 0, 1, 0, 0}), "the record state");
    std::printf("updatePointCloudRecording ok: %zu + %zu + %zu events\n", events[0], events[1], events[3]);
    std::printf(fails ? "mirror FAILED\n" : "mirror ok\n");
    return fails ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--no-gpu")) return no_gpu();
    if (argc == 2 && !std::strcmp(argv[1], "--gpu")) return gpu();
    std::printf("usage: map_publish_smoke --no-gpu | --gpu\n");
    return 2;
}
