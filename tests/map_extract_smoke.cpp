// Compile + link check of the partial map copy of the host mirror (extractMap, copyMapToFrontend in mi355slam/map_update.hpp) against
// libmi355slam.so, and its comparison with a sequential std::map / std::set restatement of MapDB(mapDB, activeKeyframes) (mapdb.cpp:116-159) and
// MapPoint(mp, activeKeyframes) (map_point.cpp:22-43) on a hand-computed map (tests/test_map_extract_smoke.py).
//   map_extract_smoke --no-gpu   the restatement against the hand-computed results (no context, no device)
//   map_extract_smoke --gpu      extractMap for a list, copyMapToFrontend partial and full, the cut and translated links, and the
//                                std::invalid_argument cases, which leave the destination alone
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

constexpr int kStride = 8, kRows = 12, kSlots = 6, kTrackBase = 100, kWindow = 128;
using Rows = std::vector<std::int32_t>;

// ---- the reference's map and its copy constructor, sequentially ------------------------------------------------------------------------
struct HostKeyframe {
    Rows mapPoints;                                          // Keyframe::mapPoints (-1 = none)
    std::int32_t previous = -1, next = -1;                   // KfIds
};
struct HostMapPoint {
    std::int32_t trackId = -1;
    std::map<std::int32_t, Rows> observations;               // KfId -> keypoints
};
struct HostMap {
    std::map<std::int32_t, HostKeyframe> keyframes;          // by KfId
    std::map<std::int32_t, HostMapPoint> mapPoints;          // by MpId = table row
    std::map<std::int32_t, std::int32_t> trackIdToMapPoint;
};

// mapdb.cpp:116-159.  An entry whose map point is not in mapDB.mapPoints (a row that is not live) is dropped, where the reference's .at throws.
HostMap partial_copy(const HostMap &mapDB, const std::set<std::int32_t> &activeKeyframes, std::size_t *dropped) {
    HostMap out;
    std::set<std::int32_t> activeMapPoints;
    for (std::int32_t kfId : activeKeyframes) {
        HostKeyframe kf = mapDB.keyframes.at(kfId);
        if (kf.next >= 0 && !activeKeyframes.count(kf.next)) kf.next = -1;
        if (kf.previous >= 0 && !activeKeyframes.count(kf.previous)) kf.previous = -1;
        for (std::int32_t mpId : kf.mapPoints) {
            if (mpId < 0) continue;
            if (mapDB.mapPoints.count(mpId)) activeMapPoints.insert(mpId); else ++*dropped;
        }
        out.keyframes.emplace(kfId, kf);
    }
    for (std::int32_t mpId : activeMapPoints) {              // MapPoint(mp, activeKeyframes), map_point.cpp:22-36
        const HostMapPoint &mp = mapDB.mapPoints.at(mpId);
        HostMapPoint copy;
        copy.trackId = mp.trackId;
        for (const auto &o : mp.observations) if (activeKeyframes.count(o.first)) copy.observations.insert(o);
        out.mapPoints.emplace(mpId, copy);
    }
    for (const auto &p : mapDB.trackIdToMapPoint) if (activeMapPoints.count(p.second)) out.trackIdToMapPoint.insert(p);      // :141-145
    return out;
}

// The tables of the hand-computed map: five keyframes in a chain (slots 0 - 4 in KfId order) and an empty slot with a stale entry.
//   row 2: seen by everybody   row 6: slots 3 and 4   row 7: twice in slot 4   rows 8, 10: slot 4 alone   row 9: slot 4 alone, not live
//   row 5: twice in slot 2     row 4: slots 1 and 2   row 3: slot 1 alone     row 1: slots 0 and 1       row 0: slots 0 and 3   row 11: nobody, not live
struct Tables {
    std::vector<Rows> mapPoints = {{0, 1, 2, -1, -1, -1, -1, -1}, {1, 2, 3, 4, -1, -1, -1, -1}, {2, 4, 5, 5, -1, -1, -1, -1}, {0, 6, -1, 2, -1, -1, -1, -1},
                                   {2, 6, 7, 8, -1, 9, 7, 10}, {3, -1, -1, -1, -1, -1, -1, -1}};
    std::vector<std::uint8_t> flags = std::vector<std::uint8_t>(kRows, 2), live = std::vector<std::uint8_t>(kRows, 1);
    Rows track, keyPointCounts = {3, 4, 4, 4, 8, 0};
    KeyframeSlots chain;
    Tables() {
        for (int r : {0, 2, 6, 7, 9, 10}) flags[r] = 3;
        live[9] = live[11] = 0;
        for (int r = 0; r < kRows; ++r) track.push_back(kTrackBase + 7 * r);
        chain.id = {1, 2, 3, 5, 8, -1};
        chain.previous = {-1, 0, 1, 2, 3, -1};
        chain.next = {1, 2, 3, 4, -1, -1};
        chain.t = {0.1, 0.2, 0.3, 0.5, 0.8, 0.0};
        for (int k = 0; k < kSlots; ++k) {
            chain.cameraCenter.push_back({1.0 * k, 0.0, 0.0});
            chain.camera.push_back(ms_pinhole{500.0 + k, 501.0, 320.0, 240.0, 640, 480});
            chain.focalLength.push_back(500 + k);
            chain.descBase.push_back(k < 5 && k != 3 ? 8 * k + 1 : -1);      // slot 3 has no descriptors
            chain.frames.push_back(nullptr);
        }
    }
    // the reference's containers: the observations are the transpose of mapPoints over the occupied slots
    HostMap map() const {
        HostMap M;
        for (int r = 0; r < kRows; ++r) if (live[r]) { M.mapPoints[r].trackId = track[r]; M.trackIdToMapPoint[track[r]] = r; }
        for (int k = 0; k < kSlots; ++k) {
            if (chain.id[k] < 0) continue;
            HostKeyframe kf;
            kf.mapPoints = mapPoints[k];
            kf.previous = chain.previous[k] >= 0 ? chain.id[chain.previous[k]] : -1;
            kf.next = chain.next[k] >= 0 ? chain.id[chain.next[k]] : -1;
            M.keyframes.emplace(chain.id[k], kf);
            for (int j = 0; j < kStride; ++j) {
                const std::int32_t r = mapPoints[k][j];
                if (r >= 0 && M.mapPoints.count(r)) M.mapPoints[r].observations[chain.id[k]].push_back(j);
            }
        }
        return M;
    }
    std::set<std::int32_t> ids(const Rows &slots) const {
        std::set<std::int32_t> out;
        for (std::int32_t s : slots) out.insert(chain.id[s]);
        return out;
    }
};

#define EXPECT(cond, what) do { if (!(cond)) { std::printf("%s\n", what); return 2; } } while (0)

Rows keys(const std::map<std::int32_t, HostMapPoint> &m) { Rows out; for (const auto &p : m) out.push_back(p.first); return out; }
Rows sizes(const HostMap &M) {
    Rows out;
    for (const auto &p : M.mapPoints) { int n = 0; for (const auto &o : p.second.observations) n += (int)o.second.size(); out.push_back(n); }
    return out;
}

int check_restatement() {
    const Tables T;
    std::size_t dropped = 0;
    const HostMap C = partial_copy(T.map(), T.ids({2, 3, 4}), &dropped);
    EXPECT((keys(C.mapPoints) == Rows{0, 2, 4, 5, 6, 7, 8, 10} && dropped == 1), "restatement: the surviving map points differ from the hand-computed ones");
    EXPECT((sizes(C) == Rows{1, 3, 1, 2, 2, 2, 1, 1}), "restatement: the surviving observations differ");
    EXPECT((C.mapPoints.at(2).observations.count(1) == 0 && C.mapPoints.at(2).observations.size() == 3 && C.mapPoints.at(0).observations.begin()->first == 5), "restatement: the observations are not cut to the active keyframes");
    EXPECT((C.keyframes.at(3).previous == -1 && C.keyframes.at(3).next == 5 && C.keyframes.at(8).previous == 5 && C.keyframes.at(8).next == -1), "restatement: the links are not cut at the boundary");
    EXPECT((C.trackIdToMapPoint.size() == 8 && C.trackIdToMapPoint.count(kTrackBase + 7 * 3) == 0 && C.trackIdToMapPoint.at(kTrackBase + 70) == 10), "restatement: the filtered tracks differ");
    dropped = 0;
    const HostMap F = partial_copy(T.map(), T.ids({0, 1, 2, 3, 4}), &dropped);
    EXPECT((keys(F.mapPoints) == Rows{0, 1, 2, 3, 4, 5, 6, 7, 8, 10} && F.keyframes.at(2).previous == 1 && dropped == 1), "restatement: the full copy differs");
    return 0;
}

// ---- the mirror on the device ------------------------------------------------------------------------------------------------------------
std::vector<DeviceMapPoints::Vec3d> positions(int n) { std::vector<DeviceMapPoints::Vec3d> p; for (int r = 0; r < n; ++r) p.push_back({0.5 * r, 1.0 / (r + 1), -2.0 * r}); return p; }
std::vector<KeyPoint::Descriptor> descriptors(int n, std::uint32_t seed) {
    std::vector<KeyPoint::Descriptor> d(n);
    for (int r = 0; r < n; ++r) for (int w = 0; w < 8; ++w) d[r][w] = seed + 97u * r + w;
    return d;
}

struct Device {
    std::size_t slots, rows;
    DeviceKeyframeMapPoints table;
    DeviceMapPoints points;
    DeviceMapPointFlags flags;
    DeviceMapPointLive live;
    DeviceKeypointTable keypoints;
    DeviceKeyframePoses poses;
    DeviceTrackTable tracks;
    DeviceDescriptorPool pool;
    DeviceArray<std::int32_t> counts;
    KeyframeSlots chain;
    // the source: the hand-computed map
    Device(Context &ctx, const Tables &T)
        : slots(kSlots), rows(kRows), table(ctx, kSlots, kStride, kRows),
          points(ctx, positions(kRows), std::vector<DeviceMapPoints::Vec3f>(kRows, {1.f, 2.f, 3.f}), std::vector<float>(kRows, 0.5f), std::vector<float>(kRows, 9.f), descriptors(kRows, 1000)),
          flags(ctx, T.flags), live(ctx, T.live), keypoints(ctx, kSlots, kStride), poses(ctx, std::vector<DeviceKeyframePoses::Pose>(kSlots)), tracks(ctx, kRows, kTrackBase, kWindow),
          pool(ctx, descriptors(kSlots * kStride + 1, 5000)), counts(ctx, kRows), chain(T.chain) {
        std::vector<DeviceKeyframePoses::Pose> P(kSlots);
        for (int k = 0; k < kSlots; ++k) {
            table.update(k, T.mapPoints[k]);
            std::vector<float> x(kStride), depth(kStride);
            Rows octave(kStride);
            for (int j = 0; j < kStride; ++j) { x[j] = 100.f * k + j; depth[j] = 0.25f * j; octave[j] = (k + j) % 8; P[k][j] = 10.0 * k + j; }
            keypoints.update(k, x, depth, octave, depth);
        }
        poses.update(0, kSlots, P.data());
        Rows all(kRows);
        for (int r = 0; r < kRows; ++r) all[r] = r;
        tracks.bind(all, T.track);
    }
    // an empty destination
    Device(Context &ctx, std::size_t nSlots, std::size_t nRows, std::size_t poolSize)
        : slots(nSlots), rows(nRows), table(ctx, nSlots, kStride, nRows),
          points(ctx, std::vector<DeviceMapPoints::Vec3d>(nRows), std::vector<DeviceMapPoints::Vec3f>(nRows), std::vector<float>(nRows), std::vector<float>(nRows), std::vector<KeyPoint::Descriptor>(nRows)),
          flags(ctx, std::vector<std::uint8_t>(nRows, 7)), live(ctx, std::vector<std::uint8_t>(nRows, 7)), keypoints(ctx, nSlots, kStride),
          poses(ctx, std::vector<DeviceKeyframePoses::Pose>(nSlots)), tracks(ctx, nRows, kTrackBase, kWindow), pool(ctx, poolSize), counts(ctx, nRows) {
        chain.id.assign(nSlots, 77); chain.t.assign(nSlots, 7.0); chain.previous.assign(nSlots, 7); chain.next.assign(nSlots, 7); chain.cameraCenter.assign(nSlots, {7.0, 7.0, 7.0});
        chain.camera.assign(nSlots, ms_pinhole{}); chain.focalLength.assign(nSlots, 7); chain.descBase.assign(nSlots, 7); chain.frames.assign(nSlots, nullptr);
        counts.fill(-9);
    }
    MapTables view() {
        MapTables T{table, chain};
        T.points = &points; T.flags = &flags; T.live = &live; T.keypoints = &keypoints; T.poses = &poses; T.tracks = &tracks; T.pool = &pool; T.observationCount = counts.data();
        return T;
    }
};

// The destination against the restatement for `active` (source slots by ascending KfId): tables, row maps, counts, tracks, keypoints, poses, pool, records, links.
bool equals(Context &ctx, const Tables &T, Device &S, Device &D, const Rows &active, const MapExtract &got, std::size_t poolBase) {
    std::size_t dropped = 0;
    const HostMap C = partial_copy(T.map(), T.ids(active), &dropped);
    const Rows want = keys(C.mapPoints), obs = sizes(C);
    const std::size_t n = want.size(), nA = active.size();
    if (got.mapPoints != n || got.droppedObservations != dropped || got.tracks != C.trackIdToMapPoint.size()) return false;
    const Rows rowSrc = got.rowSource.download(), rowDst = got.rowDestination.download();
    if (Rows(rowSrc.begin(), rowSrc.begin() + n) != want) return false;
    for (int r = 0; r < kRows; ++r) {
        const auto at = std::find(want.begin(), want.end(), r);
        if (rowDst[r] != (at == want.end() ? -1 : (std::int32_t)(at - want.begin()))) return false;
    }
    const Rows kf = ctx.download(D.table.table(), D.slots * kStride), nObs = D.counts.download();
    const std::vector<std::uint8_t> flags = ctx.download(D.flags.flags(), D.rows), live = D.live.download();
    const std::vector<double> pos = ctx.download(D.points.position(), 3 * D.rows), srcPos = ctx.download(S.points.position(), 3 * (std::size_t)kRows);
    const std::vector<std::uint32_t> desc = ctx.download(D.points.descriptor(), 8 * D.rows), srcDesc = ctx.download(S.points.descriptor(), 8 * (std::size_t)kRows);
    const Rows mpTrack = D.tracks.downloadMapPointTracks(), trackRow = D.tracks.downloadTrackRows();
    std::size_t entries = 0;
    for (std::size_t d = 0; d < D.rows; ++d) {
        if (d >= n) { if (live[d] || flags[d] || mpTrack[d] != -1 || nObs[d] != 0) return false; continue; }
        const std::int32_t r = want[d];
        if (!live[d] || flags[d] != T.flags[r] || mpTrack[d] != T.track[r] || nObs[d] != obs[d]) return false;
        if (!std::equal(pos.begin() + 3 * d, pos.begin() + 3 * d + 3, srcPos.begin() + 3 * r) || !std::equal(desc.begin() + 8 * d, desc.begin() + 8 * d + 8, srcDesc.begin() + 8 * r)) return false;
        entries += (std::size_t)obs[d];
    }
    if (got.observations != entries) return false;
    for (std::size_t t = 0; t < (std::size_t)kWindow; ++t) {
        const auto at = C.trackIdToMapPoint.find(kTrackBase + (std::int32_t)t);
        if (trackRow[t] != (at == C.trackIdToMapPoint.end() ? -1 : rowDst[at->second])) return false;
    }
    const std::vector<float> x = ctx.download(D.keypoints.x(), D.slots * kStride), depth = ctx.download(D.keypoints.depth(), D.slots * kStride);
    const Rows octave = ctx.download(D.keypoints.octave(), D.slots * kStride);
    const std::vector<DeviceKeyframePoses::Pose> poses = D.poses.download();
    const std::vector<std::uint32_t> pool = ctx.download(D.pool.descriptor(), 8 * D.pool.size()), srcPool = ctx.download(S.pool.descriptor(), 8 * S.pool.size());
    std::size_t nextBase = poolBase;
    for (std::size_t i = 0; i < D.slots; ++i) {
        const bool copied = i < nA;
        const std::int32_t s = copied ? active[i] : 0;
        for (int j = 0; j < kStride; ++j) {
            const std::int32_t r = copied ? T.mapPoints[s][j] : -1;
            const std::int32_t e = r >= 0 && T.live[r] ? rowDst[r] : -1;
            if (kf[i * kStride + j] != e || x[i * kStride + j] != (copied ? 100.f * s + j : 0.f) || depth[i * kStride + j] != (copied ? 0.25f * j : 0.f) || octave[i * kStride + j] != (copied ? (s + j) % 8 : 0)) return false;
        }
        const KeyframeSlots &B = D.chain;
        if (!copied) { if (B.id[i] != -1 || B.previous[i] != -1 || B.next[i] != -1 || B.descBase[i] != -1) return false; continue; }
        for (int j = 0; j < 8; ++j) if (poses[i][j] != 10.0 * s + j) return false;
        const HostKeyframe &kfC = C.keyframes.at(T.chain.id[s]);
        auto slotOf = [&](std::int32_t id) { for (std::size_t a = 0; a < nA; ++a) if (T.chain.id[active[a]] == id) return (std::int32_t)a; return -1; };
        if (B.id[i] != T.chain.id[s] || B.t[i] != T.chain.t[s] || B.cameraCenter[i] != T.chain.cameraCenter[s] || B.camera[i].fx != T.chain.camera[s].fx || B.focalLength[i] != T.chain.focalLength[s]) return false;
        if (B.previous[i] != (kfC.previous < 0 ? -1 : slotOf(kfC.previous)) || B.next[i] != (kfC.next < 0 ? -1 : slotOf(kfC.next))) return false;      // cut and translated
        if (T.chain.descBase[s] < 0) { if (B.descBase[i] != -1) return false; continue; }
        if (B.descBase[i] != (std::int32_t)nextBase) return false;
        const std::size_t m = (std::size_t)T.keyPointCounts[s];
        if (!std::equal(pool.begin() + 8 * nextBase, pool.begin() + 8 * (nextBase + m), srcPool.begin() + 8 * (std::size_t)T.chain.descBase[s])) return false;
        nextBase += m;
    }
    return got.descriptors == nextBase - poolBase && D.pool.used() == nextBase;
}

int gpu() {
    Context ctx(0);
    const Tables T;
    Device S(ctx, T);
    {   // a list, by ascending KfId
        Device D(ctx, 4, 10, 32);
        const MapExtract got = extractMap(ctx, S.view(), {2, 3, 4}, D.view(), T.keyPointCounts);
        EXPECT((got.mapPoints == 8 && got.observations == 13 && got.droppedObservations == 1 && got.tracks == 8 && got.descriptors == 12), "extractMap: the counts differ from the hand-computed ones");
        EXPECT(equals(ctx, T, S, D, {2, 3, 4}, got, 0), "extractMap: the destination differs from the restatement");
        EXPECT((D.chain.previous == Rows{-1, 0, 1, -1} && D.chain.next == Rows{1, 2, -1, -1} && D.chain.descBase == Rows{0, -1, 4, -1}), "extractMap: the links or the descriptor bases differ");
        std::printf("extractMap ok: map points %zu, observations %zu, dropped %zu, tracks %zu, descriptors %zu\n", got.mapPoints, got.observations, got.droppedObservations, got.tracks, got.descriptors);
    }
    {   // copyMap, partial: the adjacent keyframes of the latest one
        Rows active = computeAdjacentKeyframes(ctx, S.view(), 4, 5, 2);
        active.push_back(4);
        std::sort(active.begin(), active.end(), [&](std::int32_t a, std::int32_t b) { return T.chain.id[a] < T.chain.id[b]; });
        Device D(ctx, 5, 12, 40);
        D.pool.reserve(3);                                   // the destination's pool is in use already
        const MapExtract got = copyMapToFrontend(ctx, S.view(), 4, 2, true, D.view(), T.keyPointCounts);
        EXPECT(active.size() >= 2 && active.size() < 5 && equals(ctx, T, S, D, active, got, 3), "copyMapToFrontend (partial): the destination differs from the restatement");
        std::printf("copyMapToFrontend partial ok: %zu keyframes, map points %zu\n", active.size(), got.mapPoints);
    }
    {   // copyMap, full: every occupied slot, also without a latest keyframe
        for (int pass = 0; pass < 2; ++pass) {
            Device D(ctx, 6, 12, 40);
            const MapExtract got = copyMapToFrontend(ctx, S.view(), pass ? -1 : 4, 2, pass != 0, D.view(), T.keyPointCounts);
            EXPECT(got.mapPoints == 10 && equals(ctx, T, S, D, {0, 1, 2, 3, 4}, got, 0), "copyMapToFrontend (full): the destination differs from the restatement");
            EXPECT((D.chain.previous == Rows{-1, 0, 1, 2, 3, -1} && D.chain.next == Rows{1, 2, 3, 4, -1, -1}), "copyMapToFrontend (full): the chain differs");
        }
        std::printf("copyMapToFrontend full ok: map points 10\n");
    }
    {   // the refusals, before any device call
        Device D(ctx, 2, 10, 32), wide(ctx, 4, 10, 32);
        DeviceKeyframeMapPoints other(ctx, 4, kStride + 1, 10);
        int thrown = 0;
        auto refused = [&](MapTables src, const Rows &active, MapTables dst, const char *text) {
            try { extractMap(ctx, src, active, dst, T.keyPointCounts); } catch (const std::invalid_argument &e) { thrown += std::strstr(e.what(), text) != nullptr; }
        };
        refused(S.view(), {2, 6}, wide.view(), "extractMap: active slot 6 outside the table");
        refused(S.view(), {2, 5}, wide.view(), "extractMap: active slot 5 is empty");
        refused(S.view(), {2, 3, 4}, D.view(), "extractMap: 3 active keyframes for a destination of 2 slots");
        { MapTables V = wide.view(); MapTables W{other, wide.chain}; W.points = V.points; W.flags = V.flags; W.live = V.live; W.pool = V.pool; W.tracks = V.tracks; W.poses = V.poses;
          refused(S.view(), {2, 3}, W, "is not the source's 8"); }
        { MapTables V = wide.view(); V.keypoints = nullptr; refused(S.view(), {2, 3}, V, "a keypoint table on one side only"); }
        { MapTables V = wide.view(); V.pool = nullptr; refused(S.view(), {2, 3}, V, "a descriptor pool on one side only"); }
        { MapTables V = S.view(); V.tracks = nullptr; refused(V, {2, 3}, wide.view(), "a track table on one side only"); }
        { MapTables V = S.view(); V.poses = nullptr; refused(V, {2, 3}, wide.view(), "poses on one side only"); }
        EXPECT(thrown == 8, "a refusal did not throw std::invalid_argument with its message");
        const Rows kf = ctx.download(wide.table.table(), wide.slots * kStride);
        EXPECT(std::all_of(kf.begin(), kf.end(), [](std::int32_t e) { return e == -1; }) && wide.chain.id == Rows(4, 77) && wide.pool.used() == 0 && wide.live.download() == std::vector<std::uint8_t>(10, 7),
               "a refused call changed the destination");
        std::printf("invalid_argument ok 8 cases\n");
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_map_extract, (const void *)&ms_map_extract_validate};
    std::printf("link ok %d\n", syms[0] != nullptr && syms[1] != nullptr);
    if (const int rc = check_restatement()) return rc;
    std::printf("restatement ok\n");
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu();
    return 0;
}
