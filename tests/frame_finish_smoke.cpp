// Compile + link check of the end-of-frame step of the host mirror (finishFrame, removeKeyframes in mi355slam/map_update.hpp) against
// libmi355slam.so, and its comparison with a sequential std::map / std::set restatement of setPointCloudOutput (mapper_helpers.cpp:484-497)
// and removeKeyframe (:375-431) on a hand-computed map (tests/test_frame_finish_smoke.py).
//   frame_finish_smoke --no-gpu   the restatement against the hand-computed results (no context, no device)
//   frame_finish_smoke --gpu      finishFrame with keyframeDecision = true (every table as it was) and false, removeKeyframes for a list, the
//                                 relinked chain, and the two std::invalid_argument cases, which leave the tables alone
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

constexpr int kStride = 8, kRows = 12, kFrame = 4, kFrameKeyPoints = 7;

// ---- the reference's map and loops, sequentially ---------------------------------------------------------------------------------------
struct CloudPoint {
    std::int32_t row, keyPoint, track;
    std::array<double, 3> position;
    bool operator==(const CloudPoint &o) const { return row == o.row && keyPoint == o.keyPoint && track == o.track && position == o.position; }
};
struct HostMap {
    std::vector<std::vector<std::int32_t>> mapPoints;        // Keyframe::mapPoints per slot (-1 = none)
    std::vector<std::map<std::int32_t, int>> observations;   // MapPoint::observations per row: KfId -> entries of that keyframe
    std::vector<std::uint8_t> flags, live;
    std::vector<std::int32_t> track;
    std::vector<std::array<double, 3>> position;
    KeyframeSlots chain;
    std::vector<std::int32_t> removedRows;                   // in the order of removal
    std::size_t erased = 0;
    void link() {
        observations.assign(flags.size(), {});
        for (std::size_t k = 0; k < mapPoints.size(); ++k)
            if (chain.id[k] >= 0)
                for (std::int32_t r : mapPoints[k]) if (r != -1) ++observations[r][chain.id[k]];
    }
    std::int32_t size(std::int32_t r) const {
        int n = 0;
        for (const auto &o : observations[r]) n += o.second;
        return n;
    }
};

// setPointCloudOutput, :484-497
std::vector<CloudPoint> point_cloud(const HostMap &M, std::int32_t k, std::size_t nKeyPoints) {
    std::vector<CloudPoint> out;
    for (std::size_t j = 0; j < nKeyPoints; ++j) {
        const std::int32_t r = M.mapPoints[k][j];
        if (r == -1 || !M.live[r]) continue;
        if (M.flags[r] & DeviceMapPointFlags::TRIANGULATED) out.push_back({r, (std::int32_t)j, M.track[r], M.position[r]});
    }
    return out;
}

// removeKeyframe, :375-431 (what it does to the tables and the links)
void remove_keyframe(HostMap &M, std::int32_t k) {
    std::set<std::int32_t> mapPointsToErase;
    const std::int32_t prev = M.chain.previous[k], next = M.chain.next[k], id = M.chain.id[k];
    for (std::int32_t r : M.mapPoints[k]) {
        if (r == -1) continue;
        ++M.erased;
        auto &obs = M.observations[r];
        if (--obs[id] == 0) obs.erase(id);
        if (obs.empty() && M.live[r]) mapPointsToErase.insert(r);
    }
    for (std::int32_t r : mapPointsToErase) { M.live[r] = 0; M.flags[r] = 0; M.removedRows.push_back(r); }      // MapDB::removeMapPoint
    if (next != -1) M.chain.previous[next] = prev;
    if (prev != -1) M.chain.next[prev] = next;
    M.mapPoints[k].assign(M.mapPoints[k].size(), -1);
    M.chain.previous[k] = M.chain.next[k] = -1;
    M.chain.id[k] = -1;
}

// Five keyframes in a chain (slots 0 - 4 in KfId order) and an empty slot; slot 4 is the frame, with 7 keypoints and one more entry behind them.
//   row 2: seen by everybody        row 6: slots 3 and 4          row 7: twice in slot 4 alone, TRIANGULATED      row 8: slot 4 alone, not TRIANGULATED
//   row 9: slot 4 alone, not live   row 10: slot 4 alone, behind the keypoints     row 5: twice in slot 2 alone   row 4: slots 1 and 2    row 3: slot 1 alone
HostMap hand_map() {
    HostMap M;
    M.mapPoints = {{0, 1, 2, -1, -1, -1, -1, -1}, {1, 2, 3, 4, -1, -1, -1, -1}, {2, 4, 5, 5, -1, -1, -1, -1}, {0, 6, -1, 2, -1, -1, -1, -1},
                   {2, 6, 7, 8, -1, 9, 7, 10}, {-1, -1, -1, -1, -1, -1, -1, -1}};
    M.flags.assign(kRows, 2);
    for (int r : {0, 2, 6, 7, 9, 10}) M.flags[r] = 3;
    M.live.assign(kRows, 1);
    M.live[9] = M.live[11] = 0;
    for (int r = 0; r < kRows; ++r) { M.track.push_back(100 + 7 * r); M.position.push_back({0.5 * r, 1.0 / (r + 1), -2.0 * r}); }
    M.chain.id = {1, 2, 3, 5, 8, -1};
    M.chain.previous = {-1, 0, 1, 2, 3, -1};
    M.chain.next = {1, 2, 3, 4, -1, -1};
    M.link();
    return M;
}

#define EXPECT(cond, what) do { if (!(cond)) { std::printf("%s\n", what); return 2; } } while (0)

using Rows = std::vector<std::int32_t>;

int check_restatement() {
    HostMap M = hand_map();
    const std::vector<CloudPoint> cloud = point_cloud(M, kFrame, kFrameKeyPoints);
    Rows rows, kps;
    for (const CloudPoint &p : cloud) { rows.push_back(p.row); kps.push_back(p.keyPoint); }
    EXPECT((rows == Rows{2, 6, 7, 7} && kps == Rows{0, 1, 2, 6}), "restatement: the cloud differs from the hand-computed one");
    remove_keyframe(M, kFrame);
    EXPECT((M.removedRows == Rows{7, 8, 10} && M.erased == 7 && M.live[9] == 0 && M.size(2) == 4 && M.size(6) == 1), "restatement: removing the frame differs");
    EXPECT((M.chain.next[3] == -1 && M.chain.id[kFrame] == -1), "restatement: the chain after the frame differs");
    M = hand_map();
    remove_keyframe(M, 2); remove_keyframe(M, 1);
    EXPECT((M.removedRows == Rows{5, 3, 4} && M.erased == 8 && M.size(1) == 1 && M.size(2) == 3), "restatement: removing slots 2 and 1 differs");
    EXPECT((M.chain.next[0] == 3 && M.chain.previous[3] == 0), "restatement: the chain after slots 2 and 1 differs");
    return 0;
}

// ---- the mirror on the device ------------------------------------------------------------------------------------------------------------
struct Device {
    DeviceKeyframeMapPoints table;
    DeviceMapPoints points;
    DeviceMapPointFlags flags;
    DeviceMapPointLive live;
    DeviceTrackTable tracks;
    DeviceArray<std::int32_t> counts;
    KeyframeSlots chain;
    Device(Context &ctx, const HostMap &M)
        : table(ctx, M.mapPoints.size(), kStride, kRows),
          points(ctx, M.position, std::vector<DeviceMapPoints::Vec3f>(kRows), std::vector<float>(kRows), std::vector<float>(kRows), std::vector<KeyPoint::Descriptor>(kRows)),
          flags(ctx, M.flags), live(ctx, M.live), tracks(ctx, kRows, 100, 128), counts(ctx, kRows), chain(M.chain) {
        for (std::size_t k = 0; k < M.mapPoints.size(); ++k) table.update(k, M.mapPoints[k]);
        Rows rows(kRows);
        for (int r = 0; r < kRows; ++r) rows[r] = r;
        tracks.bind(rows, M.track);
        counts.fill(-9);                                     // stale: the call never reads it
    }
    MapTables view() {
        MapTables T{table, chain};
        T.points = &points; T.flags = &flags; T.live = &live; T.tracks = &tracks; T.observationCount = counts.data();
        return T;
    }
    // the tables equal the restatement's; the counts only where a removed keyframe listed the row
    bool equals(Context &ctx, const HostMap &M, const Rows &listed) {
        const Rows kf = ctx.download(table.table(), M.mapPoints.size() * kStride);
        for (std::size_t k = 0; k < M.mapPoints.size(); ++k)
            if (!std::equal(M.mapPoints[k].begin(), M.mapPoints[k].end(), kf.begin() + k * kStride)) return false;
        if (ctx.download(flags.flags(), (std::size_t)kRows) != M.flags || live.download() != M.live) return false;
        const Rows n = counts.download();
        for (int r = 0; r < kRows; ++r) {
            const bool was = std::find(listed.begin(), listed.end(), r) != listed.end();
            if (n[r] != (was ? M.size(r) : -9)) return false;
        }
        return chain.previous == M.chain.previous && chain.next == M.chain.next && chain.id == M.chain.id;
    }
};

bool same_cloud(const FrameFinish &got, const std::vector<CloudPoint> &want) {
    if (got.cloudRows.size() != want.size() || got.cloudKeyPoints.size() != want.size() || got.cloudTracks.size() != want.size() || got.cloudPositions.size() != 3 * want.size()) return false;
    for (std::size_t i = 0; i < want.size(); ++i) {
        const CloudPoint p{got.cloudRows[i], got.cloudKeyPoints[i], got.cloudTracks[i], {got.cloudPositions[3 * i], got.cloudPositions[3 * i + 1], got.cloudPositions[3 * i + 2]}};
        if (!(p == want[i])) return false;
    }
    return true;
}

int gpu() {
    Context ctx(0);
    {   // a frame that becomes a keyframe: the cloud, and every table as it was
        HostMap M = hand_map();
        Device D(ctx, M);
        const FrameFinish got = finishFrame(ctx, D.view(), kFrame, kFrameKeyPoints, true, {});
        EXPECT(same_cloud(got, point_cloud(M, kFrame, kFrameKeyPoints)) && got.cloudRows.size() == 4, "finishFrame (keyframe): the cloud differs");
        EXPECT(got.removedRows.empty() && got.removedPrevious.empty() && got.erasedObservations == 0 && D.equals(ctx, M, {}), "finishFrame (keyframe): a table changed");
        std::printf("keyframeDecision = true leaves every table as it was\n");
    }
    {   // a frame that does not: the cloud of the tables before the removal, then removeKeyframe
        HostMap M = hand_map();
        Device D(ctx, M);
        const std::vector<CloudPoint> cloud = point_cloud(M, kFrame, kFrameKeyPoints);
        const FrameFinish got = finishFrame(ctx, D.view(), kFrame, kFrameKeyPoints, false, {1});
        remove_keyframe(M, kFrame);
        EXPECT(same_cloud(got, cloud), "finishFrame: the cloud differs");
        EXPECT((got.removedRows == M.removedRows && got.removedRows == Rows{7, 8, 10} && got.erasedObservations == M.erased), "finishFrame: the removed rows differ");
        EXPECT((got.removedPrevious == Rows{3} && got.removedNext == Rows{-1}), "finishFrame: the removed keyframe's links differ");
        EXPECT(D.equals(ctx, M, {2, 6, 7, 8, 9, 10}), "finishFrame: the tables or the relinked chain differ");
        std::printf("finishFrame ok: cloud %zu, removed rows %zu, erased observations %zu\n", got.cloudRows.size(), got.removedRows.size(), got.erasedObservations);
    }
    {   // keyframes that dropped out of the pose trail, as a list
        HostMap M = hand_map();
        Device D(ctx, M);
        const FrameFinish got = removeKeyframes(ctx, D.view(), {2, 1}, {4});
        remove_keyframe(M, 2); remove_keyframe(M, 1);
        Rows have = got.removedRows, want = M.removedRows;
        std::sort(have.begin(), have.end()); std::sort(want.begin(), want.end());
        EXPECT((have == want && got.removedRows == Rows{4, 5, 3} && got.erasedObservations == M.erased && got.cloudRows.empty()), "removeKeyframes: the removed rows differ");
        EXPECT((got.removedPrevious == Rows{1, 0} && got.removedNext == Rows{3, 3}), "removeKeyframes: the removed keyframes' links differ");
        EXPECT(D.equals(ctx, M, {1, 2, 3, 4, 5}), "removeKeyframes: the tables or the relinked chain differ");
        std::printf("removeKeyframes ok: removed rows %zu; relinked chain ok\n", got.removedRows.size());
    }
    {   // the two refusals of removeKeyframe, before any device call
        HostMap M = hand_map();
        Device D(ctx, M);
        int thrown = 0;
        try { finishFrame(ctx, D.view(), 0, 3, false, {}); } catch (const std::invalid_argument &e) { thrown += std::strstr(e.what(), "finishFrame: slot 0 has no previous keyframe") != nullptr; }
        try { finishFrame(ctx, D.view(), kFrame, kFrameKeyPoints, false, {2, kFrame}); } catch (const std::invalid_argument &e) { thrown += std::strstr(e.what(), "loop-closure edge") != nullptr; }
        try { removeKeyframes(ctx, D.view(), {2, 0}, {}); } catch (const std::invalid_argument &e) { thrown += std::strstr(e.what(), "removeKeyframes: slot 0 has no previous keyframe") != nullptr; }
        try { removeKeyframes(ctx, D.view(), {2, 3}, {3}); } catch (const std::invalid_argument &e) { thrown += std::strstr(e.what(), "removeKeyframes: slot 3 is named by a loop-closure edge") != nullptr; }
        EXPECT(thrown == 4, "a refusal did not throw std::invalid_argument with its message");
        EXPECT(D.equals(ctx, M, {}), "a refused call changed a table");
        EXPECT(finishFrame(ctx, D.view(), 0, 3, true, {}).cloudRows == (Rows{0, 2}), "the first keyframe's cloud differs");      // as a keyframe it is fine
        std::printf("invalid_argument ok 4 cases\n");
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_frame_finish, (const void *)&ms_frame_finish_validate};
    std::printf("link ok %d\n", syms[0] != nullptr && syms[1] != nullptr);
    if (const int rc = check_restatement()) return rc;
    std::printf("restatement ok\n");
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu();
    return 0;
}
