// Compile + link check of the tracker-frame arrival step of the host mirror (admitTrackerFrame and makeKeyframeDecision in
// mi355slam/map_update.hpp) against libmi355slam.so, makeKeyframeDecision against a literal std::set restatement of
// mapper_helpers.cpp:28-65 on hand-computed cases, and admitTrackerFrame on a hand-computed frame (tests/test_frame_admit_smoke.py).
//   frame_admit_smoke --no-gpu   the decision against its restatement and the hand-computed answers (no context, no device)
//   frame_admit_smoke --gpu      two frames admitted into a chain: the tables, the slot record and the links; the refusals, which leave everything
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

int fails = 0;
void expect(bool ok, const char *what) { if (!ok) { std::printf("FAILED: %s\n", what); ++fails; } }

// ---- mapper_helpers.cpp:28-65, statement by statement -------------------------------------------------------------------------------------
struct Kf {
    double t;
    std::array<double, 3> center;
    std::vector<std::int32_t> keyPointToTrackId;             // the values of the map
};
bool restated(const Kf &current, const Kf *previous, const std::vector<std::int32_t> &currentTracks, const KeyframeDecisionParameters &parameters) {
    if (!previous) return true;
    double age = current.t - previous->t;
    if (age < parameters.keyframeDecisionMinIntervalSeconds) return false;
    const double dx = current.center[0] - previous->center[0], dy = current.center[1] - previous->center[1], dz = current.center[2] - previous->center[2];
    const double distance = std::sqrt(dx * dx + dy * dy + dz * dz);
    if (distance > parameters.keyframeDecisionDistanceThreshold) return true;
    int prevCovisiblities = 0;
    unsigned nTracks = 0;
    std::set<std::int32_t> prevTrackIds;
    for (std::int32_t id : previous->keyPointToTrackId) prevTrackIds.insert(id);
    for (std::int32_t id : currentTracks) {
        nTracks++;
        if (prevTrackIds.count(id)) prevCovisiblities++;
    }
    const float maxCovis = static_cast<float>(nTracks) * parameters.keyframeDecisionCovisibilityRatio;
    if (prevCovisiblities <= maxCovis) return true;
    return false;
}

// both forms, and they agree
bool decide(const Kf &current, const Kf *previous, const std::vector<std::int32_t> &tracks, const KeyframeDecisionParameters &p, const char *what) {
    static const Kf none{0.0, {0.0, 0.0, 0.0}, {}};
    const Kf &prev = previous ? *previous : none;
    const bool a = makeKeyframeDecision(previous != nullptr, current.t, prev.t, current.center, prev.center, prev.keyPointToTrackId, tracks, p);
    expect(a == restated(current, previous, tracks, p), what);
    return a;
}

int no_gpu() {
    std::printf("link ok %d\n", ms_version() != nullptr);
    KeyframeDecisionParameters p;
    p.keyframeDecisionMinIntervalSeconds = 0.5; p.keyframeDecisionDistanceThreshold = 2.0; p.keyframeDecisionCovisibilityRatio = 0.75f;
    const Kf prev{10.0, {1.0, 2.0, 3.0}, {5, 9, 7, 3, 9, 11}};                          // an id twice: a set holds it once
    const std::vector<std::int32_t> eight = {3, 5, 7, 9, 11, 100, 101, 102};           // 5 of 8 seen before; maxCovis = 6
    Kf cur{11.0, {1.0, 2.0, 4.0}, {}};
    expect(decide(cur, nullptr, eight, p, "no previous keyframe") == true, "no previous keyframe: a keyframe");
    cur.t = 10.25;
    expect(decide(cur, &prev, eight, p, "age gate") == false, "younger than the interval: no keyframe, whatever else holds");
    cur.t = 10.5;                                            // age == the interval: the gate is <
    expect(decide(cur, &prev, eight, p, "age at the interval") == true, "age == interval passes the gate; 5 <= 6: a keyframe");
    cur.t = 11.0; cur.center = {1.0, 2.0, 5.5};              // 2.5 away
    const std::vector<std::int32_t> all = {3, 5, 7, 9, 11};  // all seen before: the ratio alone would say no
    expect(decide(cur, &prev, all, p, "distance gate") == true, "farther than the threshold: a keyframe");
    cur.center = {1.0, 2.0, 5.0};                            // exactly 2.0: the gate is >
    expect(decide(cur, &prev, all, p, "distance at the threshold") == false, "distance == threshold falls through to the ratio; 5 > 3.75: no keyframe");
    const std::vector<std::int32_t> four = {3, 5, 7, 200};   // 3 of 4 seen; maxCovis = 4 * 0.75f = 3: equality
    expect(decide(cur, &prev, four, p, "ratio at equality") == true, "prevCovisibilities == maxCovis: <= says a keyframe");
    const std::vector<std::int32_t> four_seen = {3, 5, 7, 9};
    expect(decide(cur, &prev, four_seen, p, "ratio above") == false, "4 > 3: no keyframe");
    expect(decide(cur, &prev, {}, p, "no tracks") == true, "no tracks: 0 <= 0");
    // 10 * 0.7f is 6.99999988 as a double product and rounds to exactly 7 as a float product: with 7 of 10 seen the float product decides
    p.keyframeDecisionCovisibilityRatio = 0.7f;
    const Kf seven{10.0, {1.0, 2.0, 3.0}, {1, 2, 3, 4, 5, 6, 7}};
    const std::vector<std::int32_t> ten = {1, 2, 3, 4, 5, 6, 7, 300, 301, 302};
    expect(decide(cur, &seven, ten, p, "float product") == true, "7 <= 10 * 0.7f in float");
    expect(!(7.0 <= 10.0 * (double)0.7f), "the same product in double would have said no");
    std::printf(fails ? "decision FAILED\n" : "decision ok\n");
    return fails ? 1 : 0;
}

// ---- the device side ----------------------------------------------------------------------------------------------------------------------
constexpr int kStride = 6, kSlots = 4, kWidth = 6, kHeight = 4;

int gpu() {
    Context ctx(0);
    std::vector<float> img(kWidth * kHeight);
    for (int i = 0; i < kWidth * kHeight; ++i) img[i] = 100.0f + (float)i;
    std::vector<std::uint8_t> mask(kWidth * kHeight, 1);
    mask[1 * kWidth + 4] = 0;
    DeviceArray<float> dImg(ctx, img.size());
    dImg.upload(0, img.size(), img.data());
    DeviceArray<std::uint8_t> dMask(ctx, mask.size());
    dMask.upload(0, mask.size(), mask.data());

    DeviceKeyframeMapPoints keyframes(ctx, kSlots, kStride, 20);
    DeviceKeypointTable keypoints(ctx, kSlots, kStride);
    DeviceKeyframePoses poses(ctx, std::vector<DeviceKeyframePoses::Pose>(kSlots, DeviceKeyframePoses::Pose{}));
    DeviceKeyframe stale(ctx, 4);
    KeyframeSlots slots;
    slots.id.assign(kSlots, -1); slots.t.assign(kSlots, 0.0); slots.previous.assign(kSlots, -1); slots.next.assign(kSlots, -1);
    slots.cameraCenter.assign(kSlots, {}); slots.camera.assign(kSlots, ms_pinhole{}); slots.focalLength.assign(kSlots, 0); slots.descBase.assign(kSlots, 7);
    slots.frames = {nullptr, &stale, nullptr, nullptr};      // what an earlier keyframe in slot 1 left behind
    MapTables M{keyframes, slots};
    M.keypoints = &keypoints; M.poses = &poses;
    keyframes.update(1, {-1, 3});                            // an entry nobody erased: the slot is NOT empty

    // six features: 0 kept with its depth; 1 dropped by isValidPixel; 2 kept, no depth -> the image at (round(2.5) = 2, 1) = 108; 3 dropped by the mask
    // at (4, 1); 4 at column round(5.5) = 6, outside the mask's raster: dropped by the mask; 5 kept, depth -2 -> the image at (3, 3) = 121
    TrackerFrameAdmission a;
    a.id = 40; a.t = 1.25; a.camera = ms_pinhole{2.0, 4.0, 1.0, 2.0, kWidth, kHeight}; a.focalLength = 3;
    a.poseCW = {0, -1, 0, 1.0, 1, 0, 0, 2.0, 0, 0, 1, 3.0};   // R = a quarter turn about z, t = (1, 2, 3): the centre is -R^T t = (-2, 1, -3)
    a.x = {1.0f, 0.0f, 2.5f, 4.0f, 5.5f, 3.0f}; a.y = {2.0f, 0.0f, 1.0f, 1.0f, 1.0f, 3.0f}; a.depth = {9.0f, 1.0f, -1.0f, 2.0f, -1.0f, -2.0f};
    a.trackIds = {11, 12, 13, 14, 15, 16}; a.validPixel = {1, 0, 1, 1, 1, 1};
    a.depthImage = dImg.data(); a.depthWidth = kWidth; a.depthHeight = kHeight; a.depthStride = kWidth;
    a.validMask = dMask.data(); a.maskWidth = kWidth; a.maskHeight = kHeight; a.maskStride = kWidth;

    // ---- the refusals: a bound entry in the row (the device's verdict), an occupied slot, the slot as its own predecessor, an empty predecessor, a
    // length that does not match, a duplicate id (the validation's verdict)
    int refused = 0;
    try { admitTrackerFrame(ctx, M, 1, -1, a); } catch (const std::runtime_error &e) { refused += std::strstr(e.what(), "is not empty") != nullptr; }
    expect(slots.id[1] == -1 && slots.descBase[1] == 7 && slots.frames[1] == &stale, "a refused call leaves the record");
    expect(ctx.download(keyframes.table() + kStride, 3) == std::vector<std::int32_t>({-1, 3, -1}), "a refused call leaves the row");
    expect(ctx.download(keypoints.x() + kStride, 3) == std::vector<float>(3, 0.0f), "a refused call leaves the keypoints");
    keyframes.clear(1);
    slots.id[2] = 7;
    try { admitTrackerFrame(ctx, M, 2, -1, a); } catch (const std::invalid_argument &) { ++refused; }
    slots.id[2] = -1;
    try { admitTrackerFrame(ctx, M, 1, 1, a); } catch (const std::invalid_argument &) { ++refused; }
    try { admitTrackerFrame(ctx, M, 1, 3, a); } catch (const std::invalid_argument &) { ++refused; }
    { TrackerFrameAdmission b = a; b.depth.pop_back(); try { admitTrackerFrame(ctx, M, 1, -1, b); } catch (const std::invalid_argument &) { ++refused; } }
    { TrackerFrameAdmission b = a; b.trackIds[5] = 11; try { admitTrackerFrame(ctx, M, 1, -1, b); } catch (const std::runtime_error &e) { refused += std::strstr(e.what(), "listed twice") != nullptr; } }
    expect(slots.id[1] == -1 && slots.next[1] == -1, "refusals leave the chain");
    std::printf("refusals ok %d cases\n", refused);
    expect(refused == 6, "six refusals");

    // ---- frame 40 into slot 1
    const AdmittedTrackerFrame r0 = admitTrackerFrame(ctx, M, 1, -1, a);
    expect(r0.keyPoints == 3 && r0.droppedByValidPixel == 1 && r0.droppedByMask == 2 && r0.depthsFromImage == 2, "counts");
    expect(r0.keyPointTrackIds == std::vector<std::int32_t>({11, 13, 16}) && r0.keyPointFeature == std::vector<std::int32_t>({0, 2, 5}), "keyPointTrackIds, keyPointFeature");
    expect(ctx.download(keypoints.x() + kStride, 4) == std::vector<float>({1.0f, 2.5f, 3.0f, 0.0f}) && ctx.download(keypoints.y() + kStride, 3) == std::vector<float>({2.0f, 1.0f, 3.0f}),
           "positions; the entry behind n_kp keeps its bytes");
    expect(ctx.download(keypoints.depth() + kStride, 3) == std::vector<float>({9.0f, 108.0f, 121.0f}) && ctx.download(keypoints.octave() + kStride, 3) == std::vector<std::int32_t>(3, 0),
           "depths (the tracker's, the image's twice) and octave 0");
    expect(ctx.download(keyframes.table() + kStride, kStride) == std::vector<std::int32_t>(kStride, -1), "the row is cleared");
    expect(poses.download()[1] == a.poseCW && poses.download()[0] == DeviceKeyframePoses::Pose{}, "pose; the neighbour's stays");
    expect(slots.id[1] == 40 && slots.t[1] == 1.25 && slots.previous[1] == -1 && slots.next[1] == -1 && slots.descBase[1] == -1 && slots.frames[1] == nullptr, "record");
    expect(slots.cameraCenter[1] == std::array<double, 3>({-2.0, 1.0, -3.0}) && slots.focalLength[1] == 3 && slots.camera[1].fy == 4.0, "camera centre, camera");
    std::printf("admitTrackerFrame ok: %zu keypoints of %zu features\n", r0.keyPoints, a.x.size());

    // ---- frame 41 into slot 3, behind 40; no validPixel, no mask, no image; then no features at all into slot 0 behind it
    TrackerFrameAdmission b = a;
    b.id = 41; b.validPixel.clear(); b.validMask = nullptr; b.depthImage = nullptr;
    const AdmittedTrackerFrame r1 = admitTrackerFrame(ctx, M, 3, 1, b);
    expect(r1.keyPoints == 6 && r1.keyPointTrackIds == b.trackIds && r1.depthsFromImage == 0, "the second frame keeps every feature");
    expect(ctx.download(keypoints.depth() + 3 * kStride, 6) == std::vector<float>({9.0f, 1.0f, -1.0f, 2.0f, -1.0f, -1.0f}), "no image: a negative depth is -1");
    expect(slots.previous[3] == 1 && slots.next[1] == 3 && slots.next[3] == -1, "chain");
    TrackerFrameAdmission none;
    none.id = 42; none.poseCW = a.poseCW;
    const AdmittedTrackerFrame r2 = admitTrackerFrame(ctx, M, 0, 3, none);
    expect(r2.keyPoints == 0 && r2.keyPointTrackIds.empty() && slots.next[3] == 0 && poses.download()[0] == a.poseCW, "a frame without features");
    std::printf("chain ok: 40 -> 41 -> 42\n");

    // ---- one feature too many for the row
    TrackerFrameAdmission big = b;
    big.id = 43;
    big.x.push_back(1.0f); big.y.push_back(1.0f); big.depth.push_back(1.0f); big.trackIds.push_back(17);
    int full = 0;
    try { admitTrackerFrame(ctx, M, 2, 0, big); } catch (const std::runtime_error &e) { full += std::strstr(e.what(), "7 keypoints") != nullptr; }
    expect(full == 1 && slots.id[2] == -1 && slots.next[0] == -1, "a full row is the call's capacity verdict and leaves everything");
    std::printf(fails ? "mirror FAILED\n" : "mirror ok\n");
    return fails ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--no-gpu")) return no_gpu();
    if (argc == 2 && !std::strcmp(argv[1], "--gpu")) return gpu();
    std::printf("usage: frame_admit_smoke --no-gpu | --gpu\n");
    return 2;
}
