// Compile + link check of the keyframe-arrival step of the host mirror (admitKeyframe in mi355slam/map_update.hpp, DeviceKeyframe(ctx, capacity),
// DeviceDescriptorPool(ctx, capacity), BowIndex::assembleVector) against libmi355slam.so, and its comparison with a sequential std::map /
// std::stable_sort restatement of Keyframe::addFullFeatures / processKeyPoints (keyframe.cpp:34-116) and BowIndex::assemble on a hand-computed
// frame (tests/test_keyframe_admit_smoke.py).
//   keyframe_admit_smoke --no-gpu   the restatement against the hand-computed results (no context, no device)
//   keyframe_admit_smoke --gpu      two keyframes admitted from a two-frame device view: the tables, the DeviceKeyframe, the slot record, the chain and
//                                   the pool against the restatement; the refusals, which leave everything as it was
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

constexpr int kCapacity = 8, kStride = 7, kSlots = 3, kWidth = 6, kHeight = 4;

struct HostFrame {                           // what the extractor leaves for one frame
    std::vector<float> x, y, angle;
    std::vector<std::int32_t> octave, trackId;
    std::vector<KeyPoint::Descriptor> desc;
    std::size_t size() const { return x.size(); }
};
struct Tracker {                             // mapperInput.trackerFeatures
    std::vector<std::int32_t> id;
    std::vector<float> depth;
};
struct Expected {
    std::vector<float> depth, sortedX, sortedY;
    std::vector<std::int32_t> sortedIndex, nodeId, nodeStart, kpIdx;
    std::vector<std::array<double, 3>> bearing;
    BowVector bowVector;
};

// the two leaves of the vocabulary: all zeros (word 0, weight 2) and all ones (word 1, a stop word)
KeyPoint::Descriptor descriptor(bool ones) {
    KeyPoint::Descriptor d;
    d.fill(ones ? 0xffffffffu : 0u);
    return d;
}

// Frame 0: five keypoints; y has two pairs of equal values; keypoints 0 - 2 are tracked, track 11 is listed twice (the last entry counts), track 12
// has a negative depth (the image decides), keypoint 3 rounds to column 6 (outside), keypoint 4 has no track.
HostFrame frame0() {
    HostFrame f;
    f.x = {1.0f, 2.5f, 4.0f, 5.5f, 0.0f}; f.y = {2.0f, 1.0f, 2.0f, 1.0f, 3.0f}; f.angle = {10.f, 20.f, 30.f, 40.f, 50.f};
    f.octave = {0, 1, 2, 3, 0}; f.trackId = {11, 12, 13, -1, -1};
    f.desc = {descriptor(false), descriptor(true), descriptor(false), descriptor(false), descriptor(true)};
    return f;
}
HostFrame frame1() {
    HostFrame f;
    f.x = {3.0f, 0.5f}; f.y = {0.0f, 0.0f}; f.angle = {1.f, 2.f}; f.octave = {1, 0}; f.trackId = {-1, -1};
    f.desc = {descriptor(true), descriptor(false)};
    return f;
}
Tracker tracker() { return Tracker{{11, 13, 12, 11}, {9.0f, 0.25f, -1.0f, 1.5f}}; }
std::vector<float> depth_image() {
    std::vector<float> img(kWidth * kHeight);
    for (int i = 0; i < kWidth * kHeight; ++i) img[i] = 100.0f + (float)i;
    return img;
}
ms_pinhole camera() { return ms_pinhole{2.0, 4.0, 1.0, 2.0, kWidth, kHeight}; }

// ---- the reference, sequentially: processKeyPoints (:51-64), FeatureSearch::create, BowIndex::assemble --------------------------------------
Expected restate(const HostFrame &f, const Tracker *tr, const std::vector<float> *image) {
    Expected e;
    std::map<std::int32_t, std::size_t> trackIdToIndex;
    if (tr) for (std::size_t i = 0; i < tr->id.size(); ++i) trackIdToIndex[tr->id[i]] = i;
    const ms_pinhole c = camera();
    for (std::size_t j = 0; j < f.size(); ++j) {
        float depth = -1;
        if (f.trackId[j] >= 0 && tr) depth = tr->depth[trackIdToIndex.at(f.trackId[j])];
        if (depth < 0) {
            depth = -1;
            const long ix = std::lrintf(f.x[j]), iy = std::lrintf(f.y[j]);      // round to nearest even, as __float2int_rn
            if (image && ix >= 0 && ix < kWidth && iy >= 0 && iy < kHeight) depth = (*image)[iy * kWidth + ix];
        }
        e.depth.push_back(depth);
        const double xn = ((double)f.x[j] - c.cx) / c.fx, yn = ((double)f.y[j] - c.cy) / c.fy, nrm = std::sqrt(xn * xn + yn * yn + 1.0);
        e.bearing.push_back({xn / nrm, yn / nrm, 1.0 / nrm});
    }
    std::vector<std::int32_t> order(f.size());
    for (std::size_t j = 0; j < f.size(); ++j) order[j] = (std::int32_t)j;
    std::stable_sort(order.begin(), order.end(), [&](std::int32_t a, std::int32_t b) { return f.y[a] < f.y[b]; });
    for (std::int32_t j : order) { e.sortedX.push_back(f.x[j]); e.sortedY.push_back(f.y[j]); e.sortedIndex.push_back(j); }
    std::vector<std::int32_t> word, node;
    std::vector<double> weight;
    for (std::size_t j = 0; j < f.size(); ++j) {              // the descent on the two-leaf tree; levelsUp = 4 from depth 1: the node is the root
        const bool ones = f.desc[j][0] != 0;
        word.push_back(ones ? 1 : 0); weight.push_back(ones ? 0.0 : 2.0); node.push_back(0);
    }
    FeatureVector fv;
    BowIndex::assemble(word, weight, node, e.bowVector, fv);
    e.nodeStart.push_back(0);
    for (const auto &kv : fv) {
        e.nodeId.push_back((std::int32_t)kv.first);
        for (unsigned j : kv.second) e.kpIdx.push_back((std::int32_t)j);
        e.nodeStart.push_back((std::int32_t)e.kpIdx.size());
    }
    BowVector alone;
    BowIndex::assembleVector(word, weight, alone);
    if (alone != e.bowVector) { std::printf("assembleVector differs from assemble\n"); std::exit(1); }
    return e;
}

int fails = 0;
void expect(bool ok, const char *what) { if (!ok) { std::printf("FAILED: %s\n", what); ++fails; } }

int no_gpu() {
    std::printf("link ok %d\n", ms_version() != nullptr);
    const std::vector<float> img = depth_image();
    const Tracker tr = tracker();
    const Expected e = restate(frame0(), &tr, &img);
    // track 11 -> its LAST entry, 1.5; track 12 -> -1 < 0 -> the image at (round(2.5) = 2, 1) = 100 + 8; track 13 -> 0.25; column round(5.5) = 6 is outside; (0, 3) = 118
    expect(e.depth == std::vector<float>({1.5f, 108.0f, 0.25f, -1.0f, 118.0f}), "depths");
    expect(e.sortedIndex == std::vector<std::int32_t>({1, 3, 0, 2, 4}), "stable order by y");
    expect(e.sortedX == std::vector<float>({2.5f, 5.5f, 1.0f, 4.0f, 0.0f}), "sorted x");
    expect(e.nodeId == std::vector<std::int32_t>({0}) && e.nodeStart == std::vector<std::int32_t>({0, 3}) && e.kpIdx == std::vector<std::int32_t>({0, 2, 3}), "node lists without the stop words");
    expect(e.bowVector.size() == 1 && e.bowVector.at(0) == 1.0, "L1-normalised BowVector");
    expect(e.bearing[0][0] == 0.0 && e.bearing[0][1] == 0.0 && e.bearing[0][2] == 1.0, "the principal point looks along z");
    const Expected none = restate(frame0(), nullptr, nullptr);
    expect(none.depth == std::vector<float>(5, -1.0f), "no tracker features, no image");
    const Expected empty = restate(HostFrame{}, &tr, &img);
    expect(empty.depth.empty() && empty.nodeStart == std::vector<std::int32_t>({0}) && empty.bowVector.empty(), "n = 0");
    std::printf(fails ? "restatement FAILED\n" : "restatement ok\n");
    return fails ? 1 : 0;
}

// ---- the device side ----------------------------------------------------------------------------------------------------------------------
struct DeviceView {                          // a two-frame ms_keypoints of capacity kCapacity, as the extractor lays it out
    DeviceArray<std::int32_t> count, octave, track;
    DeviceArray<float> x, y, angle;
    DeviceArray<std::uint32_t> desc;
    ms_keypoints view{};
    DeviceView(Context &ctx, const HostFrame &a, const HostFrame &b)
        : count(ctx, 2), octave(ctx, 2 * kCapacity), track(ctx, 2 * kCapacity), x(ctx, 2 * kCapacity), y(ctx, 2 * kCapacity), angle(ctx, 2 * kCapacity),
          desc(ctx, 16 * kCapacity) {
        const std::int32_t n[2] = {(std::int32_t)a.size(), (std::int32_t)b.size()};
        count.upload(0, 2, n);
        const HostFrame *f[2] = {&a, &b};
        for (int k = 0; k < 2; ++k) {
            const std::size_t at = (std::size_t)k * kCapacity, m = f[k]->size();
            x.upload(at, m, f[k]->x.data()); y.upload(at, m, f[k]->y.data()); angle.upload(at, m, f[k]->angle.data());
            octave.upload(at, m, f[k]->octave.data()); track.upload(at, m, f[k]->trackId.data());
            if (m) desc.upload(8 * at, 8 * m, f[k]->desc[0].data());
        }
        view = ms_keypoints{kCapacity, count.data(), x.data(), y.data(), angle.data(), octave.data(), desc.data(), track.data()};
    }
};

bool same(const std::vector<double> &got, const std::vector<std::array<double, 3>> &want) {
    return got.size() >= 3 * want.size() && (want.empty() || std::memcmp(got.data(), want.data(), 24 * want.size()) == 0);
}

int gpu() {
    Context ctx(0);
    VocabularyTree tree;
    tree.branchingFactor = 2; tree.depthLevels = 1;
    tree.parent = {0, 0, 0}; tree.wordId = {-1, 0, 1}; tree.weight = {0.0, 2.0, 0.0};
    tree.descriptor.assign(24, 0u);
    for (int w = 0; w < 8; ++w) tree.descriptor[16 + w] = 0xffffffffu;
    BowIndex bow(ctx, tree);
    const HostFrame f0 = frame0(), f1 = frame1();
    const Tracker tr = tracker();
    const std::vector<float> img = depth_image();
    DeviceView dv(ctx, f0, f1);
    DeviceArray<float> dImg(ctx, img.size());
    dImg.upload(0, img.size(), img.data());

    DeviceKeyframeMapPoints keyframes(ctx, kSlots, kStride, 20);
    DeviceKeypointTable keypoints(ctx, kSlots, kStride);
    DeviceKeyframePoses poses(ctx, std::vector<DeviceKeyframePoses::Pose>(kSlots, DeviceKeyframePoses::Pose{}));
    DeviceDescriptorPool pool(ctx, 9);
    DeviceKeyframe kfA(ctx, kCapacity), kfB(ctx, kCapacity);
    KeyframeSlots slots;
    slots.id.assign(kSlots, -1); slots.t.assign(kSlots, 0.0); slots.previous.assign(kSlots, -1); slots.next.assign(kSlots, -1);
    slots.cameraCenter.assign(kSlots, {}); slots.camera.assign(kSlots, ms_pinhole{}); slots.focalLength.assign(kSlots, 0); slots.descBase.assign(kSlots, -1);
    slots.frames = {nullptr, &kfA, &kfB};
    MapTables M{keyframes, slots};
    M.keypoints = &keypoints; M.poses = &poses; M.pool = &pool;
    keyframes.update(1, {-1, 3});                            // an entry of an earlier keyframe that nobody erased: the slot is NOT empty

    KeyframeAdmission a;
    a.id = 40; a.t = 1.25; a.camera = camera(); a.focalLength = 3;
    a.poseCW = {0, -1, 0, 1.0, 1, 0, 0, 2.0, 0, 0, 1, 3.0};   // R = a quarter turn about z, t = (1, 2, 3): the centre is -R^T t = (-2, 1, -3)
    a.trackIds = tr.id; a.trackDepths = tr.depth; a.hasTrackerFeatures = true;
    a.depthImage = dImg.data(); a.depthWidth = kWidth; a.depthHeight = kHeight; a.depthStride = kWidth;

    // ---- the refusals: a bound entry in the row (the device's verdict), then an occupied slot, a slot without a DeviceKeyframe, a full pool
    int refused = 0;
    try { admitKeyframe(ctx, M, dv.view, 0, 1, -1, a, &bow); } catch (const std::runtime_error &e) { refused += std::strstr(e.what(), "is not empty") != nullptr; }
    expect(pool.used() == 0 && slots.id[1] == -1 && slots.descBase[1] == -1 && kfA.keyPointCount() == 0, "a refused call leaves the pool and the record");
    expect(ctx.download(keyframes.table() + kStride, 3) == std::vector<std::int32_t>({-1, 3, -1}), "a refused call leaves the row");
    keyframes.clear(1);
    slots.id[2] = 7;
    try { admitKeyframe(ctx, M, dv.view, 0, 2, -1, a, &bow); } catch (const std::invalid_argument &) { ++refused; }
    slots.id[2] = -1;
    try { admitKeyframe(ctx, M, dv.view, 0, 0, -1, a, &bow); } catch (const std::invalid_argument &) { ++refused; }
    try { admitKeyframe(ctx, M, dv.view, 0, 1, 1, a, &bow); } catch (const std::invalid_argument &) { ++refused; }
    std::printf("refusals ok %d cases\n", refused);
    expect(refused == 4, "four refusals");

    // ---- keyframe 40 from frame 0 into slot 1
    const Expected e0 = restate(f0, &tr, &img);
    const AdmittedKeyframe r0 = admitKeyframe(ctx, M, dv.view, 0, 1, -1, a, &bow);
    expect(r0.keyPoints == 5 && r0.keyPointTrackIds == f0.trackId && r0.bowVector == e0.bowVector, "n, keyPointTrackIds, BowVector");
    expect(pool.used() == 5 && slots.descBase[1] == 0 && slots.id[1] == 40 && slots.t[1] == 1.25 && slots.previous[1] == -1 && slots.next[1] == -1, "pool and record");
    expect(slots.cameraCenter[1] == std::array<double, 3>({-2.0, 1.0, -3.0}) && slots.focalLength[1] == 3 && slots.camera[1].fy == 4.0, "camera centre, camera");
    expect(kfA.keyPointCount() == 5 && kfA.frame().bow.n_nodes == 1, "the ms_match_frame");
    expect(kfA.hostSortedX() == e0.sortedX && kfA.hostSortedY() == e0.sortedY && kfA.hostSortedIndex() == e0.sortedIndex, "host copies of the sorted arrays");
    expect(kfA.hostOctave(3) == 3 && std::memcmp(kfA.hostDescriptor(1), f0.desc[1].data(), 32) == 0, "host copies of octave and descriptor");
    expect(ctx.download(kfA.sortedIndex(), 5) == e0.sortedIndex && ctx.download(kfA.sortedX(), 5) == e0.sortedX, "device sorted arrays");
    expect(ctx.download(kfA.frame().bow.kp_idx, 3) == e0.kpIdx && ctx.download(kfA.frame().bow.node_start, 2) == e0.nodeStart && ctx.download(kfA.frame().bow.node_id, 1) == e0.nodeId,
           "device node lists");
    expect(same(ctx.download(kfA.frame().bearing, 15), e0.bearing) && ctx.download(kfA.frame().usable, 5) == std::vector<std::uint8_t>(5, 1), "bearing, usable");
    expect(ctx.download(keypoints.depth() + kStride, 5) == e0.depth && ctx.download(keypoints.x() + kStride, 5) == f0.x && ctx.download(keypoints.octave() + kStride, 5) == f0.octave,
           "keypoint table");
    expect(ctx.download(keypoints.x() + kStride + 5, 2) == std::vector<float>(2, 0.0f), "entries behind n keep their bytes");
    expect(ctx.download(keyframes.table() + kStride, kStride) == std::vector<std::int32_t>(kStride, -1), "the row is cleared");
    expect(std::memcmp(ctx.download(pool.descriptor(), 40).data(), f0.desc[0].data(), 160) == 0, "descriptor pool");
    expect(poses.download()[1] == a.poseCW, "pose");
    std::printf("admitKeyframe ok: %zu keypoints, %d node, %d in the lists\n", r0.keyPoints, kfA.frame().bow.n_nodes, (int)e0.kpIdx.size());

    // ---- keyframe 41 from frame 1 into slot 2, behind 40; no tracker features, no image, no BowIndex
    KeyframeAdmission b = a;
    b.id = 41; b.hasTrackerFeatures = false; b.trackIds.clear(); b.trackDepths.clear(); b.depthImage = nullptr;
    const Expected e1 = restate(f1, nullptr, nullptr);
    const AdmittedKeyframe r1 = admitKeyframe(ctx, M, dv.view, 1, 2, 1, b, nullptr);
    expect(r1.keyPoints == 2 && r1.bowVector.empty() && kfB.frame().bow.n_nodes == 0 && kfB.hostSortedIndex() == e1.sortedIndex, "the second keyframe");
    expect(pool.used() == 7 && slots.descBase[2] == 5 && slots.previous[2] == 1 && slots.next[1] == 2 && slots.next[2] == -1, "pool base and chain");
    expect(ctx.download(keypoints.depth() + 2 * kStride, 2) == e1.depth && ctx.download(keypoints.depth() + kStride, 5) == e0.depth, "depths; slot 1 as it was");
    expect(std::memcmp(ctx.download(pool.descriptor() + 40, 16).data(), f1.desc[0].data(), 64) == 0, "descriptor pool behind the first keyframe");
    std::printf("chain ok: 40 -> 41, pool %zu of %zu\n", pool.used(), pool.size());

    // ---- the pool runs out: three descriptors are wanted, two are free
    int full = 0;
    slots.id[1] = -1; keyframes.clear(1);
    HostFrame f2 = f0; f2.x.resize(3); f2.y.resize(3); f2.angle.resize(3); f2.octave.resize(3); f2.trackId.resize(3); f2.desc.resize(3);
    DeviceView dv2(ctx, f2, f1);
    try { admitKeyframe(ctx, M, dv2.view, 0, 1, 2, a, &bow); } catch (const std::runtime_error &e) { full += std::strstr(e.what(), "3 keypoints") != nullptr; }
    expect(full == 1 && pool.used() == 7 && slots.id[1] == -1 && slots.next[2] == -1, "a full pool is the call's capacity verdict and leaves everything");
    std::printf(fails ? "mirror FAILED\n" : "mirror ok\n");
    return fails ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--no-gpu")) return no_gpu();
    if (argc == 2 && !std::strcmp(argv[1], "--gpu")) return gpu();
    std::printf("usage: keyframe_admit_smoke --no-gpu | --gpu\n");
    return 2;
}
