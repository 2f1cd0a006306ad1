// Compile + link check of the device BowVector in the host mirror (BowIndex::addAdmitted / addWords / bowVector in mi355slam/bow_index.hpp,
// DESIGN 9.20) against libmi355slam.so, and its comparison with BowIndex::assembleVector + add on a hand-computed frame
// (tests/test_bow_vector_smoke.py).
//   bow_vector_smoke --no-gpu   assembleVector against the hand-computed vectors (no context, no device)
//   bow_vector_smoke --gpu      one index filled through admitKeyframe + addAdmitted and through addWords, its twin through assembleVector +
//                               add: every bowVector() and every getBowSimilar() equal; the refusals
#include <cstdio>
#include <cstring>
#include <vector>
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

constexpr int kCapacity = 8, kStride = 7, kSlots = 3;

// the three leaves of the vocabulary: all zeros (word 0, weight 2), all ones (word 1, a stop word), the first half ones (word 2, weight 0.5)
KeyPoint::Descriptor descriptor(int word) {
    KeyPoint::Descriptor d;
    d.fill(0u);
    for (int k = 0; k < (word == 1 ? 8 : word == 2 ? 4 : 0); ++k) d[(std::size_t)k] = 0xffffffffu;
    return d;
}
VocabularyTree vocabulary() {
    VocabularyTree tree;
    tree.branchingFactor = 3; tree.depthLevels = 1;
    tree.parent = {0, 0, 0, 0}; tree.wordId = {-1, 0, 1, 2}; tree.weight = {0.0, 2.0, 0.0, 0.5};
    tree.descriptor.assign(8, 0u);
    for (int w = 0; w < 3; ++w) { const KeyPoint::Descriptor d = descriptor(w); tree.descriptor.insert(tree.descriptor.end(), d.begin(), d.end()); }
    return tree;
}

// The frame: six keypoints on the words 0, 1, 2, 0, 2, 0.  v[0] = 2 + 2 + 2 = 6, v[2] = 0.5 + 0.5 = 1, the stop word is skipped; the norm is 7.
const std::vector<std::int32_t> kFrameWords = {0, 1, 2, 0, 2, 0};
const std::vector<double> kFrameWeights = {2.0, 0.0, 0.5, 2.0, 0.5, 2.0};
BowVector frame_vector() { return BowVector{{0u, 6.0 / 7.0}, {2u, 1.0 / 7.0}}; }
// A descent given as arrays: the words 2, 2, 0, 1 -> v[0] = 2, v[2] = 1, the norm is 3.
const std::vector<std::int32_t> kListWords = {2, 2, 0, 1};
const std::vector<double> kListWeights = {0.5, 0.5, 2.0, 0.0};
BowVector list_vector() { return BowVector{{0u, 2.0 / 3.0}, {2u, 1.0 / 3.0}}; }

int fails = 0;
void expect(bool ok, const char *what) { if (!ok) { std::printf("FAILED: %s\n", what); ++fails; } }

bool same(const std::vector<BowSimilar> &a, const std::vector<BowSimilar> &b) {
    if (a.size() != b.size()) return false;
    for (std::size_t i = 0; i < a.size(); ++i)
        if (!(a[i].mapKf == b[i].mapKf) || std::memcmp(&a[i].score, &b[i].score, 4) != 0) return false;
    return true;
}

int no_gpu() {
    int (BowIndex::*w)(const std::int32_t *, const double *, int, MapKf) = &BowIndex::addWords;
    int (BowIndex::*a)(MapKf) = &BowIndex::addAdmitted;
    BowVector (BowIndex::*v)(MapKf) = &BowIndex::bowVector;
    std::printf("link ok %d\n", w != nullptr && a != nullptr && v != nullptr && ms_version() != nullptr);
    BowVector frame, list, none;
    BowIndex::assembleVector(kFrameWords, kFrameWeights, frame);
    BowIndex::assembleVector(kListWords, kListWeights, list);
    BowIndex::assembleVector({1, 1}, {0.0, 0.0}, none);
    expect(frame == frame_vector() && list == list_vector() && none.empty(), "assembleVector gives the hand-computed vectors");
    std::printf(fails ? "restatement FAILED\n" : "restatement ok\n");
    return fails ? 1 : 0;
}

int gpu() {
    Context ctx(0);
    const VocabularyTree tree = vocabulary();
    BowIndex device(ctx, tree), host(ctx, tree);
    int refused = 0;
    try { device.addAdmitted(MapKf{1, 40}); } catch (const std::runtime_error &) { ++refused; }      // nothing was admitted yet

    // ---- the frame through the extractor's view and admitKeyframe
    const std::int32_t n = (std::int32_t)kFrameWords.size();
    const std::int32_t counts[2] = {n, 0};
    std::vector<float> x = {1.0f, 2.5f, 4.0f, 5.5f, 0.0f, 3.0f}, y = {2.0f, 1.0f, 2.5f, 1.5f, 3.0f, 0.5f}, angle(6, 0.f);
    std::vector<std::int32_t> octave(6, 0), track(6, -1);
    std::vector<KeyPoint::Descriptor> desc;
    for (std::int32_t word : kFrameWords) desc.push_back(descriptor(word));
    DeviceArray<std::int32_t> dCount(ctx, 2), dOctave(ctx, 2 * kCapacity), dTrack(ctx, 2 * kCapacity);
    DeviceArray<float> dX(ctx, 2 * kCapacity), dY(ctx, 2 * kCapacity), dAngle(ctx, 2 * kCapacity);
    DeviceArray<std::uint32_t> dDesc(ctx, 16 * kCapacity);
    dCount.upload(0, 2, counts);
    dX.upload(0, 6, x.data()); dY.upload(0, 6, y.data()); dAngle.upload(0, 6, angle.data()); dOctave.upload(0, 6, octave.data()); dTrack.upload(0, 6, track.data());
    dDesc.upload(0, 48, desc[0].data());
    const ms_keypoints view{kCapacity, dCount.data(), dX.data(), dY.data(), dAngle.data(), dOctave.data(), dDesc.data(), dTrack.data()};
    DeviceKeyframeMapPoints keyframes(ctx, kSlots, kStride, 20);
    DeviceKeypointTable keypoints(ctx, kSlots, kStride);
    DeviceKeyframePoses poses(ctx, std::vector<DeviceKeyframePoses::Pose>(kSlots, DeviceKeyframePoses::Pose{}));
    DeviceDescriptorPool pool(ctx, 16);
    DeviceKeyframe kfA(ctx, kCapacity);
    KeyframeSlots slots;
    slots.id.assign(kSlots, -1); slots.t.assign(kSlots, 0.0); slots.previous.assign(kSlots, -1); slots.next.assign(kSlots, -1);
    slots.cameraCenter.assign(kSlots, {}); slots.camera.assign(kSlots, ms_pinhole{}); slots.focalLength.assign(kSlots, 0); slots.descBase.assign(kSlots, -1);
    slots.frames = {nullptr, &kfA, nullptr};
    MapTables M{keyframes, slots};
    M.keypoints = &keypoints; M.poses = &poses; M.pool = &pool;
    KeyframeAdmission a;
    a.id = 40; a.t = 1.25; a.camera = ms_pinhole{2.0, 4.0, 1.0, 2.0, 6, 4}; a.focalLength = 3;
    a.poseCW = {1, 0, 0, 0.0, 0, 1, 0, 0.0, 0, 0, 1, 0.0};
    const AdmittedKeyframe r = admitKeyframe(ctx, M, view, 0, 1, -1, a, &device);
    expect(r.keyPoints == 6 && r.bowVector == frame_vector(), "the admission's host vector is the hand-computed one");
    expect(device.addAdmitted(MapKf{1, 40}) == 2, "addAdmitted: two words");
    host.add(r.bowVector, MapKf{1, 40});
    expect(device.bowVector(MapKf{1, 40}) == frame_vector() && host.bowVector(MapKf{1, 40}) == frame_vector(), "bowVector of the admitted keyframe, both indices");

    // ---- a descent given as device arrays, and a keyframe of stop words alone
    DeviceArray<std::int32_t> dWord(ctx, 8);
    DeviceArray<double> dWeight(ctx, 8);
    dWord.upload(0, 4, kListWords.data()); dWeight.upload(0, 4, kListWeights.data());
    expect(device.addWords(dWord.data(), dWeight.data(), 4, MapKf{1, 41}) == 2, "addWords: two words");
    BowVector list, none;
    BowIndex::assembleVector(kListWords, kListWeights, list);
    host.add(list, MapKf{1, 41});
    expect(device.bowVector(MapKf{1, 41}) == list_vector() && host.bowVector(MapKf{1, 41}) == list, "bowVector of the listed descent");
    expect(device.addWords(dWord.data() + 3, dWeight.data() + 3, 1, MapKf{1, 42}) == 0 && device.bowVector(MapKf{1, 42}).empty(), "stop words alone: an empty entry");
    host.add(none, MapKf{1, 42});
    expect(device.addWords(dWord.data() + 2, dWeight.data() + 2, 1, MapKf{2, 7}) == 1 && device.bowVector(MapKf{2, 7}) == BowVector{{0u, 1.0}}, "one keypoint");
    host.add(BowVector{{0u, 1.0}}, MapKf{2, 7});
    std::printf("bowVector ok: 4 entries\n");

    // ---- getBowSimilar from both indices
    int results = 0;
    for (const BowVector &q : {frame_vector(), list_vector(), BowVector{{2u, 1.0}}})
        for (float minInCommon : {0.0f, 0.8f})
            for (MapKf self : {MapKf{1, 40}, MapKf{9, 9}}) {
                const std::vector<BowSimilar> got = device.getBowSimilar(q, self, minInCommon, 0.0f), want = host.getBowSimilar(q, self, minInCommon, 0.0f);
                expect(same(got, want), "getBowSimilar differs between the indices");
                results += (int)got.size();
            }
    expect(results > 10, "the queries found entries");
    std::printf("getBowSimilar ok: %d results\n", results);

    // ---- the refusals: a duplicate id, an id that is not live
    try { device.addWords(dWord.data(), dWeight.data(), 4, MapKf{1, 41}); } catch (const std::runtime_error &e) { refused += std::strstr(e.what(), "already in the database") != nullptr; }
    try { device.bowVector(MapKf{5, 5}); } catch (const std::runtime_error &e) { refused += std::strstr(e.what(), "is not in the database") != nullptr; }
    device.remove(MapKf{1, 41});
    try { device.bowVector(MapKf{1, 41}); } catch (const std::runtime_error &) { ++refused; }
    expect(device.addWords(dWord.data(), dWeight.data(), 4, MapKf{1, 41}) == 2 && device.bowVector(MapKf{1, 41}) == list_vector(), "a removed id is free again");
    std::printf("refusals ok %d cases\n", refused);
    expect(refused == 4, "four refusals");
    std::printf(fails ? "mirror FAILED\n" : "mirror ok\n");
    return fails ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--no-gpu")) return no_gpu();
    if (argc == 2 && !std::strcmp(argv[1], "--gpu")) return gpu();
    std::printf("usage: bow_vector_smoke --no-gpu | --gpu\n");
    return 2;
}
