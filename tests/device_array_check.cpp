// Ownership check of the host mirror's device memory (mi355slam::DeviceArray in mi355slam/common.hpp and every owner built on it: the tables
// of map_tables.hpp, DeviceKeyframe and updateDescriptors in keyframe_matcher.hpp, BowIndex) on the CPU (tests/test_device_array_check.py).
// The program links no library: it defines the few ABI functions the exercised inline code reaches, with the four ms_dev_* calls over malloc
// and memcpy.  They keep the set of live blocks, a log of the calls ("a" alloc, "f" free, "u<bytes>" upload, "d<bytes>" download) and a
// counter that makes the k-th allocation fail; a free of a block that is not live and a copy outside a live block abort.
//   1  DeviceArray alone: zero length, range checks, round trip, moves, reset
//   2  every owner, no failure: nothing stays live, and the call log is the one recorded from the headers before DeviceArray existed
//   3  the same scenarios with the k-th allocation failing, for every k: std::runtime_error, nothing leaks, and the three grow-only owners
//      stay usable (DeviceObservationLists and BowIndex allocate again on the next call, DeviceTrackTable keeps its old window)
//   4  updateDescriptors when the kernel call fails: it throws and nothing stays live
// Built with -DDEVICE_ARRAY_CHECK_RECORD the program leaves part 1 out and prints the logs of part 2 instead of comparing them: that is how the
// expected text below was taken from the earlier headers (the command is in tests/test_device_array_check.py).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>
#include "mi355slam/keyframe_matcher.hpp"
#include "mi355slam/bow_index.hpp"

using namespace mi355slam;

// ---- the stand-in ABI ---------------------------------------------------------------------------------------------------------------
struct ms_ctx { int unused; };
struct ms_bow_vocab { int unused; };

namespace {
std::map<char *, std::size_t> g_live;        // block -> bytes
std::string g_log;
long g_allocs = 0, g_failAt = -1;            // the g_failAt-th allocation since reset_stand_in() returns MS_ERR_HIP
int g_medoidRc = MS_OK, g_vocabRc = MS_OK, g_transformRc = MS_OK;
int g_needRows = 0, g_needObs = 0;           // what ms_observation_lists reports as needed
int g_failures = 0;

void reset_stand_in() { g_log.clear(); g_allocs = 0; g_failAt = -1; g_medoidRc = g_vocabRc = g_transformRc = MS_OK; g_needRows = g_needObs = 0; }

void require_inside_live_block(const void *p, std::size_t bytes, const char *what) {
    const char *c = static_cast<const char *>(p);
    auto it = g_live.upper_bound(const_cast<char *>(c));
    if (it != g_live.begin()) { --it; if (c >= it->first && c + bytes <= it->first + it->second) return; }
    std::fprintf(stderr, "%s of %zu bytes outside every live block\n", what, bytes);
    std::abort();
}
}  // namespace

extern "C" {
int ms_ctx_create(int, ms_ctx **out) { static ms_ctx c; *out = &c; return MS_OK; }
void ms_ctx_destroy(ms_ctx *) {}
const char *ms_last_error(const ms_ctx *) { return "stand-in"; }
int ms_dev_alloc(ms_ctx *, size_t bytes, void **out) {
    *out = nullptr;
    if (g_allocs++ == g_failAt) return MS_ERR_HIP;
    char *p = static_cast<char *>(std::calloc(bytes ? bytes : 1, 1));
    g_live[p] = bytes;
    g_log += "a ";
    *out = p;
    return MS_OK;
}
int ms_dev_free(ms_ctx *, void *p) {
    if (!g_live.erase(static_cast<char *>(p))) { std::fprintf(stderr, "free of a block that is not live\n"); std::abort(); }
    std::free(p);
    g_log += "f ";
    return MS_OK;
}
int ms_dev_upload(ms_ctx *, void *dst, const void *src, size_t bytes) {
    require_inside_live_block(dst, bytes, "upload");
    std::memcpy(dst, src, bytes);
    g_log += "u" + std::to_string(bytes) + " ";
    return MS_OK;
}
int ms_dev_download(ms_ctx *, void *dst, const void *src, size_t bytes) {
    require_inside_live_block(src, bytes, "download");
    std::memcpy(dst, src, bytes);
    g_log += "d" + std::to_string(bytes) + " ";
    return MS_OK;
}
int ms_feature_search_sort(const float *x, const float *y, int n, float *sx, float *sy, int32_t *si) {
    std::iota(si, si + n, 0);
    std::stable_sort(si, si + n, [&](int32_t a, int32_t b) { return y[a] < y[b]; });
    for (int i = 0; i < n; ++i) { sx[i] = x[si[i]]; sy[i] = y[si[i]]; }
    return MS_OK;
}
int ms_descriptor_medoid(ms_ctx *, const uint32_t *, const int32_t *, const int32_t *, int n_points, int, int32_t *best_local, int32_t *) {
    if (g_medoidRc == MS_OK) std::fill(best_local, best_local + n_points, 0);
    return g_medoidRc;
}
int ms_bow_vocab_create(ms_ctx *, int, const int32_t *, const uint32_t *, const double *, const int32_t *, int, ms_bow_vocab **out) {
    static ms_bow_vocab v;
    *out = g_vocabRc == MS_OK ? &v : nullptr;
    return g_vocabRc;
}
void ms_bow_vocab_destroy(ms_bow_vocab *) {}
void ms_bow_db_destroy(ms_bow_db *) {}
int ms_bow_transform(ms_ctx *, const ms_bow_vocab *, const uint32_t *, int n, int, int32_t *word, double *weight, int32_t *node) {
    if (g_transformRc == MS_OK) { std::fill(word, word + n, 0); std::fill(weight, weight + n, 1.0); std::fill(node, node + n, 1); }
    return g_transformRc;
}
// MS_ERR_CAPACITY with the needed counts while the buffers are too small for them, MS_OK and rows 0 .. n_rows - 1 afterwards
int ms_observation_lists(ms_ctx *, const int32_t *, int, int, int, const int32_t *, const uint8_t *, const float *, const float *, const int32_t *, const float *,
                         const int32_t *, const ms_obs_select *, int, const ms_obs_lists *lists, int cap_rows, int cap_obs, int32_t *n_rows, int32_t *n_obs) {
    *n_rows = g_needRows; *n_obs = g_needObs;
    if (g_needRows > cap_rows || g_needObs > cap_obs) return MS_ERR_CAPACITY;
    std::iota(lists->rows, lists->rows + g_needRows, 0);
    return MS_OK;
}
}  // extern "C"

// ---- the checks ---------------------------------------------------------------------------------------------------------------------
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)

namespace {
template <class F> bool throws_runtime_error(F f) {
    try { f(); } catch (const std::runtime_error &) { return true; }
    return false;
}
std::size_t count_in_log(const char *token) {
    std::size_t n = 0;
    for (std::size_t at = g_log.find(token); at != std::string::npos; at = g_log.find(token, at + 1)) ++n;
    return n;
}

#ifndef DEVICE_ARRAY_CHECK_RECORD
void device_array_alone(Context &ctx) {
    reset_stand_in();
    {   // length 0: a pointer all the same, and neither copy reaches the ABI
        DeviceArray<std::int32_t> z(ctx, 0);
        CHECK(z.data() != nullptr && z.size() == 0);
        z.upload(0, 0, nullptr);
        z.fill(5);
        CHECK(z.download().empty());
        CHECK(ctx.download(z.data(), 0).empty());
        CHECK(g_log == "a ");
    }
    CHECK(g_log == "a f " && g_live.empty());
    reset_stand_in();
    {   // a default-constructed array owns nothing and frees nothing
        DeviceArray<float> none;
        CHECK(none.data() == nullptr && none.size() == 0 && none.download().empty());
        none.upload(0, 0, nullptr);
        none.reset();
    }
    CHECK(g_log.empty());
    {   // ranges: outside throws and writes nothing; a sub-range goes up and comes back
        DeviceArray<std::int32_t> a(ctx, 6);
        a.fill(-1);
        reset_stand_in();
        const std::int32_t v[3] = {7, 8, 9};
        CHECK(throws_runtime_error([&] { a.upload(4, 3, v); }));
        CHECK(throws_runtime_error([&] { a.upload(7, 0, v); }));
        CHECK(throws_runtime_error([&] { a.download(6, 1); }));
        CHECK(g_log.empty());
        CHECK((a.download() == std::vector<std::int32_t>{-1, -1, -1, -1, -1, -1}));
        a.upload(2, 3, v);
        CHECK((a.download(1, 4) == std::vector<std::int32_t>{-1, 7, 8, 9}));
        CHECK((a.download() == std::vector<std::int32_t>{-1, -1, 7, 8, 9, -1}));
        CHECK(g_log == "d24 u12 d16 d24 ");
        const DeviceArray<std::int32_t> &ca = a;
        CHECK(ca.data() == a.data());
    }
    CHECK(g_live.empty());
    reset_stand_in();
    {   // moves: each block is freed exactly once (a second free aborts in the stand-in), move assignment frees the old block at once
        DeviceArray<std::uint8_t> a(ctx, 3);
        const std::uint8_t *block = a.data();
        DeviceArray<std::uint8_t> b(std::move(a));
        CHECK(a.data() == nullptr && a.size() == 0 && b.data() == block && b.size() == 3);
        DeviceArray<std::uint8_t> c(ctx, 2);
        CHECK(g_log == "a a ");
        c = std::move(b);
        CHECK(g_log == "a a f " && c.data() == block && c.size() == 3 && b.data() == nullptr && g_live.size() == 1);
    }
    CHECK(g_log == "a a f f " && g_live.empty());
    reset_stand_in();
    {   // reset() frees now, the destructor then has nothing to free
        DeviceArray<double> a(ctx, 4);
        a.reset();
        CHECK(g_log == "a f " && a.data() == nullptr && a.size() == 0 && g_live.empty());
    }
    CHECK(g_log == "a f ");
}
#endif

// ---- one scenario per owner, at the smallest sizes that have every branch: 3 slots, stride 5, 10 map points, a track window of 4, 2 keypoints
KeyPointVector keypoints(std::size_t n) {
    KeyPointVector kps(n);
    for (std::size_t i = 0; i < n; ++i) { kps[i].pt = {float(i), float(n - i)}; kps[i].angle = 0.f; kps[i].octave = 0; kps[i].bearing = {0, 0, 1}; kps[i].descriptor.fill((std::uint32_t)i); }
    return kps;
}

void device_keyframe(Context &ctx) {
    const KeyPointVector kps = keypoints(2);
    KeyframeFeatures f;
    f.keyPoints = &kps; f.usable = {1, 1}; f.bowFeatureVec[7] = {0, 1};
    DeviceKeyframe kf(ctx, f);
    CHECK(kf.frame().n == 2 && kf.frame().bow.n_nodes == 1 && kf.hostSortedIndex()[0] == 1);
}
void keyframe_poses(Context &ctx) {
    std::vector<DeviceKeyframePoses::Pose> p(3);
    for (std::size_t i = 0; i < 3; ++i) p[i].fill(double(i));
    DeviceKeyframePoses poses(ctx, p);
    p[1].fill(9.0);
    poses.update(1, 1, &p[1]);
    CHECK(throws_runtime_error([&] { poses.update(2, 2, p.data()); }));
    CHECK(poses.download() == p && poses.size() == 3 && poses.pose() != nullptr);
}
void descriptor_pool(Context &ctx) {
    DeviceDescriptorPool pool(ctx, std::vector<KeyPoint::Descriptor>(2)), none(ctx, {});
    CHECK(pool.size() == 2 && none.size() == 0 && none.descriptor() != nullptr);
}
void map_points(Context &ctx) {
    const std::size_t n = 10;
    std::vector<DeviceMapPoints::Vec3d> pos(n);
    std::vector<DeviceMapPoints::Vec3f> norm(n);
    std::vector<float> lo(n, 1.f), hi(n, 2.f);
    std::vector<KeyPoint::Descriptor> desc(n);
    DeviceMapPoints mp(ctx, pos, norm, lo, hi, desc);
    mp.update(2, 3, pos.data(), nullptr, lo.data(), nullptr, desc.data());
    mp.update(10, 0, pos.data(), norm.data(), lo.data(), hi.data(), desc.data());
    CHECK(throws_runtime_error([&] { mp.update(8, 3, pos.data(), nullptr, nullptr, nullptr, nullptr); }));
    CHECK(mp.size() == n && mp.position() == mp.mutablePosition());
}
void keyframe_map_points(Context &ctx) {
    DeviceKeyframeMapPoints table(ctx, 3, 5, 10);
    table.update(1, {0, 9, -1});
    table.clear(1);
    CHECK(table.size() == 3 && table.stride() == 5 && table.table() == table.mutableTable());
}
void flags_and_live(Context &ctx) {
    const std::vector<std::uint8_t> ten(10, 3);
    DeviceMapPointFlags flags(ctx, ten), none(ctx, {});
    flags.update(4, 2, ten.data());
    CHECK(throws_runtime_error([&] { flags.update(9, 2, ten.data()); }));
    DeviceMapPointLive live(ctx, ten);
    live.update(0, 10, ten.data());
    CHECK(live.download() == ten && flags.size() == 10 && none.size() == 0 && none.flags() != nullptr);
}
void keypoint_table(Context &ctx) {
    DeviceKeypointTable kp(ctx, 3, 5);
    kp.update(2, {1.f, 2.f}, {3.f, 4.f}, {0, 1}, {});
    kp.update(0, {}, {}, {}, {});
    CHECK(kp.size() == 3 && kp.stride() == 5 && kp.octave() != nullptr);
}
void observation_lists(Context &ctx) {
    DeviceKeyframeMapPoints table(ctx, 3, 5, 10);
    DeviceKeypointTable kp(ctx, 3, 5);
    KeyframeSlots slots;
    slots.id = {0, 1, 2};
    MapTables tables{table, slots};
    tables.keypoints = &kp;
    DeviceObservationLists lists(ctx, 2, 4);
    ObservationSelection sel;
    sel.slot = 0;
    g_needRows = 2; g_needObs = 3;
    lists.build(tables, false, sel, 0);                       // fits
    g_needRows = 5; g_needObs = 9;
    lists.build(tables, false, sel, 0);                       // regrows once
    CHECK(lists.rowCount() == 5 && lists.observationCount() == 9);
    CHECK((lists.download(lists.lists().rows, 5) == std::vector<std::int32_t>{0, 1, 2, 3, 4}));
}
void track_table(Context &ctx) {
    DeviceTrackTable tracks(ctx, 10, 0, 4);
    tracks.bind({1, 2}, {0, 3});
    tracks.ensureTrack(3);                                                        // inside the window
    tracks.ensureTrack(4);                                                        // grows to 8
    CHECK(tracks.window() == 8 && tracks.mapPointCount() == 10);
    CHECK((tracks.downloadTrackRows() == std::vector<std::int32_t>{1, -1, -1, 2, -1, -1, -1, -1}));
    CHECK((tracks.downloadMapPointTracks() == std::vector<std::int32_t>{-1, 0, 3, -1, -1, -1, -1, -1, -1, -1}));
}
VocabularyTree one_word_tree() {
    VocabularyTree t;
    t.branchingFactor = 1; t.depthLevels = 1;
    t.parent = {0, 0}; t.wordId = {-1, 0}; t.weight = {0.0, 1.0}; t.descriptor.assign(16, 0u);
    return t;
}
void bow_index(Context &ctx) {
    BowIndex index(ctx, one_word_tree());
    BowVector v;
    FeatureVector fv;
    index.transform(keypoints(1), v, fv);                                         // the first buffers hold 65 keypoints
    index.transform(keypoints(2), v, fv);                                         // fits
    index.transform(keypoints(66), v, fv);                                        // grows
    CHECK(v.size() == 1 && fv[1].size() == 66);
}
void update_descriptors(Context &ctx) {
    const std::vector<int> best = updateDescriptors(ctx, {std::vector<KeyPoint::Descriptor>(2), {}, std::vector<KeyPoint::Descriptor>(1)});
    CHECK(best.size() == 3 && best[0] == 0);
}

struct Scenario {
    const char *name;
    void (*run)(Context &);
    const char *log;                         // of the headers before DeviceArray: the kinds of calls in order, the bytes of every copy
};
const Scenario kScenarios[] = {
    {"DeviceKeyframe", device_keyframe, "a u64 a u8 a u8 a u48 a u2 a u4 a u8 a u8 a u8 a u8 a u8 f f f f f f f f f f f "},
    {"DeviceKeyframePoses", keyframe_poses, "a u288 u96 d288 f "},
    {"DeviceDescriptorPool", descriptor_pool, "a u64 a f f "},
    {"DeviceMapPoints", map_points, "a a a a a u240 u120 u40 u40 u320 u72 u12 u96 f f f f f "},
    {"DeviceKeyframeMapPoints", keyframe_map_points, "a u60 u20 u20 f "},
    {"DeviceMapPointFlags and DeviceMapPointLive", flags_and_live, "a u10 a u2 a u10 u10 d10 f f f "},
    {"DeviceKeypointTable", keypoint_table, "a a a a u60 u60 u60 u60 u8 u8 u8 u8 f f f f "},
    {"DeviceObservationLists", observation_lists,
     "a u60 a a a a u60 u60 u60 u60 a a a a a a a a a a a a f f f f f f f f f f f f a a a a a a a a a a a a d20 f f f f f f f f f f f f f f f f f "},
    {"DeviceTrackTable", track_table, "a u40 a u16 u4 u4 u4 u4 d16 a u32 f d32 d40 f f "},
    {"BowIndex", bow_index, "a a a a u32 d4 d8 d4 u64 d8 d16 d8 f f f f a a a a u2112 d264 d528 d264 f f f f "},
    {"updateDescriptors", update_descriptors, "a u96 a u16 a u12 a d12 f f f f "},
};

void every_owner_without_failure(Context &ctx) {
    for (const Scenario &s : kScenarios) {
        reset_stand_in();
        s.run(ctx);
        CHECK(g_live.empty());
#ifdef DEVICE_ARRAY_CHECK_RECORD
        std::printf("    {\"%s\", ..., \"%s\"},\n", s.name, g_log.c_str());
#else
        if (g_log != s.log) { std::printf("FAILED %s: the call log is\n  %s\nand was\n  %s\n", s.name, g_log.c_str(), s.log); ++g_failures; }
#endif
    }
}

void every_owner_with_each_allocation_failing(Context &ctx) {
    for (const Scenario &s : kScenarios) {
        reset_stand_in();
        s.run(ctx);
        const long allocations = g_allocs;
        for (long k = 0; k <= allocations; ++k) {                                  // k == allocations: no failure after all
            reset_stand_in();
            g_failAt = k;
            const bool threw = throws_runtime_error([&] { s.run(ctx); });
            if (threw != (k < allocations) || !g_live.empty()) {
                std::printf("FAILED %s with allocation %ld of %ld failing: %s, %zu blocks stay live\n", s.name, k, allocations, threw ? "threw" : "did not throw", g_live.size());
                ++g_failures;
                for (auto &b : g_live) std::free(b.first);
                g_live.clear();
            }
        }
    }
}

// after a regrow that failed the lists own nothing and say so: the next build allocates again and succeeds
void observation_lists_recover(Context &ctx) {
    for (long k = 0; k < 12; ++k) {
        reset_stand_in();
        DeviceKeyframeMapPoints table(ctx, 3, 5, 10);
        DeviceKeypointTable kp(ctx, 3, 5);
            KeyframeSlots slots;
        slots.id = {0, 1, 2};
        MapTables tables{table, slots};
        tables.keypoints = &kp;
        const std::size_t others = g_live.size();
        DeviceObservationLists lists(ctx, 2, 4);
        ObservationSelection sel;
        sel.slot = 0;
        g_needRows = 5; g_needObs = 9;
        g_failAt = g_allocs + k;
        CHECK(throws_runtime_error([&] { lists.build(tables, false, sel, 0); }));
        CHECK(g_live.size() == others);
        g_failAt = -1;
        const long before = g_allocs;
        lists.build(tables, false, sel, 0);
        CHECK(g_allocs > before && lists.rowCount() == 5 && g_live.size() == others + 12);
        CHECK((lists.download(lists.lists().rows, 5) == std::vector<std::int32_t>{0, 1, 2, 3, 4}));
    }
    CHECK(g_live.empty());
}
void bow_index_recovers(Context &ctx) {
    for (long k = 0; k < 4; ++k) {
        reset_stand_in();
        BowIndex index(ctx, one_word_tree());
        BowVector v;
        FeatureVector fv;
        index.transform(keypoints(1), v, fv);
        g_failAt = g_allocs + k;
        CHECK(throws_runtime_error([&] { index.transform(keypoints(66), v, fv); }));
        CHECK(g_live.empty());
        g_failAt = -1;
        const long before = g_allocs;
        index.transform(keypoints(2), v, fv);                                     // would fit the first buffers: they are gone, so this allocates
        CHECK(g_allocs == before + 4 && g_live.size() == 4 && fv[1].size() == 2);
    }
    CHECK(g_live.empty());
}
void track_table_keeps_its_window(Context &ctx) {
    reset_stand_in();
    {
        DeviceTrackTable tracks(ctx, 10, 0, 4);
        tracks.bind({1, 2}, {0, 3});
        const std::vector<std::int32_t> window = tracks.downloadTrackRows();
        g_failAt = g_allocs;
        CHECK(throws_runtime_error([&] { tracks.ensureTrack(4); }));
        CHECK(tracks.window() == 4 && tracks.downloadTrackRows() == window && g_live.size() == 2);
        g_failAt = -1;
        tracks.ensureTrack(4);
        CHECK((tracks.downloadTrackRows() == std::vector<std::int32_t>{1, -1, -1, 2, -1, -1, -1, -1}) && g_live.size() == 2);
    }
    CHECK(g_live.empty());
}
void update_descriptors_kernel_failure(Context &ctx) {
    reset_stand_in();
    g_medoidRc = MS_ERR_CAPACITY;
    CHECK(throws_runtime_error([&] { update_descriptors(ctx); }));
    CHECK(g_live.empty() && count_in_log("a ") == 4 && count_in_log("f ") == 4 && count_in_log("d") == 0);
    reset_stand_in();
    g_vocabRc = MS_ERR_INVALID;
    CHECK(throws_runtime_error([&] { bow_index(ctx); }));
    CHECK(g_live.empty() && g_log.empty());
}
}  // namespace

int main() {
    std::setvbuf(stdout, nullptr, _IONBF, 0);            // what was found stays on the screen if a later check aborts
    {
        Context ctx;
#ifndef DEVICE_ARRAY_CHECK_RECORD
        device_array_alone(ctx);
#endif
        every_owner_without_failure(ctx);
        every_owner_with_each_allocation_failing(ctx);
        observation_lists_recover(ctx);
        bow_index_recovers(ctx);
        track_table_keeps_its_window(ctx);
        update_descriptors_kernel_failure(ctx);
    }
    CHECK(g_live.empty());
    if (g_failures) { std::printf("%d checks failed\n", g_failures); return 1; }
    std::printf("device arrays ok: %zu owners\n", sizeof(kScenarios) / sizeof(kScenarios[0]));
    return 0;
}
