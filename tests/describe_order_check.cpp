// Which workgroup of k_describe takes which keypoint (slam-module_amd/csrc/describe_strips.h: remap; describe_order.h: key) on the CPU.
//   remap   for the plan set of describe_strips_check (frames {1, 2, 3, 5, 256} x capacity {1 .. 40, 500, 2000, 2003} x resident {1, 8, 2048} x
//           forced r 0 .. 8) and hand-made plans whose regions hold 1 .. 40 blocks each:
//             - a bijection of every region onto itself (so decode(remap(b)) still visits every block once, regions in plan order);
//             - the physical blocks of a region with the same index modulo 8 map to one contiguous, rising run of logical blocks, the runs in
//               label order, their lengths differing by at most one;
//             - regions of fewer than 8 blocks (the identity) and of 8 k + 1 .. 8 k + 7 blocks both occur.
//   key     a strict total order on (x, y, index): distinct for distinct indices, band-major, left to right in even bands and right to left in
//           odd ones, ties of (band, x) by index, the extremes (0 and 32767, index 4095) inside 64 bits; sorting hand-made levels with equal
//           keys by key() gives the order written out by hand, and pack / level_of / slot_of round-trip.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "describe_order.h"
#include "describe_strips.h"

namespace ds = describe_strips;
namespace dord = describe_order;

static long long g_checks = 0;
#define CHECK(c, ...) do { ++g_checks; if (!(c)) { std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); return false; } } while (0)

static bool g_small = false, g_ragged[8] = {};

static bool check_remap(const ds::Plan &p) {
    std::vector<uint8_t> hit((size_t)p.blocks, 0);
    for (int g = 0; g < p.regions; ++g) {
        const int64_t b0 = p.reg[g].block0, b1 = g + 1 < p.regions ? p.reg[g + 1].block0 : p.blocks, n = b1 - b0;
        CHECK(n >= 1, "region %d holds %lld blocks", g, (long long)n);
        if (n < ds::kXcds) g_small = true;
        g_ragged[n % ds::kXcds] = true;
        int64_t run_start[ds::kXcds], run_len[ds::kXcds];
        for (int x = 0; x < ds::kXcds; ++x) { run_start[x] = -1; run_len[x] = 0; }
        for (int64_t b = b0; b < b1; ++b) {
            const int64_t m = ds::remap(p, (uint32_t)b);
            CHECK(m >= b0 && m < b1, "block %lld of region %d [%lld, %lld) maps to %lld", (long long)b, g, (long long)b0, (long long)b1, (long long)m);
            CHECK(hit[(size_t)m] == 0, "logical block %lld taken twice", (long long)m);
            hit[(size_t)m] = 1;
            const int x = (int)((b - b0) % ds::kXcds);
            if (run_start[x] < 0) run_start[x] = m;
            CHECK(m == run_start[x] + run_len[x], "label %d: block %lld maps to %lld, its run stands at %lld", x, (long long)b, (long long)m, (long long)(run_start[x] + run_len[x]));
            ++run_len[x];
            if (n < ds::kXcds) CHECK(m == b, "a region of %lld blocks is not left alone", (long long)n);
        }
        int64_t at = b0;                                              // the runs tile the region in label order
        for (int x = 0; x < ds::kXcds; ++x) {
            if (run_len[x] == 0) continue;
            CHECK(run_start[x] == at, "label %d starts at %lld, want %lld", x, (long long)run_start[x], (long long)at);
            CHECK(run_len[x] == n / ds::kXcds + (x < n % ds::kXcds), "label %d holds %lld of %lld blocks", x, (long long)run_len[x], (long long)n);
            at += run_len[x];
        }
        CHECK(at == b1, "runs end at %lld, region at %lld", (long long)at, (long long)b1);
    }
    for (size_t i = 0; i < hit.size(); ++i) CHECK(hit[i] == 1, "logical block %zu not taken", i);
    return true;
}

static ds::Plan hand_plan(const int *blocks, int regions) {       // regions of the given block counts, one frame each (bpf = the count)
    ds::Plan p{};
    int32_t block = 0;
    for (int g = 0; g < ds::kMaxRegions; ++g) {
        if (g < regions) { p.reg[g] = ds::Region{block, g, 1, ds::kMaxStrip >> g, blocks[g], 0xFFFFFFFFu / (uint32_t)blocks[g]}; block += blocks[g]; }
        else p.reg[g] = ds::Region{0x7FFFFFFF, regions, 0, 1, 1, 0xFFFFFFFFu};
    }
    p.regions = regions; p.blocks = block;
    return p;
}

struct Det { int x, y; };

static bool check_level(const std::vector<Det> &d, const std::vector<int> &want) {
    std::vector<uint64_t> k;
    for (size_t i = 0; i < d.size(); ++i) k.push_back(dord::key(d[i].x, d[i].y, (int)i));
    std::sort(k.begin(), k.end());
    for (size_t i = 0; i + 1 < k.size(); ++i) CHECK(k[i] < k[i + 1], "keys %zu and %zu equal", i, i + 1);
    CHECK(k.size() == want.size(), "%zu keys", k.size());
    for (size_t i = 0; i < k.size(); ++i) CHECK(dord::index_of(k[i]) == want[i], "position %zu holds detection %d, want %d", i, dord::index_of(k[i]), want[i]);
    return true;
}

static bool check_key() {
    // band-major; even bands by rising x, odd bands by falling x; (band, x) ties by index whatever y is inside the band
    CHECK(dord::key(32767, 31, 4095) < dord::key(0, 32, 0), "band 0 before band 1");
    CHECK(dord::key(5, 0, 7) < dord::key(6, 31, 0) && dord::key(6, 40, 0) < dord::key(5, 63, 0), "direction alternates");
    CHECK(dord::key(9, 3, 1) < dord::key(9, 30, 2) && dord::key(9, 30, 1) < dord::key(9, 3, 2), "ties by index");
    CHECK(dord::key(0, 0, 0) == 0 && dord::key(0, 32767, 4095) == ((1ull << 37) - 1), "extremes: %llx", (unsigned long long)dord::key(0, 32767, 4095));
    const int xs[] = {0, 1, 22, 23, 640, 32766, 32767}, ys[] = {0, 31, 32, 33, 63, 64, 719, 32736, 32767}, is[] = {0, 1, 255, 256, 4095};
    std::vector<uint64_t> all;
    for (int x : xs) for (int y : ys) for (int i : is) {
        const uint64_t k = dord::key(x, y, i);
        CHECK(dord::index_of(k) == i && (k >> 27) == (uint64_t)(y >> 5), "key(%d, %d, %d)", x, y, i);
        all.push_back(k);
    }
    // a function of (band, x, index) alone, and injective in them
    std::sort(all.begin(), all.end());
    size_t distinct = std::unique(all.begin(), all.end()) - all.begin();
    std::vector<int> bands;
    for (int y : ys) bands.push_back(y >> 5);
    std::sort(bands.begin(), bands.end());
    const size_t nb = std::unique(bands.begin(), bands.end()) - bands.begin();
    CHECK(distinct == 7 * nb * 5, "%zu distinct keys, want %zu", distinct, 7 * nb * 5);
    // hand-made levels
    if (!check_level({}, {})) return false;
    if (!check_level({{7, 7}}, {0})) return false;
    if (!check_level({{50, 10}, {50, 20}, {50, 0}, {50, 31}}, {0, 1, 2, 3})) return false;                       // one band, one x: the index decides
    if (!check_level({{50, 40}, {50, 33}, {60, 35}, {40, 63}, {60, 32}}, {2, 4, 0, 1, 3})) return false;         // an odd band: right to left, ties by index
    if (!check_level({{10, 70}, {300, 5}, {10, 5}, {300, 40}, {10, 40}, {10, 6}, {300, 64}}, {2, 5, 1, 3, 4, 0, 6})) return false;   // three bands, the walk turns round
    // pack
    CHECK(dord::level_of(dord::pack(15, (1 << 24) - 1)) == 15 && dord::slot_of(dord::pack(15, (1 << 24) - 1)) == (1 << 24) - 1, "pack at the limits");
    CHECK(dord::level_of(dord::pack(0, 0)) == 0 && dord::slot_of(dord::pack(3, 2002)) == 2002 && dord::level_of(dord::pack(3, 2002)) == 3, "pack");
    CHECK((dord::kDefaultMode & ~dord::kModeMask) == 0, "default mode %d", dord::kDefaultMode);
    return true;
}

int main() {
    const int frames_set[] = {1, 2, 3, 5, 256}, resident_set[] = {1, 8, 2048};
    std::vector<int> caps;
    for (int c = 1; c <= 40; ++c) caps.push_back(c);
    caps.push_back(500); caps.push_back(2000); caps.push_back(2003);
    long long plans = 0;
    for (int frames : frames_set) for (int cap : caps) for (int res : resident_set) for (int forced = 0; forced <= ds::kMaxStrip; ++forced) {
        ds::Plan p{};
        if (!ds::build(frames, cap, res, forced, p)) { std::printf("FAIL: build(%d, %d, %d, %d)\n", frames, cap, res, forced); return 1; }
        if (!check_remap(p)) { std::printf("  in plan frames %d capacity %d resident %d forced %d\n", frames, cap, res, forced); return 1; }
        ++plans;
    }
    for (int long_r : {2, 8}) { ds::Plan p{}; if (!ds::build(256, 2000, 2048, 0, p, long_r) || !check_remap(p)) return 1; ++plans; }
    for (int a = 1; a <= 40; ++a) for (int regions = 1; regions <= ds::kMaxRegions; ++regions) {
        const int blocks[ds::kMaxRegions] = {a, (a * 7) % 23 + 1, (a * 5) % 17 + 1, (a * 3) % 9 + 1};
        if (!check_remap(hand_plan(blocks, regions))) { std::printf("  in hand-made plan a = %d, %d regions\n", a, regions); return 1; }
        ++plans;
    }
    if (!g_small) { std::printf("FAIL: no region of fewer than 8 blocks\n"); return 1; }
    for (int x = 0; x < ds::kXcds; ++x) if (!g_ragged[x]) { std::printf("FAIL: no region of 8 k + %d blocks\n", x); return 1; }
    if (!check_key()) return 1;
    std::printf("order ok: %lld plans, %lld checks\n", plans, g_checks);
    return 0;
}
