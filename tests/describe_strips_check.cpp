// k_describe's launch plan (slam-module_amd/csrc/describe_strips.h) on the CPU: for every combination of
//   frames in {1, 2, 3, 5, 256}, capacity in {1 .. 40, 500, 2000, 2003}, resident blocks in {1, 8, 2048}, forced r in {0 .. 8}
// the plan is built and every block of its grid is decoded and walked as the kernel walks it (wave wv, trip k -> slot0 + wv + 4 k):
//   - every (frame, slot < capacity) is visited by exactly one (block, wave, trip), and nothing else is visited below the capacity;
//   - no strip crosses a frame (a block's slots belong to the frame it decodes to, and its first slot lies inside the frame);
//   - at most four regions, whole frames each, contiguous in blocks and frames, strip lengths falling; the block count within the grid limit;
//   - a forced r gives one region of that r; the automatic plan ends in >= 2 x resident blocks of r = 1, or is all r = 1 when the launch has
//     no more than 2 x resident blocks at r = 1;
//   - decode's multiply-high quotient equals the division, also for block indices up to the grid limit on hand-made regions;
//   - trips() equals the count of a wave's slots below the frame's total, for every total 0 .. capacity (small capacities).
// Arguments out of range are refused.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "describe_strips.h"

namespace ds = describe_strips;

static long long g_checks = 0;
#define CHECK(c, ...) do { ++g_checks; if (!(c)) { std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); return false; } } while (0)

static bool check_plan(int frames, int capacity, int resident, int forced) {
    ds::Plan p{};
    CHECK(ds::build(frames, capacity, resident, forced, p), "frames %d capacity %d resident %d forced %d", frames, capacity, resident, forced);
    CHECK(p.regions >= 1 && p.regions <= ds::kMaxRegions, "regions %d", p.regions);
    CHECK(p.blocks >= 1 && (int64_t)p.blocks <= ds::kGridLimit, "blocks %d", p.blocks);
    int64_t block = 0;
    int frame = 0;
    for (int g = 0; g < p.regions; ++g) {
        const ds::Region &R = p.reg[g];
        CHECK(R.block0 == block && R.frame0 == frame && R.frames >= 1, "region %d starts at block %d frame %d (%d frames)", g, R.block0, R.frame0, R.frames);
        CHECK(R.r >= 1 && R.r <= ds::kMaxStrip && R.bpf == ds::blocks_per_frame(capacity, R.r), "region %d r %d bpf %d", g, R.r, R.bpf);
        CHECK(g == 0 || R.r < p.reg[g - 1].r, "region %d: r %d after %d", g, R.r, p.reg[g - 1].r);
        block += (int64_t)R.frames * R.bpf; frame += R.frames;
    }
    CHECK(block == p.blocks && frame == frames, "%lld blocks, %d frames", (long long)block, frame);
    for (int g = p.regions; g < ds::kMaxRegions; ++g) CHECK((int64_t)p.reg[g].block0 >= (int64_t)p.blocks, "unused region %d reachable", g);
    const int64_t bpf1 = ds::blocks_per_frame(capacity, 1);
    if (forced > 0) CHECK(p.regions == 1 && p.reg[0].r == forced, "forced %d: %d regions, r %d", forced, p.regions, p.reg[0].r);
    else if ((int64_t)frames * bpf1 <= 2ll * resident) CHECK(p.regions == 1 && p.reg[0].r == 1, "small launch: %d regions, r %d", p.regions, p.reg[0].r);
    else {
        const ds::Region &T = p.reg[p.regions - 1];
        CHECK(T.r == 1 && (int64_t)T.frames * T.bpf >= 2ll * resident, "tail r %d, %lld blocks, resident %d", T.r, (long long)T.frames * T.bpf, resident);
    }
    // the walk
    std::vector<uint8_t> seen((size_t)frames * capacity, 0);
    for (int64_t b = 0; b < p.blocks; ++b) {
        const ds::Strip S = ds::decode(p, (uint32_t)b);
        int g = 0;
        while (g + 1 < p.regions && b >= p.reg[g + 1].block0) ++g;
        const int64_t local = b - p.reg[g].block0;
        CHECK(S.frame == p.reg[g].frame0 + (int)(local / p.reg[g].bpf) && S.slot0 == (int)(local % p.reg[g].bpf) * ds::kWaves * p.reg[g].r && S.r == p.reg[g].r,
              "block %lld decodes to frame %d slot %d r %d", (long long)b, S.frame, S.slot0, S.r);
        CHECK(S.frame >= 0 && S.frame < frames && S.slot0 >= 0 && S.slot0 < capacity, "block %lld: frame %d slot0 %d", (long long)b, S.frame, S.slot0);
        for (int wv = 0; wv < ds::kWaves; ++wv) {
            const int n = ds::trips(S.slot0, wv, S.r, capacity);           // (a frame filled to its capacity)
            for (int k = 0; k < n; ++k) {
                const int slot = S.slot0 + wv + ds::kWaves * k;
                CHECK(slot < capacity, "block %lld wave %d trip %d: slot %d", (long long)b, wv, k, slot);
                uint8_t &s = seen[(size_t)S.frame * capacity + slot];
                CHECK(s == 0, "frame %d slot %d visited twice", S.frame, slot);
                s = 1;
            }
            CHECK(n == S.r || S.slot0 + wv + ds::kWaves * n >= capacity, "block %lld wave %d stops at trip %d of %d below the capacity", (long long)b, wv, n, S.r);
        }
    }
    for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "frame %zu slot %zu not visited", i / capacity, i % capacity);
    return true;
}

static bool check_trips(int capacity) {
    for (int r = 1; r <= ds::kMaxStrip; ++r)
        for (int slot0 = 0; slot0 < capacity; slot0 += ds::kWaves * r)
            for (int wv = 0; wv < ds::kWaves; ++wv)
                for (int total = 0; total <= capacity; ++total) {
                    int want = 0;
                    for (int k = 0; k < r; ++k) want += slot0 + wv + ds::kWaves * k < total;
                    CHECK(ds::trips(slot0, wv, r, total) == want, "trips(%d, %d, %d, %d) = %d, want %d", slot0, wv, r, total, ds::trips(slot0, wv, r, total), want);
                }
    return true;
}

// decode's quotient on regions that reach the grid limit (no plan of a real launch is that large, the arithmetic must not care)
static bool check_quotient() {
    const int bpfs[] = {1, 2, 3, 5, 7, 63, 64, 125, 250, 500, 501, 65535, 65536, 1000003, 0x3FFFFFFF, 0x7FFFFFFF};
    for (int bpf : bpfs) {
        ds::Plan p{};
        for (int g = 0; g < ds::kMaxRegions; ++g) p.reg[g] = ds::Region{0x7FFFFFFF, 0, 0, 1, 1, 0xFFFFFFFFu};
        p.reg[0] = ds::Region{0, 0, (int32_t)(ds::kGridLimit / bpf), 1, bpf, 0xFFFFFFFFu / (uint32_t)bpf};
        p.regions = 1; p.blocks = (int32_t)((int64_t)p.reg[0].frames * bpf);
        uint32_t b = 0;
        for (int i = 0; i < 500000; ++i) {
            const uint32_t probes[3] = {b % (uint32_t)p.blocks, (uint32_t)p.blocks - 1 - b % (uint32_t)p.blocks, (uint32_t)((uint64_t)(b % (uint32_t)p.reg[0].frames) * bpf + (i & 1 ? bpf - 1 : 0))};
            for (uint32_t x : probes) {
                const ds::Strip S = ds::decode(p, x);
                CHECK(S.frame == (int32_t)(x / (uint32_t)bpf) && (uint32_t)S.slot0 == (x % (uint32_t)bpf) * 4u, "bpf %d block %u: frame %d slot0 %d", bpf, x, S.frame, S.slot0);
            }
            b = b * 1664525u + 1013904223u;
        }
    }
    return true;
}

int main() {
    const int frames_set[] = {1, 2, 3, 5, 256}, resident_set[] = {1, 8, 2048};
    std::vector<int> caps;
    for (int c = 1; c <= 40; ++c) caps.push_back(c);
    caps.push_back(500); caps.push_back(2000); caps.push_back(2003);
    long long plans = 0;
    for (int frames : frames_set) for (int cap : caps) for (int res : resident_set) for (int forced = 0; forced <= ds::kMaxStrip; ++forced) {
        if (!check_plan(frames, cap, res, forced)) return 1;
        ++plans;
    }
    for (int cap = 1; cap <= 40; ++cap) if (!check_trips(cap)) return 1;
    if (!check_quotient()) return 1;
    ds::Plan p{};
    if (ds::build(0, 10, 8, 0, p) || ds::build(1, 0, 8, 0, p) || ds::build(1, 10, 0, 0, p) || ds::build(1, 10, 8, -1, p) || ds::build(1, 10, 8, 9, p) || ds::build(1, 10, 8, 0, p, 3)) {
        std::printf("FAIL: arguments out of range accepted\n"); return 1;
    }
    if (ds::build(0x7FFFFFFF, 2003, 8, 1, p)) { std::printf("FAIL: a grid beyond the limit accepted\n"); return 1; }
    // the flagship launch, for the record
    ds::build(256, 2000, 2048, 0, p);
    std::printf("256 frames x 2000 slots on 2048 resident blocks:");
    for (int g = 0; g < p.regions; ++g) std::printf("  r=%d: %d frames, %d blocks", p.reg[g].r, p.reg[g].frames, p.reg[g].frames * p.reg[g].bpf);
    std::printf("  (%d blocks, %d at r = 1 throughout)\n", p.blocks, 256 * ds::blocks_per_frame(2000, 1));
    std::printf("strips ok: %lld plans, %lld checks\n", plans, g_checks);
    return 0;
}
