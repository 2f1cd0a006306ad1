// The launch plan of k_describe (orb.hip): which workgroup describes which output slots.  Plain C++, no HIP: the library builds the
// plan from it, the kernel decodes its block index with it, and tests/describe_strips_check.cpp checks both on the CPU
// (remap, which deals the logical blocks to the physical ones: tests/describe_order_check.cpp).
//
// A workgroup is four waves.  A wave pays its setup once (tables to LDS, lane tables, the frame's counts and pointers, one block barrier)
// and then walks a STRIP of r keypoints, 1 <= r <= 8, one after another in the same registers and the same LDS slab: wave wv of the block
// whose first slot is s0 takes slots s0 + wv, s0 + wv + 4, ..., s0 + wv + 4 (r - 1).  A block therefore covers 4 r consecutive slots of ONE
// frame and its four waves stay on neighbouring slots.
//
// Blocks are dispatched in index order, so with one r for the whole launch the device would drain for up to a strip's duration at the
// end.  The plan is a short list of REGIONS, each a run of whole frames with its own r, long strips first: r = kLongStrip, then every
// halved r down to 2 with as many frames as give one device-full of blocks each, and at the end frames with r = 1 whose blocks number
// at least twice what the device holds at once.  A block of the long region that starts last still has (4 +) 2 + 2 keypoint durations of
// shorter work behind it.  A launch that has no more than those two device-fulls of blocks at r = 1 is all r = 1.
// Long strips are not free: the slots the device works on at one time span r times as many frames, and their pyramids share the caches
// (remap, below, keeps a frame's blocks on one L2, which is what lets the long region run at 8).
#pragma once
#include <cstdint>

namespace describe_strips {

constexpr int kWaves = 4;            // waves of a workgroup = slots between two keypoints of a wave
constexpr int kMaxStrip = 8;         // longest strip (the kernel's per-wave tables hold this many keypoints)
constexpr int kMaxRegions = 4;
constexpr int kLongStrip = 8;        // r of the automatic plan's first region (measured: with remap 8 beats 4 and 2; without it 4 beat 8)
constexpr int64_t kGridLimit = 0x7FFFFFFF;

// Blocks [block0, next region's block0) describe frames frame0 .., bpf blocks each.  inv = (2^32 - 1) / bpf: the quotient by one
// multiply-high and one correction, exact for every block index below the grid limit (decode).
struct Region { int32_t block0, frame0, frames, r, bpf; uint32_t inv; };
struct Plan { Region reg[kMaxRegions]; int32_t regions, blocks; };
struct Strip { int32_t frame, slot0, r; };

constexpr int blocks_per_frame(int capacity, int r) { return (capacity + kWaves * r - 1) / (kWaves * r); }
constexpr int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// frames >= 1 frames of `capacity` slots each on a device that holds `resident` blocks of the kernel at once.  forced_r = 0: the automatic
// plan; 1 .. 8: every block walks strips of forced_r, no taper.  False (plan untouched) for arguments out of range or a grid beyond the limit.
inline bool build(int frames, int capacity, int64_t resident, int forced_r, Plan &out, int long_r = kLongStrip) {
    if (frames < 1 || capacity < 1 || resident < 1 || forced_r < 0 || forced_r > kMaxStrip) return false;
    if (long_r != 2 && long_r != 4 && long_r != 8) return false;
    int r_of[kMaxRegions], n_of[kMaxRegions], n = 0;                 // long strips first
    const int64_t bpf1 = blocks_per_frame(capacity, 1);
    if (forced_r > 0) { r_of[0] = forced_r; n_of[0] = frames; n = 1; }
    else if ((int64_t)frames * bpf1 <= 2 * resident) { r_of[0] = 1; n_of[0] = frames; n = 1; }
    else {
        // shared out from the end of the launch: the r = 1 tail first, then one device-full for each halved strip, the rest to the long strips
        int rest = frames, tail_r[kMaxRegions], tail_n[kMaxRegions], m = 0;
        for (int r = 1; r < long_r && rest > 0; r *= 2) {
            const int64_t want = ceil_div((r == 1 ? 2 : 1) * resident, blocks_per_frame(capacity, r));
            const int take = (int)(want < rest ? want : rest);
            tail_r[m] = r; tail_n[m] = take; ++m; rest -= take;
        }
        if (rest > 0) { r_of[n] = long_r; n_of[n] = rest; ++n; }
        while (m > 0) { --m; r_of[n] = tail_r[m]; n_of[n] = tail_n[m]; ++n; }
    }
    Plan p{};
    int64_t block = 0;
    int frame = 0;
    for (int g = 0; g < kMaxRegions; ++g) {
        if (g < n) {
            const int bpf = blocks_per_frame(capacity, r_of[g]);
            p.reg[g] = Region{(int32_t)block, frame, n_of[g], r_of[g], bpf, 0xFFFFFFFFu / (uint32_t)bpf};
            block += (int64_t)n_of[g] * bpf; frame += n_of[g];
            if (block > kGridLimit) return false;
        } else p.reg[g] = Region{0x7FFFFFFF, frame, 0, 1, 1, 0xFFFFFFFFu};       // never selected: no block index reaches it
    }
    p.regions = n; p.blocks = (int32_t)block;
    out = p;
    return true;
}

// Block index -> (frame, first slot, r): compares and selects on the region records, one multiply-high.  q = mulhi(local, inv) is
// floor(local / bpf) or one less (inv * bpf lies in (2^32 - 1 - bpf, 2^32 - 1], so local * inv / 2^32 falls short of local / bpf by less
// than local * (bpf + 1) / (bpf * 2^32) <= local / 2^31 < 1).
constexpr Strip decode(const Plan &p, uint32_t block) {
    // (field by field: selects between scalars.  Selecting a whole record makes the kernel's compiler index a copy of the plan in memory)
    uint32_t block0 = (uint32_t)p.reg[0].block0, bpf = (uint32_t)p.reg[0].bpf, inv = p.reg[0].inv;
    int32_t frame0 = p.reg[0].frame0, r = p.reg[0].r;
    for (int k = 1; k < kMaxRegions; ++k) {
        const bool in = block >= (uint32_t)p.reg[k].block0;
        block0 = in ? (uint32_t)p.reg[k].block0 : block0; bpf = in ? (uint32_t)p.reg[k].bpf : bpf; inv = in ? p.reg[k].inv : inv;
        frame0 = in ? p.reg[k].frame0 : frame0; r = in ? p.reg[k].r : r;
    }
    const uint32_t local = block - block0;
    uint32_t q = (uint32_t)(((uint64_t)local * inv) >> 32), s = local - q * bpf;
    if (s >= bpf) { ++q; s -= bpf; }
    return Strip{frame0 + (int32_t)q, (int32_t)(s * (uint32_t)(kWaves * r)), r};
}

// Physical block index -> logical block index (the one decode takes): which workgroup describes which strip, for the caches' sake alone.
// The dispatcher deals consecutive workgroups round robin to the device's eight XCDs, each with an L2 of its own, so with the identity the
// blocks of a frame land on all eight L2s and every L2 pulls every frame's pyramid.  Here each region of the plan is permuted within itself:
// the blocks whose index inside the region is x modulo kXcds get ONE contiguous run of logical blocks -- whole frames one after another -- and
// walk it in rising order.  With n = 8 q + rem blocks in the region the run of label x starts at x (q + 1) for x < rem and at
// rem (q + 1) + (x - rem) q behind them; it holds q + (x < rem) blocks, one for every physical block of that label.  A bijection of every
// region onto itself for every n >= 1 (n < 8: the identity), so the regions still run in plan order and the taper keeps its meaning.
// Nothing depends on where a block really runs: a dispatcher that deals otherwise only loses the reuse.
constexpr int kXcds = 8;
constexpr uint32_t remap(const Plan &p, uint32_t block) {
    // (field by field, as in decode.  A region ends where the next one starts; the last one of the plan at the block count -- an unused record's
    // block0 is not below it)
    uint32_t block0 = (uint32_t)p.reg[0].block0, end = (uint32_t)p.reg[1].block0;
    for (int k = 1; k < kMaxRegions; ++k) {
        const bool in = block >= (uint32_t)p.reg[k].block0;
        block0 = in ? (uint32_t)p.reg[k].block0 : block0;
        const uint32_t next = k + 1 < kMaxRegions ? (uint32_t)p.reg[k + 1 < kMaxRegions ? k + 1 : k].block0 : (uint32_t)p.blocks;
        end = in ? next : end;
    }
    end = end < (uint32_t)p.blocks ? end : (uint32_t)p.blocks;
    const uint32_t local = block - block0, n = end - block0;
    const uint32_t x = local % kXcds, j = local / kXcds, q = n / kXcds, rem = n % kXcds;
    const uint32_t start = x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q;
    return block0 + start + j;
}

// Trips of wave wv of a strip that starts at slot0 in a frame of `total` keypoints: its slots slot0 + wv + 4 k < total, k < r.
constexpr int trips(int slot0, int wv, int r, int total) {
    const int t = (total - (slot0 + wv) + kWaves - 1) >> 2;         // (arithmetic shift: <= 0 for a wave at or beyond the total)
    return t < 0 ? 0 : (t < r ? t : r);
}

}   // namespace describe_strips
