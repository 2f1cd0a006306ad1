// The order in which k_describe (orb.hip) visits a level's detections, and the switch for it.  Plain C++, no HIP: k_slots sorts by the key,
// tests/describe_order_check.cpp checks it on the CPU.
//
// k_select leaves a level's detections in score order, which is spatially random: consecutive output slots -- the four waves of a block, the
// keypoints of a wave's strip, the blocks that share an L2 (describe_strips::remap) -- fetch windows from all over the level.  k_slots
// therefore hands the slots out in a spatial order: row bands of kBandRows rows from the top, inside a band by x, every second band from
// right to left, so that the walk turns round at a band's end instead of jumping back across the level.  Only the VISIT order changes: the table entry
// of visit position p carries the output slot of its detection, and that stays where score order put it.
#pragma once
#include <cstdint>

namespace describe_order {

constexpr int kRemap = 1;            // mode bit 0: describe_strips::remap in front of the block decode
constexpr int kSpatial = 2;          // mode bit 1: k_slots orders a level's visit positions by key()
constexpr int kModeMask = kRemap | kSpatial;
// Measured on 256 x 720p (profiles/r09_a_ab_describe_order.txt): the remap cuts the kernel's L2-miss traffic to 31 % and its time by 2 % (4.4 % with the
// long strips of 8 it makes affordable); the spatial order on top takes another 10 - 35 % off the traffic and 0 .. 0.006 ms off the kernel, and costs
// 0.007 ms in k_slots: not below the remap alone in any run, so it stays a switch and is off.
constexpr int kDefaultMode = kRemap;

constexpr int kBandShift = 5, kBandRows = 1 << kBandShift;
constexpr int kCoordBits = 15, kIndexBits = 12;      // coordinates up to 32767 (ms_orb_create), up to 4096 detections in a level

// A strict total order on a level's detections: (band, x along the band's direction, index in the level).  0 <= x, y <= 32767,
// 0 <= index < 4096: 10 + 15 + 12 bits, and the index is the key's low kIndexBits bits.
constexpr int kMaxBands = 1 << (kCoordBits - kBandShift);
constexpr uint32_t band_of(int y) { return (uint32_t)y >> kBandShift; }
// the key's part below the band, 27 bits: distinct inside a band, which is all k_slots compares (it buckets by band first)
constexpr uint32_t in_band_key(int x, uint32_t band, int index) {
    const uint32_t along = (band & 1u) ? (uint32_t)((1 << kCoordBits) - 1 - x) : (uint32_t)x;
    return (along << kIndexBits) | (uint32_t)index;
}
constexpr uint64_t key(int x, int y, int index) {
    return ((uint64_t)band_of(y) << (kCoordBits + kIndexBits)) | in_band_key(x, band_of(y), index);
}
constexpr int index_of(uint64_t k) { return (int)(k & ((1u << kIndexBits) - 1)); }

// A table entry's second dword: the detection's level and its output slot (slots stay below 2^24: ms_orb_create)
constexpr int kSlotShift = 8;
constexpr uint32_t pack(int level, int slot) { return (uint32_t)level | ((uint32_t)slot << kSlotShift); }
constexpr int level_of(uint32_t e) { return (int)(e & ((1u << kSlotShift) - 1)); }
constexpr int slot_of(uint32_t e) { return (int)(e >> kSlotShift); }

}   // namespace describe_order
