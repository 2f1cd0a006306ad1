// hamming_fp4.h -- operand encoding of k_hamming_mfma (match.hip): 256-bit descriptors as FP4 (E2M1) nibbles for
// v_mfma_scale_f32_32x32x64_f8f6f4.  Plain C++ so that a CPU program can check it (tests/hamming_fp4_check.cpp).
//
// A 32x32 tile of distances is four k-steps of 64 bits.  Slot rule (the same for queries and targets): descriptor bit i, i.e. bit b = i & 31
// of word wi = i >> 5, sits in k-step wi >> 1, lane half wi & 1, dword b & 3 of the lane's four operand dwords, nibble b >> 2 of that dword.
// Both expansions are then one shift and one mask per dword: (w >> j) & 0x11111111 puts bits j, j + 4, ..., j + 28 into bit 0 of the eight nibbles.
//   target nibble 0b0001 = 0.5, A scale 2^1               -> 0 / 1
//   query  nibble 0b0010 | bit << 3 = +1 / -1, B scale 2^4 -> +16 / -16, so the accumulator is 16 * dot and its low four bits are free for a row tag
// hamming(q, t) = popcount(q) + sum_k t_k * (1 - 2 q_k).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HM4_HD __host__ __device__ __forceinline__
#else
#define HM4_HD inline
#endif

// E8M0 scale bytes (value 2^(e - 127)), the same in all four bytes of the scale operand so that every op_sel reads it
constexpr uint32_t kHm4ScaleA = 0x80808080u;      // 2^1
constexpr uint32_t kHm4ScaleB = 0x83838383u;      // 2^4
constexpr int kHm4Steps = 4;                      // k-steps (MFMAs) per 256-bit tile

struct Hm4Slot { int step, half, dword, nibble; };
HM4_HD Hm4Slot hm4_slot(int bit) {
    const int wi = bit >> 5, b = bit & 31;
    return Hm4Slot{wi >> 1, wi & 1, b & 3, b >> 2};
}
// operand dword j (0..3) of the lane half that owns descriptor word w
HM4_HD uint32_t hm4_target_dword(uint32_t w, int j) { return (w >> j) & 0x11111111u; }
HM4_HD uint32_t hm4_query_dword(uint32_t w, int j) { return ((j < 3 ? w << (3 - j) : w) & 0x88888888u) | 0x22222222u; }

// ---- 32-bit keys straight from the accumulator (k_hamming_mfma<true>: sets of at most kHmKeyMaxRows targets) ----
// With the B scale 2^13 the accumulator is S * dot, S = 2^13, and the chain starts from 2^23 + 256 S + rel0: every partial sum is an integer in
// [2^23, 2^24), where the float's mantissa field IS the integer, so the register's bit pattern is  kHmKeyBase + S * (dot + 256) + rel  -- a 32-bit key
// that orders by (distance, rel) as it stands.  rel0 = S - 32 + row-in-tile, and before a tile's keys are pushed the kept best / second lose 32:
// older rows keep smaller rel (the lowest row wins a tie), rel stays >= 0 for 256 tiles, and row = rel - S + 32 * (tiles seen).
constexpr uint32_t kHm4ScaleBKey = 0x8C8C8C8Cu;   // 2^13
constexpr int kHmKeyShift = 13;
constexpr uint32_t kHmKeyS = 1u << kHmKeyShift;
constexpr int kHmKeyMaxRows = (int)kHmKeyS;       // 256 tiles of 32 rows: rel of the first tile's rows ends at 0 .. 31
constexpr uint32_t kHmKeyBase = 0x4B000000u;      // bit pattern of 2^23
constexpr uint32_t kHmKeyNone = 0xFFFFFFFFu;      // empty slot; ageing leaves it above every real key (< 0x4C000000)

HM4_HD int hm_key_row_in_tile(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }            // accumulator register r of lane half h
HM4_HD float hm_key_start(int r, int h) { return 8388608.0f + (float)(256u * kHmKeyS) + (float)((int)kHmKeyS - 32 + hm_key_row_in_tile(r, h)); }
HM4_HD uint32_t hm_key_umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
HM4_HD uint32_t hm_key_umax(uint32_t a, uint32_t b) { return a < b ? b : a; }
HM4_HD void hm_key_age(uint32_t &best, uint32_t &second) { best -= 32u; second -= 32u; }
// two new keys into the sorted pair best <= second: v_min3_u32, v_med3_u32, v_min_u32
HM4_HD void hm_key_push2(uint32_t &best, uint32_t &second, uint32_t k0, uint32_t k1) {
    const uint32_t med = hm_key_umin(hm_key_umax(k0, k1), hm_key_umax(hm_key_umin(k0, k1), best));     // median of (best, k0, k1), in the form the compiler selects v_med3_u32 from
    second = hm_key_umin(second, med);
    best = hm_key_umin(hm_key_umin(best, k0), k1);
}
HM4_HD bool hm_key_empty(uint32_t key) { return key >= 0x80000000u; }
HM4_HD int hm_key_dot256(uint32_t key) { return (int)((key - kHmKeyBase) >> kHmKeyShift); }       // dot + 256
HM4_HD int hm_key_row(uint32_t key, int tiles_seen) { return (int)((key - kHmKeyBase) & (kHmKeyS - 1u)) - (int)kHmKeyS + 32 * tiles_seen; }
