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
