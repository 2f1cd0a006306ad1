// The vertical pass of k_resize<false> (orb.hip) and the packing of its four pixels.  Plain C++, host- and device-callable: the kernel calls
// these functions, and tests/resize_vpass_check.cpp checks them on the CPU, exhaustively, against the form they replace:
//
//     v = ((b0 * (r0 >> 4) >> 16) + (b1 * (r1 >> 4) >> 16) + 2) >> 2,     r = p * a0 + p' * a1 (the horizontal pass, v_dot2_u32_u16)
//
// with taps a0 + a1 = 2048 +- 1, b0 + b1 = 2048 +- 1, each in 0 .. 2048, and bytes p, p'.  Three vector instructions per pixel instead of five:
//   - the column taps are shifted up by 4 once per lane (both halves of the dword at once: a <= 2048 keeps a << 4 inside 16 bits), so the
//     horizontal pass delivers 16 r, and (r >> 4) << 8 is one AND with 0xFFFFFF00 where r >> 4 was one shift;
//   - with the row tap shifted up by 8 (a scalar, once per row), (b * (r >> 4)) >> 16 is the HIGH half of a 24 x 24-bit product:
//     (b << 8) < 2^20 and ((r >> 4) << 8) < 2^23, one v_mul_hi_u32_u24 where a v_mul_u32_u24 and a shift were;
//   - the four sums (<= 1023: no saturation) are shifted down by 2 as two packed 16-bit pairs and their low bytes gathered by one v_perm_b32.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RVPASS_HD __host__ __device__ __forceinline__
#else
#define RVPASS_HD inline
#endif

namespace resize_vpass {

constexpr uint32_t kPackSelector = 0x06040200u;      // v_perm_b32: byte 0 of each 16-bit half of (second operand, first operand)

// the column's tap pair (a0 | a1 << 16) as the horizontal pass takes it: both taps times 16 in one shift of the dword
RVPASS_HD uint32_t preshift_taps(uint32_t a01) { return a01 << 4; }
// the row tap as the vertical pass takes it
RVPASS_HD uint32_t row_tap(uint32_t b) { return b << 8; }
// dot = 16 r from the pre-shifted taps  ->  (r >> 4) << 8
RVPASS_HD uint32_t f8(uint32_t dot) { return dot & 0xFFFFFF00u; }

// High 32 bits of the product of the operands' low 24 bits (v_mul_hi_u32_u24); on the device `a` is wave-uniform (the row tap).  The compiler has no
// builtin for the instruction (__has_builtin(__builtin_amdgcn_mul_hi_u24) is false) and matches the 64-bit expression below only where it can prove both
// operands below 2^24 inside one basic block: behind k_resize's scalar branches it emitted the two masks (two v_and_b32 per product) or a full
// v_mul_hi_u32 + v_mad_u64_u32 pair instead, so the device names the instruction.
RVPASS_HD uint32_t mul_hi_u24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_mul_hi_u32_u24_e32 %0, %1, %2" : "=v"(r) : "s"(a), "v"(b));
    return r;
#else
    return (uint32_t)(((uint64_t)(a & 0xFFFFFFu) * (uint64_t)(b & 0xFFFFFFu)) >> 32);
#endif
}

// the sum of a pixel before its last shift: (b0 * (r0 >> 4) >> 16) + (b1 * (r1 >> 4) >> 16) + 2, from row_tap() and f8() operands
RVPASS_HD uint32_t vsum(uint32_t b0_8, uint32_t f0_8, uint32_t b1_8, uint32_t f1_8) { return mul_hi_u24(b0_8, f0_8) + mul_hi_u24(b1_8, f1_8) + 2u; }

// v_perm_b32 for the selector bytes used here (0 .. 7: bytes of {hi, lo}; >= 0x0C: zero)
RVPASS_HD uint32_t perm_b32(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t src = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = (sel >> (8 * i)) & 255u;
        if (s < 8) out |= (uint32_t)((src >> (8 * s)) & 255u) << (8 * i);
    }
    return out;
#endif
}

// four sums s <= 1023  ->  the dword of their (s >> 2) bytes: two 16-bit pairs, each shifted down by 2 in both halves at once, one byte gather
RVPASS_HD uint32_t pack4(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short pair_t __attribute__((ext_vector_type(2)));
    const pair_t p01 = __builtin_bit_cast(pair_t, s0 | (s1 << 16)) >> (unsigned short)2, p23 = __builtin_bit_cast(pair_t, s2 | (s3 << 16)) >> (unsigned short)2;
    return perm_b32(__builtin_bit_cast(uint32_t, p23), __builtin_bit_cast(uint32_t, p01), kPackSelector);
#else
    const uint32_t p01 = s0 | (s1 << 16), p23 = s2 | (s3 << 16);
    const uint32_t q01 = ((p01 & 0xFFFFu) >> 2) | ((p01 >> 16) >> 2) << 16, q23 = ((p23 & 0xFFFFu) >> 2) | ((p23 >> 16) >> 2) << 16;     // v_pk_lshrrev_b16
    return perm_b32(q23, q01, kPackSelector);
#endif
}

}  // namespace resize_vpass
