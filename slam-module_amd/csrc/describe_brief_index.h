// From a steered BRIEF point (row, column as floats, |v| <= 19 by the pattern's radius) to its byte in k_describe's 39 x 39 blurred patch (40-byte
// rows, the keypoint at (19, 19)): index = 40 (rint(row) + 19) + rint(column) + 19.  Plain C++, host- and device-callable: the kernel calls these
// functions, and tests/describe_brief_index_check.cpp checks them on the CPU against the form they replace (__float2int_rn per coordinate, two
// integer adds of 19, a multiply-add).
//
// Rounding is one more float add: for |v| < 2^22 the float v + 1.5 * 2^23 lies in [2^23, 2^24), where the spacing is 1, so the add itself rounds
// v to an integer -- to nearest, ties to even, as v_rndne_f32 / __float2int_rn do -- and the result's bits are 0x4B400000 + rint(v).  The
// conversion to an integer, the + 19 of either coordinate and the patch base then fold into one constant behind one 24-bit multiply-add:
//     umul24(Rbits, 40) takes the low 24 bits of Rbits = 0x400000 + r > 0:       40 r + 40 * 0x400000
//     + Cbits                                                                    + c + 0x4B400000
//     + kIndexBias = 779 - (40 * 0x400000 + 0x4B400000)  (mod 2^32)              = 40 (r + 19) + c + 19, in 0 .. 1558; nothing wraps on the way but the bias
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DBRIEF_HD __host__ __device__ __forceinline__
#else
#define DBRIEF_HD inline
#endif

namespace describe_brief_index {

constexpr float kMagic = 12582912.0f;                    // 1.5 * 2^23, bits 0x4B400000
constexpr uint32_t kMagicBits = 0x4B400000u;
constexpr uint32_t kRadius = 19, kRowBytes = 40;
constexpr uint32_t kIndexBias = (kRowBytes * kRadius + kRadius) - (kRowBytes * 0x400000u + kMagicBits);      // unsigned arithmetic: mod 2^32

// bits of v + 1.5 * 2^23 = 0x4B400000 + rint(v); one correctly rounded float add (build with -ffp-contract=off)
DBRIEF_HD uint32_t round_bits(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint32_t, __fadd_rn(v, kMagic));
#else
    const float s = v + kMagic;
    uint32_t b;
    memcpy(&b, &s, 4);
    return b;
#endif
}

// byte index + base from the two coordinates' round_bits(); `base` = kIndexBias + whatever the caller adds to every index (the patch's address)
// (k_describe stores its patch COLUMN-major, 39 columns of 40 bytes, and passes (column, row): the same sum with the roles swapped, and kIndexBias is
// symmetric in the two -- both coordinates carry the same radius and the same magic bits)
DBRIEF_HD uint32_t index_from_bits(uint32_t row_bits, uint32_t col_bits, uint32_t base) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(row_bits, kRowBytes) + col_bits + base;
#else
    return (row_bits & 0xFFFFFFu) * kRowBytes + col_bits + base;
#endif
}

DBRIEF_HD uint32_t index(float row, float col) { return index_from_bits(round_bits(row), round_bits(col), kIndexBias); }

}  // namespace describe_brief_index
