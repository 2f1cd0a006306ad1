// The lane maps of k_describe (orb.hip): which dwords of a keypoint's window, orientation patch and blur-tap table each of a wave's 64
// lanes touches, and the orientation moments as dword arithmetic.  Plain C++, no HIP: the kernel and the library's host tables are built
// from these functions, and tests/describe_lanes_check.cpp checks them on the CPU for all 64 lanes.
//
// A wave is one keypoint.  Everything below depends on the lane index alone, so none of it is recomputed per load inside the kernel:
// it comes from a table the kernel loads first thing (win_pack, disc_mask), from one lane base plus immediate offsets (ori_base), or
// from two lane constants (moment_col_weights, moment_row_bias).
#pragma once
#include <cstdint>

namespace describe_lanes {

constexpr int kWinRows = 45, kWinDwords = 12, kWinPieces = 9;     // the window: rows y-22 .. y+22, bytes x-23 .. x+24
constexpr int kPatchRows = 32, kPatchDwords = 8, kHalfPatch = 15; // the orientation patch: rows y-15 .. y+15 (+ one zero row), bytes x-15 .. x+16
constexpr int kOriRow0 = 7, kOriDword0 = 2;                       // where the patch starts inside the window

// ---- window fetch: piece t of a lane is window dword i = lane + 64 t (t = 0 .. 8, i < 45 * 12), row i / 12, dword i % 12 ----
// 64 = 5 * 12 + 4, so three pieces on the dword column is back where it was, 16 rows down: piece 3 a + b is piece b's dword, 16 a rows below.
// A lane therefore needs the (row, byte) of its first three pieces only: 3 x (4 + 6) bits in one dword, no division in the kernel.
constexpr uint32_t win_pack(int lane) {
    uint32_t p = 0;
    for (int b = 0; b < 3; ++b) {
        const int i = lane + 64 * b;
        p |= (uint32_t)((i / kWinDwords) | ((4 * (i % kWinDwords)) << 4)) << (10 * b);
    }
    return p;
}
constexpr int win_row(uint32_t pack, int t) { return (int)((pack >> (10 * (t % 3))) & 15u) + 16 * (t / 3); }
constexpr int win_byte(uint32_t pack, int t) { return (int)((pack >> (10 * (t % 3) + 4)) & 63u); }
// The ninth piece exists for 28 lanes only.  The other 36 are not switched off: they fetch dword 0 of the piece's row base (window row 16 (t / 3),
// always inside the window) and their slot lies behind the window, in the 36 dwords of the wave's slab that nothing reads as data.
constexpr bool win_active(int lane, int t) { return t < kWinPieces - 1 || lane < kWinRows * kWinDwords - 64 * (kWinPieces - 1); }
constexpr int win_src_row(uint32_t pack, int lane, int t) { return win_active(lane, t) ? win_row(pack, t) : 16 * (t / 3); }
constexpr int win_src_byte(uint32_t pack, int lane, int t) { return win_active(lane, t) ? win_byte(pack, t) : 0; }
constexpr int win_slot(int lane, int t) { return lane + 64 * t; }         // where the piece lands in the wave's LDS slab (dwords)
constexpr int kSlabDwords = kWinRows * kWinDwords + kPatchRows * kPatchDwords + 4;   // the window and the 32 x 8 + 4 dwords behind it

// ---- orientation patch: patch dword i = lane + 64 t (t = 0 .. 3) is row i >> 3, dword i & 7 = window row + 7, window dword + 2 ----
// 64 = 8 rows of 8 dwords: one lane base, the four pieces 8 window rows (96 dwords) apart.  The last 8 dwords (row 31) have no source:
// they are the zero row that rounds the patch to 32 x 32.
constexpr int ori_base(int lane) { return ((lane >> 3) + kOriRow0) * kWinDwords + (lane & 7) + kOriDword0; }
constexpr int ori_src(int lane, int t) { return ori_base(lane) + 8 * kWinDwords * t; }   // window dword read
constexpr int ori_dst(int lane, int t) { return lane + 64 * t; }                          // patch dword it becomes
constexpr bool ori_active(int lane, int t) { return t < 3 || lane < (kPatchRows - 1) * kPatchDwords - 64 * 3; }

// The disc of orb_extractor.cpp:174-186 / :259-271 on patch dword `ori_dst(lane, t)`: byte b is kept when |u| <= u_max[|v|],
// u = 4 (i & 7) + b - 15, v = (i >> 3) - 15; the 32nd column and row are cleared.
inline uint32_t disc_mask(int lane, int t, const int *u_max) {
    const int i = ori_dst(lane, t), r = i >> 3, c4 = i & 7;
    if (r >= kPatchRows - 1) return 0u;
    uint32_t m = 0;
    for (int b = 0; b < 4; ++b) {
        const int u = 4 * c4 + b - kHalfPatch, v = r - kHalfPatch;
        if (u <= kHalfPatch && (u < 0 ? -u : u) <= u_max[v < 0 ? -v : v]) m |= 0xFFu << (8 * b);
    }
    return m;
}

// ---- moments m10 = sum u I, m01 = sum v I over the masked patch, on the lane's own four dwords d[t] = patch dword lane + 64 t ----
// The four dwords share their columns (u = 4 (lane & 7) + b - 15) and lie 8 rows apart (v = (lane >> 3) + 8 t - 15).  With S_t the byte sum
// of d[t], T = S_0 + .. + S_3 and the running sums P_k = S_0 + .. + S_k that a chain of v_sad_u8 leaves behind:
//     m10 = sum_t dot4(d[t], u + 15) - 15 T                                   (non-negative byte weights 4 (lane & 7) + b)
//     m01 = sum_t (v_0 + 8 t) S_t = (v_0 + 24) T - 8 (P_0 + P_1 + P_2)        (sum_t t S_t = 3 T - P_0 - P_1 - P_2)
// All of it is exact integer arithmetic far inside 32 bits (T <= 1024 * 255), so the wave's totals are the reference's.
constexpr uint32_t moment_col_weights(int lane) { return 0x03020100u + 0x04040404u * (uint32_t)(lane & 7); }   // (the one full 32-bit multiply k_describe keeps: its constant has 27 bits, and shift-ors in its place are folded back into it)
constexpr int moment_row_bias(int lane) { return (lane >> 3) - kHalfPatch + 24; }

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint32_t sad_u8(uint32_t a, uint32_t acc) { return __builtin_amdgcn_sad_u8(a, 0u, acc); }
__device__ __forceinline__ uint32_t dot4_u8(uint32_t a, uint32_t w, uint32_t acc) { return __builtin_amdgcn_udot4(a, w, acc, false); }
__device__ __forceinline__ int mul_small(int a, int b) { return __mul24(a, b); }          // both factors far below 2^23: v_mul_i32_i24, full rate
#define DESCRIBE_LANES_FN __device__ __forceinline__
#else
inline int mul_small(int a, int b) { return a * b; }
inline uint32_t sad_u8(uint32_t a, uint32_t acc) { return acc + (a & 255u) + ((a >> 8) & 255u) + ((a >> 16) & 255u) + (a >> 24); }
inline uint32_t dot4_u8(uint32_t a, uint32_t w, uint32_t acc) {
    for (int b = 0; b < 4; ++b) acc += ((a >> (8 * b)) & 255u) * ((w >> (8 * b)) & 255u);
    return acc;
}
#define DESCRIBE_LANES_FN inline
#endif

DESCRIBE_LANES_FN void lane_moments(const uint32_t (&d)[4], uint32_t col_weights, int row_bias, int &m10, int &m01) {
    const uint32_t p0 = sad_u8(d[0], 0u), p1 = sad_u8(d[1], p0), p2 = sad_u8(d[2], p1), T = sad_u8(d[3], p2);
    const uint32_t D = dot4_u8(d[3], col_weights, dot4_u8(d[2], col_weights, dot4_u8(d[1], col_weights, dot4_u8(d[0], col_weights, 0u))));
    m10 = (int)D - kHalfPatch * (int)T;
    m01 = mul_small(row_bias, (int)T) - 8 * (int)(p0 + p1 + p2);        // row_bias 9 .. 16, T <= 16 * 255
}
#undef DESCRIBE_LANES_FN

// ---- blur taps, pass 1: s_tab[0 .. 31] horizontal taps [dt][n], 16 bytes each (B operands of the i8 MFMA) ----
// Tile t's operand of lane (n = lane & 15, kg = lane >> 4) is entry [dt = kg - t][n] when dt is 0 or 1 (and, in the last tile, the column
// 32 + n is one of the patch's 39), all zero otherwise.  [dt][n] = 16 dt + n = lane - 16 t, and entry [1][0] holds no tap at all (its
// 16 rows start 16 - 0 - 1 >= 15 past the column), in both tables: it is the zero operand, so the lane selects an INDEX and reads once.
// (tap_table still writes the vertical taps in the same B form behind the horizontal ones; the kernel takes the first half only: pass 2
// has the taps as its A operand, vert_operand below.)
constexpr int kTapZeroSlot = 16;
constexpr int tap_slot(int lane, int t) {
    return ((unsigned)(lane - 16 * t) < 32u && (t < 2 || (lane & 15) <= 6)) ? lane - 16 * t : kTapZeroSlot;
}
// [table 0 = horizontal, 1 = vertical][dt][n][4 dwords]: the taps 18 34 48 56 48 34 18 by patch column x -- window byte k contributes to x
// when 0 <= k - x - 1 <= 6 -- and by patch row y (window row k, 0 <= k - y <= 6)
inline void tap_table(uint32_t *out /* 64 * 4 dwords */) {
    const int w7[7] = {18, 34, 48, 56, 48, 34, 18};
    for (int i = 0; i < 64 * 4; ++i) out[i] = 0u;
    for (int tab = 0; tab < 2; ++tab)
        for (int dt = 0; dt < 2; ++dt)
            for (int n = 0; n < 16; ++n)
                for (int j = 0; j < 16; ++j) {
                    const int tap = 16 * dt + j - n - (tab == 0 ? 1 : 0);
                    const uint32_t v = (tap >= 0 && tap <= 6) ? (uint32_t)w7[tap] : 0u;
                    out[((tab * 2 + dt) * 16 + n) * 4 + j / 4] |= v << (8 * (j % 4));
                }
}

// ---- blur taps, pass 2: out = V T' with the vertical taps as the A operand and pass 1's result, as it leaves the accumulators, as B ----
// Pass 1 leaves T' in the C layout: lane (n, q), accumulator tile m, element r is T' row 16 m + 4 q + r of column n, so the lane's dword m (one byte
// plane of the four elements) is K bytes 16 q + 4 m .. + 3 of a B operand {dword 0, dword 1, dword 2, 0} whose K index is ordered
//     k' = 16 q + 4 m + r   <->   T' row 16 m + 4 q + r                     (q = the K group, m = the dword, r = the byte)
// The order of K is free as long as A is permuted the same way: lane (i = lane & 15, kg = lane >> 4) of A holds, for output row 16 yt + i, at dword m
// byte r the tap of T' row 16 m + 4 kg + r, w7[16 (m - yt) + 4 kg + r - i] -- non-zero for m - yt = 0 or 1 only, and dependent on (lane, m - yt)
// alone.  So a lane carries two dwords D0, D1 (vert_operand) and output row tile yt takes them at dword positions yt and yt + 1, zero elsewhere:
// {D0, D1, 0, 0}, {0, D0, D1, 0}, {0, 0, D0, D1}.  In the last one D1 stands at dword 3 = T' rows 48 .. 63, where B is zero.
constexpr uint32_t vert_operand(int lane, int dm) {
    const int w7[7] = {18, 34, 48, 56, 48, 34, 18};
    const int i = lane & 15, kg = lane >> 4;
    uint32_t d = 0;
    for (int r = 0; r < 4; ++r) {
        const int tap = 16 * dm + 4 * kg + r - i;
        if (tap >= 0 && tap <= 6) d |= (uint32_t)w7[tap] << (8 * r);
    }
    return d;
}
constexpr uint32_t vert_operand_dword(int lane, int yt, int m) { return (m == yt || m == yt + 1) ? vert_operand(lane, m - yt) : 0u; }   // dword m of A for row tile yt
constexpr int vert_k_row(int kg, int m, int r) { return 16 * m + 4 * kg + r; }      // the T' row that K byte 16 kg + 4 m + r stands for
// The result's C layout: lane (n, q) holds patch rows 16 yt + 4 q .. + 3 of column 16 t + n, one dword of a COLUMN-major patch (39 columns of 40 bytes)
constexpr int kBlurCols = 39, kBlurColDwords = 10;
// (16 t + n < 39 and 4 yt + q < 10 for t, yt in 0 .. 2 and a lane of 0 .. 63, written so that the tiles that are valid in every lane carry no test)
constexpr bool blur_store_valid(int lane, int t, int yt) { return (t < 2 || (lane & 15) < kBlurCols - 32) && (yt < 2 || (lane >> 4) < kBlurColDwords - 8); }
constexpr int blur_store_dword(int lane, int t, int yt) { return (16 * t + (lane & 15)) * kBlurColDwords + 4 * yt + (lane >> 4); }

}   // namespace describe_lanes
