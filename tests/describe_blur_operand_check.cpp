// CPU check of pass 2 of k_describe's blur as out = V T' with the vertical taps as the A operand and pass 1's result, as it leaves the
// accumulators, as the B operand (slam-module_amd/csrc/describe_lanes.h: vert_operand, blur_store_*; describe_brief_index.h).
//
// v_mfma_i32_16x16x64_i8 is modelled with the lane layouts that orb.hip's comments and tools/mfma_i8_probe.hip state:
//   A   lane (i = lane & 15, kg = lane >> 4) holds row i,    K bytes 16 kg .. + 15
//   B   lane (n = lane & 15, kg = lane >> 4) holds column n, K bytes 16 kg .. + 15
//   C   lane (n = lane & 15, q  = lane >> 4) holds rows 4 q .. + 3 of column n
//
//   (a) for random T' in -32768 .. 32767 (48 rows x 16 columns, three seeds), all-minimum and all-maximum T': the lane's byte planes {d[0], d[1], d[2], 0}
//       as B and {D0, D1} at dword positions yt, yt + 1 as A give, in the chained high / low form (start 33024, shift by 8), for every lane, every r and
//       every yt with a patch row 16 yt + 4 q + r in 0 .. 38, the direct banded sum  sum_s w7[s - y] T'[s][x]  + 33024 * 256 - 128 * 256, and byte 2 of it is
//       k_blur's pixel, byte 2 of sum w T + 32768 with T = T' + 32768
//   (b) T' rows 45 .. 47 and the fourth dword of B (K bytes 12 .. 15 of every group: T' rows 48 .. 63, which the kernel sets to zero) never reach a
//       patch row below 39: filled with garbage, every sum of (a) is unchanged
//   (c) for every integer (row, col) in -19 .. 19 squared the index with its arguments swapped addresses, in the column-major patch, the pixel that the
//       old index addresses in the row-major one
//   (d) the store map (t, yt, lane) -> dword is injective on its valid set, covers exactly 39 columns x 10 dwords, byte r of a stored dword is patch row
//       16 yt + 4 q + r of column 16 t + n, and the valid set is 16 t + n < 39 and 4 yt + q < 10
// Prints "blur operand ok" and exits 0, or the first violation and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "describe_brief_index.h"
#include "describe_lanes.h"

namespace dl = describe_lanes;
namespace bi = describe_brief_index;

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return false; } while (0)

static const int kW7[7] = {18, 34, 48, 56, 48, 34, 18};

struct Op { uint32_t d[4]; };                                // a lane's 16 K bytes
static int8_t op_byte(const Op &o, int j) { return (int8_t)(o.d[j / 4] >> (8 * (j % 4))); }

// D = A B + C on one wave: D[lane (n, q)][r] = C[lane][r] + sum over K = 16 kg + j of A[lane (i = 4 q + r, kg)] byte j * B[lane (n, kg)] byte j
static void mfma_i8(const Op (&A)[64], const Op (&B)[64], const int32_t (&C)[64][4], int32_t (&D)[64][4]) {
    for (int lane = 0; lane < 64; ++lane) {
        const int n = lane & 15, q = lane >> 4;
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * q + r;
            int64_t s = C[lane][r];
            for (int kg = 0; kg < 4; ++kg)
                for (int j = 0; j < 16; ++j) s += (int)op_byte(A[i + 16 * kg], j) * (int)op_byte(B[n + 16 * kg], j);
            D[lane][r] = (int32_t)(uint32_t)(uint64_t)s;     // (the accumulator wraps; nothing here comes near it)
        }
    }
}

// pass 2 of one column tile as the kernel runs it: T'[s][x], s = 0 .. 47, x = 0 .. 15; `fourth` is what stands in B's fourth dword (the kernel: zero)
static void pass2(const int32_t (&T)[48][16], uint32_t fourth, int32_t (&out)[3][64][4]) {
    Op Bh[64], Bl[64];
    for (int lane = 0; lane < 64; ++lane) {
        const int n = lane & 15, q = lane >> 4;
        for (int m = 0; m < 3; ++m) {                        // the C layout of pass 1: tile m, element r is T' row 16 m + 4 q + r
            uint32_t hd = 0, ld = 0;
            for (int r = 0; r < 4; ++r) {
                const uint32_t v = (uint32_t)T[16 * m + 4 * q + r][n];
                hd |= ((v >> 8) & 255u) << (8 * r);
                ld |= (v & 255u) << (8 * r);
            }
            Bh[lane].d[m] = hd;
            Bl[lane].d[m] = ld ^ 0x80808080u;
        }
        Bh[lane].d[3] = Bl[lane].d[3] = fourth;
    }
    for (int yt = 0; yt < 3; ++yt) {
        Op A[64];
        for (int lane = 0; lane < 64; ++lane)
            for (int m = 0; m < 4; ++m) A[lane].d[m] = dl::vert_operand_dword(lane, yt, m);
        int32_t acc[64][4], hi[64][4];
        for (auto &l : acc) for (auto &v : l) v = 33024;
        mfma_i8(A, Bh, acc, hi);
        for (auto &l : hi) for (auto &v : l) v = (int32_t)((uint32_t)v << 8);
        mfma_i8(A, Bl, hi, out[yt]);
    }
}

static bool check_sums(const int32_t (&T)[48][16], const char *what, int k) {
    static int32_t clean[3][64][4], dirty[3][64][4];
    pass2(T, 0u, clean);
    int32_t G[48][16];
    std::memcpy(G, T, sizeof G);
    uint32_t s = 777u + (uint32_t)k;
    for (int row = 45; row < 48; ++row)
        for (int x = 0; x < 16; ++x) { s = s * 1664525u + 1013904223u; G[row][x] = (int32_t)(s >> 16) - 32768; }
    pass2(G, 0x7F80A55Au, dirty);
    for (int yt = 0; yt < 3; ++yt)
        for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 4; ++r) {
                const int x = lane & 15, y = 16 * yt + 4 * (lane >> 4) + r;
                if (y > 38) continue;
                long S = 0, ST = 0;
                for (int tap = 0; tap < 7; ++tap) { S += (long)kW7[tap] * T[y + tap][x]; ST += (long)kW7[tap] * (T[y + tap][x] + 32768); }
                const long want = S + 33024L * 256 - 128L * 256;
                if (clean[yt][lane][r] != want) FAIL("sums: %s %d: row %d column %d (tile %d lane %d r %d): %d, the banded sum gives %ld", what, k, y, x, yt, lane, r, clean[yt][lane][r], want);
                if (((clean[yt][lane][r] >> 16) & 255) != (((ST + 32768) >> 16) & 255))      // (a real T stays below 65281 and the sum below 2^24; 32767 + 32768 does not)
                    FAIL("sums: %s %d: row %d column %d: byte 2 is not the blurred pixel", what, k, y, x);
                if (dirty[yt][lane][r] != clean[yt][lane][r]) FAIL("garbage: %s %d: rows 45 .. 47 or the fourth dword reach row %d column %d", what, k, y, x);
            }
    return true;
}

static bool check_operands() {
    static int32_t T[48][16];
    for (int k = 0; k < 3; ++k) {
        uint32_t s = 12345u + 1000u * (uint32_t)k;
        for (auto &row : T) for (auto &v : row) { s = s * 1664525u + 1013904223u; v = (int32_t)(s >> 16) - 32768; }
        if (!check_sums(T, "random T'", k)) return false;
    }
    for (auto &row : T) for (auto &v : row) v = -32768;
    if (!check_sums(T, "all-minimum T'", 0)) return false;
    for (auto &row : T) for (auto &v : row) v = 32767;
    if (!check_sums(T, "all-maximum T'", 0)) return false;
    // the K order itself: K byte 16 kg + 4 m + r of either operand stands for the same T' row
    for (int kg = 0; kg < 4; ++kg)
        for (int m = 0; m < 4; ++m)
            for (int r = 0; r < 4; ++r)
                if (dl::vert_k_row(kg, m, r) != 16 * m + 4 * kg + r) FAIL("K order: group %d dword %d byte %d", kg, m, r);
    return true;
}

static bool check_index() {
    for (int row = -19; row <= 19; ++row)
        for (int col = -19; col <= 19; ++col) {
            const uint32_t rb = bi::round_bits((float)row), cb = bi::round_bits((float)col);
            const uint32_t was = bi::index_from_bits(rb, cb, bi::kIndexBias), now = bi::index_from_bits(cb, rb, bi::kIndexBias);
            // row-major: 40 (row + 19) + col + 19; column-major: 40 (col + 19) + row + 19
            if (was >= 39u * 40u || now >= 39u * 40u) FAIL("index: (%d, %d) leaves the patch: %u, %u", row, col, was, now);
            if ((int)(was / 40u) != row + 19 || (int)(was % 40u) != col + 19) FAIL("index: (%d, %d): the old index is %u", row, col, was);
            if ((int)(now / 40u) != col + 19 || (int)(now % 40u) != row + 19) FAIL("index: (%d, %d): the swapped index is %u", row, col, now);
        }
    return true;
}

static bool check_stores() {
    std::vector<int> hit(dl::kBlurCols * dl::kBlurColDwords, 0);
    for (int t = 0; t < 3; ++t)
        for (int yt = 0; yt < 3; ++yt)
            for (int lane = 0; lane < 64; ++lane) {
                const int n = lane & 15, q = lane >> 4;
                const bool want = 16 * t + n < 39 && 4 * yt + q < 10;
                if (dl::blur_store_valid(lane, t, yt) != want) FAIL("stores: tile (%d, %d) lane %d: valid = %d", t, yt, lane, (int)!want);
                if (!want) continue;
                const int dw = dl::blur_store_dword(lane, t, yt);
                if (dw < 0 || dw >= (int)hit.size()) FAIL("stores: tile (%d, %d) lane %d stores dword %d", t, yt, lane, dw);
                for (int r = 0; r < 4; ++r)                  // byte r: patch row 16 yt + 4 q + r of column 16 t + n, at 40 column + row
                    if (4 * dw + r != 40 * (16 * t + n) + 16 * yt + 4 * q + r) FAIL("stores: tile (%d, %d) lane %d byte %d lands on byte %d", t, yt, lane, r, 4 * dw + r);
                ++hit[dw];
            }
    for (size_t i = 0; i < hit.size(); ++i)
        if (hit[i] != 1) FAIL("stores: dword %d stored %d times", (int)i, hit[i]);
    return true;
}

int main() {
    if (!check_operands() || !check_index() || !check_stores()) return 1;
    std::printf("blur operand ok\n");
    return 0;
}
