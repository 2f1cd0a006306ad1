// CPU check of the 32-bit keys of k_hamming_mfma<true> (slam-module_amd/csrc/hamming_fp4.h): the float arithmetic that leaves the key in the
// accumulator register, the ageing by 32 per tile over the 256 tiles a set may have, the recovery of (row, distance) from the final key, the empty
// sentinel, and the three-instruction update of a sorted (best, second) pair by two keys.  Prints "keys ok" and returns 0 when everything holds.
#include "hamming_fp4.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_bad++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static double e8m0(uint32_t s) { int e = (int)(s & 255) - 127; double v = 1; for (; e > 0; --e) v *= 2; for (; e < 0; ++e) v /= 2; return v; }

// the accumulator chain as the matrix instruction runs it: four k-steps, each adds S * (its share of the dot product) in float
static uint32_t chain_bits(int r, int h, const int part[4]) {
    volatile float acc = hm_key_start(r, h);
    for (int s = 0; s < 4; ++s) {
        acc = acc + (float)kHmKeyS * (float)part[s];
        CHECK(acc >= 8388608.0f && acc < 16777216.0f, "partial sum %g leaves [2^23, 2^24) (r %d h %d step %d)", (double)acc, r, h, s);
    }
    return bits_of(acc);
}

static void check_arithmetic() {
    for (int b = 0; b < 4; ++b) CHECK(e8m0(kHm4ScaleBKey >> (8 * b)) == (double)kHmKeyS, "B scale byte %d is not 2^13", b);
    CHECK(bits_of(8388608.0f) == kHmKeyBase, "key base");
    CHECK(kHmKeyMaxRows == 32 * 256 && kHmKeyS == 8192u, "S");
    bool seen[32] = {};
    for (int h = 0; h < 2; ++h)
        for (int r = 0; r < 16; ++r) {
            const int row = hm_key_row_in_tile(r, h);
            CHECK(row >= 0 && row < 32 && !seen[row], "row in tile of r %d h %d", r, h);
            if (row >= 0 && row < 32) seen[row] = true;
            const int parts[5][4] = {{-64, -64, -64, -64}, {0, 0, 0, 0}, {64, 64, 64, 64}, {64, -64, 64, -64}, {-64, -64, 64, 37}};
            for (const auto &p : parts) {
                const int dot = p[0] + p[1] + p[2] + p[3];
                const uint32_t key = chain_bits(r, h, p), want = kHmKeyBase + kHmKeyS * (uint32_t)(dot + 256) + (kHmKeyS - 32u + (uint32_t)row);
                CHECK(key == want, "key 0x%08X, want 0x%08X (dot %d r %d h %d)", key, want, dot, r, h);
                CHECK(!hm_key_empty(key) && hm_key_dot256(key) == dot + 256 && hm_key_row(key, 1) == row, "fresh key decodes to dot %d row %d", hm_key_dot256(key) - 256, hm_key_row(key, 1));
            }
        }
}

// all quadruples (best <= second, k0, k1) over a small key range plus the sentinel: the update must leave the two smallest of the four
static void check_update_rule() {
    std::vector<uint32_t> vals;
    for (uint32_t v = 0; v < 9; ++v) vals.push_back(kHmKeyBase + v);
    vals.push_back(kHmKeyNone - 8192u); vals.push_back(kHmKeyNone - 32u); vals.push_back(kHmKeyNone);
    long n = 0;
    for (uint32_t b : vals) for (uint32_t s : vals) { if (s < b) continue;
        for (uint32_t k0 : vals) for (uint32_t k1 : vals) {
            uint32_t all[4] = {b, s, k0, k1};
            std::sort(all, all + 4);
            uint32_t nb = b, ns = s;
            hm_key_push2(nb, ns, k0, k1);
            CHECK(nb == all[0] && ns == all[1], "push2(%08X %08X ; %08X %08X) = %08X %08X", b, s, k0, k1, nb, ns);
            ++n;
        } }
    CHECK(n > 9000, "update rule: only %ld cases", n);
}

// a whole search of one query as the kernel runs it: two lane halves with 16 rows of every tile each, aged before each tile, merged at the end
static void check_search(int nt, const std::vector<int> &dot /* per row, -256 .. 256 */) {
    uint32_t best[2] = {kHmKeyNone, kHmKeyNone}, second[2] = {kHmKeyNone, kHmKeyNone};
    const int tiles = (nt + 31) >> 5;
    for (int t = 0; t < tiles; ++t)
        for (int h = 0; h < 2; ++h) {
            hm_key_age(best[h], second[h]);
            for (int r = 0; r < 16; r += 2) {
                uint32_t k[2];
                for (int e = 0; e < 2; ++e) {
                    const int row = 32 * t + hm_key_row_in_tile(r + e, h);
                    k[e] = row < nt ? bits_of(hm_key_start(r + e, h) + (float)kHmKeyS * (float)dot[row]) : kHmKeyNone;
                }
                hm_key_push2(best[h], second[h], k[0], k[1]);
            }
        }
    const uint32_t b = hm_key_umin(best[0], best[1]), s2 = hm_key_umin(hm_key_umax(best[0], best[1]), hm_key_umin(second[0], second[1]));
    // the reference order: (dot, row), the lowest row first among equal dots
    int wb = -1, ws = -1;
    for (int j = 0; j < nt; ++j) {
        if (wb < 0 || dot[j] < dot[wb]) { ws = wb; wb = j; }
        else if (ws < 0 || dot[j] < dot[ws]) ws = j;
    }
    if (nt == 0) { CHECK(hm_key_empty(b) && hm_key_empty(s2), "empty set leaves keys"); return; }
    CHECK(!hm_key_empty(b) && hm_key_row(b, tiles) == wb && hm_key_dot256(b) == dot[wb] + 256, "nt %d: best row %d dot %d, want row %d dot %d", nt, hm_key_row(b, tiles), hm_key_dot256(b) - 256, wb, dot[wb]);
    if (nt == 1) { CHECK(hm_key_empty(s2), "nt 1: second is not the sentinel (0x%08X)", s2); return; }
    CHECK(!hm_key_empty(s2) && hm_key_row(s2, tiles) == ws && hm_key_dot256(s2) == dot[ws] + 256, "nt %d: second row %d dot %d, want row %d dot %d", nt, hm_key_row(s2, tiles), hm_key_dot256(s2) - 256, ws, dot[ws]);
}

int main() {
    check_arithmetic();
    check_update_rule();
    // the sentinel under the longest ageing stays empty and above every real key
    {
        uint32_t b = kHmKeyNone, s = kHmKeyNone;
        for (int t = 0; t < kHmKeyMaxRows / 32; ++t) hm_key_age(b, s);
        CHECK(hm_key_empty(b) && hm_key_empty(s) && b > kHmKeyBase + (1u << 23), "aged sentinel 0x%08X", b);
    }
    srand(9);
    const int sizes[] = {0, 1, 2, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160, 4096, 8160, 8161, 8191, 8192};
    for (int nt : sizes)
        for (int mode = 0; mode < 6; ++mode) {
            std::vector<int> dot((size_t)nt);
            for (int j = 0; j < nt; ++j)
                dot[(size_t)j] = mode == 0 ? -256 : mode == 1 ? 256 : mode == 2 ? 0 : mode == 3 ? rand() % 3 - 1 : mode == 4 ? rand() % 513 - 256 : (j == nt - 1 || j == 0 ? -200 : rand() % 100);
            check_search(nt, dot);
        }
    // the first and the last row the ageing can hold carry the same (smallest) distance: row 0 wins with rel 0
    {
        std::vector<int> dot(8192, 17);
        dot[0] = dot[8191] = -3;
        check_search(8192, dot);
        dot[0] = 17; dot[1] = -3;
        check_search(8192, dot);
    }
    printf(g_bad ? "keys WRONG (%d failures)\n" : "keys ok\n", g_bad);
    return g_bad ? 1 : 0;
}
