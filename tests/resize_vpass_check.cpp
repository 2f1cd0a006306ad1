// CPU check of k_resize's vertical pass and pixel packing (slam-module_amd/csrc/resize_vpass.h) against the form they replace,
//     v = ((b0 * (r0 >> 4) >> 16) + (b1 * (r1 >> 4) >> 16) + 2) >> 2,   packed = v0 | v1 << 8 | v2 << 16 | v3 << 24,
// exhaustively over the operands' ranges.  Prints "vpass ok" and returns 0 when everything holds.
#include "resize_vpass.h"
#include <cstdio>
#include <cstdlib>

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_bad++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// v_dot2_u32_u16 with a zero accumulator
static uint32_t dot2(uint32_t a, uint32_t b) { return (a & 0xFFFFu) * (b & 0xFFFFu) + (a >> 16) * (b >> 16); }

int main() {
    using namespace resize_vpass;
    long n = 0;
    // 1. the high half of the 24-bit product IS the old product shifted down by 16: every row tap b and every F = r >> 4 <= 255 * 2049 >> 4 (67 M pairs)
    const uint32_t kFmax = 255u * 2048u >> 4;       // 32640 for taps that sum to 2048; a sum of 2049 reaches 32655, inside the + 16 below
    for (uint32_t b = 0; b <= 2048; ++b) {
        const uint32_t b8 = row_tap(b);
        CHECK(b8 < (1u << 20), "row tap %u", b);
        for (uint32_t F = 0; F <= kFmax + 16; ++F, ++n) {
            const uint32_t got = mul_hi_u24(b8, F << 8), want = (b * F) >> 16;
            if (got != want) CHECK(false, "mul_hi_u24(%u << 8, %u << 8) = %u, want %u", b, F, got, want);
        }
    }
    // 2. the horizontal pass with the taps shifted up by 4, masked: (r >> 4) << 8 for every tap pair whose sum is 2047, 2048 or 2049 and every pair of bytes
    //    (r = p0 a0 + p1 a1 takes every value the kernel can see, 0 .. 255 * 2049)
    for (int sum = 2047; sum <= 2049; ++sum)
        for (uint32_t a0 = 0; a0 <= 2048; ++a0) {
            const uint32_t a1 = (uint32_t)sum - a0;
            if (a1 > 2048) continue;
            const uint32_t A = a0 | (a1 << 16), P = preshift_taps(A);
            CHECK(P == ((a0 << 4) | ((a1 << 4) << 16)) && (a0 << 4) <= 0xFFFFu && (a1 << 4) <= 0xFFFFu, "taps %u, %u do not stay in their halves", a0, a1);
            for (uint32_t p0 = 0; p0 < 256; ++p0)
                for (uint32_t p1 = 0; p1 < 256; ++p1, ++n) {
                    const uint32_t px = p0 | (p1 << 16), r = dot2(px, A), got = f8(dot2(px, P));
                    if (got != (r >> 4) << 8 || got >= (1u << 23)) CHECK(false, "taps %u, %u bytes %u, %u: 0x%X, want 0x%X", a0, a1, p0, p1, got, (r >> 4) << 8);
                }
        }
    // the same statement by value of r alone, 0 .. 255 * 2049
    for (uint32_t r = 0; r <= 255u * 2049u; ++r, ++n) CHECK(f8(16u * r) == (r >> 4) << 8 && f8(16u * r) < (1u << 23), "r = %u", r);
    // 3. a whole pixel, old form against new, on operands drawn from the ranges above
    unsigned long long st = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    for (int it = 0; it < 20000000; ++it, ++n) {
        const unsigned long long u = next(), w = next();
        const uint32_t b0 = (uint32_t)(u % 2049), b1 = 2048u + (uint32_t)((u >> 20) % 3) - 1u - b0;
        if (b1 > 2048) continue;
        const uint32_t r0 = (uint32_t)(w % (255u * 2049u + 1)), r1 = (uint32_t)((w >> 32) % (255u * 2049u + 1));
        const uint32_t want = ((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2, got = vsum(row_tap(b0), f8(16u * r0), row_tap(b1), f8(16u * r1));
        if (got != want || got > 1023) CHECK(false, "pixel b %u, %u r %u, %u: %u, want %u", b0, b1, r0, r1, got, want);
    }
    // 4. packing: every sum 0 .. 1023 in each of the four positions, beside every corner value and a running one in the others
    const uint32_t others[] = {0, 1, 2, 3, 4, 255, 256, 511, 512, 1020, 1023};
    for (int pos = 0; pos < 4; ++pos)
        for (uint32_t s = 0; s <= 1023; ++s)
            for (uint32_t o : others)
                for (int run = 0; run < 2; ++run, ++n) {
                    uint32_t v[4];
                    for (int k = 0; k < 4; ++k) v[k] = run ? (s * 37u + o + 211u * (uint32_t)k) & 1023u : o;
                    v[pos] = s;
                    const uint32_t want = (v[0] >> 2) | (v[1] >> 2) << 8 | (v[2] >> 2) << 16 | (v[3] >> 2) << 24, got = pack4(v[0], v[1], v[2], v[3]);
                    CHECK(got == want, "pack4(%u, %u, %u, %u) = 0x%08X, want 0x%08X", v[0], v[1], v[2], v[3], got, want);
                }
    CHECK(n > 67000000L + 400000000L, "only %ld cases", n);
    if (g_bad) printf("vpass WRONG (%d failures)\n", g_bad);
    else printf("vpass ok (%ld cases)\n", n);
    return g_bad ? 1 : 0;
}
