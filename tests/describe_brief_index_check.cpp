// CPU check of k_describe's BRIEF byte index (slam-module_amd/csrc/describe_brief_index.h) against the form it replaces: __float2int_rn per coordinate
// (round to nearest, ties to even), + 19 each, row * 40 + column.  Build with -ffp-contract=off.  Prints "brief index ok" and returns 0 when everything holds.
#include "describe_brief_index.h"
#include "describe_steer.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#if defined(__SSE__)
#include <xmmintrin.h>
#endif

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_bad++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)
static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static float float_of(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
// (int)rintf(v) in the default rounding mode (to nearest, ties to even) = __float2int_rn; cvtss2si is the same operation without the library call
static int round_rn(float v) {
#if defined(__SSE__)
    return _mm_cvtss_si32(_mm_set_ss(v));
#else
    return (int)rintf(v);
#endif
}

static const int8_t kPattern[1024] = {
#include "orb_pattern.inc"
};

int main() {
    using namespace describe_brief_index;
    long n = 0;
    CHECK(bits_of(kMagic) == kMagicBits, "the magic constant's bits are 0x%08X", bits_of(kMagic));
    const float ties[] = {-64.f, -19.5f, -2.5f, -1.5f, -0.5f, -0.f, 0.f, 0.5f, 1.5f, 2.5f, 18.5f, 19.49999f, 64.f};
    for (float v : ties) CHECK(round_rn(v) == (int)rintf(v), "round_rn(%g)", (double)v);
    // 1. every float in [-64, 64]: all bit patterns 0 .. bits(64.0f) under both signs (denormals and both zeros included)
    const uint32_t top = bits_of(64.0f);
    for (uint32_t sign = 0; sign < 2; ++sign)
        for (uint32_t b = 0; b <= top; ++b, ++n) {
            const float v = float_of(b | sign << 31);
            const int got = (int)(round_bits(v) - kMagicBits), want = round_rn(v);
            if (got != want) CHECK(false, "round_bits(%.9g) - magic = %d, want %d", (double)v, got, want);
        }
    // 2. the steered pattern: all 512 points under (cos, sin) of every angle 0 .. 360 degrees in steps of 1 / 64, as the kernel computes them
    for (int a = 0; a <= 360 * 64; ++a) {
        const float deg = (float)a / 64.0f, rad = describe_steer::deg_to_rad(deg);
        const float ca = describe_steer::cos_approx(rad), sa = describe_steer::sin_approx(rad), nsa = -sa;
        for (int p = 0; p < 512; ++p, ++n) {
            const float x = (float)kPattern[2 * p], y = (float)kPattern[2 * p + 1];
            const float row = x * sa + y * ca, col = x * ca - y * sa, col_k = x * ca + y * nsa;       // col_k: the kernel's form, the same float
            if (bits_of(col) != bits_of(col_k)) CHECK(false, "angle %g point %d: column 0x%08X as a sum, 0x%08X as a difference", (double)deg, p, bits_of(col_k), bits_of(col));
            const int r = round_rn(row), c = round_rn(col);
            const uint32_t want = (uint32_t)(r + 19) * 40u + (uint32_t)(c + 19), got = index(row, col_k);
            if (got != want || got > 1558u || r < -19 || r > 19 || c < -19 || c > 19)
                CHECK(false, "angle %g point %d (%g, %g): index %u, want %u (row %d, column %d)", (double)deg, p, (double)x, (double)y, got, want, r, c);
        }
    }
    CHECK(n == 2L * ((long)top + 1) + 512L * (360 * 64 + 1), "%ld cases", n);
    if (g_bad) printf("brief index WRONG (%d failures)\n", g_bad);
    else printf("brief index ok (%ld cases)\n", n);
    return g_bad ? 1 : 0;
}
