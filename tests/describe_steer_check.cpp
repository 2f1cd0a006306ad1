// CPU check of k_describe's steering arithmetic (slam-module_amd/csrc/describe_steer.h) against the forms it replaces, bit for bit: the two-branch
// cv::fastAtan2 (two divisions, two polynomials) and the four-branch cosine of openvslam/trigonometric.h, as the kernel evaluated them before.
// Build with -ffp-contract=off.  Prints "steer ok" and returns 0 when everything holds.
#include "describe_steer.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_bad++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)
static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

// ---- the earlier forms ----
static float old_fast_atan2(float y, float x) {
    const float p1 = 0.9997878412794807f * (float)(180 / 3.1415926535897932384626433832795);
    const float p3 = -0.3258083974640975f * (float)(180 / 3.1415926535897932384626433832795);
    const float p5 = 0.1555786518463281f * (float)(180 / 3.1415926535897932384626433832795);
    const float p7 = -0.04432655554792128f * (float)(180 / 3.1415926535897932384626433832795);
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)DBL_EPSILON);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + (float)DBL_EPSILON);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}
static float old_poly_cos(float v) {
    const float c1 = 0.99940307f, c2 = -0.49558072f, c3 = 0.03679168f;
    const float v2 = v * v;
    return c1 + v2 * (c2 + c3 * v2);
}
static float old_cos(float v) {
    const float PI = 3.14159265358979f, PI_2 = PI / 2.0f, TWO_PI = 2.0f * PI, INV_TWO_PI = 1.0f / TWO_PI, THREE_PI_2 = 3.0f * PI_2;
    v = v - (float)(int)floorf(v * INV_TWO_PI) * TWO_PI;
    v = (0.0f < v) ? v : -v;
    if (v < PI_2) return old_poly_cos(v);
    else if (v < PI) return -old_poly_cos(PI - v);
    else if (v < THREE_PI_2) return -old_poly_cos(v - PI);
    else return old_poly_cos(TWO_PI - v);
}
static float old_sin(float v) { return old_cos(3.14159265358979f / 2.0f - v); }

static long g_n = 0;
static void check_pair(float m01, float m10) {
    const float want = old_fast_atan2(m01, m10), got = describe_steer::fast_atan2(m01, m10);
    CHECK(bits_of(want) == bits_of(got), "atan2(%g, %g): 0x%08X, want 0x%08X", (double)m01, (double)m10, bits_of(got), bits_of(want));
    const float rad = describe_steer::deg_to_rad(got);
    CHECK(bits_of(rad) == bits_of((float)((double)want * M_PI / 180.0)), "radians of %g", (double)want);
    const float c = describe_steer::cos_approx(rad), s = describe_steer::cos_approx(describe_steer::sin_argument(rad));
    CHECK(bits_of(c) == bits_of(old_cos(rad)), "cos(%g): 0x%08X, want 0x%08X", (double)rad, bits_of(c), bits_of(old_cos(rad)));
    CHECK(bits_of(s) == bits_of(old_sin(rad)) && bits_of(s) == bits_of(describe_steer::sin_approx(rad)), "sin(%g): 0x%08X, want 0x%08X", (double)rad, bits_of(s), bits_of(old_sin(rad)));
    ++g_n;
}

int main() {
    for (int y = -300; y <= 300; ++y)
        for (int x = -300; x <= 300; ++x) check_pair((float)y, (float)x);
    // the moments' full range: |m| <= 15 * 255 * 709 disc pixels < 2^22
    const int kMax = 15 * 255 * 709;
    unsigned long long st = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    for (int it = 0; it < 10000000; ++it) {
        const unsigned long long a = next(), b = next();
        int y = (int)(a % (2ull * kMax + 1)) - kMax, x = (int)(b % (2ull * kMax + 1)) - kMax;
        if ((it & 15) == 0) { const int sh = (int)((a >> 40) % 22); y >>= sh; x >>= (int)((b >> 40) % 22); }     // small and mixed magnitudes as well
        check_pair((float)y, (float)x);
    }
    const int mags[] = {0, 1, 2, 3, 255, 256, 1000, 65535, 65536, 1 << 20, kMax - 1, kMax};
    for (int m : mags)
        for (int sy = -1; sy <= 1; ++sy)
            for (int sx = -1; sx <= 1; ++sx) {
                check_pair((float)(sy * m), (float)(sx * m));                                   // the axes, the diagonals, (0, 0)
                if (m > 0) { check_pair((float)(sy * m), (float)(sx * (m - 1))); check_pair((float)(sy * (m - 1)), (float)(sx * m)); }   // either side of a diagonal
            }
    CHECK(g_n > 10361000, "only %ld pairs", g_n);
    if (g_bad) printf("steer WRONG (%d failures)\n", g_bad);
    else printf("steer ok (%ld pairs)\n", g_n);
    return g_bad ? 1 : 0;
}
