// CPU check of the FP4 operand encoding of k_hamming_mfma (slam-module_amd/csrc/hamming_fp4.h): query bit i and target bit i must land in the
// same (k-step, lane half, dword, nibble) slot, the slot rule must name that slot, and with the nibbles decoded as E2M1 and the kernel's
// scales  popcount(q) + sum of products / 16 = hamming(q, t).  Prints "encoding ok" and returns 0 when everything holds.
#include "hamming_fp4.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static const double kE2M1[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
static double e2m1(uint32_t c) { return (c & 8) ? -kE2M1[c & 7] : kE2M1[c & 7]; }
static double e8m0(uint32_t s) { int e = (int)(s & 255) - 127; double v = 1; for (; e > 0; --e) v *= 2; for (; e < 0; ++e) v /= 2; return v; }

struct Desc { uint32_t w[8]; };
struct Frag { uint32_t d[kHm4Steps][2][4]; };           // [k-step][lane half][dword]: what one (row, lane half) pair of lanes holds

static Frag expand(const Desc &x, bool query) {
    Frag f;
    for (int s = 0; s < kHm4Steps; ++s)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 4; ++j) f.d[s][h][j] = query ? hm4_query_dword(x.w[2 * s + h], j) : hm4_target_dword(x.w[2 * s + h], j);
    return f;
}
static int popcount256(const Desc &x) { int n = 0; for (int k = 0; k < 8; ++k) n += __builtin_popcount(x.w[k]); return n; }
static int hamming(const Desc &a, const Desc &b) { int n = 0; for (int k = 0; k < 8; ++k) n += __builtin_popcount(a.w[k] ^ b.w[k]); return n; }

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_bad++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the matrix product as the instruction defines it: sum over all slots of (A nibble x A scale) x (B nibble x B scale)
static void check_pair(const Desc &q, const Desc &t) {
    const Frag fq = expand(q, true), ft = expand(t, false);
    double acc = 0;
    for (int s = 0; s < kHm4Steps; ++s)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 4; ++j)
                for (int n = 0; n < 8; ++n) {
                    const double a = e2m1((ft.d[s][h][j] >> (4 * n)) & 15) * e8m0(kHm4ScaleA), b = e2m1((fq.d[s][h][j] >> (4 * n)) & 15) * e8m0(kHm4ScaleB);
                    CHECK(a == 0 || a == 1, "target value %g at step %d half %d dword %d nibble %d", a, s, h, j, n);
                    CHECK(b == 16 || b == -16, "query value %g at step %d half %d dword %d nibble %d", b, s, h, j, n);
                    acc += a * b;
                }
    const int dot16 = (int)acc;
    CHECK((double)dot16 == acc && dot16 % 16 == 0, "accumulator %g is no multiple of 16", acc);
    CHECK(popcount256(q) + dot16 / 16 == hamming(q, t), "popcount %d + dot %d != hamming %d", popcount256(q), dot16 / 16, hamming(q, t));
    // the key the kernel reads: low 16 bits of the float 2^23 + 4096 + r + 16 dot
    for (int r = 0; r < 16; r += 15) {
        const float f = 8388608.0f + 4096.0f + (float)r + (float)dot16;
        uint32_t bits; memcpy(&bits, &f, 4);
        CHECK((bits & 0xFFFFu) == (uint32_t)(16 * (dot16 / 16 + 256) + r) && (bits >> 16) == 0x4B00u, "key bits 0x%08X for dot %d r %d", bits, dot16 / 16, r);
    }
}

int main() {
    Desc zero{}, ones{};
    for (int k = 0; k < 8; ++k) ones.w[k] = 0xFFFFFFFFu;
    // each of the 256 bit positions alone: exactly one nibble of each expansion changes, the same one, and it is the slot hm4_slot names
    const Frag q0 = expand(zero, true), t0 = expand(zero, false);
    bool seen[kHm4Steps][2][4][8] = {};
    for (int i = 0; i < 256; ++i) {
        Desc x{}; x.w[i >> 5] = 1u << (i & 31);
        const Frag fq = expand(x, true), ft = expand(x, false);
        const Hm4Slot sl = hm4_slot(i);
        CHECK(sl.step >= 0 && sl.step < kHm4Steps && sl.half >= 0 && sl.half < 2 && sl.dword >= 0 && sl.dword < 4 && sl.nibble >= 0 && sl.nibble < 8, "slot of bit %d out of range", i);
        int nq = 0, nt = 0;
        for (int s = 0; s < kHm4Steps; ++s) for (int h = 0; h < 2; ++h) for (int j = 0; j < 4; ++j) for (int n = 0; n < 8; ++n) {
            const bool dq = ((fq.d[s][h][j] ^ q0.d[s][h][j]) >> (4 * n)) & 15, dt = ((ft.d[s][h][j] ^ t0.d[s][h][j]) >> (4 * n)) & 15;
            nq += dq; nt += dt;
            const bool here = s == sl.step && h == sl.half && j == sl.dword && n == sl.nibble;
            CHECK(dq == here && dt == here, "bit %d: query %d target %d at step %d half %d dword %d nibble %d, slot rule says %d", i, dq, dt, s, h, j, n, here);
        }
        CHECK(nq == 1 && nt == 1, "bit %d changes %d query and %d target nibbles", i, nq, nt);
        CHECK(!seen[sl.step][sl.half][sl.dword][sl.nibble], "bit %d shares its slot", i);
        seen[sl.step][sl.half][sl.dword][sl.nibble] = true;
        CHECK(((ft.d[sl.step][sl.half][sl.dword] >> (4 * sl.nibble)) & 15) == 1u, "bit %d: target nibble is not 0b0001", i);
        CHECK(((fq.d[sl.step][sl.half][sl.dword] >> (4 * sl.nibble)) & 15) == 10u, "bit %d: query nibble is not 0b1010", i);
        check_pair(x, x); check_pair(x, zero); check_pair(zero, x); check_pair(x, ones); check_pair(ones, x);
        Desc y{}; y.w[((i + 37) & 255) >> 5] = 1u << ((i + 37) & 31);
        check_pair(x, y);
    }
    check_pair(zero, zero); check_pair(zero, ones); check_pair(ones, zero); check_pair(ones, ones);
    srand(5);
    for (int it = 0; it < 1000; ++it) {
        Desc q, t;
        for (int k = 0; k < 8; ++k) { q.w[k] = ((uint32_t)rand() << 17) ^ ((uint32_t)rand() << 3) ^ (uint32_t)rand(); t.w[k] = ((uint32_t)rand() << 17) ^ ((uint32_t)rand() << 3) ^ (uint32_t)rand(); }
        if (it & 1) for (int k = 0; k < 8; ++k) t.w[k] = q.w[k] ^ (t.w[k] & q.w[(k + 1) & 7] & t.w[(k + 3) & 7]);      // near pairs as well as unrelated ones
        check_pair(q, t);
    }
    printf(g_bad ? "encoding WRONG (%d failures)\n" : "encoding ok\n", g_bad);
    return g_bad ? 1 : 0;
}
