// Checks, on the device, what k_hamming_mfma (slam-module_amd/csrc/match.hip) assumes of v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 (E2M1) operands
// (cbsz:4 blgp:4), with exact data and an asymmetric B:
//   1. the A / B lane -> (row, k) maps: lane l holds A[l & 31][32 (l >> 5) + 8 d + n] and B[32 (l >> 5) + 8 d + n][l & 31] in nibble n of dword d;
//   2. the scale operand: a lane's E8M0 byte scales that lane's own 32-element block (row l & 31, k block l >> 5), and op_sel picks the byte;
//   3. the kernel's encoding: targets 0b0001 (0.5) x 2^1 or 0b0010 (1.0) x 2^0, queries 0b0010 | bit << 3 (+1 / -1) x 2^4  ->  16 * dot, an integer;
//   4. a chain of four from C = 2^23 + 4096 + r stays an exact integer in the mantissa at the extremes (all products +16, all -16, all 0).
// hipcc --offload-arch=gfx950 tools/mfma_fp4_probe.hip -o /tmp/mfma_fp4_probe && /tmp/mfma_fp4_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
typedef int v8i_t __attribute__((ext_vector_type(8)));
typedef float v16f_t __attribute__((ext_vector_type(16)));

static const float kE2M1[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
static float e2m1(int c) { return (c & 8) ? -kE2M1[c & 7] : kE2M1[c & 7]; }

// An [32][64] nibble codes, Bn [64][32] nibble codes, sa / sb [64] scale dwords per lane, C0 / D [64][16] start values / results (lane, register)
template <int OPSEL>
__global__ void k_probe(const uint8_t *An, const uint8_t *Bn, const uint32_t *sa, const uint32_t *sb, const float *C0, int chain, float *D) {
    const int l = threadIdx.x, r = l & 31, h = l >> 5;
    v8i_t a = {0, 0, 0, 0, 0, 0, 0, 0}, b = a;
    for (int d = 0; d < 4; ++d) {
        uint32_t wa = 0, wb = 0;
        for (int n = 0; n < 8; ++n) {
            const int k = 32 * h + 8 * d + n;
            wa |= (uint32_t)(An[r * 64 + k] & 15) << (4 * n);
            wb |= (uint32_t)(Bn[k * 32 + r] & 15) << (4 * n);
        }
        a[d] = (int)wa; b[d] = (int)wb;
    }
    v16f_t c;
    for (int i = 0; i < 16; ++i) c[i] = C0[l * 16 + i];
    for (int s = 0; s < chain; ++s) c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4, 4, OPSEL, (int)sa[l], OPSEL, (int)sb[l]);
    for (int i = 0; i < 16; ++i) D[l * 16 + i] = c[i];
}

static uint8_t *dA, *dB; static uint32_t *dsa, *dsb; static float *dC, *dD;
static uint8_t hA[32 * 64], hB[64 * 32]; static uint32_t hsa[64], hsb[64]; static float hC[64 * 16], hD[64 * 16];

static void run(int opsel, int chain) {
    hipMemcpy(dA, hA, sizeof hA, hipMemcpyHostToDevice); hipMemcpy(dB, hB, sizeof hB, hipMemcpyHostToDevice);
    hipMemcpy(dsa, hsa, sizeof hsa, hipMemcpyHostToDevice); hipMemcpy(dsb, hsb, sizeof hsb, hipMemcpyHostToDevice);
    hipMemcpy(dC, hC, sizeof hC, hipMemcpyHostToDevice);
    switch (opsel) {
    case 0: hipLaunchKernelGGL(k_probe<0>, dim3(1), dim3(64), 0, 0, dA, dB, dsa, dsb, dC, chain, dD); break;
    case 1: hipLaunchKernelGGL(k_probe<1>, dim3(1), dim3(64), 0, 0, dA, dB, dsa, dsb, dC, chain, dD); break;
    case 2: hipLaunchKernelGGL(k_probe<2>, dim3(1), dim3(64), 0, 0, dA, dB, dsa, dsb, dC, chain, dD); break;
    default: hipLaunchKernelGGL(k_probe<3>, dim3(1), dim3(64), 0, 0, dA, dB, dsa, dsb, dC, chain, dD); break;
    }
    if (hipMemcpy(hD, dD, sizeof hD, hipMemcpyDeviceToHost) != hipSuccess) { printf("HIP error: %s\n", hipGetErrorString(hipGetLastError())); exit(2); }
}
// mismatches against  C0 + chain * sum_k 2^(ea - 127) A[row][k] * 2^(eb - 127) B[k][col],  ea / eb = byte `byte` of the scale dword of lane (k >> 5) * 32 + row / col
static int check(int byte, int chain) {
    int bad = 0;
    for (int l = 0; l < 64; ++l)
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * (l >> 5), col = l & 31;
            double want = hC[l * 16 + i];
            for (int k = 0; k < 64; ++k) {
                const int ea = (int)((hsa[(k >> 5) * 32 + row] >> (8 * byte)) & 255) - 127, eb = (int)((hsb[(k >> 5) * 32 + col] >> (8 * byte)) & 255) - 127;
                want += chain * (double)e2m1(hA[row * 64 + k]) * (double)e2m1(hB[k * 32 + col]) * (double)(1 << ea) * (double)(1 << eb);
            }
            if ((double)hD[l * 16 + i] != want) ++bad;
        }
    return bad;
}

int main() {
    hipMalloc(&dA, sizeof hA); hipMalloc(&dB, sizeof hB); hipMalloc(&dsa, sizeof hsa); hipMalloc(&dsb, sizeof hsb); hipMalloc(&dC, sizeof hC); hipMalloc(&dD, sizeof hD);
    srand(11);
    int fail = 0;
    // 1. lane maps: random E2M1 codes on both sides (products are multiples of 1/4, every sum exact), scale 2^0 everywhere, C = 0
    for (auto &v : hA) v = (uint8_t)(rand() & 15);
    for (auto &v : hB) v = (uint8_t)(rand() & 15);
    for (int l = 0; l < 64; ++l) hsa[l] = hsb[l] = 0x7F7F7F7Fu;
    memset(hC, 0, sizeof hC);
    run(0, 1);
    int bad = check(0, 1); fail |= bad;
    printf("lane maps A[l&31][32(l>>5)+8d+n], B[32(l>>5)+8d+n][l&31], D[(reg&3)+8(reg>>2)+4(l>>5)][l&31], nibble n of dword d: %s (%d mismatches)\n", bad ? "WRONG" : "ok", bad);
    // 2. scales: every lane and every byte of its scale dword gets an exponent of its own (2^0 .. 2^4)
    for (int l = 0; l < 64; ++l) {
        hsa[l] = hsb[l] = 0;
        for (int b = 0; b < 4; ++b) { hsa[l] |= (uint32_t)(127 + (l * 7 + b * 3) % 5) << (8 * b); hsb[l] |= (uint32_t)(127 + (l * 5 + b + 1) % 5) << (8 * b); }
    }
    for (int op = 0; op < 4; ++op) {
        run(op, 1);
        int which = -1;
        for (int b = 0; b < 4; ++b) if (check(b, 1) == 0) which = b;
        printf("scale operand, op_sel %d: lane l's byte %d scales its own block (row / col l&31, k block l>>5): %s\n", op, which, which == op ? "ok" : "UNEXPECTED");
        if (op == 0 && which != 0) fail |= 1;          // the kernel uses op_sel 0 with all four bytes equal; the other rows are for the record
    }
    // 3. the kernel's encoding: random bits, both target forms, queries +-1 x 2^4 -> 16 * dot
    for (int form = 0; form < 2; ++form) {
        for (auto &v : hA) v = (uint8_t)((rand() & 1) ? (form ? 2 : 1) : 0);
        for (auto &v : hB) v = (uint8_t)(2 | ((rand() & 1) << 3));
        for (int l = 0; l < 64; ++l) { hsa[l] = form ? 0x7F7F7F7Fu : 0x80808080u; hsb[l] = 0x83838383u; }
        run(0, 1);
        bad = check(0, 1);
        for (int l = 0; l < 64 && !bad; ++l)
            for (int i = 0; i < 16; ++i) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * (l >> 5), col = l & 31;
                int dot = 0;
                for (int k = 0; k < 64; ++k) dot += (hA[row * 64 + k] ? 1 : 0) * ((hB[k * 32 + col] & 8) ? -1 : 1);
                if (hD[l * 16 + i] != (float)(16 * dot)) ++bad;
            }
        fail |= bad;
        printf("targets 0b%s x 2^%d, queries 0b0010|bit<<3 x 2^4 -> 16 * dot: %s (%d mismatches)\n", form ? "0010" : "0001", form ? 0 : 1, bad ? "WRONG" : "ok", bad);
    }
    // 4. chains of four from 2^23 + 4096 + r at the extremes: the low 16 bits of the result's bit pattern must be 16 * (dot + 256) + r
    const char *names[3] = {"all +16", "all -16", "all 0"};
    for (int ext = 0; ext < 3; ++ext) {
        for (auto &v : hA) v = (uint8_t)(ext == 2 ? 0 : 1);
        for (auto &v : hB) v = (uint8_t)(ext == 1 ? 10 : 2);
        for (int l = 0; l < 64; ++l) { hsa[l] = 0x80808080u; hsb[l] = 0x83838383u; }
        for (int l = 0; l < 64; ++l) for (int i = 0; i < 16; ++i) hC[l * 16 + i] = 8388608.0f + 4096.0f + (float)i;
        run(0, 4);
        const int dot = ext == 0 ? 256 : ext == 1 ? -256 : 0;
        bad = 0;
        for (int l = 0; l < 64; ++l) for (int i = 0; i < 16; ++i) {
            uint32_t bits; memcpy(&bits, &hD[l * 16 + i], 4);
            if (bits != (0x4B000000u | (uint32_t)(16 * (dot + 256) + i))) ++bad;
        }
        fail |= bad;
        uint32_t b0; memcpy(&b0, &hD[5], 4);
        printf("chain of 4 from 2^23 + 4096 + r, %s: %s (%d mismatches; lane 0 reg 5 = 0x%08X)\n", names[ext], bad ? "WRONG" : "ok", bad, b0);
    }
    printf(fail ? "mfma_fp4_probe: FAILED\n" : "mfma_fp4_probe: all ok\n");
    return fail ? 1 : 0;
}
