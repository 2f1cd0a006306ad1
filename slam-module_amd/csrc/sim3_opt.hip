// sim3_opt.hip -- N5: the Sim3 refinement behind OptimizeSim3Transform (optimize_transform.cpp:63-155), g2o's solve restated in tests/sim3_opt_ref.py.
//
// Every problem of a call is one loop candidate: ONE free g2o::Sim3 S12 = (r, t, s), every point fixed, two projection edges per match
// (S12 maps keyframe 2's point into image 1, S12^-1 maps keyframe 1's point into image 2), Huber kernel, up to max_iters Levenberg-Marquardt
// iterations of up to 10 damped trials on a 7 x 7 system.  The problems are independent, so a call is ONE launch of k_sim3_opt with one
// workgroup (kThreads lanes) per problem and the whole LM loop inside it, in the manner of k_ba_pose_only (ba.hip):
//   * a SWEEP at a state evaluates both edges of every match and linearises there: per thread the upper triangle of H (28), b (7) and the
//     robust chi2 (1).  The sweep of an accepted trial already holds H and b of the next iteration and a rejected trial keeps the old
//     ones, so a solve costs 1 + trials sweeps;
//   * the first kResident matches of a problem live in registers (kSlots per thread, loaded once from coalesced SoA planes); the ones beyond
//     them stream from the same planes in every sweep, so any count up to the cap works;
//   * the 36 sums are reduced in a FIXED order: neighbouring lanes add over the DPP network, the even lanes write their 36 values to LDS
//     transposed (value-major rows), 4 lanes per value add 32 entries each and meet over DPP again.  No float atomics: the same input gives
//     the same bits on every run and at every position of a batch;
//   * every thread then factors the 7 x 7 matrix for itself (fully unrolled Cholesky in registers) and moves its own copy of the state:
//     the same arithmetic in every lane, no broadcast, no barrier.
// All arithmetic is fp64, without contraction (the library's -ffp-contract=off); the Jacobian is the ANALYTIC derivative of the left update
// S <- exp(dx) S, where g2o differentiates these two edges numerically.
#include "ms_internal.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include "ms_lanes_f64.h"

namespace {

constexpr int kThreads = 256;                    // one wave per SIMD: the whole register file is each wave's
constexpr int kSlots = 8;                        // matches a thread keeps in registers
constexpr int kResident = kThreads * kSlots;     // 2048 (tests/sim3_opt_ref.py RESIDENT)
constexpr int kSums = 36;                        // 28 (upper triangle of H) + 7 (b) + 1 (robust chi2)
constexpr int kRow = kThreads / 2 + 4;           // row stride (doubles) of the transposed partial sums
constexpr int kPlanes = 10;                      // p1 xyz, p2 xyz, obs1 uv, obs2 uv
static_assert(4 * kSums <= kThreads, "stage 2 of the reduction: 4 lanes per sum");

struct S3State { double R[9], t[3], s; };

struct S3Desc {                                  // one problem as the kernel sees it
    long long m_off;                             // first match in the call's planes
    int32_t n, fix_scale, max_iters, want_chi2;
    double delta;
    S3State S0;
};

struct S3Acc { double H[28], b[7], chi; };

// one edge into the sums: H += J^T (w info) J, b += -J^T (w info) e, chi += rho
__device__ __forceinline__ void add_edge(S3Acc &A, const double (&J0)[7], const double (&J1)[7], double e0, double e1, double info, double delta) {
    const double chi2 = info * (e0 * e0 + e1 * e1);
    double rho, w;
    huber(chi2, delta, rho, w);
    A.chi += rho;
    const double wi = w * info;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 7; ++a) {
        A.b[a] += -(J0[a] * e0 + J1[a] * e1) * wi;
#pragma unroll
        for (int c = a; c < 7; ++c) A.H[k++] += wi * (J0[a] * J0[c] + J1[a] * J1[c]);
    }
}

// the errors of both edges of one match: e12 = obs1 - proj(S.map(p2)), e21 = obs2 - proj(S^-1.map(p1)), proj a plain division;
// (u, v, 1 / z) of both mapped points come back for the Jacobians
struct S3Edge { double u, v, iz, e0, e1; };
__device__ __forceinline__ void edge_errors(const S3State &S, double is, const double (&p1)[3], const double (&p2)[3], const double (&o1)[2], const double (&o2)[2],
                                            S3Edge &a, S3Edge &b) {
    const double y0 = S.s * (S.R[0] * p2[0] + S.R[1] * p2[1] + S.R[2] * p2[2]) + S.t[0];
    const double y1 = S.s * (S.R[3] * p2[0] + S.R[4] * p2[1] + S.R[5] * p2[2]) + S.t[1];
    const double y2 = S.s * (S.R[6] * p2[0] + S.R[7] * p2[1] + S.R[8] * p2[2]) + S.t[2];
    a.iz = 1.0 / y2; a.u = y0 / y2; a.v = y1 / y2;                   // (true divisions: the restatement's operations, term for term)
    a.e0 = o1[0] - a.u; a.e1 = o1[1] - a.v;
    const double q0 = p1[0] - S.t[0], q1 = p1[1] - S.t[1], q2 = p1[2] - S.t[2];
    const double z0 = is * (S.R[0] * q0 + S.R[3] * q1 + S.R[6] * q2);
    const double z1 = is * (S.R[1] * q0 + S.R[4] * q1 + S.R[7] * q2);
    const double z2 = is * (S.R[2] * q0 + S.R[5] * q1 + S.R[8] * q2);
    b.iz = 1.0 / z2; b.u = z0 / z2; b.v = z1 / z2;
    b.e0 = o2[0] - b.u; b.e1 = o2[1] - b.v;
}

// both edges of one match, evaluated and linearised at S.  With y the mapped point, d(exp(dx) y) / d dx = [-[y]x | I | y]:
//   edge 12: J = -dproj(y) [-[y]x | I | y]; in (u, v, 1 / z) that is the closed form below, whose scale column vanishes (proj(c y) = proj(y));
//   edge 21: S'^-1 = S^-1 exp(-dx), so J = M [-[p1]x | I | p1] with M = dproj(z) (1 / s) R^T.
__device__ __forceinline__ void match_sweep(const S3State &S, double is, bool fix, double delta, const double (&p1)[3], const double (&p2)[3], const double (&o1)[2],
                                            const double (&o2)[2], double i1, double i2, S3Acc &A) {
    S3Edge a, b;
    edge_errors(S, is, p1, p2, o1, o2, a, b);
    {
        const double u = a.u, v = a.v, iz = a.iz;
        const double J0[7] = {u * v, -(1.0 + u * u), v, -iz, 0.0, u * iz, 0.0};
        const double J1[7] = {1.0 + v * v, -(u * v), -u, 0.0, -iz, v * iz, 0.0};
        add_edge(A, J0, J1, a.e0, a.e1, i1, delta);
    }
    {
        const double u = b.u, v = b.v, g = is * b.iz;
        double M0[3], M1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { M0[c] = g * (S.R[3 * c] - u * S.R[3 * c + 2]); M1[c] = g * (S.R[3 * c + 1] - v * S.R[3 * c + 2]); }
        const double J0[7] = {M0[2] * p1[1] - M0[1] * p1[2], M0[0] * p1[2] - M0[2] * p1[0], M0[1] * p1[0] - M0[0] * p1[1], M0[0], M0[1], M0[2],
                              fix ? 0.0 : M0[0] * p1[0] + M0[1] * p1[1] + M0[2] * p1[2]};
        const double J1[7] = {M1[2] * p1[1] - M1[1] * p1[2], M1[0] * p1[2] - M1[2] * p1[0], M1[1] * p1[0] - M1[0] * p1[1], M1[0], M1[1], M1[2],
                              fix ? 0.0 : M1[0] * p1[0] + M1[1] * p1[1] + M1[2] * p1[2]};
        add_edge(A, J0, J1, b.e0, b.e1, i2, delta);
    }
}

// Sim3::exp (sim3.h): s = exp(sigma), the rotation by Rodrigues, t = (A Omega + B Omega^2 + C I) upsilon with g2o's four (A, B, C) cases, eps = 1e-5
__device__ __forceinline__ void sim3_exp(const double (&dx)[7], S3State &E) {
    constexpr double eps = 1e-5;
    const double w0 = dx[0], w1 = dx[1], w2 = dx[2], sigma = dx[6];
    const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double s = exp(sigma);
    const double O[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    double O2[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    double a, b2, A, B, C;
    const bool small_theta = theta < eps, small_sigma = fabs(sigma) < eps;
    const double sn = sin(theta), cs = cos(theta);
    if (small_theta) { a = 1.0; b2 = 0.5; }
    else { a = sn / theta; b2 = (1.0 - cs) / (theta * theta); }
    if (small_sigma) {
        C = 1.0;
        if (small_theta) { A = 0.5; B = 1.0 / 6.0; }
        else { A = (1.0 - cs) / (theta * theta); B = (theta - sn) / (theta * theta * theta); }
    } else {
        C = (s - 1.0) / sigma;
        if (small_theta) {
            A = ((sigma - 1.0) * s + 1.0) / (sigma * sigma);
            B = ((0.5 * sigma * sigma - sigma + 1.0) * s - 1.0) / (sigma * sigma * sigma);
        } else {
            const double ca = s * sn, cb = s * cs, cc = theta * theta + sigma * sigma;
            A = (ca * sigma + (1.0 - cb) * theta) / (theta * cc);
            B = (C - ((cb - 1.0) * sigma + ca * theta) / cc) / (theta * theta);
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) E.R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + a * O[i] + b2 * O2[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double v = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) v += (A * O[3 * i + j] + B * O2[3 * i + j] + (i == j ? C : 0.0)) * dx[3 + j];
        E.t[i] = v;
    }
    E.s = s;
}

// (A * B) = (A.r B.r, A.s (A.r B.t) + A.t, A.s B.s)
__device__ __forceinline__ void sim3_mul(const S3State &A, const S3State &B, S3State &out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out.R[3 * i + j] = A.R[3 * i] * B.R[j] + A.R[3 * i + 1] * B.R[3 + j] + A.R[3 * i + 2] * B.R[6 + j];
        out.t[i] = A.s * (A.R[3 * i] * B.t[0] + A.R[3 * i + 1] * B.t[1] + A.R[3 * i + 2] * B.t[2]) + A.t[i];
    }
    out.s = A.s * B.s;
}

__global__ __launch_bounds__(kThreads) void k_sim3_opt(const S3Desc *__restrict__ descs, const double *__restrict__ planes, long long plane_stride,
                                                       const float *__restrict__ info, ms_sim3_opt_result *__restrict__ results, double *__restrict__ chi2_out) {
    __shared__ __attribute__((aligned(16))) double s_red[kSums * kRow];
    __shared__ __attribute__((aligned(16))) double s_sum[2][kSums];        // [cur] belongs to the accepted state (its H, b, chi2), the other to the trial
    const S3Desc &D = descs[blockIdx.x];
    const int tid = threadIdx.x, n = D.n;
    const bool fix = D.fix_scale != 0;
    const double delta = D.delta;
    S3State S = D.S0;
    if (n == 0) {                                                          // no edge: g2o has no active vertex, the estimate comes back unchanged
        if (tid == 0) {
            ms_sim3_opt_result r;
            for (int i = 0; i < 9; ++i) r.R12[i] = S.R[i];
            for (int i = 0; i < 3; ++i) r.t12[i] = S.t[i];
            r.scale12 = S.s; r.chi2_init = 0; r.chi2_final = 0; r.lambda = 0; r.iters = 0; r.trials_total = 0; r.stop_reason = 0; r.reserved = 0;
            results[blockIdx.x] = r;
        }
        return;
    }
    const double *pl = planes + D.m_off;
    const float *in1 = info + D.m_off, *in2 = info + plane_stride + D.m_off;
    // the resident matches: slot j of thread tid is match tid + kThreads j
    double X1[kSlots][3], X2[kSlots][3], U1[kSlots][2], U2[kSlots][2], I1[kSlots], I2[kSlots];
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
        const int m = tid + kThreads * j;
        const bool have = m < n;
#pragma unroll
        for (int k = 0; k < 3; ++k) { X1[j][k] = have ? pl[k * plane_stride + m] : 0.0; X2[j][k] = have ? pl[(3 + k) * plane_stride + m] : 0.0; }
#pragma unroll
        for (int k = 0; k < 2; ++k) { U1[j][k] = have ? pl[(6 + k) * plane_stride + m] : 0.0; U2[j][k] = have ? pl[(8 + k) * plane_stride + m] : 0.0; }
        I1[j] = have ? (double)in1[m] : 0.0;
        I2[j] = have ? (double)in2[m] : 0.0;
    }
    int cur = 1;
    // ---- one sweep over the matches at St: the sums land in s_sum[1 - cur]; returns the robust chi2
    auto sweep = [&](const S3State &St) {
        S3Acc A;
#pragma unroll
        for (int a = 0; a < 28; ++a) A.H[a] = 0;
#pragma unroll
        for (int a = 0; a < 7; ++a) A.b[a] = 0;
        A.chi = 0;
        const double is = 1.0 / St.s;
#pragma unroll
        for (int j = 0; j < kSlots; ++j)
            if (tid + kThreads * j < n) match_sweep(St, is, fix, delta, X1[j], X2[j], U1[j], U2[j], I1[j], I2[j], A);
        for (int m = kResident + tid; m < n; m += kThreads) {             // beyond the registers: streamed, coalesced
            const double p1[3] = {pl[m], pl[plane_stride + m], pl[2 * plane_stride + m]};
            const double p2[3] = {pl[3 * plane_stride + m], pl[4 * plane_stride + m], pl[5 * plane_stride + m]};
            const double o1[2] = {pl[6 * plane_stride + m], pl[7 * plane_stride + m]}, o2[2] = {pl[8 * plane_stride + m], pl[9 * plane_stride + m]};
            match_sweep(St, is, fix, delta, p1, p2, o1, o2, (double)in1[m], (double)in2[m], A);
        }
        // neighbouring lanes meet first (quad_perm [1 0 3 2]: both get the same sum), the even one writes
        double *row = s_red + (tid >> 1);
#pragma unroll
        for (int a = 0; a < 28; ++a) { const double v = A.H[a] + dpp_d<0xB1>(A.H[a]); if (!(tid & 1)) row[a * kRow] = v; }
#pragma unroll
        for (int a = 0; a < 7; ++a) { const double v = A.b[a] + dpp_d<0xB1>(A.b[a]); if (!(tid & 1)) row[(28 + a) * kRow] = v; }
        { const double v = A.chi + dpp_d<0xB1>(A.chi); if (!(tid & 1)) row[35 * kRow] = v; }
        __syncthreads();
        if (tid < 4 * kSums) {                                            // lanes 4 v .. 4 v + 3 add row v up, 32 entries each, then among themselves
            const int v = tid >> 2, part = tid & 3;
            const double *r = s_red + v * kRow + part;
            double s0 = 0, s1 = 0;
#pragma unroll
            for (int k = 0; k < kThreads / 8; k += 2) { s0 += r[4 * k]; s1 += r[4 * k + 4]; }
            double s = s0 + s1;
            s += dpp_d<0xB1>(s);                                          // quad_perm [1 0 3 2]
            s += dpp_d<0x4E>(s);                                          // quad_perm [2 3 0 1]
            if (part == 0) s_sum[1 - cur][v] = s;
        }
        __syncthreads();
        return s_sum[1 - cur][35];
    };
    double lambda = 0, ni = 2;
    int it = 0, trials = 0, stop = 0;
    const double chi2_init = sweep(S);
    cur = 1 - cur;
    double chi2_carried = chi2_init;
    for (it = 0; it < D.max_iters; ++it) {
        double current = chi2_carried, temp = current;
        const double *H = s_sum[cur];
        if (it == 0) {                                                     // computeLambdaInit: 1e-5 x the largest diagonal entry (a NaN stays a NaN)
            double md = 0;
            int k = 0;
#pragma unroll
            for (int a = 0; a < 7; ++a) { const double d = fabs(H[k]); md = (d > md || d != d) ? d : md; k += 7 - a; }
            lambda = 1e-5 * md; ni = 2;
        }
        double rho = 0;
        int qmax = 0;
        do {
            // (H + lambda I) dx = b: Cholesky of the 7 x 7 matrix by every thread for itself, lower triangle row-major Lm[i (i + 1) / 2 + j]
            double Lm[28], dxv[7], b[7];
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 7; ++a) b[a] = H[28 + a];
            {
                int k = 0;
#pragma unroll
                for (int a = 0; a < 7; ++a)
#pragma unroll
                    for (int c = a; c < 7; ++c) { Lm[c * (c + 1) / 2 + a] = H[k] + (a == c ? lambda : 0.0); ++k; }
            }
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                double d = Lm[j * (j + 1) / 2 + j];
#pragma unroll
                for (int k = 0; k < j; ++k) d -= Lm[j * (j + 1) / 2 + k] * Lm[j * (j + 1) / 2 + k];
                if (!(d > 0) || !isfinite(d)) ok = false;
                const double inv = rsqrt_d(d);
                Lm[j * (j + 1) / 2 + j] = inv;                             // the reciprocal pivot is what the substitutions use
#pragma unroll
                for (int i = j + 1; i < 7; ++i) {
                    double v = Lm[i * (i + 1) / 2 + j];
#pragma unroll
                    for (int k = 0; k < j; ++k) v -= Lm[i * (i + 1) / 2 + k] * Lm[j * (j + 1) / 2 + k];
                    Lm[i * (i + 1) / 2 + j] = v * inv;
                }
            }
            {
                double y[7];
#pragma unroll
                for (int i = 0; i < 7; ++i) {
                    double v = b[i];
#pragma unroll
                    for (int k = 0; k < i; ++k) v -= Lm[i * (i + 1) / 2 + k] * y[k];
                    y[i] = v * Lm[i * (i + 1) / 2 + i];
                }
#pragma unroll
                for (int i = 6; i >= 0; --i) {
                    double v = y[i];
#pragma unroll
                    for (int k = i + 1; k < 7; ++k) v -= Lm[k * (k + 1) / 2 + i] * dxv[k];
                    dxv[i] = v * Lm[i * (i + 1) / 2 + i];
                }
            }
            ok = __builtin_amdgcn_readfirstlane(ok ? 1 : 0) != 0;          // (the same in every lane: say so to the compiler)
            S3State T = S;
            double sc = 0;
            if (ok) {
#pragma unroll
                for (int a = 0; a < 7; ++a) sc += dxv[a] * (lambda * dxv[a] + b[a]);
                if (fix) dxv[6] = 0.0;                                      // VertexSim3Expmap::oplusImpl under _fix_scale
                S3State E;
                sim3_exp(dxv, E);
                sim3_mul(E, S, T);
                temp = sweep(T);
            } else temp = DBL_MAX;
            const double scale = sc + 1e-3;
            rho = (current - temp) / scale;
            if (rho > 0 && isfinite(temp)) {
                const double t3 = 2 * rho - 1;
                double alpha = 1. - t3 * t3 * t3;
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2; current = temp; chi2_carried = temp;
                S = T;
                cur = 1 - cur;                                             // the trial's sums are the accepted state's
                H = s_sum[cur];
            } else {
                lambda *= ni; ni *= 2;
                if (!isfinite(lambda)) break;
            }
            ++qmax; ++trials;
        } while (rho < 0 && qmax < 10);
        if (qmax == 10 || rho == 0 || !isfinite(lambda)) { stop = 1; ++it; break; }       // Terminate
    }
    if (D.want_chi2) {                                                     // chi2 per edge at the returned state: edge 12 then edge 21 of each match
        double *out = chi2_out + 2 * D.m_off;
        const double is = 1.0 / S.s;
        for (int m = tid; m < n; m += kThreads) {
            const double p1[3] = {pl[m], pl[plane_stride + m], pl[2 * plane_stride + m]};
            const double p2[3] = {pl[3 * plane_stride + m], pl[4 * plane_stride + m], pl[5 * plane_stride + m]};
            const double o1[2] = {pl[6 * plane_stride + m], pl[7 * plane_stride + m]}, o2[2] = {pl[8 * plane_stride + m], pl[9 * plane_stride + m]};
            S3Edge a, b;
            edge_errors(S, is, p1, p2, o1, o2, a, b);
            out[2 * (size_t)m] = (double)in1[m] * (a.e0 * a.e0 + a.e1 * a.e1);
            out[2 * (size_t)m + 1] = (double)in2[m] * (b.e0 * b.e0 + b.e1 * b.e1);
        }
    }
    if (tid == 0) {
        ms_sim3_opt_result r;
        for (int i = 0; i < 9; ++i) r.R12[i] = S.R[i];
        for (int i = 0; i < 3; ++i) r.t12[i] = S.t[i];
        r.scale12 = S.s; r.chi2_init = chi2_init; r.chi2_final = chi2_carried; r.lambda = lambda;
        r.iters = it; r.trials_total = trials; r.stop_reason = stop; r.reserved = 0;
        results[blockIdx.x] = r;
    }
}

}  // namespace

extern "C" int ms_sim3_optimize(ms_ctx *c, const ms_sim3_opt_problem *problems, int n, ms_sim3_opt_result *results, double *const *chi2_per_edge) {
    if (!c) return MS_ERR_INVALID;
    if (n < 0 || (n > 0 && (!problems || !results))) return ms_fail(c, MS_ERR_INVALID, "sim3 optimize: bad arguments");
    if (n > MS_SIM3_OPT_MAX_PROBLEMS) return ms_fail(c, MS_ERR_CAPACITY, "sim3 optimize: %d problems, at most %d per call", n, MS_SIM3_OPT_MAX_PROBLEMS);
    if (n == 0) return MS_OK;
    MsRange range("OptimizeSim3Transform");
    // validate everything before anything is written
    long long M = 0;
    for (int p = 0; p < n; ++p) {
        const ms_sim3_opt_problem &P = problems[p];
        if (P.n_matches < 0 || P.max_iters < 0 || !std::isfinite(P.huber_delta))
            return ms_fail(c, MS_ERR_INVALID, "sim3 optimize: problem %d: bad count, iteration limit or Huber delta", p);
        if (P.n_matches > MS_SIM3_OPT_MAX_MATCHES)
            return ms_fail(c, MS_ERR_CAPACITY, "sim3 optimize: problem %d: %d matches, cap %d", p, P.n_matches, MS_SIM3_OPT_MAX_MATCHES);
        if (P.n_matches > 0 && (!P.pts1 || !P.pts2 || !P.obs1 || !P.obs2 || !P.info1 || !P.info2))
            return ms_fail(c, MS_ERR_INVALID, "sim3 optimize: problem %d: missing match data", p);
        M += P.n_matches;
    }
    bool want_chi2 = false;
    if (chi2_per_edge)
        for (int p = 0; p < n; ++p) want_chi2 |= chi2_per_edge[p] != nullptr && problems[p].n_matches > 0;
    // upload block: descriptors | 10 planes of doubles (p1 xyz, p2 xyz, obs1 uv, obs2 uv) | 2 planes of floats (info1, info2); a plane holds every problem's matches
    const size_t stride = ms_align_up((size_t)std::max<long long>(M, 1), 32);
    // (the planes lie back to back: stride is a multiple of 32 elements, so each group of planes ends on a 256-byte boundary by itself)
    MsLayout up;
    const auto l_desc = up.array<S3Desc>((size_t)n);
    const auto l_pl = up.array<double>(kPlanes * stride);
    const auto l_info = up.array<float>(2 * stride);
    // download block (offsets from its own start): results | chi2 per edge
    MsLayout down;
    const auto l_res = down.array<ms_sim3_opt_result>((size_t)n);
    const auto l_chi = down.array<double>(2 * (size_t)M);
    const size_t down_bytes = want_chi2 ? down.end : l_chi.off;
    // host block and device block alike: upload block | download block
    MsLayout both = up;
    const size_t o_down = both.take(down.end);
    MS_HIP(c, hipSetDevice(c->device));
    int rc;
    MsWorkspace &W = c->ws[MS_WS_SIM3_OPT];
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, both.end, false)) || (rc = ms_grow(c, W.host, W.host_bytes, both.end, true))) return rc;
    void *hs = W.host, *ds = W.dev;
    S3Desc *hd = l_desc.at(hs);
    double *hp = l_pl.at(hs);
    float *hi = l_info.at(hs);
    long long mo = 0;
    for (int p = 0; p < n; ++p) {
        const ms_sim3_opt_problem &P = problems[p];
        S3Desc &d = hd[p];
        d.m_off = mo; d.n = P.n_matches; d.fix_scale = P.fix_scale ? 1 : 0; d.max_iters = P.max_iters;
        d.want_chi2 = chi2_per_edge && chi2_per_edge[p] && P.n_matches > 0 ? 1 : 0;
        d.delta = P.huber_delta;
        std::memcpy(d.S0.R, P.R12, sizeof(d.S0.R));
        std::memcpy(d.S0.t, P.t12, sizeof(d.S0.t));
        d.S0.s = P.scale12;
        for (int i = 0; i < P.n_matches; ++i) {
            for (int k = 0; k < 3; ++k) { hp[k * stride + mo + i] = P.pts1[3 * (size_t)i + k]; hp[(3 + k) * stride + mo + i] = P.pts2[3 * (size_t)i + k]; }
            for (int k = 0; k < 2; ++k) { hp[(6 + k) * stride + mo + i] = P.obs1[2 * (size_t)i + k]; hp[(8 + k) * stride + mo + i] = P.obs2[2 * (size_t)i + k]; }
            hi[mo + i] = P.info1[i];
            hi[stride + mo + i] = P.info2[i];
        }
        mo += P.n_matches;
    }
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    void *dout = ms_at<uint8_t>(ds, o_down), *hout = ms_at<uint8_t>(hs, o_down);
    hipLaunchKernelGGL(k_sim3_opt, dim3((unsigned)n), dim3(kThreads), 0, c->stream, l_desc.at(ds), l_pl.at(ds), (long long)stride, l_info.at(ds),
                       l_res.at(dout), l_chi.at(dout));
    MS_KERNEL_CHECK(c, "k_sim3_opt");
    MS_HIP(c, hipMemcpyAsync(hout, dout, down_bytes, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    l_res.get(hout, 0, results, (size_t)n);
    mo = 0;
    for (int p = 0; p < n; ++p) {
        const int nm = problems[p].n_matches;
        if (chi2_per_edge && chi2_per_edge[p]) l_chi.get(hout, 2 * (size_t)mo, chi2_per_edge[p], 2 * (size_t)nm);
        mo += nm;
    }
    return MS_OK;
}
