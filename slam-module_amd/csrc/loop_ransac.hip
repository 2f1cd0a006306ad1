// loop_ransac.hip -- N4: the loop-closure RANSAC behind LoopRansac::ransacSolve (loop_ransac.cpp:8-314).
//
// Every problem of a call is one LoopRansac object: n matched points seen from two keyframes and n_iter sampled triplets.  The work
// is hypotheses x matches, independent except for the choice of the best hypothesis, so one call is one chain on the context stream:
//
//   k_ransac_hyp     grid (64 hypotheses, problem), one lane per hypothesis: the triplet's Horn (SIM3: 4x4 symmetric N, cyclic Jacobi in
//                    registers, eigenvector of the largest eigenvalue) or z-rotation (ZROT: closed form) solution, the float scale, the
//                    fix-scale and s12 / R12 / t12 steps of :85-91; one record per hypothesis.  Also resets the problem's best key and
//                    its per-match "first inlier iteration" words.
//   k_ransac_count   grid (16 hypotheses, problem), 4 waves: the problem's matches are staged through LDS in chunks of kChunk (points,
//                    own-image reprojections, thresholds with the own-image visibility folded in); a wave tests one hypothesis against
//                    64 matches at a time and counts with a ballot.  Per hypothesis: its count, and an integer atomicMax of
//                    (count << 32 | ~iter) into the problem's key -- the largest count, then the earliest iteration (:98).  Per match:
//                    the earliest iteration that made it an inlier (LDS atomicMin per chunk, one global atomicMin per match).
//   k_ransac_finish  one workgroup per problem: ok / count / best iteration from the key, the best record, the reference's union mask
//                    (first inlier iteration <= best: its inlier vector is never cleared, :64, :202) and the best hypothesis's own mask
//                    (re-tested); everything lands in one block that is downloaded once.
//
// Only integer atomics: the result does not depend on scheduling.  All arithmetic is IEEE fp64 (division and sqrt included; the library
// builds with -ffp-contract=off), the two float roundings of the reference (the scale, s12) are explicit.
#include "ms_internal.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int kHypPerLane = 64;          // k_ransac_hyp: hypotheses per workgroup (one wave)
constexpr int kHypPerBlock = 16;         // k_ransac_count: 4 waves x 4 hypotheses
constexpr int kChunk = 512;              // k_ransac_count: matches staged in LDS at a time (88 B each: 44 KiB)
constexpr int kJacobiSweeps = 16;        // cap of the cyclic Jacobi (a 4x4 converges in 4-6)

struct LrDesc {                          // one problem as the kernels see it
    long long m_off, h_off;              // first match / hypothesis in the call's packed arrays
    int32_t n, n_iter;                   // n_iter = 0 when the early return applies
    int32_t dof, fix_scale, min_inliers, early;
    ms_pinhole cam1, cam2;
};

struct LrHyp {                           // one hypothesis: what k_ransac_count applies and what the result reports
    double A21[9], t21[3];               // (s21 * R21, t21): keyframe 1 points into camera 2
    double A12[9], t12[3];               // (s12 * R12, t12): keyframe 2 points into camera 1
    double R12[9];
    float s12;
    int32_t pad;
};

// the pinhole stand-in for reprojectToImage (keyframe.cpp:340-356): p_c = A p + t, visible iff z > 0 and the pixel is in the image;
// every comparison with NaN is false, so a non-finite point is invisible
__device__ __forceinline__ bool project(const ms_pinhole &c, const double *A, const double *t, double x, double y, double z, double &u, double &v) {
    const double px = A[0] * x + A[1] * y + A[2] * z + t[0];
    const double py = A[3] * x + A[4] * y + A[5] * z + t[1];
    const double pz = A[6] * x + A[7] * y + A[8] * z + t[2];
    u = c.fx * (px / pz) + c.cx;
    v = c.fy * (py / pz) + c.cy;
    return pz > 0.0 && u >= 0.0 && u < (double)c.width && v >= 0.0 && v < (double)c.height;
}

// own-image reprojection (identity pose, :43-44, :256-275): I p + 0 == p exactly, so the projection of p itself
__device__ __forceinline__ bool project_own(const ms_pinhole &c, double x, double y, double z, double &u, double &v) {
    u = c.fx * (x / z) + c.cx;
    v = c.fy * (y / z) + c.cy;
    return z > 0.0 && u >= 0.0 && u < (double)c.width && v >= 0.0 && v < (double)c.height;
}

// one match against one hypothesis (:212-225), given its own-image projections and its thresholds (-inf when an own-image projection is invisible)
__device__ __forceinline__ bool is_inlier(const LrDesc &D, const LrHyp &H, const double *p1, const double *p2, double r1u, double r1v, double r2u,
                                          double r2v, float thr1, float thr2) {
    double u2, v2, u1, v1;
    const bool vis1 = project(D.cam2, H.A21, H.t21, p1[0], p1[1], p1[2], u2, v2);
    const bool vis2 = project(D.cam1, H.A12, H.t12, p2[0], p2[1], p2[2], u1, v1);
    const double dx2 = u2 - r2u, dy2 = v2 - r2v, dx1 = u1 - r1u, dy1 = v1 - r1v;
    const double e2 = dx2 * dx2 + dy2 * dy2, e1 = dx1 * dx1 + dy1 * dy1;
    return vis1 && vis2 && e2 < (double)thr2 && e1 < (double)thr1;
}

// thresholds with the own-image visibility folded in: an invisible match can never pass e < thr
__device__ __forceinline__ void own_image(const LrDesc &D, const double *p1, const double *p2, const float *thr1, const float *thr2, long long i,
                                          double &r1u, double &r1v, double &r2u, double &r2v, float &t1, float &t2) {
    const bool vs1 = project_own(D.cam1, p1[0], p1[1], p1[2], r1u, r1v);
    const bool vs2 = project_own(D.cam2, p2[0], p2[1], p2[2], r2u, r2v);
    t1 = (vs1 && vs2) ? thr1[i] : -INFINITY;
    t2 = (vs1 && vs2) ? thr2[i] : -INFINITY;
}

// Horn's N of the centred sets (:135-151), M = sum_k a1_k a2_k^T
__device__ __forceinline__ void horn_n(const double (&a1)[3][3], const double (&a2)[3][3], double (&N)[4][4]) {
    double M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i][j] = a1[0][i] * a2[0][j] + a1[1][i] * a2[1][j] + a1[2][i] * a2[2][j];
    const double Sxx = M[0][0], Syx = M[1][0], Szx = M[2][0], Sxy = M[0][1], Syy = M[1][1], Szy = M[2][1], Sxz = M[0][2], Syz = M[1][2], Szz = M[2][2];
    N[0][0] = Sxx + Syy + Szz; N[0][1] = Syz - Szy;       N[0][2] = Szx - Sxz;        N[0][3] = Sxy - Syx;
    N[1][0] = Syz - Szy;       N[1][1] = Sxx - Syy - Szz; N[1][2] = Sxy + Syx;        N[1][3] = Szx + Sxz;
    N[2][0] = Szx - Sxz;       N[2][1] = Sxy + Syx;       N[2][2] = -Sxx + Syy - Szz; N[2][3] = Syz + Szy;
    N[3][0] = Sxy - Syx;       N[3][1] = Szx + Sxz;       N[3][2] = Syz + Szy;        N[3][3] = -Sxx - Syy + Szz;
}

// cyclic Jacobi on a symmetric 4x4, in registers (every index is a compile-time constant); V = eigenvectors in columns, diag(a) = eigenvalues.
// Stops when the off-diagonal mass is below 1e-30 of the total (rounding level) or after kJacobiSweeps sweeps (a NaN matrix runs to the cap).
__device__ __forceinline__ void jacobi4(double (&a)[4][4], double (&V)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        double off = 0.0, tot = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double s = a[i][j] * a[i][j];
                tot += s;
                if (i != j) off += s;
            }
        if (off <= 1e-30 * tot) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double at = fabs(theta);
                double t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {            // columns p, q
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {            // rows p, q
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

// s * R * c1 subtracted from c2, with s the float scale widened (:195)
__device__ __forceinline__ void trans_from(const double (&R)[9], float s, const double (&c1)[3], const double (&c2)[3], double (&t)[3]) {
    const double sd = (double)s;
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = c2[i] - ((sd * R[3 * i]) * c1[0] + (sd * R[3 * i + 1]) * c1[1] + (sd * R[3 * i + 2]) * c1[2]);
}

// scale numer / denom of :184-191 and :309, rounded to float
__device__ __forceinline__ float scale_of(const double (&R)[9], const double (&a1)[3][3], const double (&a2)[3][3]) {
    double numer = 0.0, denom = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double r = R[3 * i] * a1[k][0] + R[3 * i + 1] * a1[k][1] + R[3 * i + 2] * a1[k][2];
            numer += a2[k][i] * r;
            denom += a1[k][i] * a1[k][i];
        }
    }
    return (float)(numer / denom);
}

__global__ __launch_bounds__(kHypPerLane) void k_ransac_hyp(const LrDesc *__restrict__ descs, const double *__restrict__ pts1, const double *__restrict__ pts2,
                                                            const int32_t *__restrict__ samples, LrHyp *__restrict__ hyps,
                                                            unsigned long long *__restrict__ keys, uint32_t *__restrict__ first_iter) {
    const LrDesc D = descs[blockIdx.y];
    for (long long i = (long long)blockIdx.x * kHypPerLane + threadIdx.x; i < D.n; i += (long long)gridDim.x * kHypPerLane) first_iter[D.m_off + i] = 0xFFFFFFFFu;
    if (blockIdx.x == 0 && threadIdx.x == 0) keys[blockIdx.y] = 0ull;
    const int h = blockIdx.x * kHypPerLane + threadIdx.x;
    if (h >= D.n_iter) return;
    const int32_t *smp = samples + 3 * (D.h_off + h);
    double P1[3][3], P2[3][3];             // [sample][coordinate]
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long m = D.m_off + smp[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) { P1[k][j] = pts1[3 * m + j]; P2[k][j] = pts2[3 * m + j]; }
    }
    double c1[3], c2[3], a1[3][3], a2[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        c1[j] = (P1[0][j] + P1[1][j] + P1[2][j]) / 3.0;
        c2[j] = (P2[0][j] + P2[1][j] + P2[2][j]) / 3.0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) { a1[k][j] = P1[k][j] - c1[j]; a2[k][j] = P2[k][j] - c2[j]; }

    double R[9];
    if (D.dof == MS_RANSAC_ZROT) {         // :293-307
        double C = 0.0, S = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { C += a1[k][0] * a2[k][0]; C += a1[k][1] * a2[k][1]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) S += a1[k][0] * a2[k][1] - a1[k][1] * a2[k][0];
        const double h2 = sqrt(C * C + S * S);
        const double ct = C / h2, st = S / h2;
        R[0] = ct; R[1] = -st; R[2] = 0.0;
        R[3] = st; R[4] = ct;  R[5] = 0.0;
        R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
    } else {                               // :135-179
        double N[4][4], V[4][4];
        horn_n(a1, a2, N);
        jacobi4(N, V);
        int best = 0;
        double bv = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (bv <= N[i][i]) { bv = N[i][i]; best = i; }        // the last maximum wins, as in :162-167
        double q[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = best == 0 ? V[i][0] : best == 1 ? V[i][1] : best == 2 ? V[i][2] : V[i][3];
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {             // Vector4d::normalize, then Quaterniond::normalized
            const double z = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
            if (z > 0.0) {
                const double nz = sqrt(z);
#pragma unroll
                for (int i = 0; i < 4; ++i) q[i] = q[i] / nz;
            }
        }
        const double w = q[0], x = q[1], y = q[2], z = q[3];  // Quaterniond(w, x, y, z) -> rotation matrix
        const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
        const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
        R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
        R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
        R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
    }
    float s21 = scale_of(R, a1, a2);
    double t21[3];
    trans_from(R, s21, c1, c2, t21);       // with the unfixed scale, also under fix-scale (:85-86)
    if (D.fix_scale) s21 = 1.0f;
    const float s12 = 1.0f / s21;
    LrHyp H;
    const double sd21 = (double)s21, sd12 = (double)s12, ns12 = (double)(-s12);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            H.R12[3 * i + j] = R[3 * j + i];
            H.A21[3 * i + j] = sd21 * R[3 * i + j];
            H.A12[3 * i + j] = sd12 * R[3 * j + i];
        }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        H.t21[i] = t21[i];
        H.t12[i] = (ns12 * H.R12[3 * i]) * t21[0] + (ns12 * H.R12[3 * i + 1]) * t21[1] + (ns12 * H.R12[3 * i + 2]) * t21[2];
    }
    H.s12 = s12;
    H.pad = 0;
    hyps[D.h_off + h] = H;
}

__global__ __launch_bounds__(256) void k_ransac_count(const LrDesc *__restrict__ descs, const double *__restrict__ pts1, const double *__restrict__ pts2,
                                                      const float *__restrict__ thr1, const float *__restrict__ thr2, const LrHyp *__restrict__ hyps,
                                                      unsigned long long *__restrict__ keys, uint32_t *__restrict__ first_iter, int32_t *__restrict__ counts) {
    __shared__ double s_p1[3][kChunk], s_p2[3][kChunk], s_r1[2][kChunk], s_r2[2][kChunk];
    __shared__ float s_t1[kChunk], s_t2[kChunk];
    __shared__ uint32_t s_first[kChunk];
    const LrDesc D = descs[blockIdx.y];
    const int h0 = blockIdx.x * kHypPerBlock;
    if (h0 >= D.n_iter) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int cnt[4] = {0, 0, 0, 0};
    for (int c0 = 0; c0 < D.n; c0 += kChunk) {
        const int cn = min(kChunk, D.n - c0);
        for (int j = threadIdx.x; j < cn; j += blockDim.x) {
            const long long i = D.m_off + c0 + j;
            double p1[3], p2[3], r1u, r1v, r2u, r2v;
            float t1, t2;
#pragma unroll
            for (int k = 0; k < 3; ++k) { p1[k] = pts1[3 * i + k]; p2[k] = pts2[3 * i + k]; }
            own_image(D, p1, p2, thr1, thr2, i, r1u, r1v, r2u, r2v, t1, t2);
#pragma unroll
            for (int k = 0; k < 3; ++k) { s_p1[k][j] = p1[k]; s_p2[k][j] = p2[k]; }
            s_r1[0][j] = r1u; s_r1[1][j] = r1v; s_r2[0][j] = r2u; s_r2[1][j] = r2v;
            s_t1[j] = t1; s_t2[j] = t2;
            s_first[j] = 0xFFFFFFFFu;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int h = h0 + 4 * wave + k;
            if (h >= D.n_iter) break;                          // wave-uniform
            const LrHyp H = hyps[D.h_off + h];
            for (int j0 = 0; j0 < cn; j0 += 64) {
                const int j = j0 + lane;
                bool in = false;
                if (j < cn) {
                    const double p1[3] = {s_p1[0][j], s_p1[1][j], s_p1[2][j]}, p2[3] = {s_p2[0][j], s_p2[1][j], s_p2[2][j]};
                    in = is_inlier(D, H, p1, p2, s_r1[0][j], s_r1[1][j], s_r2[0][j], s_r2[1][j], s_t1[j], s_t2[j]);
                    if (in) atomicMin(&s_first[j], (uint32_t)h);
                }
                cnt[k] += __popcll(__ballot(in));
            }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < cn; j += blockDim.x)
            if (s_first[j] != 0xFFFFFFFFu) atomicMin(&first_iter[D.m_off + c0 + j], s_first[j]);
        __syncthreads();                                       // the next chunk overwrites the staging
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int h = h0 + 4 * wave + k;
            if (h >= D.n_iter) break;
            counts[D.h_off + h] = cnt[k];
            atomicMax(&keys[blockIdx.y], ((unsigned long long)(uint32_t)cnt[k] << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)h));
        }
    }
}

__global__ __launch_bounds__(256) void k_ransac_finish(const LrDesc *__restrict__ descs, const double *__restrict__ pts1, const double *__restrict__ pts2,
                                                       const float *__restrict__ thr1, const float *__restrict__ thr2, const LrHyp *__restrict__ hyps,
                                                       const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ first_iter,
                                                       ms_loop_ransac_result *__restrict__ results, uint8_t *__restrict__ umask, uint8_t *__restrict__ smask) {
    const LrDesc D = descs[blockIdx.x];
    const unsigned long long key = D.early || D.n_iter == 0 ? 0ull : keys[blockIdx.x];
    const int count = (int)(key >> 32);
    const int best = count > 0 ? (int)(0xFFFFFFFFu - (uint32_t)key) : -1;
    if (threadIdx.x == 0) {
        ms_loop_ransac_result r;
        r.solution_ok = !D.early && count >= D.min_inliers;
        r.best_inlier_count = count;
        r.best_iter = best;
        const LrHyp *H = best >= 0 ? &hyps[D.h_off + best] : nullptr;
        for (int i = 0; i < 9; ++i) r.R12[i] = H ? H->R12[i] : 0.0;
        for (int i = 0; i < 3; ++i) r.t12[i] = H ? H->t12[i] : 0.0;
        r.scale12 = H ? H->s12 : 0.0f;
        results[blockIdx.x] = r;
    }
    if (best < 0) {
        for (int j = threadIdx.x; j < D.n; j += blockDim.x) { umask[D.m_off + j] = 0; smask[D.m_off + j] = 0; }
        return;
    }
    const LrHyp H = hyps[D.h_off + best];
    for (int j = threadIdx.x; j < D.n; j += blockDim.x) {
        const long long i = D.m_off + j;
        double p1[3], p2[3], r1u, r1v, r2u, r2v;
        float t1, t2;
#pragma unroll
        for (int k = 0; k < 3; ++k) { p1[k] = pts1[3 * i + k]; p2[k] = pts2[3 * i + k]; }
        own_image(D, p1, p2, thr1, thr2, i, r1u, r1v, r2u, r2v, t1, t2);
        smask[i] = is_inlier(D, H, p1, p2, r1u, r1v, r2u, r2v, t1, t2) ? 1 : 0;
        umask[i] = first_iter[i] <= (uint32_t)best ? 1 : 0;
    }
}

bool cam_ok(const ms_pinhole &c) { return c.width >= 1 && c.height >= 1; }

}  // namespace

extern "C" int ms_loop_ransac(ms_ctx *c, const ms_loop_ransac_problem *problems, int n, ms_loop_ransac_result *results,
                              uint8_t *const *union_inliers, uint8_t *const *best_inliers, int32_t *const *hyp_inliers) {
    if (!c) return MS_ERR_INVALID;
    if (n < 0 || (n > 0 && (!problems || !results))) return ms_fail(c, MS_ERR_INVALID, "loop ransac: bad arguments");
    if (n > MS_LOOP_RANSAC_MAX_PROBLEMS) return ms_fail(c, MS_ERR_CAPACITY, "loop ransac: %d problems, at most %d per call", n, MS_LOOP_RANSAC_MAX_PROBLEMS);
    if (n == 0) return MS_OK;
    MsRange range("ransacSolve");
    // validate everything before anything is written
    long long M = 0, H = 0;
    int max_iter = 0;
    for (int p = 0; p < n; ++p) {
        const ms_loop_ransac_problem &P = problems[p];
        if (P.n_matches < 0 || P.n_iter < 0 || P.min_inliers < 0 || (P.dof != MS_RANSAC_SIM3 && P.dof != MS_RANSAC_ZROT) || !cam_ok(P.cam1) || !cam_ok(P.cam2))
            return ms_fail(c, MS_ERR_INVALID, "loop ransac: problem %d: bad count, dof or camera", p);
        if (P.n_matches > MS_LOOP_RANSAC_MAX_MATCHES || P.n_iter > MS_LOOP_RANSAC_MAX_ITER)
            return ms_fail(c, MS_ERR_CAPACITY, "loop ransac: problem %d: %d matches / %d iterations, caps %d / %d", p, P.n_matches, P.n_iter,
                           MS_LOOP_RANSAC_MAX_MATCHES, MS_LOOP_RANSAC_MAX_ITER);
        if (P.n_matches > 0 && (!P.pts1 || !P.pts2 || !P.thr1 || !P.thr2)) return ms_fail(c, MS_ERR_INVALID, "loop ransac: problem %d: missing match data", p);
        M += P.n_matches;
        const bool early = P.n_matches < 3 || P.n_matches < P.min_inliers;                     // :52-54
        if (early) continue;
        if (P.n_iter > 0 && !P.samples) return ms_fail(c, MS_ERR_INVALID, "loop ransac: problem %d: no samples", p);
        for (int i = 0; i < P.n_iter; ++i) {
            const int32_t a = P.samples[3 * i], b = P.samples[3 * i + 1], d = P.samples[3 * i + 2];
            if (a < 0 || a >= P.n_matches || b < 0 || b >= P.n_matches || d < 0 || d >= P.n_matches)
                return ms_fail(c, MS_ERR_INVALID, "loop ransac: problem %d, iteration %d: sample outside [0, %d)", p, i, P.n_matches);
            if (a == b || a == d || b == d) return ms_fail(c, MS_ERR_INVALID, "loop ransac: problem %d, iteration %d: repeated sample index", p, i);
        }
        H += P.n_iter;
        max_iter = std::max(max_iter, P.n_iter);
    }
    // upload block: descriptors | pts1 | pts2 | thr1 | thr2 | samples
    const size_t np = (size_t)n, nm_all = (size_t)M, nh = (size_t)H;
    MsLayout up;
    const auto l_desc = up.array<LrDesc>(np);
    const auto l_p1 = up.array<double>(3 * nm_all), l_p2 = up.array<double>(3 * nm_all);
    const auto l_t1 = up.array<float>(nm_all), l_t2 = up.array<float>(nm_all);
    const auto l_smp = up.array<int32_t>(3 * nh);
    // download block (offsets from its own start): results | union masks | best masks | per-hypothesis counts
    MsLayout down;
    const auto l_res = down.array<ms_loop_ransac_result>(np);
    const auto l_um = down.array<uint8_t>(nm_all), l_sm = down.array<uint8_t>(nm_all);
    const auto l_cnt = down.array<int32_t>(nh);
    bool want_counts = false;
    if (hyp_inliers)
        for (int p = 0; p < n; ++p) want_counts |= hyp_inliers[p] != nullptr && problems[p].n_iter > 0;
    const size_t down_bytes = want_counts ? down.end : l_cnt.off;
    // host block: upload block | download block; the device block goes on with the work block: hypotheses | keys | first inlier iterations
    MsLayout host = up;
    const size_t o_down = host.take(down.end);
    MsLayout dev = host;
    const auto l_hyp = dev.array<LrHyp>(nh);
    const auto l_key = dev.array<unsigned long long>(np);
    const auto l_first = dev.array<uint32_t>(nm_all);
    MS_HIP(c, hipSetDevice(c->device));
    int rc;
    MsWorkspace &W = c->ws[MS_WS_LOOP_RANSAC];
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false)) || (rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    void *hs = W.host, *ds = W.dev;
    LrDesc *hd = l_desc.at(hs);
    long long mo = 0, ho = 0;
    for (int p = 0; p < n; ++p) {
        const ms_loop_ransac_problem &P = problems[p];
        const bool early = P.n_matches < 3 || P.n_matches < P.min_inliers;
        const int it = early ? 0 : P.n_iter;
        hd[p] = LrDesc{mo, ho, P.n_matches, it, P.dof, P.fix_scale ? 1 : 0, P.min_inliers, early ? 1 : 0, P.cam1, P.cam2};
        const size_t nm = (size_t)P.n_matches;
        l_p1.put(hs, 3 * (size_t)mo, P.pts1, 3 * nm);
        l_p2.put(hs, 3 * (size_t)mo, P.pts2, 3 * nm);
        l_t1.put(hs, (size_t)mo, P.thr1, nm);
        l_t2.put(hs, (size_t)mo, P.thr2, nm);
        l_smp.put(hs, 3 * (size_t)ho, P.samples, 3 * (size_t)it);
        mo += P.n_matches;
        ho += it;
    }
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    const LrDesc *dd = l_desc.at(ds);
    const double *dp1 = l_p1.at(ds), *dp2 = l_p2.at(ds);
    const float *dt1 = l_t1.at(ds), *dt2 = l_t2.at(ds);
    void *dout = ms_at<uint8_t>(ds, o_down), *hout = ms_at<uint8_t>(hs, o_down);
    LrHyp *dh = l_hyp.at(ds);
    unsigned long long *dk = l_key.at(ds);
    uint32_t *df = l_first.at(ds);
    hipLaunchKernelGGL(k_ransac_hyp, dim3((unsigned)std::max(1, ms_div_up(max_iter, kHypPerLane)), (unsigned)n), dim3(kHypPerLane), 0, c->stream,
                       dd, dp1, dp2, l_smp.at(ds), dh, dk, df);
    MS_KERNEL_CHECK(c, "k_ransac_hyp");
    if (max_iter > 0) {
        hipLaunchKernelGGL(k_ransac_count, dim3((unsigned)ms_div_up(max_iter, kHypPerBlock), (unsigned)n), dim3(256), 0, c->stream,
                           dd, dp1, dp2, dt1, dt2, dh, dk, df, l_cnt.at(dout));
        MS_KERNEL_CHECK(c, "k_ransac_count");
    }
    hipLaunchKernelGGL(k_ransac_finish, dim3((unsigned)n), dim3(256), 0, c->stream, dd, dp1, dp2, dt1, dt2, dh, dk, df,
                       l_res.at(dout), l_um.at(dout), l_sm.at(dout));
    MS_KERNEL_CHECK(c, "k_ransac_finish");
    MS_HIP(c, hipMemcpyAsync(hout, dout, down_bytes, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    l_res.get(hout, 0, results, np);
    mo = 0; ho = 0;
    for (int p = 0; p < n; ++p) {
        const int nm = problems[p].n_matches, it = hd[p].n_iter;
        if (union_inliers && union_inliers[p]) l_um.get(hout, (size_t)mo, union_inliers[p], (size_t)nm);
        if (best_inliers && best_inliers[p]) l_sm.get(hout, (size_t)mo, best_inliers[p], (size_t)nm);
        if (hyp_inliers && hyp_inliers[p] && problems[p].n_iter > 0) {
            if (it > 0) l_cnt.get(hout, (size_t)ho, hyp_inliers[p], (size_t)it);
            else std::memset(hyp_inliers[p], 0, 4 * (size_t)problems[p].n_iter);      // early return: nothing was tried
        }
        mo += nm;
        ho += it;
    }
    return MS_OK;
}
