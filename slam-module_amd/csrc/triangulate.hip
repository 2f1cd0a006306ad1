// triangulate.hip -- ms_triangulate: triangulateMapPoint / triangulateMapPointFirstLastObs (mapper_helpers.cpp:600-812) for chosen rows of
// the device map-point table, written where the table lies.  tests/triangulate_ref.py is the specification; this file follows
// it operation for operation.
//
// ms_triangulate takes the observation lists as host arrays and uploads them; ms_triangulate_lists reads the device lists of
// ms_observation_lists where they lie.  Both run the one launch sequence of tri_run.
//
// Two launches whatever the number of rows:
//   k_tri_rays    one lane per observation: the world ray R^T * bearing into the workspace (what the pair test of the angle check reads)
//   k_tri_points  a group of 16 lanes per map point, one observation per lane per round of 16:
//                   depth scan          the first observation with a depth, by ballot (TME / MIDPOINT, points that were not triangulated)
//                   angle check         the smallest dot product over the pairs of rays, pairs spread over the lanes, reduced with min
//                   sums                the ten unique entries of A (N-view) or the nine of the midpoint system: every lane forms its
//                                       observation's terms, a round is added as a butterfly inside the group, rounds in order
//                   solve               Jacobi on the 4x4 matrix / elimination on the 3x3 system, in fp64 registers, the same on every
//                                       lane of the group (no lane waits for another)
//                   checks              positive depth and reprojection error, one observation per lane; the first failing observation
//                                       by ballot (or the number of passing ones, FIRST_LAST)
//                 lane 0 writes the position, the flag byte and the status word.  Groups leave independently.
//
// Every floating-point operation is one rounded IEEE operation in the order the restatement writes it (contract(off), no fast-math; the
// float32 steps of checkReprojectionError are spelt with the *_rn intrinsics).  A butterfly sum gives every lane the same bits because
// a + b == b + a.  No atomics, no shared memory, no inline assembly.  Everything a kernel indexes with is validated on the host first.
#include "ms_internal.h"
#include "ms_bearing.h"
#include <algorithm>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kGroup = 16;               // lanes per map point; GROUP of the restatement
constexpr int kSweeps = 10;              // JACOBI_SWEEPS
constexpr double kPivotRel = 1e-10;      // PIVOT_REL
constexpr double kChi2Inv2D = 5.991;     // CHI2_INV2D, mapper_helpers.cpp:26

struct TriArgs {
    double *mp_pos;
    uint8_t *mp_flags;                   // may be null
    const double *kf_pose;
    const ms_pinhole *cam;
    const int32_t *focal;
    const float *sigma;
    const int32_t *rows;
    const uint8_t *was;
    const int32_t *obs_start, *obs_kf, *obs_oct;
    const float *obs_x, *obs_y, *obs_depth;      // obs_depth may be null
    double *ray;                         // workspace [n_obs * 3]
    int32_t *out;                        // workspace [n_rows * 2]: status | reason << 8, n_pass
    double cos_two, cos_multi;
    float rel_thr;
    int32_t n_rows, n_obs, n_levels, mode, dense;
};

struct Obs {
    double P[12];                        // rows 0-2 of poseCW
    double xn, yn, b[3];                 // normalizePixel, kp.bearing
};

__device__ __forceinline__ void load_obs(const TriArgs &A, int o, Obs &ob) {
    const int k = A.obs_kf[o];
    const double *P = A.kf_pose + 12 * (size_t)k;
#pragma unroll
    for (int i = 0; i < 12; ++i) ob.P[i] = P[i];
    const ms_pinhole c = A.cam[k];
    ms_pinhole_bearing(c, A.obs_x[o], A.obs_y[o], ob.xn, ob.yn, ob.b);
}
__device__ __forceinline__ void ray_of(const Obs &ob, double *r) {       // cameraToWorldRotation() * bearing
#pragma unroll
    for (int j = 0; j < 3; ++j) r[j] = ob.P[j] * ob.b[0] + ob.P[4 + j] * ob.b[1] + ob.P[8 + j] * ob.b[2];
}
__device__ __forceinline__ void centre_of(const Obs &ob, double *c) {    // cameraCenter()
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = -(ob.P[j] * ob.P[3] + ob.P[4 + j] * ob.P[7] + ob.P[8 + j] * ob.P[11]);
}
// depth * kf.cameraToWorldRotation() * kp.bearing + kf.cameraCenter(), :622 / :746
__device__ __forceinline__ void depth_position(const Obs &ob, float depth, double *X) {
    const double d = (double)depth;
    double c[3];
    centre_of(ob, c);
#pragma unroll
    for (int j = 0; j < 3; ++j) X[j] = (d * ob.P[j]) * ob.b[0] + (d * ob.P[4 + j]) * ob.b[1] + (d * ob.P[8 + j]) * ob.b[2] + c[j];
}

__global__ __launch_bounds__(kBlock) void k_tri_rays(const TriArgs A) {
    const int o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= A.n_obs) return;
    Obs ob;
    load_obs(A, o, ob);
    double r[3];
    ray_of(ob, r);
    double *out = A.ray + 3 * (size_t)o;
    out[0] = r[0]; out[1] = r[1]; out[2] = r[2];
}

// ------------------------------------------------------------------------------------------------ group helpers
__device__ __forceinline__ unsigned group_ballot(bool p) {   // the 16 bits of this lane's group
    return (unsigned)(__ballot(p) >> (threadIdx.x & 48)) & 0xffffu;
}
__device__ __forceinline__ double group_sum(double v) {      // the tree (i, i + 8), (i, i + 4), (i, i + 2), (0, 1); the same bits on every lane
    v = v + __shfl_xor(v, 8, kGroup);
    v = v + __shfl_xor(v, 4, kGroup);
    v = v + __shfl_xor(v, 2, kGroup);
    v = v + __shfl_xor(v, 1, kGroup);
    return v;
}
__device__ __forceinline__ double group_min(double v) {
#pragma unroll
    for (int x = 8; x >= 1; x >>= 1) {
        const double o = __shfl_xor(v, x, kGroup);
        if (o < v) v = o;
    }
    return v;
}

// ------------------------------------------------------------------------------------------------ solvers
// Cyclic Jacobi on the symmetric 4x4 matrix M; h = the column of the first smallest diagonal entry.
__device__ void smallest_eigenvector4(double (&M)[4][4], double *h) {
    double V[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = M[p][q];
                if (apq != 0.0) {
                    const double theta = (M[q][q] - M[p][p]) / (2.0 * apq);
                    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    if (theta < 0.0) t = -t;
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    M[p][p] = M[p][p] - t * apq;
                    M[q][q] = M[q][q] + t * apq;
                    M[p][q] = M[q][p] = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (k != p && k != q) {
                            const double akp = M[k][p], akq = M[k][q];
                            M[k][p] = M[p][k] = c * akp - s * akq;
                            M[k][q] = M[q][k] = s * akp + c * akq;
                        }
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
    }
    double w = M[0][0];
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = V[k][0];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        if (M[j][j] < w) {
            w = M[j][j];
#pragma unroll
            for (int k = 0; k < 4; ++k) h[k] = V[k][j];
        }
    }
}

__device__ __forceinline__ bool homogeneous_ok(const double *h) {
    return isfinite(h[0]) && isfinite(h[1]) && isfinite(h[2]) && isfinite(h[3]) && h[3] != 0.0;
}

// theia::TriangulateNView: A = sum_i C_i^T C_i over the point's observations, every lane of the group with the same sums
__device__ void nview_matrix(const TriArgs &A, int s0, int n, int l, double (&M)[4][4]) {
    double acc[10];
#pragma unroll
    for (int e = 0; e < 10; ++e) acc[e] = 0.0;
    for (int base = 0; base < n; base += kGroup) {
        double term[10];
#pragma unroll
        for (int e = 0; e < 10; ++e) term[e] = 0.0;
        if (base + l < n) {
            Obs ob;
            load_obs(A, s0 + base + l, ob);
            double q[4], C[3][4];
#pragma unroll
            for (int c = 0; c < 4; ++c) q[c] = ob.b[0] * ob.P[c] + ob.b[1] * ob.P[4 + c] + ob.b[2] * ob.P[8 + c];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) C[r][c] = ob.P[4 * r + c] - ob.b[r] * q[c];
            int e = 0;
#pragma unroll
            for (int c1 = 0; c1 < 4; ++c1)
#pragma unroll
                for (int c2 = c1; c2 < 4; ++c2) term[e++] = C[0][c1] * C[0][c2] + C[1][c1] * C[1][c2] + C[2][c1] * C[2][c2];
        }
#pragma unroll
        for (int e = 0; e < 10; ++e) acc[e] = acc[e] + group_sum(term[e]);
    }
    int e = 0;
#pragma unroll
    for (int c1 = 0; c1 < 4; ++c1)
#pragma unroll
        for (int c2 = c1; c2 < 4; ++c2) { M[c1][c2] = acc[e]; M[c2][c1] = acc[e]; ++e; }
}

// theia::Triangulate for the observations o1 and o2: Lindstrom's niter2, then the DLT matrix D^T D
__device__ void two_view_matrix(const TriArgs &A, int o1, int o2, double (&G)[4][4]) {
    Obs a, b;
    load_obs(A, o1, a);
    load_obs(A, o2, b);
    const double *P1 = a.P, *P2 = b.P;
    double R21[3][3], t[3], E[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R21[i][j] = P2[4 * i] * P1[4 * j] + P2[4 * i + 1] * P1[4 * j + 1] + P2[4 * i + 2] * P1[4 * j + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = P2[4 * i + 3] - (R21[i][0] * P1[3] + R21[i][1] * P1[7] + R21[i][2] * P1[11]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        E[0][c] = t[1] * R21[2][c] - t[2] * R21[1][c];
        E[1][c] = t[2] * R21[0][c] - t[0] * R21[2][c];
        E[2][c] = t[0] * R21[1][c] - t[1] * R21[0][c];
    }
    double x[2] = {b.xn, b.yn}, xp[2] = {a.xn, a.yn};                   // x = the second view's point, x' = the first's
    double n[2], m[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        n[k] = E[k][0] * xp[0] + E[k][1] * xp[1] + E[k][2];              // S E x'
        m[k] = E[0][k] * x[0] + E[1][k] * x[1] + E[2][k];                // S E^T x
    }
    const double qa = n[0] * (E[0][0] * m[0] + E[0][1] * m[1]) + n[1] * (E[1][0] * m[0] + E[1][1] * m[1]);
    const double qb = (n[0] * n[0] + n[1] * n[1] + m[0] * m[0] + m[1] * m[1]) * 0.5;
    const double qc = x[0] * n[0] + x[1] * n[1] + (E[2][0] * xp[0] + E[2][1] * xp[1] + E[2][2]);
    const double d = sqrt(qb * qb - qa * qc);
    double lam = qc / (qb + d);
    const double dx[2] = {lam * n[0], lam * n[1]}, dxp[2] = {lam * m[0], lam * m[1]};
    double n2[2], m2[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        n2[k] = n[k] - (E[k][0] * dxp[0] + E[k][1] * dxp[1]);
        m2[k] = m[k] - (E[0][k] * dx[0] + E[1][k] * dx[1]);
    }
    lam = lam * (2.0 * d / (n2[0] * n2[0] + n2[1] * n2[1] + m2[0] * m2[0] + m2[1] * m2[1]));
    const double x2c[2] = {x[0] - lam * n2[0], x[1] - lam * n2[1]}, x1c[2] = {xp[0] - lam * m2[0], xp[1] - lam * m2[1]};
    double rows[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        rows[0][c] = x1c[0] * P1[8 + c] - P1[c];
        rows[1][c] = x1c[1] * P1[8 + c] - P1[4 + c];
        rows[2][c] = x2c[0] * P2[8 + c] - P2[c];
        rows[3][c] = x2c[1] * P2[8 + c] - P2[4 + c];
    }
#pragma unroll
    for (int c1 = 0; c1 < 4; ++c1)
#pragma unroll
        for (int c2 = c1; c2 < 4; ++c2) {
            const double g = rows[0][c1] * rows[0][c2] + rows[1][c1] * rows[1][c2] + rows[2][c1] * rows[2][c2] + rows[3][c1] * rows[3][c2];
            G[c1][c2] = g; G[c2][c1] = g;
        }
}

// theia::TriangulateMidpoint: elimination without interchanges on the symmetric 3x3 system
__device__ bool midpoint(const TriArgs &A, int s0, int n, int l, double *h) {
    double acc[9];                       // m00 m01 m02 m11 m12 m22 | rhs
#pragma unroll
    for (int e = 0; e < 9; ++e) acc[e] = 0.0;
    for (int base = 0; base < n; base += kGroup) {
        double term[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) term[e] = 0.0;
        if (base + l < n) {
            Obs ob;
            load_obs(A, s0 + base + l, ob);
            double d[3], c[3];
            ray_of(ob, d);
            centre_of(ob, c);
            const double m00 = 1.0 - d[0] * d[0], m01 = 0.0 - d[0] * d[1], m02 = 0.0 - d[0] * d[2], m11 = 1.0 - d[1] * d[1], m12 = 0.0 - d[1] * d[2],
                         m22 = 1.0 - d[2] * d[2];
            term[0] = m00; term[1] = m01; term[2] = m02; term[3] = m11; term[4] = m12; term[5] = m22;
            term[6] = m00 * c[0] + m01 * c[1] + m02 * c[2];
            term[7] = m01 * c[0] + m11 * c[1] + m12 * c[2];
            term[8] = m02 * c[0] + m12 * c[1] + m22 * c[2];
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) acc[e] = acc[e] + group_sum(term[e]);
    }
    const double m00 = acc[0], m01 = acc[1], m02 = acc[2], m11 = acc[3], m12 = acc[4], m22 = acc[5], b0 = acc[6], b1 = acc[7], b2 = acc[8];
    double big = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e)
        if (fabs(acc[e]) > big) big = fabs(acc[e]);
    const double thr = kPivotRel * big;
    h[0] = h[1] = h[2] = h[3] = 0.0;
    if (!(m00 > thr)) return false;
    const double l10 = m01 / m00, l20 = m02 / m00;
    const double a11 = m11 - l10 * m01, a12 = m12 - l10 * m02, r1 = b1 - l10 * b0;
    double a22 = m22 - l20 * m02, r2 = b2 - l20 * b0;
    if (!(a11 > thr)) return false;
    const double l21 = a12 / a11;
    a22 = a22 - l21 * a12; r2 = r2 - l21 * r1;
    if (!(a22 > thr)) return false;
    const double z = r2 / a22, y = (r1 - a12 * z) / a11, x = (b0 - m01 * y - m02 * z) / m00;
    h[0] = x; h[1] = y; h[2] = z; h[3] = 1.0;
    return true;
}

// ------------------------------------------------------------------------------------------------ the per-observation checks
// 0 = passes, 4 = checkPositiveDepth fails (only with depth_test), 5 = checkReprojectionError fails (:576-598, with the reference's types)
__device__ int check_observation(const TriArgs &A, int o, const double *X, bool depth_test) {
    const int k = A.obs_kf[o];
    const double *P = A.kf_pose + 12 * (size_t)k;
    double pc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) pc[r] = P[4 * r] * X[0] + P[4 * r + 1] * X[1] + P[4 * r + 2] * X[2] + P[4 * r + 3];
    if (depth_test && !(pc[2] > 0.0)) return 4;
    const ms_pinhole c = A.cam[k];
    const double u = c.fx * (pc[0] / pc[2]) + c.cx, v = c.fy * (pc[1] / pc[2]) + c.cy;
    if (!(pc[2] > 0.0 && u >= 0.0 && u < (double)c.width && v >= 0.0 && v < (double)c.height)) return 5;
    const float du = __fsub_rn((float)u, A.obs_x[o]), dv = __fsub_rn((float)v, A.obs_y[o]);
    const float sq = __fadd_rn(__fmul_rn(du, du), __fmul_rn(dv, dv));
    const double rel_sigma_base = (double)__fmul_rn((float)A.focal[k], A.rel_thr);
    const double sigma2 = (double)__fdiv_rn(A.sigma[A.obs_oct[o]], A.sigma[A.n_levels / 2]) * rel_sigma_base * rel_sigma_base;
    return (double)sq <= kChi2Inv2D * sigma2 ? 0 : 5;
}

// the smallest dot product over the pairs i < j of the point's rays (+inf without a pair; a NaN product is never the smallest)
__device__ double min_pair_dot(const TriArgs &A, int s0, int n, int l) {
    double m = INFINITY;
    for (int i = 0; i + 1 < n; ++i) {
        const double *ri = A.ray + 3 * (size_t)(s0 + i);
        const double rx = ri[0], ry = ri[1], rz = ri[2];
        for (int j = i + 1 + l; j < n; j += kGroup) {
            const double *rj = A.ray + 3 * (size_t)(s0 + j);
            const double d = rx * rj[0] + ry * rj[1] + rz * rj[2];
            if (d < m) m = d;
        }
    }
    return group_min(m);
}

struct PointResult { int status, reason, n_pass; };

__device__ __forceinline__ void write_position(const TriArgs &A, int row, int l, const double *X) {
    if (l == 0) {
        double *p = A.mp_pos + 3 * (size_t)row;
        p[0] = X[0]; p[1] = X[1]; p[2] = X[2];
    }
}

// One map point; every lane of the group takes the same path.
__device__ PointResult triangulate_point(const TriArgs &A, int r, int l) {
    const int row = A.rows[r], s0 = A.obs_start[r], n = A.obs_start[r + 1] - s0;
    if (n < 2) return {0, 1, 0};                             // :611 / :733
    double X[3], h[4], M[4][4];
    if (A.mode == MS_TRI_FIRST_LAST) {
        const int last = s0 + n - 1;
        const float depth = A.obs_depth ? A.obs_depth[last] : 0.f;
        if (depth > 0.f) {
            Obs ob;
            load_obs(A, last, ob);
            depth_position(ob, depth, X);                    // :746
        } else {
            if (A.dense) return {0, 7, 0};                   // :748
            const double *r0 = A.ray + 3 * (size_t)s0, *r1 = A.ray + 3 * (size_t)last;
            const double dot = r0[0] * r1[0] + r0[1] * r1[1] + r0[2] * r1[2];
            if (!(dot < A.cos_two)) return {0, 2, 0};        // :753
            two_view_matrix(A, s0, last, M);
            smallest_eigenvector4(M, h);
            if (!homogeneous_ok(h)) return {0, 3, 0};        // :773
            X[0] = h[0] / h[3]; X[1] = h[1] / h[3]; X[2] = h[2] / h[3];
        }
        write_position(A, row, l, X);                        // :746 / :776: written before the checks
        int n_new = 0;
        for (int base = 0; base < n; base += kGroup) {
            const bool pass = base + l < n && check_observation(A, s0 + base + l, X, false) == 0;
            n_new += __popc(group_ballot(pass));
        }
        if (n_new < 2) return {0, 6, n_new};                 // :809
        return {n > 2 ? 2 : 1, 0, n_new};
    }

    int status_if_ok = 1;
    int first_depth = -1;
    if (A.obs_depth && !A.was[r]) {                          // :617-627
        for (int base = 0; base < n && first_depth < 0; base += kGroup) {
            const unsigned has = group_ballot(base + l < n && A.obs_depth[s0 + base + l] > 0.f);
            if (has) first_depth = base + (__ffs(has) - 1);
        }
    }
    if (first_depth >= 0) {
        Obs ob;
        load_obs(A, s0 + first_depth, ob);
        depth_position(ob, A.obs_depth[s0 + first_depth], X);
        write_position(A, row, l, X);                        // :622: stays written whatever the checks say
    } else {
        const double dot = min_pair_dot(A, s0, n, l);
        if (n > 2 && dot < A.cos_multi) status_if_ok = 2;    // :631
        else if (!(dot < A.cos_two)) return {0, 2, 0};       // :633
        bool ok;
        if (A.mode == MS_TRI_MIDPOINT) {
            ok = midpoint(A, s0, n, l, h);
        } else {
            if (n == 2) two_view_matrix(A, s0, s0 + 1, M);
            else nview_matrix(A, s0, n, l, M);
            smallest_eigenvector4(M, h);
            ok = homogeneous_ok(h);
        }
        if (!ok) return {0, 3, 0};                           // :694
        X[0] = h[0] / h[3]; X[1] = h[1] / h[3]; X[2] = h[2] / h[3];
    }
    for (int base = 0; base < n; base += kGroup) {           // :700-718: the first failing observation stops the point
        const int code = base + l < n ? check_observation(A, s0 + base + l, X, true) : 0;
        const unsigned failed = group_ballot(code != 0);
        if (failed) return {0, __shfl(code, __ffs(failed) - 1, kGroup), 0};
    }
    if (first_depth < 0) write_position(A, row, l, X);       // :720
    return {status_if_ok, 0, 0};
}

__global__ __launch_bounds__(kBlock) void k_tri_points(const TriArgs A) {
    const int r = (blockIdx.x * kBlock + (int)threadIdx.x) / kGroup, l = threadIdx.x & (kGroup - 1);
    if (r >= A.n_rows) return;                               // whole groups leave together
    const PointResult res = triangulate_point(A, r, l);
    if (l != 0) return;
    if (A.mp_flags) A.mp_flags[A.rows[r]] = res.status == 2 ? 3 : res.status == 1 ? 2 : 0;       // the 9.6 encoding; reset at entry, :608 / :730
    A.out[2 * (size_t)r] = res.status | res.reason << 8;
    A.out[2 * (size_t)r + 1] = res.n_pass;
}

// The lists of one call: HOST arrays that are uploaded (ms_triangulate), or DEVICE arrays the kernels read where they lie (ms_triangulate_lists).
struct TriLists {
    const int32_t *rows;
    const uint8_t *was;
    const int32_t *obs_start, *obs_kf, *obs_octave;
    const float *obs_x, *obs_y, *obs_depth;                  // obs_depth may be null
    bool on_device;
};

// the one launch sequence of both entry points; everything is validated by the caller
int tri_run(ms_ctx *c, double *mp_pos, uint8_t *mp_flags, const double *kf_pose, int n_kf, const ms_pinhole *kf_cam, const int32_t *kf_focal, const TriLists &L, int n_rows,
            int n_obs, const ms_tri_settings *settings, int mode, uint8_t *status, uint8_t *reason, int32_t *n_pass) {
    int rc;
    MsRange range("triangulate");
    const size_t nr = (size_t)n_rows, no = (size_t)n_obs, nk = (size_t)n_kf, nl = (size_t)settings->n_levels;
    const size_t ur = L.on_device ? 0 : nr, uo = L.on_device ? 0 : no;               // what of the lists is uploaded
    // upload block: cameras | focal lengths | sigmas | rows | was | obs_start | obs_kf | obs_octave | obs_x | obs_y | obs_depth; then (host only) the results
    MsLayout up;
    const auto l_cam = up.array<ms_pinhole>(nk);
    const auto l_focal = up.array<int32_t>(nk);
    const auto l_sigma = up.array<float>(nl);
    const auto l_rows = up.array<int32_t>(ur);
    const auto l_was = up.array<uint8_t>(ur);
    const auto l_start = up.array<int32_t>(L.on_device ? 0 : nr + 1);
    const auto l_kf = up.array<int32_t>(uo), l_oct = up.array<int32_t>(uo);
    const auto l_x = up.array<float>(uo), l_y = up.array<float>(uo), l_depth = up.array<float>(uo);
    MsLayout host = up, dev = up;
    const auto l_down = host.array<int32_t>(2 * nr);
    // device-only block: rays | results
    const auto l_ray = dev.array<double>(3 * no);
    const auto l_out = dev.array<int32_t>(2 * nr);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_TRIANGULATE];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    l_cam.fill(hs, kf_cam);
    l_focal.fill(hs, kf_focal);
    l_sigma.fill(hs, settings->level_sigma_sq);
    TriArgs A;
    if (L.on_device) {
        A.rows = L.rows; A.was = L.was; A.obs_start = L.obs_start;
        A.obs_kf = L.obs_kf; A.obs_oct = L.obs_octave; A.obs_x = L.obs_x; A.obs_y = L.obs_y;
        A.obs_depth = L.obs_depth;
    } else {
        l_rows.fill(hs, L.rows);
        l_was.fill(hs, L.was);
        l_start.fill(hs, L.obs_start);
        l_kf.fill(hs, L.obs_kf);
        l_oct.fill(hs, L.obs_octave);
        l_x.fill(hs, L.obs_x);
        l_y.fill(hs, L.obs_y);
        if (L.obs_depth) l_depth.fill(hs, L.obs_depth);
        A.rows = l_rows.at(ds); A.was = l_was.at(ds); A.obs_start = l_start.at(ds);
        A.obs_kf = l_kf.at(ds); A.obs_oct = l_oct.at(ds); A.obs_x = l_x.at(ds); A.obs_y = l_y.at(ds);
        A.obs_depth = L.obs_depth ? l_depth.at(ds) : nullptr;
    }
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    A.mp_pos = mp_pos; A.mp_flags = mp_flags; A.kf_pose = kf_pose;
    A.cam = l_cam.at(ds); A.focal = l_focal.at(ds); A.sigma = l_sigma.at(ds);
    A.ray = l_ray.at(ds);
    A.out = l_out.at(ds);
    A.cos_two = std::cos(settings->min_angle_two_obs * M_PI / 180.0);            // checkTriangulationAngle, :560
    A.cos_multi = std::cos(settings->min_angle_multiple_obs * M_PI / 180.0);
    A.rel_thr = settings->rel_reprojection_threshold;
    A.n_rows = n_rows; A.n_obs = (int32_t)no; A.n_levels = settings->n_levels; A.mode = mode; A.dense = settings->dense_stereo_depth != 0;
    hipLaunchKernelGGL(k_tri_rays, dim3((unsigned)((std::max(no, (size_t)1) + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_tri_rays");
    hipLaunchKernelGGL(k_tri_points, dim3((unsigned)((nr * kGroup + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_tri_points");
    const bool want = status || reason || n_pass;
    if (want) MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_out.at(ds), l_out.bytes(), hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    if (want) {
        const int32_t *out = l_down.at(hs);
        for (size_t r = 0; r < nr; ++r) {
            if (status) status[r] = (uint8_t)(out[2 * r] & 0xff);
            if (reason) reason[r] = (uint8_t)(out[2 * r] >> 8);
            if (n_pass) n_pass[r] = out[2 * r + 1];
        }
    }
    return MS_OK;
}

}  // namespace

extern "C" int ms_triangulate(ms_ctx *c, double *mp_pos, uint8_t *mp_flags, int n_mp, const double *kf_pose, int n_kf, const ms_pinhole *kf_cam,
                              const int32_t *kf_focal, const int32_t *rows, const uint8_t *was_triangulated, int n_rows, const int32_t *obs_start,
                              const int32_t *obs_kf, const float *obs_x, const float *obs_y, const int32_t *obs_octave, const float *obs_depth,
                              const ms_tri_settings *settings, int mode, uint8_t *status, uint8_t *reason, int32_t *n_pass) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_triangulate_check(mp_pos, n_mp, kf_pose, n_kf, kf_cam, kf_focal, rows, was_triangulated, n_rows, obs_start, obs_kf, obs_x, obs_y, obs_octave,
                                   settings, mode, c->err, sizeof(c->err))))
        return rc;
    if (n_rows == 0) return MS_OK;
    const TriLists L{rows, was_triangulated, obs_start, obs_kf, obs_octave, obs_x, obs_y, obs_depth, false};
    return tri_run(c, mp_pos, mp_flags, kf_pose, n_kf, kf_cam, kf_focal, L, n_rows, obs_start[n_rows], settings, mode, status, reason, n_pass);
}

#define TRI_INVALID(...) return ms_why(MS_ERR_INVALID, why, why_bytes, "triangulate: " __VA_ARGS__)

// The lists are DEVICE arrays here, so only the host arguments can be looked at: the settings and the mode as ms_triangulate_check does, the
// sizes and the pointers.  What the lists hold is the caller's: ms_observation_lists makes them valid by construction.
extern "C" int ms_triangulate_lists(ms_ctx *c, double *mp_pos, uint8_t *mp_flags, int n_mp, const double *kf_pose, int n_kf, const ms_pinhole *kf_cam,
                                    const int32_t *kf_focal, const ms_obs_lists *lists, int n_rows, int n_obs, const ms_tri_settings *settings, int mode,
                                    uint8_t *status, uint8_t *reason, int32_t *n_pass) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    char *why = c->err;
    const size_t why_bytes = sizeof(c->err);
    if ((rc = ms_triangulate_check(mp_pos, n_mp, kf_pose, n_kf, kf_cam, kf_focal, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, settings, mode, why,
                                   why_bytes)))
        return rc;
    if (n_rows < 0 || n_obs < 0) TRI_INVALID("bad arguments");
    if (n_rows == 0) return MS_OK;
    if (n_rows > MS_TRI_MAX_ROWS) return ms_why(MS_ERR_CAPACITY, why, why_bytes, "triangulate: %d rows, at most %d per call", n_rows, MS_TRI_MAX_ROWS);
    if (n_obs > MS_TRI_MAX_OBS) return ms_why(MS_ERR_CAPACITY, why, why_bytes, "triangulate: %d observations, at most %d per call", n_obs, MS_TRI_MAX_OBS);
    if (!mp_pos || !kf_pose || !kf_cam || !kf_focal || !lists || !lists->rows || !lists->was_triangulated || !lists->obs_start) TRI_INVALID("missing array");
    if (n_obs > 0 && (!lists->obs_kf || !lists->obs_x || !lists->obs_y || !lists->obs_octave || n_kf < 1)) TRI_INVALID("missing array");
    const TriLists L{lists->rows, lists->was_triangulated, lists->obs_start, lists->obs_kf, lists->obs_octave, lists->obs_x, lists->obs_y, lists->obs_depth, true};
    return tri_run(c, mp_pos, mp_flags, kf_pose, n_kf, kf_cam, kf_focal, L, n_rows, n_obs, settings, mode, status, reason, n_pass);
}
