// map_refresh.hip -- the two writers of the device map-point table:
//   ms_map_refresh   MapPoint::updateDescriptor + MapPoint::updateDistanceAndNorm (map_point.cpp:75-116, :158-172) for chosen rows,
//                    as mapper_helpers.cpp:1062-1077 runs them for the map points of a new keyframe
//   ms_loop_correct  the pose correction and map-point transfer of LoopCloser::correctLoop (loop_closer.cpp:398-503)
//
// ms_map_refresh takes the observation lists as host arrays and uploads them; ms_map_refresh_lists reads the device lists of
// ms_observation_lists where they lie, builds the descriptor lists with k_refresh_dcount / k_refresh_dscan / k_refresh_dpack,
// maps the medoid to its list position with k_refresh_medoid_pos and, for promote_min_obs > 0, sets the status flags at the end of
// k_refresh_geom.  Both run the one launch sequence of refresh_run.
//
// Refresh, five launches whatever the number of rows (two without a descriptor pool):
//   k_refresh_centres  one lane per keyframe slot: the camera centre -R^T t
//   k_refresh_geom     a team of 8 lanes per row: the lanes compute eight observations' unit vectors at a time, then every lane of the team
//                      adds the eight terms in list order (shuffles inside the team) -- the sum is the reference's left-to-right sum whatever
//                      the team width; lane 0 writes normal, min and max distance
//   k_refresh_gather   the rows' observation descriptors, packed list after list into the workspace
//   k_descriptor_medoid (match.hip, through ms_descriptor_medoid) on the packed lists
//   k_refresh_winner   the chosen descriptor into mp_desc[row]
// Loop correction, two launches:
//   k_loop_poses       one lane per corrected keyframe: keeps the previous pose, writes sim3ToSe3(se3ToSim3(pose) * Tl) and leaves the
//                      transfer corrected^-1 * previous of the keyframe's map points as a matrix in the workspace
//   k_loop_points      one lane per point: p <- transfer(reference keyframe).map(p)
//
// Every floating-point operation is one rounded IEEE operation and every sum has one order: the refresh kernels spell them with the *_rn
// intrinsics, the Sim3 algebra of the loop correction is plain C++ under contract(off) (no fast-math: the compiler may neither fuse nor
// reassociate).  Square roots and divisions are the correctly rounded ones (sqrt / sqrtf, operator/); acos and sin of the slerp are the device
// library's and carry its error.  No atomics anywhere.  Everything a kernel indexes with is validated on the host first.
#include "ms_internal.h"
#include "ms_scan.h"
#include <algorithm>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kTeam = 8;                 // lanes per row in k_refresh_geom

// ------------------------------------------------------------------------------------------------ refresh
__global__ __launch_bounds__(kBlock) void k_refresh_centres(const double *__restrict__ kf_pose, int n_kf, double *__restrict__ centre) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_kf) return;
    const double *P = kf_pose + 12 * (size_t)k;              // rows 0-2 of poseCW: R[i][j] = P[4 i + j], t[i] = P[4 i + 3]
#pragma unroll
    for (int j = 0; j < 3; ++j)                              // worldToCameraMatrixCameraCenter: -R^T t, summed left to right
        centre[3 * (size_t)k + j] = -__dadd_rn(__dadd_rn(__dmul_rn(P[j], P[3]), __dmul_rn(P[4 + j], P[7])), __dmul_rn(P[8 + j], P[11]));
}

struct RefreshArgs {
    const double *mp_pos, *centre;
    float *mp_norm, *mp_min, *mp_max;
    const int32_t *rows, *obs_start, *obs_kf, *octave;
    const float *sf;
    uint8_t *mp_flags;                       // written for promote_min_obs > 0 only
    int32_t n_rows, n_levels, promote_min_obs;
};

__device__ __forceinline__ double sq_norm3(double x, double y, double z) {       // Eigen's unrolled redux of three elements: x^2 + (y^2 + z^2)
    return __dadd_rn(__dmul_rn(x, x), __dadd_rn(__dmul_rn(y, y), __dmul_rn(z, z)));
}

__global__ __launch_bounds__(kBlock) void k_refresh_geom(const RefreshArgs A) {
    const int r = (blockIdx.x * kBlock + (int)threadIdx.x) / kTeam, l = threadIdx.x & (kTeam - 1);
    if (r >= A.n_rows) return;                               // whole teams leave together
    const int row = A.rows[r], s0 = A.obs_start[r], n = A.obs_start[r + 1] - s0;
    const double px = A.mp_pos[3 * (size_t)row], py = A.mp_pos[3 * (size_t)row + 1], pz = A.mp_pos[3 * (size_t)row + 2];
    double sx = 0.0, sy = 0.0, sz = 0.0;                     // normSum, :159
    for (int base = 0; base < n; base += kTeam) {            // n is the same in every lane of the team
        double tx = 0.0, ty = 0.0, tz = 0.0;
        if (base + l < n) {                                  // (kf.cameraCenter() - position).normalized(), :162
            const double *c = A.centre + 3 * (size_t)A.obs_kf[s0 + base + l];
            tx = __dsub_rn(c[0], px); ty = __dsub_rn(c[1], py); tz = __dsub_rn(c[2], pz);
            const double z = sq_norm3(tx, ty, tz);
            if (z > 0.0) {
                const double len = sqrt(z);
                tx = __ddiv_rn(tx, len); ty = __ddiv_rn(ty, len); tz = __ddiv_rn(tz, len);
            }
        }
        const int m = min(kTeam, n - base);
#pragma unroll
        for (int j = 0; j < kTeam; ++j) {                    // the terms in list order, the same additions in every lane of the team
            const double ax = __shfl(tx, j, kTeam), ay = __shfl(ty, j, kTeam), az = __shfl(tz, j, kTeam);
            if (j < m) { sx = __dadd_rn(sx, ax); sy = __dadd_rn(sy, ay); sz = __dadd_rn(sz, az); }
        }
    }
    if (l != 0) return;
    const float fn = (float)n;                               // norm = normSum.cast<float>() / observations.size(), :164
    A.mp_norm[3 * (size_t)row] = __fdiv_rn((float)sx, fn);
    A.mp_norm[3 * (size_t)row + 1] = __fdiv_rn((float)sy, fn);
    A.mp_norm[3 * (size_t)row + 2] = __fdiv_rn((float)sz, fn);
    const double *c0 = A.centre + 3 * (size_t)A.obs_kf[s0];  // getFirstObservation(), :166-167
    const float dist = (float)sqrt(sq_norm3(__dsub_rn(c0[0], px), __dsub_rn(c0[1], py), __dsub_rn(c0[2], pz)));
    const float sfo = A.sf[A.octave[r]];
    A.mp_max[row] = __fmul_rn(dist, sfo);                                        // :170
    A.mp_min[row] = __fdiv_rn(__fmul_rn(dist, sfo), A.sf[A.n_levels - 1]);       // :171
    if (A.promote_min_obs > 0) A.mp_flags[row] = n >= A.promote_min_obs ? 3 : 2;   // mapper_helpers.cpp:1072-1076: TRIANGULATED, else UNSURE
}

// packed[e] = pool[src[e]] (two 16-byte halves per descriptor, one lane each); ident[e] = e, the index list k_descriptor_medoid walks
__global__ __launch_bounds__(kBlock) void k_refresh_gather(const uint4 *__restrict__ pool, const int32_t *__restrict__ src, int n, uint4 *__restrict__ packed,
                                                           int32_t *__restrict__ ident) {
    const int g = blockIdx.x * kBlock + threadIdx.x, e = g >> 1, h = g & 1;
    if (e >= n) return;
    packed[2 * (size_t)e + h] = pool[2 * (size_t)src[e] + h];
    if (h == 0) ident[e] = e;
}

__global__ __launch_bounds__(kBlock) void k_refresh_winner(const uint4 *__restrict__ packed, const int32_t *__restrict__ start, const int32_t *__restrict__ best,
                                                           const int32_t *__restrict__ rows, int n_rows, uint4 *__restrict__ mp_desc) {
    const int g = blockIdx.x * kBlock + threadIdx.x, r = g >> 1, h = g & 1;
    if (r >= n_rows) return;
    const int b = best[r];
    if (b < 0) return;                                       // -1: no descriptors (:86), -2: list beyond MS_MEDOID_MAX_OBS -- the row keeps its descriptor
    mp_desc[2 * (size_t)rows[r] + h] = packed[2 * ((size_t)start[r] + (size_t)b) + h];
}

// The descriptor lists of the device form (ms_map_refresh_lists), what ms_map_refresh packs on the host: a row's `descriptors` vector of
// map_point.cpp:76-84 is its observations with obs_desc != -1.  Count per row, scan, pack; the scan also leaves the total and the longest list.
constexpr int kScan = 1024;

__global__ __launch_bounds__(kBlock) void k_refresh_dcount(const int32_t *__restrict__ obs_start, const int32_t *__restrict__ obs_desc, int n_rows, int32_t *__restrict__ dstart) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_rows) return;
    int have = 0;
    for (int o = obs_start[r]; o < obs_start[r + 1]; ++o) have += obs_desc[o] != -1;
    dstart[r] = have;
}

// dstart[0 .. n_rows]: counts -> exclusive offsets, in place (one workgroup: block_offsets of ms_scan.h, kScan rows per trip); info = total,
// longest list
__global__ __launch_bounds__(kScan) void k_refresh_dscan(int32_t *__restrict__ dstart, int n_rows, int32_t *__restrict__ info) {
    __shared__ int32_t s_wave[kScan / 64], s_max[kScan / 64];
    int longest = 0;                                         // of this thread's rows, then of its wave's
    for (int r = threadIdx.x; r < n_rows; r += kScan) longest = max(longest, dstart[r]);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) longest = max(longest, __shfl_xor(longest, d));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = longest;
    __syncthreads();
    const int total = block_offsets<kScan>(dstart, dstart, n_rows, s_wave);      // a thread overwrites only the counts it read above
    if (threadIdx.x == 0) {
        for (int w = 0; w < kScan / 64; ++w) longest = max(longest, s_max[w]);
        dstart[n_rows] = total; info[0] = total; info[1] = longest;
    }
}

__global__ __launch_bounds__(kBlock) void k_refresh_dpack(const int32_t *__restrict__ obs_start, const int32_t *__restrict__ obs_desc, int n_rows,
                                                          const int32_t *__restrict__ dstart, int32_t *__restrict__ dsrc) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_rows) return;
    int at = dstart[r];
    for (int o = obs_start[r]; o < obs_start[r + 1]; ++o) {
        const int32_t d = obs_desc[o];
        if (d != -1) dsrc[at++] = d;                         // below dstart[r + 1]: the count k_refresh_dcount took from the same list
    }
}

// medoid[r]: the position among the row's descriptors -> the position in the row's observation list; -1 / -2 stay
__global__ __launch_bounds__(kBlock) void k_refresh_medoid_pos(const int32_t *__restrict__ obs_start, const int32_t *__restrict__ obs_desc, int n_rows,
                                                               int32_t *__restrict__ best_pos, const int32_t *__restrict__ best) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_rows) return;
    int m = best[r];
    if (m >= 0)
        for (int o = obs_start[r], k = 0; o < obs_start[r + 1]; ++o)
            if (obs_desc[o] != -1 && k++ == m) { m = o - obs_start[r]; break; }
    best_pos[r] = m;
}

// ------------------------------------------------------------------------------------------------ loop correction
// mi355slam::Sim3 (host/mi355slam/optimize_transform.hpp) on the device, operation for operation
struct Quat { double w, x, y, z; };
struct S3 { Quat q; double t[3]; double s; };

__device__ __forceinline__ Quat q_normalized(Quat q) {
    const double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    if (n > 0.0) { q.w /= n; q.x /= n; q.y /= n; q.z /= n; }
    return q;
}
__device__ Quat q_of_matrix(const double *R) {               // row-major; Sim3(R, t, s)
    const double tr = R[0] + R[4] + R[8];
    Quat q;
    if (tr > 0.0) {
        const double w4 = 2.0 * sqrt(tr + 1.0);
        q = {0.25 * w4, (R[7] - R[5]) / w4, (R[2] - R[6]) / w4, (R[3] - R[1]) / w4};
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double x4 = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
        q = {(R[7] - R[5]) / x4, 0.25 * x4, (R[1] + R[3]) / x4, (R[2] + R[6]) / x4};
    } else if (R[4] > R[8]) {
        const double y4 = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
        q = {(R[2] - R[6]) / y4, (R[1] + R[3]) / y4, 0.25 * y4, (R[5] + R[7]) / y4};
    } else {
        const double z4 = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
        q = {(R[3] - R[1]) / z4, (R[2] + R[6]) / z4, (R[5] + R[7]) / z4, 0.25 * z4};
    }
    return q_normalized(q);
}
__device__ __forceinline__ void matrix_of_q(const Quat &q, double *R) {
    const double w = q.w, x = q.x, y = q.y, z = q.z;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}
__device__ __forceinline__ void rotate(const Quat &q, const double *p, double *out) {
    double R[9];
    matrix_of_q(q, R);
    out[0] = R[0] * p[0] + R[1] * p[1] + R[2] * p[2];
    out[1] = R[3] * p[0] + R[4] * p[1] + R[5] * p[2];
    out[2] = R[6] * p[0] + R[7] * p[1] + R[8] * p[2];
}
__device__ S3 s3_mul(const S3 &a, const S3 &b) {             // (A.r * B.r, A.s * (A.r * B.t) + A.t, A.s * B.s)
    S3 o;
    o.q = q_normalized({a.q.w * b.q.w - a.q.x * b.q.x - a.q.y * b.q.y - a.q.z * b.q.z, a.q.w * b.q.x + a.q.x * b.q.w + a.q.y * b.q.z - a.q.z * b.q.y,
                        a.q.w * b.q.y - a.q.x * b.q.z + a.q.y * b.q.w + a.q.z * b.q.x, a.q.w * b.q.z + a.q.x * b.q.y - a.q.y * b.q.x + a.q.z * b.q.w});
    double rt[3];
    rotate(a.q, b.t, rt);
    for (int j = 0; j < 3; ++j) o.t[j] = a.s * rt[j] + a.t[j];
    o.s = a.s * b.s;
    return o;
}
__device__ S3 s3_inverse(const S3 &a) {                      // (r^-1, -(1 / s) * (r^-1 * t), 1 / s)
    S3 o;
    o.q = {a.q.w, -a.q.x, -a.q.y, -a.q.z};
    double rt[3];
    rotate(o.q, a.t, rt);
    o.s = 1.0 / a.s;
    for (int j = 0; j < 3; ++j) o.t[j] = -o.s * rt[j];
    return o;
}
// interpolateSim3(identity, T, lambda), loop_closer.cpp:69-76, with Eigen's QuaternionBase::slerp
__device__ S3 s3_interpolate(const S3 &T, double lambda) {
    const double one = 1.0 - 2.220446049250313e-16;
    const double d = T.q.w;                                  // identity . T.r
    const double ad = fabs(d);
    double scale0, scale1;
    if (ad >= one) {
        scale0 = 1.0 - lambda; scale1 = lambda;
    } else {
        const double theta = acos(ad), sin_theta = sin(theta);
        scale0 = sin((1.0 - lambda) * theta) / sin_theta;
        scale1 = sin(lambda * theta) / sin_theta;
    }
    if (d < 0.0) scale1 = -scale1;
    S3 o;
    o.q = q_normalized({scale0 * 1.0 + scale1 * T.q.w, scale0 * 0.0 + scale1 * T.q.x, scale0 * 0.0 + scale1 * T.q.y, scale0 * 0.0 + scale1 * T.q.z});
    for (int j = 0; j < 3; ++j) o.t[j] = 0.0 + lambda * (T.t[j] - 0.0);
    o.s = 1.0 + lambda * (T.s - 1.0);
    return o;
}

constexpr int kXfer = 16;                                    // doubles per keyframe transfer: R[9], t[3], s, padding

struct LoopArgs {
    double *kf_pose, *mp_pos;
    double *prev, *xfer;                                     // workspace: [n_corr * 12], [n_corr * kXfer]
    const double *T;                                         // w, x, y, z, tx, ty, tz, s
    const int32_t *kf_slot, *mp_row, *mp_ref;
    const double *kf_lambda;
    const uint8_t *kf_rigid;
    int32_t n_corr, n_pts;
};

__global__ __launch_bounds__(64) void k_loop_poses(const LoopArgs A) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= A.n_corr) return;
    double *P = A.kf_pose + 12 * (size_t)A.kf_slot[i];
    double R[9];
    S3 prev;                                                 // se3ToSim3(kf.poseCW)
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) R[3 * a + b] = P[4 * a + b];
        prev.t[a] = P[4 * a + 3];
    }
    for (int k = 0; k < 12; ++k) A.prev[12 * (size_t)i + k] = P[k];               // prevPoses, :398-401
    prev.q = q_of_matrix(R); prev.s = 1.0;
    S3 T;
    T.q = {A.T[0], A.T[1], A.T[2], A.T[3]}; T.t[0] = A.T[4]; T.t[1] = A.T[5]; T.t[2] = A.T[6]; T.s = A.T[7];
    const S3 Tl = A.kf_rigid[i] ? T : s3_interpolate(T, A.kf_lambda[i]);          // :427, :459
    const S3 now = s3_mul(prev, Tl);
    matrix_of_q(now.q, R);                                   // sim3ToSe3: the scale is dropped
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) P[4 * a + b] = R[3 * a + b];
        P[4 * a + 3] = now.t[a];
    }
    S3 corrected;                                            // se3ToSim3(corrected poseCW), :500 -- from the stored matrix, as the reference reads it back
    corrected.q = q_of_matrix(R); corrected.s = 1.0;
    for (int a = 0; a < 3; ++a) corrected.t[a] = now.t[a];
    const S3 x = s3_mul(s3_inverse(corrected), prev);        // :503
    double *X = A.xfer + kXfer * (size_t)i;
    matrix_of_q(x.q, R);
    for (int k = 0; k < 9; ++k) X[k] = R[k];
    for (int a = 0; a < 3; ++a) X[9 + a] = x.t[a];
    X[12] = x.s;
}

__global__ __launch_bounds__(kBlock) void k_loop_points(const LoopArgs A) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= A.n_pts) return;
    const double *X = A.xfer + kXfer * (size_t)A.mp_ref[j];
    double *p = A.mp_pos + 3 * (size_t)A.mp_row[j];
    const double x = p[0], y = p[1], z = p[2], s = X[12];
    p[0] = s * (X[0] * x + X[1] * y + X[2] * z) + X[9];      // Sim3::map: s * (r * p) + t
    p[1] = s * (X[3] * x + X[4] * y + X[5] * z) + X[10];
    p[2] = s * (X[6] * x + X[7] * y + X[8] * z) + X[11];
}

// The lists of one call: HOST arrays that are uploaded (ms_map_refresh), or DEVICE arrays the kernels read where they lie (ms_map_refresh_lists).
struct RefreshLists {
    const int32_t *rows, *obs_start, *obs_kf, *obs_desc, *first_octave;
    bool on_device;
};

// the one launch sequence of both entry points; everything is validated by the caller
int refresh_run(ms_ctx *c, const double *mp_pos, float *mp_norm, float *mp_min_dist, float *mp_max_dist, uint32_t *mp_desc, const double *kf_pose, int n_kf,
                const uint32_t *desc_pool, const RefreshLists &L, int n_rows, int n_obs, const float *scale_factors, int n_levels, int promote_min_obs, uint8_t *mp_flags,
                int32_t *medoid) {
    int rc;
    const bool with_desc = desc_pool != nullptr && L.obs_desc != nullptr, on_dev = L.on_device;
    int n_dobs = 0, longest = 0;
    for (int r = 0; !on_dev && with_desc && r < n_rows; ++r) {
        int have = 0;
        for (int o = L.obs_start[r]; o < L.obs_start[r + 1]; ++o) have += L.obs_desc[o] != -1;
        n_dobs += have;
        longest = std::max(longest, have);
    }
    MsRange range("mapRefresh");
    // upload block: rows | octaves | obs_start | obs_kf | scale factors | packed descriptor lists: start, pool index; then (host only) medoids
    // (device lists: only the scale factors are uploaded; the descriptor lists are built on the device, for n_obs descriptors at most)
    const size_t nr = (size_t)n_rows, nd = on_dev ? (with_desc ? (size_t)n_obs : 0) : (size_t)n_dobs, ur = on_dev ? 0 : nr;
    MsLayout up;
    const auto l_rows = up.array<int32_t>(ur), l_oct = up.array<int32_t>(ur), l_start = up.array<int32_t>(on_dev ? 0 : nr + 1), l_kf = up.array<int32_t>(on_dev ? 0 : (size_t)n_obs);
    const auto l_sf = up.array<float>((size_t)n_levels);
    const auto l_dstart = up.array<int32_t>(on_dev ? 0 : nr + 1), l_dsrc = up.array<int32_t>(on_dev ? 0 : nd);
    MsLayout host = up, dev = up;
    const auto l_down = host.array<int32_t>(std::max(nr, (size_t)2));
    // device-only block: camera centres | packed descriptors | identity list | medoids (the descriptors and the list with one entry of slack);
    // for device lists also: descriptor starts | pool indices | total and longest | medoid positions
    const auto l_centre = dev.array<double>(3 * (size_t)n_kf);
    const auto l_packed = dev.array<uint4>(2 * nd + 2);
    const auto l_ident = dev.array<int32_t>(nd + 1), l_best = dev.array<int32_t>(nr);
    const auto l_ddstart = dev.array<int32_t>(on_dev ? nr + 1 : 0), l_ddsrc = dev.array<int32_t>(on_dev ? nd : 0);
    const auto l_info = dev.array<int32_t>(on_dev ? 2 : 0), l_pos = dev.array<int32_t>(on_dev ? nr : 0);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_MAP_REFRESH];
    if ((rc = ms_grow(c, W.host, W.host_bytes, host.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    l_sf.fill(hs, scale_factors);
    const int32_t *d_rows = L.rows, *d_start = L.obs_start, *d_kf = L.obs_kf, *d_oct = L.first_octave, *d_dstart = l_ddstart.at(ds), *d_dsrc = l_ddsrc.at(ds);
    if (!on_dev) {
        l_rows.fill(hs, L.rows);
        l_oct.fill(hs, L.first_octave);
        l_start.fill(hs, L.obs_start);
        l_kf.fill(hs, L.obs_kf);
        int32_t *dstart = l_dstart.at(hs), *dsrc = l_dsrc.at(hs);
        dstart[0] = 0;
        for (int r = 0, at = 0; r < n_rows; ++r) {           // the `descriptors` vector of :76-84: observations of keyframes that have descriptors
            if (with_desc)
                for (int o = L.obs_start[r]; o < L.obs_start[r + 1]; ++o)
                    if (L.obs_desc[o] != -1) dsrc[at++] = L.obs_desc[o];
            dstart[r + 1] = at;
        }
        d_rows = l_rows.at(ds); d_start = l_start.at(ds); d_kf = l_kf.at(ds); d_oct = l_oct.at(ds); d_dstart = l_dstart.at(ds); d_dsrc = l_dsrc.at(ds);
    }
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    double *centre = l_centre.at(ds);
    hipLaunchKernelGGL(k_refresh_centres, dim3(ms_div_up(std::max(n_kf, 1), kBlock)), dim3(kBlock), 0, c->stream, kf_pose, n_kf, centre);
    MS_KERNEL_CHECK(c, "k_refresh_centres");
    RefreshArgs A;
    A.mp_pos = mp_pos; A.centre = centre; A.mp_norm = mp_norm; A.mp_min = mp_min_dist; A.mp_max = mp_max_dist;
    A.rows = d_rows; A.obs_start = d_start; A.obs_kf = d_kf; A.octave = d_oct;
    A.sf = l_sf.at(ds);
    A.mp_flags = mp_flags;
    A.n_rows = n_rows; A.n_levels = n_levels; A.promote_min_obs = promote_min_obs;
    hipLaunchKernelGGL(k_refresh_geom, dim3((unsigned)((nr * kTeam + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_refresh_geom");
    if (with_desc) {
        const dim3 by_row((unsigned)ms_div_up(n_rows, kBlock));
        if (on_dev) {                                        // the descriptor lists, their total and the longest one
            int32_t *dstart = l_ddstart.at(ds);
            hipLaunchKernelGGL(k_refresh_dcount, by_row, dim3(kBlock), 0, c->stream, d_start, L.obs_desc, n_rows, dstart);
            MS_KERNEL_CHECK(c, "k_refresh_dcount");
            hipLaunchKernelGGL(k_refresh_dscan, dim3(1), dim3(kScan), 0, c->stream, dstart, n_rows, l_info.at(ds));
            MS_KERNEL_CHECK(c, "k_refresh_dscan");
            hipLaunchKernelGGL(k_refresh_dpack, by_row, dim3(kBlock), 0, c->stream, d_start, L.obs_desc, n_rows, dstart, l_ddsrc.at(ds));
            MS_KERNEL_CHECK(c, "k_refresh_dpack");
            MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_info.at(ds), l_info.bytes(), hipMemcpyDeviceToHost, c->stream));
            MS_HIP(c, hipStreamSynchronize(c->stream));      // the medoid kernel's LDS is sized by the longest list
            n_dobs = l_down.at(hs)[0]; longest = l_down.at(hs)[1];
        }
        uint4 *packed = l_packed.at(ds);
        hipLaunchKernelGGL(k_refresh_gather, dim3(ms_div_up(std::max(2 * n_dobs, 1), kBlock)), dim3(kBlock), 0, c->stream,
                           reinterpret_cast<const uint4 *>(desc_pool), d_dsrc, n_dobs, packed, l_ident.at(ds));
        MS_KERNEL_CHECK(c, "k_refresh_gather");
        if ((rc = ms_descriptor_medoid(c, reinterpret_cast<const uint32_t *>(packed), d_dstart, l_ident.at(ds), n_rows, std::min(longest, MS_MEDOID_MAX_OBS),
                                       l_best.at(ds), nullptr)))
            return rc;
        hipLaunchKernelGGL(k_refresh_winner, dim3(ms_div_up(2 * n_rows, kBlock)), dim3(kBlock), 0, c->stream, packed, d_dstart, l_best.at(ds), d_rows, n_rows,
                           reinterpret_cast<uint4 *>(mp_desc));
        MS_KERNEL_CHECK(c, "k_refresh_winner");
        if (medoid && on_dev) {
            hipLaunchKernelGGL(k_refresh_medoid_pos, by_row, dim3(kBlock), 0, c->stream, d_start, L.obs_desc, n_rows, l_pos.at(ds), l_best.at(ds));
            MS_KERNEL_CHECK(c, "k_refresh_medoid_pos");
            MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_pos.at(ds), l_pos.bytes(), hipMemcpyDeviceToHost, c->stream));
        } else if (medoid) {
            MS_HIP(c, hipMemcpyAsync(l_down.at(hs), l_best.at(ds), l_best.bytes(), hipMemcpyDeviceToHost, c->stream));
        }
    }
    MS_HIP(c, hipStreamSynchronize(c->stream));
    if (medoid) {
        const int32_t *best = l_down.at(hs);
        for (int r = 0; r < n_rows; ++r) {
            int m = with_desc ? best[r] : -1;
            if (m >= 0 && !on_dev)                           // position among the descriptors -> position in the row's observation list
                for (int o = L.obs_start[r], k = 0; o < L.obs_start[r + 1]; ++o)
                    if (L.obs_desc[o] != -1 && k++ == m) { m = o - L.obs_start[r]; break; }
            medoid[r] = m;
        }
    }
    return MS_OK;
}

}  // namespace

extern "C" int ms_map_refresh(ms_ctx *c, const double *mp_pos, float *mp_norm, float *mp_min_dist, float *mp_max_dist, uint32_t *mp_desc, int n_mp,
                              const double *kf_pose, int n_kf, const uint32_t *desc_pool, int n_pool, const int32_t *rows, int n_rows,
                              const int32_t *obs_start, const int32_t *obs_kf, const int32_t *obs_desc, const int32_t *first_octave,
                              const float *scale_factors, int n_levels, int32_t *medoid) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_map_refresh_check(mp_pos, mp_norm, mp_min_dist, mp_max_dist, mp_desc, n_mp, kf_pose, n_kf, desc_pool, n_pool, rows, n_rows, obs_start, obs_kf, obs_desc,
                                   first_octave, scale_factors, n_levels, c->err, sizeof(c->err))))
        return rc;
    if (n_rows == 0) return MS_OK;
    const RefreshLists L{rows, obs_start, obs_kf, obs_desc, first_octave, false};
    return refresh_run(c, mp_pos, mp_norm, mp_min_dist, mp_max_dist, mp_desc, kf_pose, n_kf, desc_pool, L, n_rows, obs_start[n_rows], scale_factors, n_levels, 0, nullptr,
                       medoid);
}

// The lists are DEVICE arrays here, so only the host arguments can be looked at.  What the lists hold -- rows in range and distinct, no
// empty list (drop_empty of ms_observation_lists), slots, octaves and descriptor indices in range -- is the caller's: ms_observation_lists
// makes them valid by construction when n_pool covers kf_desc_base + stride and n_levels is the one it was given.
extern "C" int ms_map_refresh_lists(ms_ctx *c, const double *mp_pos, float *mp_norm, float *mp_min_dist, float *mp_max_dist, uint32_t *mp_desc, int n_mp,
                                    const double *kf_pose, int n_kf, const uint32_t *desc_pool, int n_pool, const ms_obs_lists *lists, int n_rows, int n_obs,
                                    const float *scale_factors, int n_levels, int promote_min_obs, uint8_t *mp_flags, int32_t *medoid) {
    if (!c) return MS_ERR_INVALID;
    char *why = c->err;
    const size_t why_bytes = sizeof(c->err);
    if (n_mp < 0 || n_kf < 0 || n_pool < 0 || n_rows < 0 || n_obs < 0 || n_levels < 1 || promote_min_obs < 0 || !scale_factors)
        return ms_why(MS_ERR_INVALID, why, why_bytes, "map refresh: bad arguments");
    if (n_rows == 0) return MS_OK;
    if (n_obs < n_rows || n_kf < 1) return ms_why(MS_ERR_INVALID, why, why_bytes, "map refresh: %d observations for %d rows: a row entry has no observations", n_obs, n_rows);
    if (!mp_pos || !mp_norm || !mp_min_dist || !mp_max_dist || !kf_pose || !lists || !lists->rows || !lists->obs_start || !lists->obs_kf || !lists->first_octave)
        return ms_why(MS_ERR_INVALID, why, why_bytes, "map refresh: missing array");
    if (promote_min_obs > 0 && !mp_flags) return ms_why(MS_ERR_INVALID, why, why_bytes, "map refresh: promote_min_obs %d and there is no mp_flags", promote_min_obs);
    const bool with_desc = desc_pool != nullptr && lists->obs_desc != nullptr;
    if (with_desc && !mp_desc) return ms_why(MS_ERR_INVALID, why, why_bytes, "map refresh: a descriptor pool without the table's descriptors");
    if (with_desc && ((reinterpret_cast<uintptr_t>(mp_desc) | reinterpret_cast<uintptr_t>(desc_pool)) & 15u))
        return ms_why(MS_ERR_INVALID, why, why_bytes, "map refresh: descriptor arrays must be 16-byte aligned");
    const RefreshLists L{lists->rows, lists->obs_start, lists->obs_kf, lists->obs_desc, lists->first_octave, true};
    return refresh_run(c, mp_pos, mp_norm, mp_min_dist, mp_max_dist, mp_desc, kf_pose, n_kf, desc_pool, L, n_rows, n_obs, scale_factors, n_levels, promote_min_obs, mp_flags,
                       medoid);
}

extern "C" int ms_loop_correct(ms_ctx *c, double *kf_pose, int n_kf, double *mp_pos, int n_mp, const double *T, const int32_t *kf_slot,
                               const uint8_t *kf_rigid, const double *kf_lambda, int n_corr, const int32_t *mp_row, const int32_t *mp_ref, int n_pts) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_loop_correct_check(kf_pose, n_kf, mp_pos, n_mp, T, kf_slot, kf_rigid, kf_lambda, n_corr, mp_row, mp_ref, n_pts, c->err, sizeof(c->err)))) return rc;
    if (n_corr == 0) return MS_OK;                           // no point can have a reference then
    MsRange range("loopCorrect");
    const size_t nc = (size_t)n_corr, np = (size_t)n_pts;
    // upload block: T | lambda | slots | rigid flags | point rows | point references
    MsLayout up;
    const auto l_T = up.array<double>(8), l_lam = up.array<double>(nc);
    const auto l_slot = up.array<int32_t>(nc);
    const auto l_rigid = up.array<uint8_t>(nc);
    const auto l_row = up.array<int32_t>(np), l_ref = up.array<int32_t>(np);
    // device-only block: previous poses | keyframe transfers
    MsLayout dev = up;
    const auto l_prev = dev.array<double>(12 * nc), l_xfer = dev.array<double>(kXfer * nc);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_MAP_REFRESH];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    void *hs = W.host, *ds = W.dev;
    l_T.fill(hs, T);
    l_lam.fill(hs, kf_lambda);
    l_slot.fill(hs, kf_slot);
    l_rigid.fill(hs, kf_rigid);
    l_row.fill(hs, mp_row);
    l_ref.fill(hs, mp_ref);
    MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    LoopArgs A;
    A.kf_pose = kf_pose; A.mp_pos = mp_pos;
    A.prev = l_prev.at(ds); A.xfer = l_xfer.at(ds);
    A.T = l_T.at(ds); A.kf_lambda = l_lam.at(ds); A.kf_slot = l_slot.at(ds); A.kf_rigid = l_rigid.at(ds);
    A.mp_row = l_row.at(ds); A.mp_ref = l_ref.at(ds);
    A.n_corr = n_corr; A.n_pts = n_pts;
    hipLaunchKernelGGL(k_loop_poses, dim3(ms_div_up(n_corr, 64)), dim3(64), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_loop_poses");
    hipLaunchKernelGGL(k_loop_points, dim3(ms_div_up(std::max(n_pts, 1), kBlock)), dim3(kBlock), 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_loop_points");
    MS_HIP(c, hipStreamSynchronize(c->stream));
    return MS_OK;
}
