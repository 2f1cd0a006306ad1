// ba_window_dev.h -- the device helpers the BA gathers and applies on the map tables must agree on bit for bit: the pose of
// a table matrix as g2o::SE3Quat builds it, the table matrix of a solver pose, the normalised pixel and the information of an observation.
// Device code only; included by ba_window.hip and pose_tables.hip, both built without contraction: every float64 expression below is
// evaluated as written.
#pragma once
#include <hip/hip_runtime.h>

// g2o::SE3Quat(R, t): Eigen's quaternion of a rotation matrix (Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>), then
// normalizeRotation (w >= 0, unit length).  R row-major; q = x, y, z, w
__device__ void quat_of_matrix(const double *R, double *q) {
    double t = R[0] + R[4] + R[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t;
        q[1] = (R[2] - R[6]) * t;
        q[2] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[3 * k + j] - R[3 * j + k]) * t;
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
    }
    if (q[3] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}

// matrixToPose(poseCW) of the table matrix P (rows 0-2 of poseCW, row-major 3 x 4): qx, qy, qz, qw, tx, ty, tz
__device__ __forceinline__ void pose_of_table(const double *P, double *out) {
    double R[9], q[4];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R[3 * a + b] = P[4 * a + b];
    quat_of_matrix(R, q);
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; out[3] = q[3];
    out[4] = P[3]; out[5] = P[7]; out[6] = P[11];
}

// Eigen's QuaternionBase::toRotationMatrix of the quaternion as given, rows 0-2 of to_homogeneous_matrix()
__device__ __forceinline__ void write_pose(const double *s, double *P) {
    const double x = s[0], y = s[1], z = s[2], w = s[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    P[0] = 1.0 - (tyy + tzz); P[1] = txy - twz; P[2] = txz + twy; P[3] = s[4];
    P[4] = txy + twz; P[5] = 1.0 - (txx + tzz); P[6] = tyz - twx; P[7] = s[5];
    P[8] = txz - twy; P[9] = tyz + twx; P[10] = 1.0 - (txx + tyy); P[11] = s[6];
}

// normalizePixel of the pinhole stand-in, bundle_adjuster.cpp:52: one coordinate of the float32 pixel in float64
__device__ __forceinline__ double obs_normalised(float pixel, double centre, double f) { return ((double)pixel - centre) / f; }

// the information of an observation, bundle_adjuster.cpp:51
__device__ __forceinline__ double obs_information(int32_t focal_length, float level_sigma_sq) {
    const double focal = (double)focal_length;
    return focal * focal / (double)level_sigma_sq;
}
