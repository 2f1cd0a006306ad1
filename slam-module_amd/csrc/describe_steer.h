// The steering arithmetic of k_describe (orb.hip): the two orientation moments of a keypoint -> its angle in degrees (cv::fastAtan2) -> the
// cosine and sine that rotate the BRIEF pattern (openvslam/trigonometric.h).  Plain C++, host- and device-callable: the kernel calls these
// functions, and tests/describe_steer_check.cpp checks them on the CPU, bit for bit, against the reference's own two-branch forms.
//
// All of it is wave-uniform: 64 lanes execute what one keypoint needs, so every instruction here is paid once per keypoint and the forms below
// are chosen for the fewest of them -- ONE division and ONE polynomial in the arc tangent, ONE cosine evaluation for cosine and sine.
// Every operation is a single correctly rounded float operation in the reference's order (build with -ffp-contract=off; on the device the
// *_rn intrinsics say so once more).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define DSTEER_HD __host__ __device__ __forceinline__
#else
#define DSTEER_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define DSTEER_ADD(a, b) __fadd_rn(a, b)
#define DSTEER_SUB(a, b) __fsub_rn(a, b)
#define DSTEER_MUL(a, b) __fmul_rn(a, b)
#define DSTEER_DIV(a, b) __fdiv_rn(a, b)
#else
#define DSTEER_ADD(a, b) ((a) + (b))
#define DSTEER_SUB(a, b) ((a) - (b))
#define DSTEER_MUL(a, b) ((a) * (b))
#define DSTEER_DIV(a, b) ((a) / (b))
#endif

namespace describe_steer {

// cv::fastAtan2 (atan_f32), degrees.  The reference divides min(|x|, |y|) by max(|x|, |y|) + eps in two branches (|x| >= |y|: y / x, else x / y
// and a = 90 - a) and evaluates the same odd polynomial in either: one division and one polynomial on the selected operands are its two branches
// value for value (at |x| == |y| both branches divide the same numbers; the reference takes the first, and so does `swap` below).
DSTEER_HD float fast_atan2(float y, float x) {
    const float p1 = 0.9997878412794807f * (float)(180 / 3.1415926535897932384626433832795);
    const float p3 = -0.3258083974640975f * (float)(180 / 3.1415926535897932384626433832795);
    const float p5 = 0.1555786518463281f * (float)(180 / 3.1415926535897932384626433832795);
    const float p7 = -0.04432655554792128f * (float)(180 / 3.1415926535897932384626433832795);
    const float ax = fabsf(x), ay = fabsf(y);
    const bool swap = !(ax >= ay);
    const float lo = swap ? ax : ay, hi = swap ? ay : ax;
    const float c = DSTEER_DIV(lo, DSTEER_ADD(hi, (float)DBL_EPSILON));
    const float c2 = DSTEER_MUL(c, c);
    float a = DSTEER_MUL(DSTEER_ADD(DSTEER_MUL(DSTEER_ADD(DSTEER_MUL(DSTEER_ADD(DSTEER_MUL(p7, c2), p5), c2), p3), c2), p1), c);
    if (swap) a = DSTEER_SUB(90.f, a);
    if (x < 0) a = DSTEER_SUB(180.f, a);
    if (y < 0) a = DSTEER_SUB(360.f, a);
    return a;
}

// float(angleDeg * M_PI / 180.0) in double (orb_extractor.cpp:286): one multiplication by the double M_PI / 180.0 gives the same float for
// EVERY float in [0, 361] (checked exhaustively, tests/test_oracle_frontend.py::test_degree_to_radian_constant_is_exact)
DSTEER_HD float deg_to_rad(float deg) { return (float)((double)deg * (M_PI / 180.0)); }

DSTEER_HD float poly_cos(float v) {        // openvslam/trigonometric.h:17-24
    const float c1 = 0.99940307f, c2 = -0.49558072f, c3 = 0.03679168f;
    const float v2 = DSTEER_MUL(v, v);
    return DSTEER_ADD(c1, DSTEER_MUL(v2, DSTEER_ADD(c2, DSTEER_MUL(c3, v2))));
}
// openvslam/trigonometric.h:26-42.  Its four quadrants each call the polynomial once, on pi - v, v - pi, 2 pi - v or v itself, and negate in the
// middle two: the argument and the sign are selected first, and the polynomial is evaluated once.
DSTEER_HD float cos_approx(float v) {
    const float PI = 3.14159265358979f, PI_2 = PI / 2.0f, TWO_PI = 2.0f * PI, INV_TWO_PI = 1.0f / TWO_PI, THREE_PI_2 = 3.0f * PI_2;
    v = DSTEER_SUB(v, DSTEER_MUL((float)(int)floorf(DSTEER_MUL(v, INV_TWO_PI)), TWO_PI));
    v = (0.0f < v) ? v : -v;
    const bool q0 = v < PI_2, q1 = v < PI, q2 = v < THREE_PI_2;
    const float lhs = q0 ? v : q1 ? PI : q2 ? v : TWO_PI;          // q0: v (- 0 is not applied: the reference passes v itself)
    const float rhs = q1 ? v : q2 ? PI : v;
    const float arg = q0 ? v : DSTEER_SUB(lhs, rhs);
    const float r = poly_cos(arg);
    return (!q0 && q2) ? -r : r;
}
// sin(v) IS cos(pi / 2 - v) in the reference (trigonometric.h:44-46): the argument a lane hands to cos_approx for the sine
DSTEER_HD float sin_argument(float v) { return DSTEER_SUB(3.14159265358979f / 2.0f, v); }
DSTEER_HD float sin_approx(float v) { return cos_approx(sin_argument(v)); }

}  // namespace describe_steer
