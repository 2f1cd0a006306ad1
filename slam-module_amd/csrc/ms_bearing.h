// ms_bearing.h -- KeyPoint::bearing of the ms_pinhole stand-in: the unit vector of ((x - cx) / fx, (y - cy) / fy, 1) in float64,
// every step rounded on its own (no contraction).  Device code shared by triangulate.hip (the rays of an observation) and keyframe_admit.hip
// (the bearing array of an admitted keyframe): one spelling, so the two give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mi355slam.h"

// xn, yn = normalizePixel; b = the bearing
__device__ __forceinline__ void ms_pinhole_bearing(const ms_pinhole &c, float x, float y, double &xn, double &yn, double *b) {
#pragma clang fp contract(off)
    xn = ((double)x - c.cx) / c.fx;
    yn = ((double)y - c.cy) / c.fy;
    const double nrm = sqrt(xn * xn + yn * yn + 1.0);
    b[0] = xn / nrm; b[1] = yn / nrm; b[2] = 1.0 / nrm;
}
