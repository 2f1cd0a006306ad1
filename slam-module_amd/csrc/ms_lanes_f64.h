#pragma once
// ms_lanes_f64.h -- the fp64 lane helpers the small-system solvers share, one copy each, at global scope: k_ba_pose_only and k_ba_one_pose (ba.hip),
// k_sim3_opt (sim3_opt.hip).  Compiled under both contract settings (ba.o contracts, the rest of the library does not): the Newton steps are explicit fma.

template <int CTRL> __device__ __forceinline__ double dpp_d(double v) {               // the double of the lane the DPP control names (all source lanes active)
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false), hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// 1 / sqrt(d) for the pivots of the small Cholesky factorisations: v_rsq_f64 and two Newton steps (one cubic, one quadratic: full double precision) -- ~10
// instructions where sqrt and a division are ~60 on the solver's critical path
__device__ __forceinline__ double rsqrt_d(double d) {
    double y = __builtin_amdgcn_rsq(d);
    double e = fma(-d * y, y, 1.0);
    y = fma(y * e, fma(e, 0.375, 0.5), y);
    e = fma(-d * y, y, 1.0);
    return fma(y * e, 0.5, y);
}

// RobustKernelHuber as oracle/ba.c restates it
__device__ __forceinline__ void huber(double chi2, double delta, double &rho0, double &w) {
    const double dsqr = delta * delta;
    if (delta <= 0 || chi2 <= dsqr) { rho0 = chi2; w = 1; }
    else { const double s = sqrt(chi2); rho0 = 2 * s * delta - dsqr; w = delta / s; }
}
