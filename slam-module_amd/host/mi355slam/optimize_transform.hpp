// optimize_transform.hpp -- host mirror of slam::OptimizeSim3Transform (optimize_transform.hpp / optimize_transform.cpp:63-155) on top of
// ms_sim3_optimize.
//
// The reference takes two keyframes, a match list and the MapDB; those types live in the parent project, so this mirror takes the plain data
// it reads from them (INTEGRATION.md shows the glue): per match the two map points in their keyframes' camera frames
// (Isometry3d(kf.poseCW) * mp.position, getMpVertex :44-59), the two observations bearing.xy / bearing.z (:116, :131) and the two octaves.
//
// g2o::Sim3 is not part of the reference tree either: Sim3 below is the value type callers compose the result with (loop_closer.cpp:280,
// :405): unit quaternion, translation, scale, with map, inverse and operator* as sim3.h defines them.
#pragma once
#include <array>
#include <cmath>
#include <vector>
#include "common.hpp"

namespace mi355slam {

// g2o::Sim3 stand-in: S.map(p) = s * (r * p) + t
struct Sim3 {
    using Vec3 = std::array<double, 3>;
    std::array<double, 4> q{1.0, 0.0, 0.0, 0.0};           // unit quaternion (w, x, y, z)
    Vec3 t{0.0, 0.0, 0.0};
    double s = 1.0;

    Sim3() = default;
    Sim3(const std::array<double, 4> &q_, const Vec3 &t_, double s_) : q(q_), t(t_), s(s_) { normalize(); }
    // Sim3(bestR12, bestT12, bestScale12) of loop_closer.cpp:273-276: R row-major
    Sim3(const std::array<double, 9> &R, const Vec3 &t_, double s_) : t(t_), s(s_) {
        const double tr = R[0] + R[4] + R[8];
        if (tr > 0.0) {
            const double w4 = 2.0 * std::sqrt(tr + 1.0);
            q = {0.25 * w4, (R[7] - R[5]) / w4, (R[2] - R[6]) / w4, (R[3] - R[1]) / w4};
        } else if (R[0] > R[4] && R[0] > R[8]) {
            const double x4 = 2.0 * std::sqrt(1.0 + R[0] - R[4] - R[8]);
            q = {(R[7] - R[5]) / x4, 0.25 * x4, (R[1] + R[3]) / x4, (R[2] + R[6]) / x4};
        } else if (R[4] > R[8]) {
            const double y4 = 2.0 * std::sqrt(1.0 + R[4] - R[0] - R[8]);
            q = {(R[2] - R[6]) / y4, (R[1] + R[3]) / y4, 0.25 * y4, (R[5] + R[7]) / y4};
        } else {
            const double z4 = 2.0 * std::sqrt(1.0 + R[8] - R[0] - R[4]);
            q = {(R[3] - R[1]) / z4, (R[2] + R[6]) / z4, (R[5] + R[7]) / z4, 0.25 * z4};
        }
        normalize();
    }

    std::array<double, 9> rotationMatrix() const {         // row-major
        const double w = q[0], x = q[1], y = q[2], z = q[3];
        return {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)};
    }
    Vec3 rotate(const Vec3 &p) const {
        const auto R = rotationMatrix();
        return {R[0] * p[0] + R[1] * p[1] + R[2] * p[2], R[3] * p[0] + R[4] * p[1] + R[5] * p[2], R[6] * p[0] + R[7] * p[1] + R[8] * p[2]};
    }
    // s * (r * p) + t
    Vec3 map(const Vec3 &p) const {
        const Vec3 r = rotate(p);
        return {s * r[0] + t[0], s * r[1] + t[1], s * r[2] + t[2]};
    }
    // (r^-1, -(1 / s) * (r^-1 * t), 1 / s)
    Sim3 inverse() const {
        Sim3 o;
        o.q = {q[0], -q[1], -q[2], -q[3]};
        const Vec3 rt = o.rotate(t);
        o.s = 1.0 / s;
        o.t = {-o.s * rt[0], -o.s * rt[1], -o.s * rt[2]};
        return o;
    }
    // (A.r * B.r, A.s * (A.r * B.t) + A.t, A.s * B.s)
    Sim3 operator*(const Sim3 &b) const {
        Sim3 o;
        o.q = {q[0] * b.q[0] - q[1] * b.q[1] - q[2] * b.q[2] - q[3] * b.q[3], q[0] * b.q[1] + q[1] * b.q[0] + q[2] * b.q[3] - q[3] * b.q[2],
               q[0] * b.q[2] - q[1] * b.q[3] + q[2] * b.q[0] + q[3] * b.q[1], q[0] * b.q[3] + q[1] * b.q[2] - q[2] * b.q[1] + q[3] * b.q[0]};
        o.normalize();
        const Vec3 rt = rotate(b.t);
        o.t = {s * rt[0] + t[0], s * rt[1] + t[1], s * rt[2] + t[2]};
        o.s = s * b.s;
        return o;
    }

private:
    void normalize() {
        const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (n > 0.0) for (double &v : q) v /= n;
    }
};

// what OptimizeSim3Transform reads from (kf1, kf2, matches, mapDB), match by match
struct Sim3Matches {
    using Vec3 = std::array<double, 3>;
    using Vec2 = std::array<double, 2>;
    static_assert(sizeof(Vec3) == 3 * sizeof(double) && sizeof(Vec2) == 2 * sizeof(double), "handed to the C ABI as packed doubles");
    std::vector<Vec3> pts1, pts2;          // kf1.poseCW * mp1.position, kf2.poseCW * mp2.position
    std::vector<Vec2> obs1, obs2;          // keyPoint.bearing.xy / keyPoint.bearing.z in kf1, kf2
    std::vector<int> octaves1, octaves2;   // keyPoint.octave in kf1, kf2
    std::vector<float> info1, info2;       // when not empty: levelSigmaSq[octave] as ms_loop_sim3_lists gathered it, used in place of the octaves
    std::size_t size() const { return pts1.size(); }
};

// what the solve reports beside the transform (ms_sim3_opt_result)
struct Sim3OptStats {
    double chi2Initial = 0, chi2Final = 0, lambda = 0;
    int iterations = 0, trials = 0;
    bool stoppedEarly = false;
};

// the batch form: all candidates of one keyframe in one ms_sim3_optimize.  transforms12[k] is refined in place; returns matches.size() per problem
// (the reference's return value, :153-154: its inlier check is a TODO)
inline std::vector<unsigned> OptimizeSim3TransformAll(Context &ctx, const std::vector<const Sim3Matches *> &matches, std::vector<Sim3> &transforms12,
                                                      const StaticSettings &settings, std::vector<Sim3OptStats> *stats = nullptr, int maxIterations = 20) {
    const std::size_t n = matches.size();
    if (transforms12.size() != n) throw std::invalid_argument("OptimizeSim3Transform: one transform per match set");
    std::vector<std::vector<float>> info1(n), info2(n);
    std::vector<ms_sim3_opt_problem> probs(n);
    std::vector<ms_sim3_opt_result> res(n);
    const float deltaHuber = std::sqrt((float)settings.parameters.loopClosureInlierThreshold);        // :72-73, float as in the reference
    for (std::size_t k = 0; k < n; ++k) {
        const Sim3Matches &m = *matches[k];
        const std::size_t c = m.size();
        const bool gathered = !m.info1.empty() || !m.info2.empty();
        if (m.pts2.size() != c || m.obs1.size() != c || m.obs2.size() != c ||
            (gathered ? m.info1.size() != c || m.info2.size() != c : m.octaves1.size() != c || m.octaves2.size() != c))
            throw std::invalid_argument("OptimizeSim3Transform: points, observations and octaves must describe the same matches");
        if (gathered) { info1[k] = m.info1; info2[k] = m.info2; }
        for (std::size_t i = 0; i < c && !gathered; ++i) {
            info1[k].push_back(settings.levelSigmaSq.at((std::size_t)m.octaves1[i]));               // :122 (levelSigmaSq, not its inverse)
            info2[k].push_back(settings.levelSigmaSq.at((std::size_t)m.octaves2[i]));               // :137
        }
        ms_sim3_opt_problem &p = probs[k];
        p.n_matches = (int32_t)c;
        p.pts1 = c ? m.pts1[0].data() : nullptr; p.pts2 = c ? m.pts2[0].data() : nullptr;
        p.obs1 = c ? m.obs1[0].data() : nullptr; p.obs2 = c ? m.obs2[0].data() : nullptr;
        p.info1 = info1[k].data(); p.info2 = info2[k].data();
        p.huber_delta = (double)deltaHuber;
        p.fix_scale = settings.parameters.loopClosureRansacFixScale ? 1 : 0;
        p.max_iters = maxIterations;
        const auto R = transforms12[k].rotationMatrix();
        std::copy(R.begin(), R.end(), p.R12);
        std::copy(transforms12[k].t.begin(), transforms12[k].t.end(), p.t12);
        p.scale12 = transforms12[k].s;
    }
    std::vector<unsigned> counts(n);
    if (n == 0) return counts;
    ctx.check(ms_sim3_optimize(ctx.get(), probs.data(), (int)n, res.data(), nullptr), "ms_sim3_optimize");
    if (stats) stats->assign(n, Sim3OptStats{});
    for (std::size_t k = 0; k < n; ++k) {
        const ms_sim3_opt_result &r = res[k];
        std::array<double, 9> R;
        std::copy(r.R12, r.R12 + 9, R.begin());
        transforms12[k] = Sim3(R, Sim3::Vec3{r.t12[0], r.t12[1], r.t12[2]}, r.scale12);
        if (stats) (*stats)[k] = Sim3OptStats{r.chi2_init, r.chi2_final, r.lambda, r.iters, r.trials_total, r.stop_reason != 0};
        counts[k] = (unsigned)matches[k]->size();
    }
    return counts;
}

// optimize_transform.cpp:63-155 on the device
inline unsigned OptimizeSim3Transform(Context &ctx, const Sim3Matches &matches, Sim3 &transform12, const StaticSettings &settings,
                                      Sim3OptStats *stats = nullptr) {
    std::vector<Sim3> one{transform12};
    std::vector<Sim3OptStats> st;
    const std::vector<unsigned> c = OptimizeSim3TransformAll(ctx, {&matches}, one, settings, stats ? &st : nullptr);
    transform12 = one[0];
    if (stats) *stats = st[0];
    return c[0];
}

}  // namespace mi355slam
