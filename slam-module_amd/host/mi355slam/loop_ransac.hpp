// loop_ransac.hpp -- host mirror of slam::LoopRansac (loop_ransac.hpp / loop_ransac.cpp:8-314) on top of ms_loop_ransac.
//
// The reference builds a LoopRansac from two keyframes, their MapDBs and a match list; those types live in the parent project, so this
// mirror is built from the plain data they provide (INTEGRATION.md shows the glue): the matched map points in each keyframe's camera
// frame (Isometry3d(kf.poseCW) * mp.position), the octave of each observation, the two cameras and the StaticSettings.
//
// Camera: tracker::Camera is also the parent project's.  PinholeCamera is the stand-in of include/mi355slam.h (ms_pinhole): a point is
// visible iff z > 0 and its pixel lies in [0, width) x [0, height).  Other camera models are not supported.
//
// Sampling: ransacSolve draws its triplets here, on the host, in exactly the order of openvslam::util::create_random_array(3, 0, n - 1)
// on a thread_local std::mt19937(94235682) (random_array.cc:20-60), so with libstdc++ the same sequence comes out; the device only
// evaluates them.  The engine replaces openvslam's thread_local one: nothing else on the loop-closer thread draws from that engine.
#pragma once
#include <algorithm>
#include <array>
#include <random>
#include <vector>
#include "common.hpp"

namespace mi355slam {

// tracker::Camera stand-in (pinhole only)
struct PinholeCamera {
    double fx, fy, cx, cy;
    int width, height;
    ms_pinhole c() const { return ms_pinhole{fx, fy, cx, cy, width, height}; }
};

// the loop closer's engine: openvslam's `thread_local std::mt19937 random_engine(94235682)`
inline std::mt19937 &loopRansacEngine() {
    thread_local std::mt19937 engine(94235682);
    return engine;
}

// create_random_array(3, 0, n - 1): draw size_t(3 * 1.2) = 3 values, sort, drop repeats, draw again until 3 distinct remain, then shuffle
inline std::array<int32_t, 3> randomTriplet(int n, std::mt19937 &engine = loopRansacEngine()) {
    std::uniform_int_distribution<int> uniform(0, n - 1);
    std::array<int32_t, 3> v{};
    std::size_t k = 0;
    while (k != 3) {
        while (k < 3) v[k++] = uniform(engine);
        std::sort(v.begin(), v.begin() + k);
        k = (std::size_t)(std::unique(v.begin(), v.begin() + k) - v.begin());
    }
    std::shuffle(v.begin(), v.end(), engine);
    return v;
}

class LoopRansac {
public:
    enum class DoF { SIM3, ZROT };
    using Vec3 = std::array<double, 3>;
    using Vec2 = std::array<double, 2>;
    static_assert(sizeof(Vec3) == 3 * sizeof(double), "points are handed to the C ABI as packed [n*3] doubles");

    // loop_ransac.cpp:8-45: pts = the matched map points in each keyframe's camera frame, octaves = their keypoints' octaves
    LoopRansac(const std::vector<Vec3> &pts1, const std::vector<Vec3> &pts2, const std::vector<int> &octaves1, const std::vector<int> &octaves2,
               const PinholeCamera &camera1, const PinholeCamera &camera2, const StaticSettings &settings)
        : camera1(camera1), camera2(camera2), commonPtsInKeyframe1(pts1), commonPtsInKeyframe2(pts2), settings(settings) {
        if (pts2.size() != pts1.size() || octaves1.size() != pts1.size() || octaves2.size() != pts1.size())
            throw std::invalid_argument("LoopRansac: points and octaves must describe the same matches");
        matchCount = (unsigned)pts1.size();
        constexpr float CHI_SQ_2D = 9.21034f;
        for (unsigned i = 0; i < matchCount; ++i) {
            chiSqSigmaSq1.push_back(CHI_SQ_2D * settings.levelSigmaSq.at((std::size_t)octaves1[i]));
            chiSqSigmaSq2.push_back(CHI_SQ_2D * settings.levelSigmaSq.at((std::size_t)octaves2[i]));
        }
        reprojected1 = reprojectToSameImage(commonPtsInKeyframe1, camera1, visibleSame1);
        reprojected2 = reprojectToSameImage(commonPtsInKeyframe2, camera2, visibleSame2);
    }

    // the same object from thresholds that are already CHI_SQ_2D * levelSigmaSq[octave] (what ms_loop_pairs gathers from the device tables)
    LoopRansac(const std::vector<Vec3> &pts1, const std::vector<Vec3> &pts2, const std::vector<float> &thresholds1, const std::vector<float> &thresholds2,
               const PinholeCamera &camera1, const PinholeCamera &camera2, const StaticSettings &settings)
        : camera1(camera1), camera2(camera2), commonPtsInKeyframe1(pts1), commonPtsInKeyframe2(pts2), chiSqSigmaSq1(thresholds1), chiSqSigmaSq2(thresholds2),
          settings(settings) {
        if (pts2.size() != pts1.size() || thresholds1.size() != pts1.size() || thresholds2.size() != pts1.size())
            throw std::invalid_argument("LoopRansac: points and thresholds must describe the same matches");
        matchCount = (unsigned)pts1.size();
        reprojected1 = reprojectToSameImage(commonPtsInKeyframe1, camera1, visibleSame1);
        reprojected2 = reprojectToSameImage(commonPtsInKeyframe2, camera2, visibleSame2);
    }

    // :52-54
    bool earlyReturn() const { return matchCount < 3 || matchCount < settings.parameters.loopClosureRansacMinInliers; }

    // the triplets ransacSolve draws, from the mirror's engine ([max_num_iter * 3]); none on the early return
    std::vector<int32_t> drawSamples(unsigned max_num_iter) const {
        std::vector<int32_t> s;
        if (earlyReturn()) return s;
        s.reserve(3 * (std::size_t)max_num_iter);
        for (unsigned i = 0; i < max_num_iter; ++i) {
            const auto t = randomTriplet((int)matchCount);
            s.insert(s.end(), t.begin(), t.end());
        }
        return s;
    }

    // loop_ransac.cpp:47-110 on the device
    void ransacSolve(Context &ctx, unsigned max_num_iter, DoF dof = DoF::ZROT) {
        std::vector<LoopRansac *> one{this};
        solveAll(ctx, one, max_num_iter, dof);
    }

    // several objects in one ms_loop_ransac: samples are drawn in object order, the order the reference calls ransacSolve in
    static void solveAll(Context &ctx, const std::vector<LoopRansac *> &objs, unsigned max_num_iter, DoF dof) {
        const std::size_t n = objs.size();
        std::vector<std::vector<int32_t>> samples(n);
        std::vector<ms_loop_ransac_problem> probs(n);
        std::vector<ms_loop_ransac_result> res(n);
        std::vector<std::vector<uint8_t>> um(n), bm(n);
        std::vector<uint8_t *> up(n), bp(n);
        for (std::size_t k = 0; k < n; ++k) {
            LoopRansac &o = *objs[k];
            samples[k] = o.drawSamples(max_num_iter);
            um[k].resize(o.matchCount);
            bm[k].resize(o.matchCount);
            up[k] = um[k].data();
            bp[k] = bm[k].data();
            probs[k] = ms_loop_ransac_problem{(int32_t)o.matchCount,
                                              o.commonPtsInKeyframe1.empty() ? nullptr : o.commonPtsInKeyframe1[0].data(),
                                              o.commonPtsInKeyframe2.empty() ? nullptr : o.commonPtsInKeyframe2[0].data(),
                                              o.chiSqSigmaSq1.data(), o.chiSqSigmaSq2.data(), o.camera1.c(), o.camera2.c(), (int32_t)max_num_iter,
                                              samples[k].empty() ? nullptr : samples[k].data(), dof == DoF::ZROT ? MS_RANSAC_ZROT : MS_RANSAC_SIM3,
                                              o.settings.parameters.loopClosureRansacFixScale ? 1 : 0,
                                              (int32_t)o.settings.parameters.loopClosureRansacMinInliers};
        }
        if (n == 0) return;
        ctx.check(ms_loop_ransac(ctx.get(), probs.data(), (int)n, res.data(), up.data(), bp.data(), nullptr), "ms_loop_ransac");
        for (std::size_t k = 0; k < n; ++k) {
            LoopRansac &o = *objs[k];
            const ms_loop_ransac_result &r = res[k];
            o.solutionOk = r.solution_ok != 0;
            o.bestInlierCount = (unsigned)r.best_inlier_count;
            o.bestIteration = r.best_iter;
            if (r.best_iter < 0) continue;                   // nothing scored: the reference assigns none of the best* members
            std::copy(r.R12, r.R12 + 9, o.bestR12.begin());
            std::copy(r.t12, r.t12 + 3, o.bestT12.begin());
            o.bestScale12 = r.scale12;
            o.bestInliers.assign(um[k].begin(), um[k].end());
            o.bestHypothesisInliers.assign(bm[k].begin(), bm[k].end());
        }
    }

    const PinholeCamera camera1, camera2;

    // local coordinates in kf1 and kf2 of the matched map points
    std::vector<Vec3> commonPtsInKeyframe1, commonPtsInKeyframe2;
    std::vector<bool> visibleSame1, visibleSame2;
    // chi-square thresholds (two degrees of freedom) of the reprojection errors
    std::vector<float> chiSqSigmaSq1, chiSqSigmaSq2;
    unsigned matchCount = 0;

    bool solutionOk = false;
    std::array<double, 9> bestR12{};                        // row-major rotation kf2 -> kf1
    std::array<double, 3> bestT12{};
    float bestScale12 = 0.f;
    // the reference's bestInliers: the UNION of the inlier sets of iterations 0 .. best (its inlier vector is never cleared, :64, :202);
    // loop_closer.cpp:239-243 selects the matches with it.  Empty when nothing scored.
    std::vector<bool> bestInliers;
    unsigned bestInlierCount = 0;
    // not in the reference: the inlier set of the best hypothesis alone, and the iteration it came from (-1: none scored)
    std::vector<bool> bestHypothesisInliers;
    int bestIteration = -1;

    // image coordinates of the map points in their own image (identity pose)
    std::vector<Vec2> reprojected1, reprojected2;

    const StaticSettings &settings;

private:
    static std::vector<Vec2> reprojectToSameImage(const std::vector<Vec3> &pts, const PinholeCamera &c, std::vector<bool> &visible) {
        std::vector<Vec2> out;
        out.reserve(pts.size());
        visible.clear();
        for (const Vec3 &p : pts) {
            const double u = c.fx * (p[0] / p[2]) + c.cx, v = c.fy * (p[1] / p[2]) + c.cy;
            const bool vis = p[2] > 0.0 && u >= 0.0 && u < (double)c.width && v >= 0.0 && v < (double)c.height;
            visible.push_back(vis);
            out.push_back(Vec2{u, v});                        // meaningful only where visible
        }
        return out;
    }
};

// the batched form of LoopRansac::ransacSolve
inline void ransacSolveAll(Context &ctx, const std::vector<LoopRansac *> &objs, unsigned max_num_iter, LoopRansac::DoF dof) {
    LoopRansac::solveAll(ctx, objs, max_num_iter, dof);
}

}  // namespace mi355slam
