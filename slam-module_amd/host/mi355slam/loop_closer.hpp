// loop_closer.hpp -- host mirror of the candidate loop of LoopCloser::tryLoopClosure (loop_closer.cpp:132-357) on the device map tables
// (DESIGN 9.16).  The cheap rejections and the accept gates stay on the host; everything that read MapDB::mapPoints, observations.at(kf.id)
// and kf.mapPoints.at(i) is gathered on the device for all surviving candidates at once (ms_loop_usable_mask, ms_loop_pairs,
// ms_loop_sim3_lists) between the batched solvers (ms_match_loop_closure, ransacSolveAll, matchMapPointsSim3 on table rows,
// OptimizeSim3TransformAll).  The mirror keeps no map of observations, uploads no table and downloads no table row but tri_row.
#pragma once
#include <cmath>
#include "keyframe_matcher.hpp"
#include "loop_ransac.hpp"
#include "map_update.hpp"
#include "optimize_transform.hpp"

namespace mi355slam {

enum class LoopStage { BOW_MATCH, QUICK_TESTS, MAP_POINT_MATCHES, ACCEPTED };         // loop_closer.hpp:23-30 without the relocation stages
// LoopCloserStats::Loop (loop_closer_stats.hpp:9-26); UNKNOWN = the loop never reached the candidate (the heavyComputations stop)
enum class LoopCode { OK, TOO_CLOSE_TIME, UNNECESSARY_EARLY, TOO_FEW_FEATURE_MATCHES, RANSAC_FAILED, UNNECESSARY, TOO_LARGE_POSITION_DRIFT, TOO_LARGE_ANGLE_DRIFT, UNKNOWN };

// loop_closer.cpp:31-40 on slots, keypoints and table rows
struct LoopClosure {
    std::int32_t candidateSlot = -1;
    Sim3 candToCurr;
    std::vector<std::pair<int, int>> keyPointMatches;        // (keypoint of the current keyframe, keypoint of the candidate)
    std::vector<std::pair<std::int32_t, std::int32_t>> mapPointMatches;      // their table rows
};
struct LoopCandidateOutcome {
    std::int32_t slot = -1;
    LoopCode code = LoopCode::UNKNOWN;
    LoopStage stage = LoopStage::BOW_MATCH;
};
struct LoopClosureResult {
    std::vector<LoopClosure> closures;                       // accepted, by descending candidate id (:366-369)
    std::vector<LoopCandidateOutcome> candidates;            // in candidate order, up to and including the one the loop stopped at
};

namespace detail {
using Pose = std::array<double, 12>;
inline std::array<double, 3> cameraCenterOf(const Pose &P) {                 // worldToCameraMatrixCameraCenter: -R^T t
    std::array<double, 3> c;
    for (int j = 0; j < 3; ++j) c[j] = -((P[j] * P[3] + P[4 + j] * P[7]) + P[8 + j] * P[11]);
    return c;
}
inline double distance(const std::array<double, 3> &a, const std::array<double, 3> &b) {
    const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return std::sqrt(x * x + (y * y + z * z));
}
// the two poses matchMapPointsSim3 projects with: transform12^-1 * kf1.poseCW (:650) and transform12 * kf2.poseCW (:661), R | t row-major
inline void sim3ViewPoses(const std::array<double, 9> &R12, const std::array<double, 3> &t12, double s12, const Pose &P1, const Pose &P2, double R1in2[9], double t1in2[3],
                          double R2in1[9], double t2in1[3]) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            double a = 0, b = 0;
            for (int k = 0; k < 3; ++k) { a += R12[3 * k + i] * P1[4 * k + j]; b += R12[3 * i + k] * P2[4 * k + j]; }
            R1in2[3 * i + j] = a / s12; R2in1[3 * i + j] = s12 * b;
        }
        double a = 0, b = 0;
        for (int k = 0; k < 3; ++k) { a += R12[3 * k + i] * (P1[4 * k + 3] - t12[k]); b += R12[3 * i + k] * P2[4 * k + 3]; }
        t1in2[i] = a / s12; t2in1[i] = s12 * b + t12[i];
    }
}
// The accept gates of loop_closer.cpp:279-338 for one candidate whose transform was refined; distanceTraveled from the chain (:312-319).
inline LoopCode acceptGates(const Sim3 &candToCurr, const Pose &curPose, const Pose &candPose, bool isAdjacent, double timeBetweenKf, double distanceTraveled,
                            const Parameters &p) {
    std::array<double, 9> Rc;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rc[3 * i + j] = candPose[4 * i + j];
    const Sim3 updated = candToCurr * Sim3(Rc, Sim3::Vec3{candPose[3], candPose[7], candPose[11]}, 1.0);      // :280
    const std::array<double, 9> Ru = updated.rotationMatrix();
    Pose U;
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) U[4 * i + j] = Ru[3 * i + j]; U[4 * i + 3] = updated.t[i]; }
    const std::array<double, 3> cu = cameraCenterOf(U);
    const double correctionDistance = distance(cameraCenterOf(curPose), cu);                                  // :285
    if (isAdjacent && correctionDistance < 0.75) return LoopCode::UNNECESSARY;
    if (distance(cameraCenterOf(candPose), cu) > 1.0 * correctionDistance) return LoopCode::UNNECESSARY;     // :293-298
    // :306-309: R = (U * candPose).R * curPose.R^T with U = sim3ToSe3(candToCurr), which is the rotation of `updated`
    double trace = 0;
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) trace += Ru[3 * i + k] * curPose[4 * i + k];
    const double angleChange = std::acos(std::max(-1.0, std::min(1.0, 0.5 * (trace - 1.0))));
    if (correctionDistance / timeBetweenKf > p.maximumDriftMetersPerSecond || correctionDistance / distanceTraveled > p.maximumDriftMetersPerTraveled)
        return LoopCode::TOO_LARGE_POSITION_DRIFT;
    if (angleChange / timeBetweenKf > p.maximumDriftRadiansPerSecond || angleChange / distanceTraveled > p.maximumDriftRadiansPerTraveled)
        return LoopCode::TOO_LARGE_ANGLE_DRIFT;
    return LoopCode::OK;
}
// :164-187: TOO_CLOSE_TIME, UNNECESSARY_EARLY or UNKNOWN (the candidate goes on to the heavy computations)
inline LoopCode cheapRejection(const KeyframeSlots &chain, std::int32_t current, std::int32_t cand, double previousClosureT, bool isAdjacent) {
    const double correctionLength = chain.t[current] - std::max(chain.t[cand], previousClosureT);
    if (correctionLength < 5.0) return LoopCode::TOO_CLOSE_TIME;
    if (chain.t[current] - chain.t[cand] < 2.15) return LoopCode::TOO_CLOSE_TIME;
    if (isAdjacent && distance(chain.cameraCenter[cand], chain.cameraCenter[current]) < 0.5) return LoopCode::UNNECESSARY_EARLY;
    return LoopCode::UNKNOWN;
}
inline double distanceTraveled(const KeyframeSlots &chain, std::int32_t current, std::int32_t cand) {        // :312-319
    double d = 0;
    for (std::int32_t at = current; at != cand;) {
        const std::int32_t before = chain.previous.at((std::size_t)at);
        if (before < 0) throw std::invalid_argument("tryLoopClosure: the chain from the current keyframe does not reach the candidate");
        d += distance(chain.cameraCenter[at], chain.cameraCenter[before]);
        at = before;
    }
    return d;
}
}  // namespace detail

// The candidate loop of tryLoopClosure (:132-357) for the keyframe in slot `current`.  candidates = getBowSimilar's keyframes of the current
// map as slots, in its order; adjacent = the adjacent keyframes' slots.  Of M.slots it reads the previous links, camera centres, ids, times and
// cameras, and frames[slot] = the keyframe's matcher inputs on the device, whose `usable` mask is the one thing written here.  M.live may be
// null: every row is live.
inline LoopClosureResult tryLoopClosureOnTables(Context &ctx, MapTables M, std::int32_t current, const std::vector<std::int32_t> &candidates, const std::vector<std::int32_t> &adjacent,
                                                double previousClosureT, const StaticSettings &settings) {
    M.require("tryLoopClosureOnTables", M.POINTS | M.FLAGS | M.POSES | M.KEYPOINTS | M.FRAMES | M.CAMERAS | M.TIMES | M.IDS | M.CENTRES | M.LINKS);
    const Parameters &P = settings.parameters;
    const KeyframeSlots &chain = M.slots;
    const int nKf = (int)M.keyframes.size(), stride = (int)M.keyframes.stride(), nMp = (int)M.keyframes.mapPointCount();
    if (current < 0 || current >= nKf) throw std::invalid_argument("tryLoopClosureOnTables: the current keyframe lies outside the table");
    LoopClosureResult out;
    // 1. the cheap rejections, in candidate order, with the stop of :149
    std::vector<std::size_t> heavy;                          // positions in out.candidates
    for (std::int32_t cand : candidates) {
        if (cand < 0 || cand >= nKf || cand == current) throw std::invalid_argument("tryLoopClosureOnTables: candidate slot outside the table");
        out.candidates.push_back(LoopCandidateOutcome{cand, LoopCode::UNKNOWN, LoopStage::BOW_MATCH});
        if (heavy.size() > 10) break;
        const bool isAdjacent = std::find(adjacent.begin(), adjacent.end(), cand) != adjacent.end();
        LoopCandidateOutcome &o = out.candidates.back();
        o.code = detail::cheapRejection(chain, current, cand, previousClosureT, isAdjacent);
        if (o.code != LoopCode::UNKNOWN) continue;
        o.stage = LoopStage::QUICK_TESTS;
        heavy.push_back(out.candidates.size() - 1);
    }
    const int n = (int)heavy.size();
    if (n == 0) return out;
    const int nKpCur = (int)chain.frames[(std::size_t)current]->keyPointCount();
    std::vector<std::int32_t> slot(n), nKp(n);
    for (int c = 0; c < n; ++c) { slot[c] = out.candidates[heavy[c]].slot; nKp[c] = (int)chain.frames[(std::size_t)slot[c]]->keyPointCount(); }
    // 2. the matcher's masks and the TRIANGULATED rows of the current keyframe and of every survivor, one call
    std::vector<std::int32_t> mSlot{current}, mKp{nKpCur}, mReq{P.requireTringulationForLoopClosures ? 1 : 0};
    for (int c = 0; c < n; ++c) { mSlot.push_back(slot[c]); mKp.push_back(nKp[c]); mReq.push_back(1); }
    std::vector<DeviceArray<std::int32_t>> triRow;
    std::vector<std::uint8_t *> usable;
    std::vector<std::int32_t *> tri;
    for (int s = 0; s <= n; ++s) {
        triRow.emplace_back(ctx, (std::size_t)mKp[s]);
        usable.push_back(chain.frames[(std::size_t)mSlot[s]]->mutableUsable());
        tri.push_back(triRow.back().data());
    }
    const std::uint8_t *live = M.live ? M.live->live() : nullptr;
    ctx.check(ms_loop_usable_mask(ctx.get(), M.keyframes.table(), nKf, stride, M.flags->flags(), live, nMp, mSlot.data(), mKp.data(), mReq.data(), usable.data(), tri.data(), n + 1),
              "ms_loop_usable_mask");
    // 3. matchForLoopClosures of the current keyframe against every survivor, one call; `matched` stays on the device
    std::vector<ms_match_frame> f1((std::size_t)n, chain.frames[(std::size_t)current]->frame()), f2;
    std::vector<DeviceArray<std::int32_t>> matched;
    std::vector<std::int32_t *> matchedPtr;
    for (int c = 0; c < n; ++c) {
        f2.push_back(chain.frames[(std::size_t)slot[c]]->frame());
        matched.emplace_back(ctx, (std::size_t)std::max(nKpCur, 1));
        matchedPtr.push_back(matched.back().data());
    }
    DeviceArray<std::int32_t> nMatches(ctx, (std::size_t)n);
    ctx.check(ms_match_loop_closure(ctx.get(), f1.data(), f2.data(), n, P.loopClosureFeatureMatchLoweRatio, 1, matchedPtr.data(), nMatches.data()), "ms_match_loop_closure");
    // 4. the pairs, clouds and thresholds of every survivor, one call (at most one pair per keypoint of the current keyframe and candidate)
    const std::size_t cap = (std::size_t)n * (std::size_t)nKpCur;
    std::vector<std::int32_t> pairStart((std::size_t)n + 1), kp1(cap), kp2(cap), row1(cap), row2(cap);
    std::vector<LoopRansac::Vec3> pts1(cap), pts2(cap);
    std::vector<float> thr1(cap), thr2(cap);
    detail::Pose curPose{};
    std::vector<detail::Pose> candPose((std::size_t)n);
    std::int32_t nPairs = 0;
    ctx.check(ms_loop_pairs(ctx.get(), M.keyframes.table(), nKf, stride, live, M.points->position(), nMp, M.poses->pose(), M.keypoints->octave(), current, nKpCur, slot.data(),
                            nKp.data(), matchedPtr.data(), n, settings.levelSigmaSq.data(), (int)settings.levelSigmaSq.size(), (int)cap, pairStart.data(), kp1.data(), kp2.data(),
                            row1.data(), row2.data(), cap ? pts1[0].data() : nullptr, cap ? pts2[0].data() : nullptr, thr1.data(), thr2.data(), curPose.data(),
                            candPose[0].data(), &nPairs), "ms_loop_pairs");
    if (nKpCur == 0) {                                       // no pair anywhere, and the poses were not read
        for (int c = 0; c < n; ++c) out.candidates[heavy[c]].code = LoopCode::TOO_FEW_FEATURE_MATCHES;
        return out;
    }
    // 5.-7. the minimum of :215, then RANSAC for the rest in candidate order: the engine's draws are the reference's
    std::vector<std::unique_ptr<LoopRansac>> ransac((std::size_t)n);
    std::vector<LoopRansac *> solve;
    for (int c = 0; c < n; ++c) {
        const std::size_t a = (std::size_t)pairStart[c], b = (std::size_t)pairStart[c + 1];
        if (b - a < P.minLoopClosureFeatureMatches) { out.candidates[heavy[c]].code = LoopCode::TOO_FEW_FEATURE_MATCHES; continue; }
        const ms_pinhole &k1 = chain.camera[(std::size_t)current], &k2 = chain.camera[(std::size_t)slot[c]];
        ransac[c].reset(new LoopRansac(std::vector<LoopRansac::Vec3>(pts1.begin() + a, pts1.begin() + b), std::vector<LoopRansac::Vec3>(pts2.begin() + a, pts2.begin() + b),
                                       std::vector<float>(thr1.begin() + a, thr1.begin() + b), std::vector<float>(thr2.begin() + a, thr2.begin() + b),
                                       PinholeCamera{k1.fx, k1.fy, k1.cx, k1.cy, k1.width, k1.height}, PinholeCamera{k2.fx, k2.fy, k2.cx, k2.cy, k2.width, k2.height}, settings));
        solve.push_back(ransac[c].get());
    }
    ransacSolveAll(ctx, solve, P.loopClosureRansacIterations, LoopRansac::DoF::SIM3);
    // 8.-9. the inliers of the union mask (:238-243), then matchMapPointsSim3 on the downloaded tri_row
    std::vector<int> left;                                   // survivors that reach the refinement
    std::vector<std::vector<std::pair<int, int>>> lists((std::size_t)n);
    std::vector<std::int32_t> mps1;
    for (int c = 0; c < n; ++c) {
        if (!ransac[c]) continue;
        const LoopRansac &r = *ransac[c];
        if (!r.solutionOk) { out.candidates[heavy[c]].code = LoopCode::RANSAC_FAILED; continue; }
        out.candidates[heavy[c]].stage = LoopStage::MAP_POINT_MATCHES;
        const std::size_t a = (std::size_t)pairStart[c];
        for (std::size_t i = 0; i < r.bestInliers.size(); ++i)
            if (r.bestInliers[i]) lists[c].emplace_back(kp1[a + i], kp2[a + i]);
        if (mps1.empty()) mps1 = triRow[0].download();
        const std::vector<std::int32_t> mps2 = triRow[(std::size_t)c + 1].download();
        double R1in2[9], t1in2[3], R2in1[9], t2in1[3];
        detail::sim3ViewPoses(r.bestR12, r.bestT12, (double)r.bestScale12, curPose, candPose[c], R1in2, t1in2, R2in1, t2in1);
        matchMapPointsSim3(ctx, *chain.frames[(std::size_t)current], *chain.frames[(std::size_t)slot[c]], *M.points, mps1, mps2, R1in2, t1in2, R2in1, t2in1,
                           chain.camera[(std::size_t)current], chain.camera[(std::size_t)slot[c]], lists[c], settings);
        left.push_back(c);
    }
    if (left.empty()) return out;
    // 10. the arrays of every remaining candidate's Sim3 problem, one call
    std::vector<std::int32_t> lSlot, lKp, start{0}, a1, a2;
    for (int c : left) {
        lSlot.push_back(slot[c]); lKp.push_back(nKp[c]);
        for (const std::pair<int, int> &m : lists[c]) { a1.push_back(m.first); a2.push_back(m.second); }
        start.push_back((std::int32_t)a1.size());
    }
    const std::size_t nm = a1.size();
    std::vector<Sim3Matches::Vec3> q1(nm), q2(nm);
    std::vector<Sim3Matches::Vec2> o1(nm), o2(nm);
    std::vector<float> i1(nm), i2(nm);
    std::vector<std::int32_t> r1(nm), r2(nm);
    ctx.check(ms_loop_sim3_lists(ctx.get(), M.keyframes.table(), nKf, stride, live, M.points->position(), nMp, M.poses->pose(), M.keypoints->x(), M.keypoints->y(), M.keypoints->octave(),
                                 current, nKpCur, lSlot.data(), lKp.data(), (int)left.size(), chain.camera.data(), settings.levelSigmaSq.data(), (int)settings.levelSigmaSq.size(),
                                 a1.data(), a2.data(), start.data(), nm ? q1[0].data() : nullptr, nm ? q2[0].data() : nullptr, nm ? o1[0].data() : nullptr,
                                 nm ? o2[0].data() : nullptr, i1.data(), i2.data(), r1.data(), r2.data()), "ms_loop_sim3_lists");
    // 11. OptimizeSim3Transform of all of them, one call
    std::vector<Sim3Matches> problems(left.size());
    std::vector<const Sim3Matches *> problemPtr;
    std::vector<Sim3> transforms;
    for (std::size_t k = 0; k < left.size(); ++k) {
        const std::size_t a = (std::size_t)start[k], b = (std::size_t)start[k + 1];
        Sim3Matches &m = problems[k];
        m.pts1.assign(q1.begin() + a, q1.begin() + b); m.pts2.assign(q2.begin() + a, q2.begin() + b);
        m.obs1.assign(o1.begin() + a, o1.begin() + b); m.obs2.assign(o2.begin() + a, o2.begin() + b);
        m.info1.assign(i1.begin() + a, i1.begin() + b); m.info2.assign(i2.begin() + a, i2.begin() + b);
        problemPtr.push_back(&m);
        const LoopRansac &r = *ransac[(std::size_t)left[k]];
        transforms.emplace_back(r.bestR12, r.bestT12, (double)r.bestScale12);                                // :273-276
    }
    OptimizeSim3TransformAll(ctx, problemPtr, transforms, settings);
    // 12. the accept gates, in double on the host
    for (std::size_t k = 0; k < left.size(); ++k) {
        const int c = left[k];
        LoopCandidateOutcome &o = out.candidates[heavy[(std::size_t)c]];
        const bool isAdjacent = std::find(adjacent.begin(), adjacent.end(), o.slot) != adjacent.end();
        o.code = detail::acceptGates(transforms[k], curPose, candPose[(std::size_t)c], isAdjacent, chain.t[(std::size_t)current] - chain.t[(std::size_t)o.slot],
                                     detail::distanceTraveled(chain, current, o.slot), P);
        if (o.code != LoopCode::OK) continue;
        o.stage = LoopStage::ACCEPTED;
        LoopClosure lc;
        lc.candidateSlot = o.slot; lc.candToCurr = transforms[k]; lc.keyPointMatches = lists[(std::size_t)c];
        for (std::size_t e = (std::size_t)start[k]; e < (std::size_t)start[k + 1]; ++e) lc.mapPointMatches.emplace_back(r1[e], r2[e]);
        out.closures.push_back(std::move(lc));
    }
    std::sort(out.closures.begin(), out.closures.end(),
              [&](const LoopClosure &a, const LoopClosure &b) { return chain.id[(std::size_t)a.candidateSlot] > chain.id[(std::size_t)b.candidateSlot]; });
    return out;
}

}  // namespace mi355slam
