// loop_chain_smoke.cpp -- the host mirror tryLoopClosureOnTables (host/mi355slam/loop_closer.hpp) against a walk of tryLoopClosure
// (loop_closer.cpp:132-357) over std::map<MpId, MapPoint> with std::map observations, candidate by candidate, built from the host-list
// mirrors (matchForLoopClosures, LoopRansac from octaves, matchMapPointsSim3 on table rows, OptimizeSim3Transform from octaves).
//   loop_chain_smoke --no-gpu   the mirror compiles and links; the host-only validation turns bad calls away and passes the empty ones
//   loop_chain_smoke --gpu      15 candidates of one keyframe: an accepted one, one rejected at each of TOO_CLOSE_TIME, UNNECESSARY_EARLY,
//                               TOO_FEW_FEATURE_MATCHES, RANSAC_FAILED and UNNECESSARY, and more survivors of the cheap tests than the
//                               heavyComputations stop lets through; codes, stages, transforms and match lists compared for equal bits
//   loop_chain_smoke --time [points per keyframe] [map-point rows]   the mirror's and the walk's median time in milliseconds, on that scene or a larger one of the same build
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>
#include "mi355slam/loop_closer.hpp"

using namespace mi355slam;

namespace {

const ms_pinhole kCam{500.0, 500.0, 320.0, 240.0, 640, 480};
constexpr int kExtra = 20, kKf = 18, kCur = 17, kLevels = 4;
int kPts = 300, kKp = kPts + kExtra, kMp = kKf * kPts;        // --time may ask for a larger scene
const double kDrift[3] = {3.0, 0.5, -1.0};                   // how far the current end of the map has drifted from the old one
enum Kind { CONSISTENT, OLD, FEW, SCATTERED };               // drifted with the current keyframe | the old end of the loop | other descriptors | rows anywhere

struct MapPoint { std::array<double, 3> position; std::uint8_t status; std::map<int, int> observations; };   // KfId -> keypoint
struct Keyframe { int id; double t; detail::Pose poseCW; KeyPointVector keyPoints; std::vector<int> mapPoints; std::map<unsigned, std::vector<unsigned>> bow; };

struct Scene {
    std::map<int, MapPoint> mapPoints;
    std::vector<Keyframe> keyframes;                         // by slot; KfId = 100 + 3 * slot
    std::vector<float> maxDistance;
    std::vector<KeyPoint::Descriptor> mpDescriptor;
    std::vector<std::int32_t> candidates, adjacent;
    KeyframeSlots chain;
};

Kind kindOf(int slot) {
    if (slot == kCur || slot == 12 || slot >= 13) return CONSISTENT;
    if (slot == 3) return OLD;
    if (slot == 7) return SCATTERED;
    return slot == 10 || slot == 11 ? OLD : FEW;
}

Scene makeScene() {
    std::mt19937 rng(7);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    auto word = [&] { return (std::uint32_t)rng(); };
    Scene S;
    std::vector<std::array<double, 3>> X(kPts);
    std::vector<KeyPoint::Descriptor> base(kPts);
    std::vector<int> octave(kPts);
    for (int k = 0; k < kPts; ++k) {
        X[k] = {4 * U(rng) - 2, 3 * U(rng) - 1.5, 4 + 4 * U(rng)};
        for (auto &w : base[k]) w = word();
        octave[k] = (int)(rng() % kLevels);
    }
    S.maxDistance.assign(kMp, 1.f);
    S.mpDescriptor.assign(kMp, KeyPoint::Descriptor{});
    S.keyframes.resize(kKf);
    for (int s = 0; s < kKf; ++s) {
        Keyframe &kf = S.keyframes[s];
        const Kind kind = kindOf(s);
        kf.id = 100 + 3 * s; kf.t = 2.0 * s;
        const double scale = s == kCur ? 0.0 : (s == 14 ? 0.3 : 1.0);
        const double ax = 0.04 * (2 * U(rng) - 1) * scale, ay = 0.04 * (2 * U(rng) - 1) * scale;
        const double Rx[9] = {1, 0, 0, 0, std::cos(ax), -std::sin(ax), 0, std::sin(ax), std::cos(ax)}, Ry[9] = {std::cos(ay), 0, std::sin(ay), 0, 1, 0, -std::sin(ay), 0, std::cos(ay)};
        double R[9], t[3];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) { R[3 * i + j] = 0; for (int k = 0; k < 3; ++k) R[3 * i + j] += Rx[3 * i + k] * Ry[3 * k + j]; }
            t[i] = 0.25 * (2 * U(rng) - 1) * scale;
        }
        const bool drifted = kind == CONSISTENT;             // the same camera in a world moved by kDrift: t' = t - R d
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) kf.poseCW[4 * i + j] = R[3 * i + j];
            kf.poseCW[4 * i + 3] = t[i] - (drifted ? (R[3 * i] * kDrift[0] + R[3 * i + 1] * kDrift[1]) + R[3 * i + 2] * kDrift[2] : 0.0);
        }
        std::vector<int> rows(kPts);
        for (int k = 0; k < kPts; ++k) rows[k] = s * kPts + k;
        std::shuffle(rows.begin(), rows.end(), rng);
        kf.keyPoints.resize(kKp); kf.mapPoints.assign(kKp, -1);
        for (int k = 0; k < kKp; ++k) {
            KeyPoint &kp = kf.keyPoints[k];
            kp.angle = (float)(k < kPts ? 359.0 * k / kPts : 360 * U(rng)); kp.bearing = {0, 0, 1};
            if (k >= kPts) {
                kp.pt = {(float)(640 * U(rng)), (float)(480 * U(rng))}; kp.octave = (int)(rng() % kLevels);
                for (auto &w : kp.descriptor) w = word();
                kf.bow[(unsigned)(k % 24)].push_back((unsigned)k);
                continue;
            }
            const double pc[3] = {(R[0] * X[k][0] + R[1] * X[k][1]) + R[2] * X[k][2] + t[0], (R[3] * X[k][0] + R[4] * X[k][1]) + R[5] * X[k][2] + t[1],
                                  (R[6] * X[k][0] + R[7] * X[k][1]) + R[8] * X[k][2] + t[2]};
            kp.pt = {(float)(500.0 * pc[0] / pc[2] + 320.0), (float)(500.0 * pc[1] / pc[2] + 240.0)};
            kp.octave = octave[k];
            kp.descriptor = base[k];
            if (kind == FEW) for (auto &w : kp.descriptor) w = word();
            else for (int b = 0; b < 6; ++b) kp.descriptor[rng() % 8] ^= 1u << (rng() % 32);
            unsigned node = (unsigned)(k % 24);
            if (s != kCur && k % 10 == 3) node = (node + 7) % 24;           // left to matchMapPointsSim3
            kf.bow[node].push_back((unsigned)k);
            MapPoint mp;
            mp.position = drifted ? std::array<double, 3>{X[k][0] + kDrift[0], X[k][1] + kDrift[1], X[k][2] + kDrift[2]} : X[k];
            if (kind == SCATTERED) mp.position = {4 * U(rng) - 2, 3 * U(rng) - 1.5, 4 + 4 * U(rng)};
            mp.status = U(rng) < 0.1 ? 2 : 3;
            mp.observations[kf.id] = k;
            kf.mapPoints[k] = rows[k];
            S.maxDistance[rows[k]] = (float)(std::sqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]) * std::pow(1.2, octave[k] - 0.5));
            S.mpDescriptor[rows[k]] = base[k];
            S.mapPoints[rows[k]] = std::move(mp);
        }
        for (auto &kv : kf.bow) std::sort(kv.second.begin(), kv.second.end());
    }
    S.candidates = {16, 14, 3, 12, 5, 7, 0, 1, 2, 4, 6, 8, 9, 10, 11};
    S.adjacent = {16, 15, 14, 13};
    KeyframeSlots &c = S.chain;
    for (int s = 0; s < kKf; ++s) {
        c.previous.push_back(s - 1); c.next.push_back(s + 1 < kKf ? s + 1 : -1);
        c.cameraCenter.push_back(detail::cameraCenterOf(S.keyframes[s].poseCW));
        c.id.push_back(S.keyframes[s].id); c.t.push_back(S.keyframes[s].t);
        c.camera.push_back(kCam);
    }
    return S;
}

KeyframeFeatures featuresOf(const Keyframe &kf, const std::vector<std::uint8_t> &usable) {
    KeyframeFeatures f;
    f.keyPoints = &kf.keyPoints; f.usable = usable; f.bowFeatureVec = kf.bow;
    return f;
}

// the device side of the scene
struct Device {
    DeviceKeyframeMapPoints keyframes;
    DeviceMapPointFlags flags;
    DeviceMapPointLive live;
    DeviceMapPoints points;
    DeviceKeyframePoses poses;
    DeviceKeypointTable keypoints;
    static DeviceMapPoints makePoints(Context &ctx, const Scene &S) {
        std::vector<DeviceMapPoints::Vec3d> pos(kMp, DeviceMapPoints::Vec3d{0, 0, 0});
        for (const auto &kv : S.mapPoints) pos[(std::size_t)kv.first] = kv.second.position;
        return DeviceMapPoints(ctx, pos, std::vector<DeviceMapPoints::Vec3f>(kMp, DeviceMapPoints::Vec3f{0, 0, 0}), std::vector<float>(kMp, 0.1f), S.maxDistance, S.mpDescriptor);
    }
    static std::vector<std::uint8_t> flagsOf(const Scene &S) {
        std::vector<std::uint8_t> f(kMp, 0);
        for (const auto &kv : S.mapPoints) f[(std::size_t)kv.first] = kv.second.status;
        return f;
    }
    static std::vector<DeviceKeyframePoses::Pose> posesOf(const Scene &S) {
        std::vector<DeviceKeyframePoses::Pose> p;
        for (const Keyframe &kf : S.keyframes) p.push_back(kf.poseCW);
        return p;
    }
    Device(Context &ctx, const Scene &S)
        : keyframes(ctx, kKf, kKp + 12, kMp), flags(ctx, flagsOf(S)), live(ctx, std::vector<std::uint8_t>(kMp, 1)), points(makePoints(ctx, S)), poses(ctx, posesOf(S)),
          keypoints(ctx, kKf, kKp + 12) {
        for (int s = 0; s < kKf; ++s) {
            const Keyframe &kf = S.keyframes[s];
            keyframes.update((std::size_t)s, std::vector<std::int32_t>(kf.mapPoints.begin(), kf.mapPoints.end()));
            std::vector<float> x, y; std::vector<std::int32_t> o;
            for (const KeyPoint &kp : kf.keyPoints) { x.push_back(kp.pt.x); y.push_back(kp.pt.y); o.push_back(kp.octave); }
            keypoints.update((std::size_t)s, x, y, o, {});
        }
    }
};

std::array<double, 3> camPoint(const detail::Pose &P, const std::array<double, 3> &p) {
    std::array<double, 3> o;
    for (int i = 0; i < 3; ++i) o[i] = ((P[4 * i] * p[0] + P[4 * i + 1] * p[1]) + P[4 * i + 2] * p[2]) + P[4 * i + 3];
    return o;
}

// tryLoopClosure (:132-357) over the std::map, one candidate after the other
LoopClosureResult walk(Context &ctx, const Scene &S, const Device &D, const StaticSettings &settings) {
    const Parameters &P = settings.parameters;
    const Keyframe &cur = S.keyframes[kCur];
    const PinholeCamera cam{kCam.fx, kCam.fy, kCam.cx, kCam.cy, kCam.width, kCam.height};
    LoopClosureResult out;
    int heavyComputations = 0;
    auto usableOf = [&](const Keyframe &kf, bool require, std::vector<std::int32_t> &mps) {                // keyframe_matcher.cpp:79-84, :94-96, :568-571
        std::vector<std::uint8_t> u(kf.mapPoints.size(), 0);
        mps.assign(kf.mapPoints.size(), -1);
        for (std::size_t i = 0; i < u.size(); ++i) {
            if (kf.mapPoints[i] == -1) continue;
            const bool tri = S.mapPoints.at(kf.mapPoints[i]).status == 3;
            u[i] = tri || !require;
            if (tri) mps[i] = kf.mapPoints[i];
        }
        return u;
    };
    std::vector<std::int32_t> mps1;
    const std::vector<std::uint8_t> usable1 = usableOf(cur, P.requireTringulationForLoopClosures, mps1);
    DeviceKeyframe kf1(ctx, featuresOf(cur, usable1));
    for (std::int32_t slot : S.candidates) {
        out.candidates.push_back(LoopCandidateOutcome{slot, LoopCode::UNKNOWN, LoopStage::BOW_MATCH});
        LoopCandidateOutcome &o = out.candidates.back();
        if (heavyComputations > 10) break;
        const Keyframe &cand = S.keyframes[(std::size_t)slot];
        const bool isAdjacent = std::find(S.adjacent.begin(), S.adjacent.end(), slot) != S.adjacent.end();
        o.code = detail::cheapRejection(S.chain, kCur, slot, -1.0, isAdjacent);
        if (o.code != LoopCode::UNKNOWN) continue;
        heavyComputations++;
        o.stage = LoopStage::QUICK_TESTS;
        std::vector<std::int32_t> mps2;
        DeviceKeyframe kf2(ctx, featuresOf(cand, usableOf(cand, true, mps2)));
        std::vector<int> matchedFeatureIds;
        matchForLoopClosures(ctx, kf1, kf2, matchedFeatureIds, P);
        std::vector<std::pair<int, int>> matches;            // :203-213
        for (unsigned i = 0; i < matchedFeatureIds.size(); ++i) {
            const int kfIdx2 = matchedFeatureIds.at(i);
            if (kfIdx2 < 0) continue;
            const int mpId1 = cur.mapPoints.at(i), mpId2 = cand.mapPoints.at((std::size_t)kfIdx2);
            if (mpId1 != -1 && mpId2 != -1 && mpId1 != mpId2) matches.emplace_back(mpId1, mpId2);
        }
        if (matches.size() < P.minLoopClosureFeatureMatches) { o.code = LoopCode::TOO_FEW_FEATURE_MATCHES; continue; }
        std::vector<LoopRansac::Vec3> p1, p2;                // loop_ransac.cpp:17-41
        std::vector<int> o1, o2;
        for (const auto &m : matches) {
            const MapPoint &mp1 = S.mapPoints.at(m.first), &mp2 = S.mapPoints.at(m.second);
            p1.push_back(camPoint(cur.poseCW, mp1.position)); p2.push_back(camPoint(cand.poseCW, mp2.position));
            o1.push_back(cur.keyPoints.at((std::size_t)mp1.observations.at(cur.id)).octave);
            o2.push_back(cand.keyPoints.at((std::size_t)mp2.observations.at(cand.id)).octave);
        }
        LoopRansac loopRansac(p1, p2, o1, o2, cam, cam, settings);
        loopRansac.ransacSolve(ctx, P.loopClosureRansacIterations, LoopRansac::DoF::SIM3);
        if (!loopRansac.solutionOk) { o.code = LoopCode::RANSAC_FAILED; continue; }
        o.stage = LoopStage::MAP_POINT_MATCHES;
        std::vector<std::pair<int, int>> kpMatches;          // :238-243 as keypoint pairs (:258-264)
        for (unsigned i = 0; i < loopRansac.bestInliers.size(); i++)
            if (loopRansac.bestInliers.at(i))
                kpMatches.emplace_back(S.mapPoints.at(matches[i].first).observations.at(cur.id), S.mapPoints.at(matches[i].second).observations.at(cand.id));
        double R1in2[9], t1in2[3], R2in1[9], t2in1[3];
        detail::sim3ViewPoses(loopRansac.bestR12, loopRansac.bestT12, (double)loopRansac.bestScale12, cur.poseCW, cand.poseCW, R1in2, t1in2, R2in1, t2in1);
        matchMapPointsSim3(ctx, kf1, kf2, D.points, mps1, mps2, R1in2, t1in2, R2in1, t2in1, kCam, kCam, kpMatches, settings);
        Sim3Matches sm;                                      // optimize_transform.cpp:101-142
        LoopClosure lc;
        for (const auto &m : kpMatches) {
            const int id1 = cur.mapPoints.at((std::size_t)m.first), id2 = cand.mapPoints.at((std::size_t)m.second);
            const MapPoint &mp1 = S.mapPoints.at(id1), &mp2 = S.mapPoints.at(id2);
            const KeyPoint &k1 = cur.keyPoints.at((std::size_t)mp1.observations.at(cur.id)), &k2 = cand.keyPoints.at((std::size_t)mp2.observations.at(cand.id));
            sm.pts1.push_back(camPoint(cur.poseCW, mp1.position)); sm.pts2.push_back(camPoint(cand.poseCW, mp2.position));
            sm.obs1.push_back({((double)k1.pt.x - kCam.cx) / kCam.fx, ((double)k1.pt.y - kCam.cy) / kCam.fy});
            sm.obs2.push_back({((double)k2.pt.x - kCam.cx) / kCam.fx, ((double)k2.pt.y - kCam.cy) / kCam.fy});
            sm.octaves1.push_back(k1.octave); sm.octaves2.push_back(k2.octave);
            lc.mapPointMatches.emplace_back(id1, id2);
        }
        Sim3 candToCurr(loopRansac.bestR12, loopRansac.bestT12, (double)loopRansac.bestScale12);
        OptimizeSim3Transform(ctx, sm, candToCurr, settings);
        o.code = detail::acceptGates(candToCurr, cur.poseCW, cand.poseCW, isAdjacent, cur.t - cand.t, detail::distanceTraveled(S.chain, kCur, slot), P);
        if (o.code != LoopCode::OK) continue;
        o.stage = LoopStage::ACCEPTED;
        lc.candidateSlot = slot; lc.candToCurr = candToCurr; lc.keyPointMatches = kpMatches;
        out.closures.push_back(std::move(lc));
    }
    std::sort(out.closures.begin(), out.closures.end(),
              [&](const LoopClosure &a, const LoopClosure &b) { return S.keyframes[(std::size_t)a.candidateSlot].id > S.keyframes[(std::size_t)b.candidateSlot].id; });
    return out;
}

StaticSettings makeSettings() {
    Parameters p;
    p.orbScaleLevels = kLevels;
    p.requireTringulationForLoopClosures = false;
    p.loopClosureRansacIterations = 80; p.loopClosureRansacMinInliers = 15; p.minLoopClosureFeatureMatches = 20;
    p.maximumDriftMetersPerSecond = p.maximumDriftMetersPerTraveled = p.maximumDriftRadiansPerSecond = p.maximumDriftRadiansPerTraveled = 1e9;
    return StaticSettings(p);
}

struct Mirror {
    std::vector<std::unique_ptr<DeviceKeyframe>> owned;
    std::vector<DeviceKeyframe *> frames;
    KeyframeSlots slots;                                     // the scene's chain and cameras with the frames
    Mirror(Context &ctx, const Scene &S) : slots(S.chain) {
        for (const Keyframe &kf : S.keyframes) {             // the masks start empty: ms_loop_usable_mask writes them
            owned.emplace_back(new DeviceKeyframe(ctx, featuresOf(kf, std::vector<std::uint8_t>(kf.keyPoints.size(), 0))));
            frames.push_back(owned.back().get());
        }
        slots.frames = frames;
    }
};

LoopClosureResult mirror(Context &ctx, const Scene &S, Device &D, Mirror &M, const StaticSettings &settings) {
    MapTables T{D.keyframes, M.slots};
    T.flags = &D.flags; T.live = &D.live; T.points = &D.points; T.poses = &D.poses; T.keypoints = &D.keypoints;
    return tryLoopClosureOnTables(ctx, T, kCur, S.candidates, S.adjacent, -1.0, settings);
}

int no_gpu() {
    std::printf("link ok %d\n", (int)(sizeof(LoopClosureResult) > 0 && sizeof(MapTables) > 0 && sizeof(LoopClosure) > 0));
    char why[256];
    std::int32_t kf[16], slots[2] = {1, 0}, nKp[2] = {4, 3}, req[2] = {0, 1}, row[8], cand[2] = {0, 2}, start[3] = {0, 1, 2}, a[2] = {0, 1}, out[8];
    std::fill(kf, kf + 16, -1);
    std::uint8_t flags[4] = {1, 3, 0, 2}, m[8];
    std::uint8_t *usable[2] = {m, m + 4};
    std::int32_t *tri[2] = {row, nullptr};
    const std::int32_t *matched[2] = {row, row + 4};
    double d[64] = {0};
    float f[16] = {1.f, 1.44f, 2.f}, x[16] = {0};
    const ms_pinhole cams[4] = {kCam, kCam, kCam, kCam};
    int cases = 0;
    auto expect = [&](int rc, int code, const char *text) {
        ++cases;
        if (rc != code || (text && !std::strstr(why, text))) { std::printf("case %d: rc %d, %s\n", cases, rc, why); return false; }
        return true;
    };
    auto mask = [&](int nKf, int n) { return ms_loop_usable_mask_check(kf, nKf, 4, flags, nullptr, 4, slots, nKp, req, usable, tri, n, why, sizeof(why)); };
    auto pairs = [&](int cur, int nCand, int levels) {
        return ms_loop_pairs_check(kf, 4, 4, nullptr, d, 4, d, out, cur, 4, cand, nKp, matched, nCand, f, levels, 8, out, out, out, out, out, d, d, x, x, d, d, out, why, sizeof(why));
    };
    auto lists = [&](int cur, const std::int32_t *ms) {
        return ms_loop_sim3_lists_check(kf, 4, 4, nullptr, d, 4, d, x, x, out, cur, 4, cand, nKp, 2, cams, f, 3, a, a, ms, d, d, d, d, x, x, out, out, why, sizeof(why));
    };
    const std::int32_t descending[3] = {0, 2, 1};
    if (!expect(mask(2, 2), MS_OK, nullptr) || !expect(mask(2, 0), MS_OK, nullptr) || !expect(mask(1, 2), MS_ERR_INVALID, "loop mask: slot 1 outside [0, 1)")) return 1;
    if (!expect(pairs(1, 2, 3), MS_OK, nullptr) || !expect(pairs(1, 0, 3), MS_OK, nullptr) || !expect(pairs(2, 2, 3), MS_ERR_INVALID, "loop pairs: the current keyframe's slot 2")) return 1;
    if (!expect(pairs(1, 2, 0), MS_ERR_INVALID, "0 levels outside") || !expect(pairs(4, 2, 3), MS_ERR_INVALID, "slot 4 outside [0, 4)")) return 1;
    if (!expect(lists(1, start), MS_OK, nullptr) || !expect(lists(0, start), MS_ERR_INVALID, "loop sim3 lists: the current keyframe's slot 0")) return 1;
    if (!expect(lists(1, descending), MS_ERR_INVALID, "match_start descends at candidate 1")) return 1;
    std::printf("no-gpu ok %d cases\n", cases);
    return 0;
}

bool same(const LoopClosureResult &a, const LoopClosureResult &b) {
    if (a.candidates.size() != b.candidates.size() || a.closures.size() != b.closures.size()) return false;
    for (std::size_t i = 0; i < a.candidates.size(); ++i)
        if (a.candidates[i].slot != b.candidates[i].slot || a.candidates[i].code != b.candidates[i].code || a.candidates[i].stage != b.candidates[i].stage) {
            std::printf("candidate %zu (slot %d): code %d / %d, stage %d / %d\n", i, a.candidates[i].slot, (int)a.candidates[i].code, (int)b.candidates[i].code,
                        (int)a.candidates[i].stage, (int)b.candidates[i].stage);
            return false;
        }
    for (std::size_t i = 0; i < a.closures.size(); ++i) {
        const LoopClosure &x = a.closures[i], &y = b.closures[i];
        if (x.candidateSlot != y.candidateSlot || x.keyPointMatches != y.keyPointMatches || x.mapPointMatches != y.mapPointMatches) { std::printf("closure %zu: lists differ\n", i); return false; }
        if (std::memcmp(x.candToCurr.q.data(), y.candToCurr.q.data(), 32) || std::memcmp(x.candToCurr.t.data(), y.candToCurr.t.data(), 24) || x.candToCurr.s != y.candToCurr.s) {
            std::printf("closure %zu: transforms differ\n", i);
            return false;
        }
    }
    return true;
}

int gpu(bool timing) {
    Context ctx(0);
    const Scene S = makeScene();
    const StaticSettings settings = makeSettings();
    Device D(ctx, S);
    Mirror M(ctx, S);
    loopRansacEngine().seed(94235682);
    const LoopClosureResult want = walk(ctx, S, D, settings);
    loopRansacEngine().seed(94235682);
    const LoopClosureResult got = mirror(ctx, S, D, M, settings);
    if (!same(got, want)) return 1;
    int count[9] = {0};
    for (const LoopCandidateOutcome &o : want.candidates) count[(int)o.code]++;
    std::printf("codes: OK %d, TOO_CLOSE_TIME %d, UNNECESSARY_EARLY %d, TOO_FEW_FEATURE_MATCHES %d, RANSAC_FAILED %d, UNNECESSARY %d, not reached %d of %zu listed\n",
                count[0], count[1], count[2], count[3], count[4], count[5], count[8], S.candidates.size());
    const bool stopped = want.candidates.size() < S.candidates.size() && want.candidates.back().code == LoopCode::UNKNOWN;
    if (!(count[0] == 1 && count[1] >= 1 && count[2] >= 1 && count[3] >= 1 && count[4] >= 1 && count[5] >= 1 && stopped && want.closures.size() == 1)) {
        std::printf("the scene does not hold every outcome\n");
        return 1;
    }
    const LoopClosure &lc = want.closures[0];
    std::size_t added = 0;
    for (const auto &m : lc.keyPointMatches) added += m.first % 10 == 3;
    std::printf("accepted slot %d with %zu matches, %zu of them from matchMapPointsSim3's nodes, scale %.6f\n", lc.candidateSlot, lc.keyPointMatches.size(), added, lc.candToCurr.s);
    if (lc.candidateSlot != 3 || lc.keyPointMatches.size() < 100 || added == 0) return 1;
    std::printf("tryLoopClosureOnTables ok\n");
    if (timing) {
        std::vector<double> ms;
        for (int rep = 0; rep < 23; ++rep) {
            loopRansacEngine().seed(94235682);
            const auto t0 = std::chrono::steady_clock::now();
            const LoopClosureResult r = mirror(ctx, S, D, M, settings);
            const auto t1 = std::chrono::steady_clock::now();
            if (rep >= 3) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            if (!same(r, want)) return 1;
        }
        std::vector<double> ws;
        for (int rep = 0; rep < 9; ++rep) {
            loopRansacEngine().seed(94235682);
            const auto t0 = std::chrono::steady_clock::now();
            const LoopClosureResult r = walk(ctx, S, D, settings);
            const auto t1 = std::chrono::steady_clock::now();
            if (rep >= 2) ws.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            if (!same(r, want)) return 1;
        }
        std::sort(ms.begin(), ms.end()); std::sort(ws.begin(), ws.end());
        std::printf("{\"mirror_ms\": %.4f, \"walk_ms\": %.4f, \"candidates\": %zu, \"heavy\": 11, \"keypoints\": %d, \"rows\": %d}\n", ms[ms.size() / 2], ws[ws.size() / 2],
                    S.candidates.size(), kKp, kMp);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu(false);
    if (argc > 1 && std::strcmp(argv[1], "--time") == 0) {
        if (argc > 2) { kPts = std::max(100, std::atoi(argv[2])); kKp = kPts + kExtra; kMp = kKf * kPts; }
        if (argc > 3) kMp = std::max(kMp, std::atoi(argv[3]));
        return gpu(true);
    }
    std::printf("usage: loop_chain_smoke --no-gpu | --gpu | --time\n");
    return 64;
}
