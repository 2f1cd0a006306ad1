// Compile + link check of the table-based overloads of the host mirror (mi355slam/keyframe_matcher.hpp) against libmi355slam.so
// (tests/test_project_gate_abi.py), and their comparison with sequential C++ restatements of the reference's loops.
//   project_gate_smoke --no-gpu   prints the layout of ms_gate_view, checks the restatement below on hand-computed points and the argument
//                                 checks that need no device.  Creates no context.
//   project_gate_smoke --gpu      isInFrustum, searchByProjection, replaceDuplicationCandidates and matchMapPointsSim3 on one small scene each
//                                 against the loops restated here (tests/test_gpu_project_gate.py)
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "mi355slam/keyframe_matcher.hpp"

using namespace mi355slam;

namespace {

const ms_pinhole kCam{450.0, 450.0, 320.0, 240.0, 640, 480};

struct HostTable {
    std::vector<DeviceMapPoints::Vec3d> pos;
    std::vector<DeviceMapPoints::Vec3f> norm;
    std::vector<float> dmin, dmax;
    std::vector<KeyPoint::Descriptor> desc;
};

struct Gate { int status = 1; float x = 0, y = 0, dist = 0, radius = 0; int level = -1; };

// kept entries whose quotient log(ratio) / log(scaleFactor) lies within 1e-5 of an integer: there two conforming logf may give neighbouring levels
// (DESIGN 9.4), so a scene that has one cannot be held to equal match lists; the scenes below have none
int g_nearLevel = 0;

// the three loops' gates for one map point, one statement per rounded operation (keyframe_matcher.cpp:313-345, :442-471, :573-596)
Gate gate(const HostTable &T, int m, const GateView &V, const StaticSettings &st) {
    Gate g;
    const double *R = V.R, *t = V.t, *p = T.pos[(std::size_t)m].data();
    double pc[3];
    for (int i = 0; i < 3; ++i) pc[i] = ((R[3 * i] * p[0] + R[3 * i + 1] * p[1]) + R[3 * i + 2] * p[2]) + t[i];
    const double u = V.camera.fx * (pc[0] / pc[2]) + V.camera.cx, v = V.camera.fy * (pc[1] / pc[2]) + V.camera.cy;
    if (!(pc[2] > 0.0 && u >= 0.0 && u < (double)V.camera.width && v >= 0.0 && v < (double)V.camera.height)) return g;
    g.x = (float)u; g.y = (float)v;
    const float dmin = T.dmin[(std::size_t)m], dmax = T.dmax[(std::size_t)m];
    float cosv = 1.f;
    g.status = 2;
    if (V.mode == MS_GATE_SIM3) {
        const double dd = std::sqrt((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]);
        g.dist = (float)dd;
        if (dd < dmin || dmax < dd) return g;
    } else {
        float d[3];
        for (int j = 0; j < 3; ++j) d[j] = (float)(-((R[j] * t[0] + R[3 + j] * t[1]) + R[6 + j] * t[2]) - p[j]);
        g.dist = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        if (g.dist < dmin || dmax < g.dist) return g;
        const float *n = T.norm[(std::size_t)m].data();
        if (V.mode == MS_GATE_FUSE && n[0] == 0.f && n[1] == 0.f && n[2] == 0.f) { g.status = 3; return g; }
        cosv = ((d[0] / g.dist) * n[0] + (d[1] / g.dist) * n[1]) + (d[2] / g.dist) * n[2];
        if (cosv < (V.mode == MS_GATE_SEARCH ? V.cosLimit : 0.5f)) { g.status = 4; return g; }
    }
    g.status = 0;
    const float ratio = dmax / g.dist, cq = std::ceil(std::log(ratio) / std::log(st.parameters.orbScaleFactor));
    const int top = (int)st.scaleFactors.size() - 1;
    g.level = !(cq > 0.f) ? 0 : (cq >= (float)top ? top : (int)cq);
    const double q = std::log((double)ratio) / std::log((double)st.parameters.orbScaleFactor);
    if (std::fabs(q - std::round(q)) <= 1e-5 * std::max(1.0, std::fabs(q))) ++g_nearLevel;
    const float sl = st.scaleFactors[(std::size_t)g.level], sref = st.scaleFactors[st.scaleFactors.size() / 2];
    if (V.mode == MS_GATE_SEARCH) g.radius = (((cosv > 0.998f ? 0.625f : 1.f) * V.threshold) * sl) / sref;
    else if (V.mode == MS_GATE_FUSE) g.radius = ((V.threshold * sl) / sref) * 2.4477f;
    else g.radius = V.threshold * sl;
    return g;
}

// the scan behind a gate, restated from the reference: FeatureSearch (feature_search.cpp:22-48: keypoints ordered by y, ties by index; the circle test
// in float) and the best / second update of keyframe_matcher.cpp:356-378 over the keypoints that are free and inside the octave window
struct Scan { int best = -1, bestDist = 256, bestDist2 = 256, bestLevel = -1, bestLevel2 = -1; };
Scan scan(const KeyPointVector &kps, const HostTable &T, int m, const Gate &g, const std::vector<std::uint8_t> &bound, int lo, int hi) {
    std::vector<int> order(kps.size());
    for (std::size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return kps[(std::size_t)a].pt.y < kps[(std::size_t)b].pt.y; });
    Scan s;
    const float ylo = g.y - g.radius, yhi = g.y + g.radius, r2 = g.radius * g.radius;
    for (int j : order) {
        const KeyPoint &k = kps[(std::size_t)j];
        if (k.pt.y < ylo || k.pt.y > yhi) continue;
        const float dx = g.x - k.pt.x, dy = g.y - k.pt.y, dx2 = dx * dx, dy2 = dy * dy;
        if (!(dx2 + dy2 < r2)) continue;
        if (bound[(std::size_t)j] || k.octave < lo || k.octave > hi) continue;
        int d = 0;
        for (int w = 0; w < 8; ++w) d += __builtin_popcount(T.desc[(std::size_t)m][w] ^ k.descriptor[w]);
        if (d < s.bestDist) { s.bestDist2 = s.bestDist; s.bestDist = d; s.bestLevel2 = s.bestLevel; s.bestLevel = k.octave; s.best = j; }
        else if (d < s.bestDist2) { s.bestLevel2 = k.octave; s.bestDist2 = d; }
    }
    return s;
}

bool near_level_free(const char *what) {
    if (g_nearLevel) std::printf("%s: %d kept entries of the scene lie near a level boundary; draw another seed\n", what, g_nearLevel);
    return g_nearLevel == 0;
}

void make_table(std::mt19937 &rng, int nMp, HostTable &T) {
    std::uniform_real_distribution<double> U(0.0, 1.0);
    T = HostTable();
    for (int i = 0; i < nMp; ++i) {
        const double z = (1.5 + 8.0 * U(rng)) * (U(rng) < 0.05 ? -1.0 : 1.0), x = (1.8 * U(rng) - 0.9) * std::fabs(z), y = (1.3 * U(rng) - 0.65) * std::fabs(z);
        const double d = std::sqrt(x * x + y * y + z * z);
        DeviceMapPoints::Vec3f n{(float)(-x / d + 0.3 * (U(rng) - 0.5)), (float)(-y / d + 0.3 * (U(rng) - 0.5)), (float)(-z / d)};
        if (U(rng) < 0.05) n = {0.f, 0.f, 0.f};
        T.pos.push_back({x, y, z}); T.norm.push_back(n);
        const float dmax = (float)(d * (0.9 + 3.0 * U(rng)));
        T.dmax.push_back(dmax); T.dmin.push_back(dmax / (float)std::pow(1.2, 4.0 + 5.0 * U(rng)));
        KeyPoint::Descriptor ds;
        for (auto &w : ds) w = (std::uint32_t)rng();
        T.desc.push_back(ds);
    }
}

// keypoint i observes map point i % nMp: near its projection, with a descriptor a few bits off; more keypoints than points, so queries compete
void make_keypoints(std::mt19937 &rng, const HostTable &T, int nKp, KeyPointVector &kps) {
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const int nMp = (int)T.pos.size();
    kps.clear();
    for (int i = 0; i < nKp; ++i) {
        const int m = i % nMp;
        const double *p = T.pos[(std::size_t)m].data();
        KeyPoint k{};
        const double z = std::fabs(p[2]) + 1e-3;
        k.pt.x = (float)(kCam.fx * p[0] / z + kCam.cx + 6.0 * (U(rng) - 0.5)); k.pt.y = (float)(kCam.fy * p[1] / z + kCam.cy + 6.0 * (U(rng) - 0.5));
        k.angle = 0.f; k.octave = (int)(rng() % 8); k.bearing = {0, 0, 1};
        k.descriptor = T.desc[(std::size_t)m];
        for (int b = 0; b < 12; ++b) k.descriptor[rng() % 8] ^= 1u << (rng() % 32);
        kps.push_back(k);
    }
}

GateView view_of(std::mt19937 &rng, int mode, float threshold, int nMp, double scale) {
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    GateView V;
    const double a = 0.05 * U(rng), c = std::cos(a), s = std::sin(a);
    const double R[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
    for (int i = 0; i < 9; ++i) V.R[i] = scale * R[i];
    for (int i = 0; i < 3; ++i) V.t[i] = 0.03 * U(rng);
    V.camera = kCam; V.threshold = threshold; V.mode = mode;
    for (int i = 0; i < nMp; ++i) V.indices.push_back((std::int32_t)((i * 7) % nMp));
    return V;
}

int no_gpu() {
    std::printf("ms_gate_view size %zu R_cw %zu t_cw %zu cam %zu threshold %zu view_cos_limit %zu mode %zu first %zu count %zu\n", sizeof(ms_gate_view),
                offsetof(ms_gate_view, R_cw), offsetof(ms_gate_view, t_cw), offsetof(ms_gate_view, cam), offsetof(ms_gate_view, threshold),
                offsetof(ms_gate_view, view_cos_limit), offsetof(ms_gate_view, mode), offsetof(ms_gate_view, first), offsetof(ms_gate_view, count));
    std::int32_t kept = 7;
    if (ms_project_gate(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 8, 1.2f, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &kept) != MS_ERR_INVALID || kept != 7) {
        std::printf("a call without a context must fail with MS_ERR_INVALID and write nothing\n");
        return 1;
    }
    // identity pose, a point on the optical axis at depth 4 with the normal towards the camera: pixel (320, 240), dist 4, cos 1;
    // max_dist = 4 * 1.2^2.5 -> level ceil(2.5) = 3, radius 0.625 * 10 * sf[3] / sf[4] (SEARCH), 3 * sf[3] / sf[4] * 2.4477 (FUSE), 7.5 * sf[3] (SIM3)
    Parameters prm;
    StaticSettings st(prm);
    HostTable T;
    T.pos.push_back({0, 0, 4}); T.norm.push_back({0, 0, -1}); T.dmin.push_back(1.f); T.dmax.push_back(4.f * std::pow(1.2f, 2.5f)); T.desc.push_back({});
    const float sf3 = st.scaleFactors[3], sf4 = st.scaleFactors[4];
    const float want[3] = {0.625f * 10.f * sf3 / sf4, 3.f * sf3 / sf4 * 2.4477f, 7.5f * sf3};
    const float thr[3] = {10.f, 3.f, 7.5f};
    for (int mode = 0; mode < 3; ++mode) {
        GateView V; V.camera = kCam; V.mode = mode; V.threshold = thr[mode]; V.indices = {0};
        const Gate g = gate(T, 0, V, st);
        if (g.status != 0 || g.x != 320.f || g.y != 240.f || g.dist != 4.f || g.level != 3 || g.radius != want[mode]) {
            std::printf("mode %d: status %d (%g, %g) dist %g level %d radius %g, expected radius %g\n", mode, g.status, g.x, g.y, g.dist, g.level, g.radius, want[mode]);
            return 1;
        }
        std::vector<ms_gate_view> P; std::vector<std::int32_t> idx;
        detail::pack_views({V, V}, P, idx);
        if (P.size() != 2 || P[1].first != 1 || P[1].count != 1 || P[1].mode != mode || idx.size() != 2) { std::printf("pack_views\n"); return 1; }
    }
    std::printf("no-gpu ok 3 modes\n");
    return 0;
}

int gpu() {
    Context ctx(0);
    Parameters prm;
    StaticSettings st(prm);
    std::mt19937 rng(11);
    HostTable T;
    KeyPointVector kps1, kps2;
    make_table(rng, 300, T);
    make_keypoints(rng, T, 500, kps1);
    make_keypoints(rng, T, 500, kps2);                       // a second keyframe over the same points
    KeyframeFeatures f1, f2;
    f1.keyPoints = &kps1; f1.usable.assign(kps1.size(), 1);
    f2.keyPoints = &kps2; f2.usable.assign(kps2.size(), 1);
    DeviceKeyframe d1(ctx, f1), d2(ctx, f2);
    DeviceMapPoints table(ctx, T.pos, T.norm, T.dmin, T.dmax, T.desc);
    const std::vector<std::uint8_t> none1(kps1.size(), 0), none2(kps2.size(), 0);

    // isInFrustum
    GateView S = view_of(rng, MS_GATE_SEARCH, 15.f, 300, 1.0);
    {
        const std::vector<bool> in = isInFrustum(ctx, table, S.indices, S.R, S.t, S.camera, 0.5f, st);
        int n = 0;
        for (std::size_t i = 0; i < S.indices.size(); ++i) {
            if (in[i] != (gate(T, S.indices[i], S, st).status == 0)) { std::printf("isInFrustum differs at %zu\n", i); return 2; }
            n += in[i];
        }
        if (n < 50 || n > 290) { std::printf("isInFrustum: %d of 300 inside\n", n); return 2; }
        std::printf("isInFrustum ok %d\n", n);
    }
    // searchByProjection: about 30 % of the keypoints bound beforehand
    {
        std::vector<std::uint8_t> bound(kps1.size(), 0), boundRef;
        for (std::size_t i = 0; i < bound.size(); ++i) bound[i] = rng() % 10 < 3;
        boundRef = bound;
        std::vector<int> want(S.indices.size(), -1);
        int nm = 0;
        for (std::size_t i = 0; i < S.indices.size(); ++i) {
            const Gate g = gate(T, S.indices[i], S, st);
            if (g.status != 0) continue;
            const Scan b = scan(kps1, T, S.indices[i], g, boundRef, -0x7fffffff, 0x7fffffff);
            if (b.best == -1 || b.bestDist > 100 || (b.bestLevel == b.bestLevel2 && b.bestDist > 0.8 * b.bestDist2)) continue;
            want[i] = b.best; boundRef[(std::size_t)b.best] = 1; ++nm;
        }
        if (!near_level_free("searchByProjection")) return 9;
        const std::vector<int> got = searchByProjection(ctx, d1, table, S, bound, st);
        if (got != want || bound != boundRef || nm < 20) { std::printf("searchByProjection mismatch (%d matches)\n", nm); return 3; }
        std::printf("searchByProjection ok %d\n", nm);
    }
    // replaceDuplicationCandidates: three adjacent keyframes (two of them the same device keyframe under different poses)
    {
        std::vector<GateView> views{view_of(rng, MS_GATE_FUSE, 3.f, 300, 1.0), view_of(rng, MS_GATE_FUSE, 3.f, 120, 1.0), view_of(rng, MS_GATE_FUSE, 3.f, 300, 1.0)};
        const std::vector<const DeviceKeyframe *> kfs{&d1, &d2, &d1};
        const std::vector<std::vector<int>> got = replaceDuplicationCandidates(ctx, table, views, kfs, st);
        int nm = 0;
        for (std::size_t v = 0; v < views.size(); ++v)
            for (std::size_t i = 0; i < views[v].indices.size(); ++i) {
                const Gate g = gate(T, views[v].indices[i], views[v], st);
                int want = -1;
                if (g.status == 0) {
                    const Scan b = scan(v == 1 ? kps2 : kps1, T, views[v].indices[i], g, v == 1 ? none2 : none1, -0x7fffffff, 0x7fffffff);
                    if (b.best != -1 && b.bestDist <= 50) want = b.best;
                }
                if (got[v][i] != want) { std::printf("replaceDuplicationCandidates differs at view %zu entry %zu\n", v, i); return 4; }
                nm += want >= 0;
            }
        if (!near_level_free("replaceDuplicationCandidates")) return 9;
        if (nm < 20) { std::printf("replaceDuplicationCandidates: %d candidates\n", nm); return 4; }
        std::printf("replaceDuplicationCandidates ok %d\n", nm);
    }
    // matchMapPointsSim3: keypoint i of either keyframe observes map point i % 300 (every fifth none)
    {
        std::vector<std::int32_t> mps1(kps1.size()), mps2(kps2.size());
        for (std::size_t i = 0; i < mps1.size(); ++i) mps1[i] = i % 5 == 4 ? -1 : (std::int32_t)(i % 300);
        for (std::size_t i = 0; i < mps2.size(); ++i) mps2[i] = i % 5 == 3 ? -1 : (std::int32_t)(i % 300);
        const GateView A = view_of(rng, MS_GATE_SIM3, 7.5f, 1, 1.03), B = view_of(rng, MS_GATE_SIM3, 7.5f, 1, 0.97);
        std::vector<std::pair<int, int>> matches{{0, 0}}, ref{{0, 0}};
        const unsigned added = matchMapPointsSim3(ctx, d1, d2, table, mps1, mps2, A.R, A.t, B.R, B.t, kCam, kCam, matches, st);
        auto one_way = [&](const std::vector<std::int32_t> &mps, std::size_t skip, const GateView &P, const KeyPointVector &kf, const std::vector<std::uint8_t> &none) {
            std::vector<int> out(mps.size(), -1);
            for (std::size_t i = 0; i < mps.size(); ++i) {
                if (i == skip || mps[i] < 0) continue;
                const Gate g = gate(T, mps[i], P, st);
                if (g.status != 0) continue;
                const Scan b = scan(kf, T, mps[i], g, none, g.level - 1, g.level);
                if (b.bestDist <= 100) out[i] = b.best;
            }
            return out;
        };
        const std::vector<int> fwd = one_way(mps1, 0, A, kps2, none2), bwd = one_way(mps2, 0, B, kps1, none1);
        for (std::size_t i = 0; i < fwd.size(); ++i) if (fwd[i] >= 0 && bwd[(std::size_t)fwd[i]] == (int)i) ref.emplace_back((int)i, fwd[i]);
        int nf = 0;
        for (int f : fwd) nf += f >= 0;
        if (!near_level_free("matchMapPointsSim3")) return 9;
        if (matches != ref || added + 1 != ref.size() || nf < 10) { std::printf("matchMapPointsSim3 mismatch (%u added, %zu expected, %d one-way)\n", added, ref.size() - 1, nf); return 5; }
        std::printf("matchMapPointsSim3 ok %u mutual of %d\n", added, nf);
    }
    std::printf("gpu ok 4 functions\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_project_gate, (const void *)&ms_projection_topk};
    std::printf("link ok %d\n", syms[0] != nullptr && syms[1] != nullptr);
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu();
    return 0;
}
