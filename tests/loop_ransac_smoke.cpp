// Compile + link check of the host mirror of LoopRansac (mi355slam/loop_ransac.hpp) against libmi355slam.so (tests/test_loop_ransac_abi.py).
//   loop_ransac_smoke --no-gpu SAMPLES   the mirror's sampler against recorded triplets ("n a b c" per line), from a fresh engine; an
//                                        early-return object must draw nothing.  Creates no context.
//   loop_ransac_smoke --gpu              ransacSolveAll on 11 objects against their per-object ransacSolve (tests/test_gpu_loop_ransac.py)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <random>
#include <vector>
#include "mi355slam/loop_ransac.hpp"

using namespace mi355slam;

namespace {

const PinholeCamera kCam{450.0, 450.0, 320.0, 240.0, 640, 480};

// matches of a scene seen from two keyframes: kf2 = s R(z, angle) kf1 + t, with a share of unrelated points
void scene(std::mt19937 &rng, int n, double outliers, std::vector<LoopRansac::Vec3> &p1, std::vector<LoopRansac::Vec3> &p2,
           std::vector<int> &o1, std::vector<int> &o2) {
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double a = 0.3 * (U(rng) - 0.5), s = 0.9 + 0.2 * U(rng), c = std::cos(a), sn = std::sin(a);
    const double t[3] = {0.2 * (U(rng) - 0.5), 0.2 * (U(rng) - 0.5), 0.2 * (U(rng) - 0.5)};
    p1.clear(); p2.clear(); o1.clear(); o2.clear();
    for (int i = 0; i < n; ++i) {
        const double z = 2.0 + 6.0 * U(rng), u = 10 + 620 * U(rng), v = 10 + 460 * U(rng);
        const LoopRansac::Vec3 q{(u - kCam.cx) / kCam.fx * z, (v - kCam.cy) / kCam.fy * z, z};
        LoopRansac::Vec3 r{s * (c * q[0] - sn * q[1]) + t[0], s * (sn * q[0] + c * q[1]) + t[1], s * q[2] + t[2]};
        if (U(rng) < outliers) r = {r[0] + U(rng) - 0.5, r[1] + U(rng) - 0.5, r[2]};
        p1.push_back(q); p2.push_back(r);
        o1.push_back((int)(8 * U(rng))); o2.push_back((int)(8 * U(rng)));
    }
}

int sampler(const char *path) {
    Parameters prm;
    prm.loopClosureRansacMinInliers = 20;
    StaticSettings st(prm);
    std::vector<LoopRansac::Vec3> p1, p2;
    std::vector<int> o1, o2;
    std::mt19937 rng(5);
    scene(rng, 2, 0.0, p1, p2, o1, o2);
    LoopRansac tooFew(p1, p2, o1, o2, kCam, kCam, st);                      // fewer than 3 matches
    scene(rng, 15, 0.0, p1, p2, o1, o2);
    LoopRansac belowMin(p1, p2, o1, o2, kCam, kCam, st);                    // fewer than loopClosureRansacMinInliers
    if (!tooFew.drawSamples(300).empty() || !belowMin.drawSamples(300).empty()) { std::printf("early return drew samples\n"); return 1; }
    std::ifstream in(path);
    int n, a, b, c, k = 0;
    while (in >> n >> a >> b >> c) {
        const auto t = randomTriplet(n);
        if (t[0] != a || t[1] != b || t[2] != c) {
            std::printf("call %d (n = %d): got %d %d %d, recorded %d %d %d\n", k, n, t[0], t[1], t[2], a, b, c);
            return 1;
        }
        ++k;
    }
    std::printf("sampler ok %d\n", k);
    return 0;
}

int gpu() {
    Context ctx(0);
    Parameters prm;
    prm.loopClosureRansacMinInliers = 10;
    StaticSettings st(prm);
    std::mt19937 rng(7);
    std::vector<LoopRansac> objs;
    std::vector<LoopRansac::Vec3> p1, p2;
    std::vector<int> o1, o2;
    const int sizes[11] = {3, 64, 500, 2, 120, 65, 9, 300, 1000, 40, 250};
    for (int n : sizes) {
        scene(rng, n, 0.3, p1, p2, o1, o2);
        objs.emplace_back(p1, p2, o1, o2, kCam, kCam, st);
    }
    std::vector<LoopRansac> batch = objs;
    std::vector<LoopRansac *> ptrs;
    for (auto &o : batch) ptrs.push_back(&o);
    loopRansacEngine().seed(94235682);
    for (auto &o : objs) o.ransacSolve(ctx, 300, LoopRansac::DoF::SIM3);
    loopRansacEngine().seed(94235682);
    ransacSolveAll(ctx, ptrs, 300, LoopRansac::DoF::SIM3);
    int ok = 0;
    for (std::size_t k = 0; k < objs.size(); ++k) {
        const LoopRansac &a = objs[k], &b = batch[k];
        const bool same = a.solutionOk == b.solutionOk && a.bestInlierCount == b.bestInlierCount && a.bestIteration == b.bestIteration &&
                          a.bestR12 == b.bestR12 && a.bestT12 == b.bestT12 && a.bestScale12 == b.bestScale12 && a.bestInliers == b.bestInliers &&
                          a.bestHypothesisInliers == b.bestHypothesisInliers;
        if (!same) { std::printf("object %zu differs\n", k); return 1; }
        ok += a.solutionOk;
    }
    std::printf("batch ok %zu objects, %d solved, largest count %u\n", objs.size(), ok, objs[8].bestInlierCount);
    return ok >= 7 ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_loop_ransac, (const void *)&ms_ctx_create};
    std::printf("link ok %d\n", syms[0] != nullptr && syms[1] != nullptr);
    if (argc > 2 && std::strcmp(argv[1], "--no-gpu") == 0) return sampler(argv[2]);
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu();
    return 0;
}
