// Compile + link check of the host mirror of OptimizeSim3Transform (mi355slam/optimize_transform.hpp) against libmi355slam.so
// (tests/test_sim3_opt_abi.py).
//   sim3_opt_smoke --no-gpu   the Sim3 value type against a plain restatement with rotation matrices.  Creates no context.
//   sim3_opt_smoke --gpu      OptimizeSim3TransformAll on 11 problems against their per-object OptimizeSim3Transform (tests/test_gpu_sim3_opt.py)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "mi355slam/optimize_transform.hpp"

using namespace mi355slam;

namespace {

using Vec3 = Sim3::Vec3;
using Mat3 = std::array<double, 9>;

// the plain restatement: (R, t, s) with matrices, S.map(p) = s R p + t
struct Plain { Mat3 R; Vec3 t; double s; };
Vec3 mulv(const Mat3 &R, const Vec3 &p) { return {R[0] * p[0] + R[1] * p[1] + R[2] * p[2], R[3] * p[0] + R[4] * p[1] + R[5] * p[2], R[6] * p[0] + R[7] * p[1] + R[8] * p[2]}; }
Mat3 mulm(const Mat3 &A, const Mat3 &B) {
    Mat3 C{};
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) C[3 * i + j] += A[3 * i + k] * B[3 * k + j];
    return C;
}
Mat3 transpose(const Mat3 &A) { return {A[0], A[3], A[6], A[1], A[4], A[7], A[2], A[5], A[8]}; }
Vec3 pmap(const Plain &S, const Vec3 &p) { const Vec3 r = mulv(S.R, p); return {S.s * r[0] + S.t[0], S.s * r[1] + S.t[1], S.s * r[2] + S.t[2]}; }
Plain pinv(const Plain &S) { const Mat3 Rt = transpose(S.R); const Vec3 r = mulv(Rt, S.t); return {Rt, {-r[0] / S.s, -r[1] / S.s, -r[2] / S.s}, 1.0 / S.s}; }
Plain pmul(const Plain &A, const Plain &B) { const Vec3 r = mulv(A.R, B.t); return {mulm(A.R, B.R), {A.s * r[0] + A.t[0], A.s * r[1] + A.t[1], A.s * r[2] + A.t[2]}, A.s * B.s}; }

Mat3 rodrigues(const Vec3 &axis, double angle) {
    const double n = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    const double x = axis[0] / n, y = axis[1] / n, z = axis[2] / n, c = std::cos(angle), s = std::sin(angle), v = 1 - c;
    return {c + x * x * v, x * y * v - z * s, x * z * v + y * s, y * x * v + z * s, c + y * y * v, y * z * v - x * s, z * x * v - y * s, z * y * v + x * s, c + z * z * v};
}

double gap(const Vec3 &a, const Vec3 &b) { return std::fmax(std::fabs(a[0] - b[0]), std::fmax(std::fabs(a[1] - b[1]), std::fabs(a[2] - b[2]))); }

Plain randomPlain(std::mt19937 &rng, double maxAngle) {
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    return {rodrigues({U(rng), U(rng), U(rng) + 1e-3}, maxAngle * U(rng)), {U(rng), U(rng), U(rng)}, 0.5 + 0.75 * (U(rng) + 1.0)};
}

int valueType() {
    std::mt19937 rng(11);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    double worst = 0;
    for (int k = 0; k < 200; ++k) {
        const Plain A = randomPlain(rng, k % 4 == 0 ? 3.14159 : 1.0), B = randomPlain(rng, 3.0);      // angles near pi exercise every branch of the conversion
        const Sim3 a(A.R, A.t, A.s), b(B.R, B.t, B.s);
        const Vec3 p{5 * U(rng), 5 * U(rng), 5 * U(rng)};
        worst = std::fmax(worst, gap(a.map(p), pmap(A, p)));
        worst = std::fmax(worst, gap(a.inverse().map(p), pmap(pinv(A), p)));
        worst = std::fmax(worst, gap((a * b).map(p), pmap(pmul(A, B), p)));
        worst = std::fmax(worst, gap((a * a.inverse()).map(p), p));
        const Mat3 R = a.rotationMatrix();
        for (int i = 0; i < 9; ++i) worst = std::fmax(worst, std::fabs(R[i] - A.R[i]));
    }
    std::printf("value type ok %d, largest gap %.2e\n", worst < 1e-12, worst);
    return worst < 1e-12 ? 0 : 1;
}

// matches of a scene seen from two keyframes related by truth (p1 = truth.map(p2)), noisy observations
void scene(std::mt19937 &rng, int n, const Plain &truth, Sim3Matches &m) {
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 0.002);
    m = Sim3Matches{};
    for (int i = 0; i < n; ++i) {
        const Vec3 p2{4 * U(rng) - 2, 3 * U(rng) - 1.5, 3 + 5 * U(rng)}, p1 = pmap(truth, p2);
        m.pts1.push_back(p1); m.pts2.push_back(p2);
        m.obs1.push_back({p1[0] / p1[2] + N(rng), p1[1] / p1[2] + N(rng)});
        m.obs2.push_back({p2[0] / p2[2] + N(rng), p2[1] / p2[2] + N(rng)});
        m.octaves1.push_back((int)(8 * U(rng)) % 8); m.octaves2.push_back((int)(8 * U(rng)) % 8);
    }
}

bool same(const Sim3 &a, const Sim3 &b) { return a.q == b.q && a.t == b.t && a.s == b.s; }

int gpu() {
    Context ctx(0);
    Parameters prm;
    StaticSettings st(prm);
    std::mt19937 rng(7);
    const int sizes[11] = {3, 64, 500, 0, 120, 65, 9, 300, 2500, 40, 250};
    std::vector<Sim3Matches> sets(11);
    std::vector<Sim3> start, truths;
    for (int k = 0; k < 11; ++k) {
        const Plain T = randomPlain(rng, 0.3);
        scene(rng, sizes[k], T, sets[k]);
        Plain P = T;
        P.t = {T.t[0] + 0.05, T.t[1] - 0.03, T.t[2] + 0.02};
        P.s = T.s * 1.02;
        start.emplace_back(P.R, P.t, P.s);
        truths.emplace_back(T.R, T.t, T.s);
    }
    std::vector<Sim3> single = start, batch = start;
    std::vector<Sim3OptStats> one(11), all;
    unsigned total = 0;
    for (int k = 0; k < 11; ++k) total += OptimizeSim3Transform(ctx, sets[k], single[k], st, &one[k]);
    std::vector<const Sim3Matches *> ptrs;
    for (auto &s : sets) ptrs.push_back(&s);
    const std::vector<unsigned> counts = OptimizeSim3TransformAll(ctx, ptrs, batch, st, &all);
    int improved = 0;
    for (int k = 0; k < 11; ++k) {
        if (!same(single[k], batch[k]) || one[k].chi2Final != all[k].chi2Final || one[k].iterations != all[k].iterations || counts[k] != (unsigned)sizes[k]) {
            std::printf("problem %d differs\n", k);
            return 1;
        }
        if (sizes[k] == 0) { if (!same(batch[k], start[k]) || all[k].iterations != 0) { std::printf("empty problem moved\n"); return 1; } continue; }
        const Vec3 p{0.5, -0.25, 5.0};
        improved += all[k].chi2Final < all[k].chi2Initial && gap(batch[k].map(p), truths[k].map(p)) < gap(start[k].map(p), truths[k].map(p));
    }
    std::printf("batch ok 11 problems, %u matches, %d nearer the truth\n", total, improved);
    return improved == 10 ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_sim3_optimize, (const void *)&ms_ctx_create};
    std::printf("link ok %d\n", syms[0] != nullptr && syms[1] != nullptr);
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return valueType();
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu();
    return 0;
}
