// Compile + link check of the table writers of the host mirror (DeviceKeyframePoses, DeviceMapPoints::refresh, mi355slam::correctLoop in
// mi355slam/map_tables.hpp and map_update.hpp) against libmi355slam.so (tests/test_map_refresh_abi.py), their comparison with a sequential C++ restatement
// of the reference's loops, and the one-core baseline tools/map_refresh_probe.py times the device path against.
//   map_refresh_smoke --no-gpu            every MS_ERR_INVALID case of ms_map_refresh / ms_loop_correct through their _check halves (no context,
//                                         no device), and the restatement below on a hand-computed point
//   map_refresh_smoke --gpu               correctLoop through the mirror against ms_loop_correct followed by refresh, and both against the
//                                         restatement (tests/test_gpu_map_refresh.py)
//   map_refresh_smoke --baseline K M O    the restatement on one core + DeviceMapPoints::update for K keyframes, M moved map points, O observations
//                                         per point on average: the per-keyframe shape when K = 0 (refresh only), the loop shape otherwise
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "mi355slam/keyframe_matcher.hpp"       // detail::hamming256, the restatement's distance
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

using Pose = DeviceKeyframePoses::Pose;
using Vec3d = DeviceMapPoints::Vec3d;
using Vec3f = DeviceMapPoints::Vec3f;

struct HostMap {
    std::vector<Pose> pose;
    std::vector<Vec3d> pos;
    std::vector<Vec3f> norm;
    std::vector<float> dmin, dmax;
    std::vector<KeyPoint::Descriptor> desc, pool;
};

// ---- the reference's loops, sequentially ----------------------------------------------------------------------------------------------
Vec3d centre_of(const Pose &P) {                             // worldToCameraMatrixCameraCenter: -R^T t, summed left to right
    Vec3d c;
    for (int j = 0; j < 3; ++j) c[j] = -((P[j] * P[3] + P[4 + j] * P[7]) + P[8 + j] * P[11]);
    return c;
}
double sq_norm3(const Vec3d &v) { return v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]); }       // Eigen's unrolled redux

int medoid_of(const std::vector<const std::uint32_t *> &d) {     // map_point.cpp:88-115
    const std::size_t n = d.size();
    unsigned best = 256, bestIdx = 0;
    std::vector<unsigned> row(n);
    for (std::size_t i = 0; i < n; ++i) {
        for (std::size_t j = 0; j < n; ++j) row[j] = (unsigned)detail::hamming256(d[i], d[j]);
        std::sort(row.begin(), row.end());
        const unsigned med = row[(unsigned)(0.5 * (n - 1))];
        if (med < best) { best = med; bestIdx = (unsigned)i; }
    }
    return (int)bestIdx;
}

// MapPoint::updateDescriptor + updateDistanceAndNorm (map_point.cpp:75-116, :158-172) for one row; returns the medoid's position in the list
int refresh_row(HostMap &M, std::int32_t row, const std::vector<MapObservation> &obs, int octave, const StaticSettings &st, bool withDesc) {
    const Vec3d &p = M.pos[row];
    Vec3d sum{0.0, 0.0, 0.0};
    for (const MapObservation &o : obs) {
        const Vec3d c = centre_of(M.pose[o.keyframe]);
        Vec3d v{c[0] - p[0], c[1] - p[1], c[2] - p[2]};
        const double z = sq_norm3(v);
        if (z > 0.0) { const double len = std::sqrt(z); v = {v[0] / len, v[1] / len, v[2] / len}; }
        sum = {sum[0] + v[0], sum[1] + v[1], sum[2] + v[2]};
    }
    const float fn = (float)obs.size();
    M.norm[row] = {(float)sum[0] / fn, (float)sum[1] / fn, (float)sum[2] / fn};
    const Vec3d c0 = centre_of(M.pose[obs[0].keyframe]);
    const float dist = (float)std::sqrt(sq_norm3({c0[0] - p[0], c0[1] - p[1], c0[2] - p[2]}));
    const float top = dist * st.scaleFactors[octave];
    M.dmax[row] = top;
    M.dmin[row] = top / st.scaleFactors.back();
    if (!withDesc) return -1;
    std::vector<const std::uint32_t *> d;
    std::vector<int> at;
    for (std::size_t i = 0; i < obs.size(); ++i)
        if (obs[i].descriptor != -1) { d.push_back(M.pool[obs[i].descriptor].data()); at.push_back((int)i); }
    if (d.empty()) return -1;
    if (d.size() > MS_MEDOID_MAX_OBS) return -2;
    const int b = medoid_of(d);
    std::memcpy(M.desc[row].data(), d[b], 32);
    return at[b];
}

Sim3 se3ToSim3(const Pose &P) { return Sim3(std::array<double, 9>{P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]}, Sim3::Vec3{P[3], P[7], P[11]}, 1.0); }
Pose sim3ToSe3(const Sim3 &S) {
    const auto R = S.rotationMatrix();
    return {R[0], R[1], R[2], S.t[0], R[3], R[4], R[5], S.t[1], R[6], R[7], R[8], S.t[2]};
}
Sim3 interpolateFromIdentity(const Sim3 &T, double lambda) {     // loop_closer.cpp:69-76 with Eigen's slerp
    const double one = 1.0 - 2.220446049250313e-16, d = T.q[0], ad = std::fabs(d);
    double scale0, scale1;
    if (ad >= one) { scale0 = 1.0 - lambda; scale1 = lambda; }
    else {
        const double theta = std::acos(ad), sinTheta = std::sin(theta);
        scale0 = std::sin((1.0 - lambda) * theta) / sinTheta;
        scale1 = std::sin(lambda * theta) / sinTheta;
    }
    if (d < 0.0) scale1 = -scale1;
    return Sim3(std::array<double, 4>{scale0 * 1.0 + scale1 * T.q[0], scale0 * 0.0 + scale1 * T.q[1], scale0 * 0.0 + scale1 * T.q[2], scale0 * 0.0 + scale1 * T.q[3]},
                Sim3::Vec3{0.0 + lambda * (T.t[0] - 0.0), 0.0 + lambda * (T.t[1] - 0.0), 0.0 + lambda * (T.t[2] - 0.0)}, 1.0 + lambda * (T.s - 1.0));
}
// loop_closer.cpp:398-503 on the host map
void correct_loop(HostMap &M, const Sim3 &T, const LoopCorrections &C, const LoopPoints &P) {
    std::vector<Sim3> xfer;
    for (std::size_t i = 0; i < C.slot.size(); ++i) {
        Pose &pose = M.pose[C.slot[i]];
        const Sim3 prev = se3ToSim3(pose);
        Sim3 Tl = T;
        if (!C.rigid[i]) Tl = interpolateFromIdentity(T, C.lambda[i]);
        pose = sim3ToSe3(prev * Tl);
        xfer.push_back(se3ToSim3(pose).inverse() * prev);
    }
    for (std::size_t j = 0; j < P.row.size(); ++j) M.pos[P.row[j]] = xfer[P.reference[j]].map(M.pos[P.row[j]]);
}

// ---- scenes ---------------------------------------------------------------------------------------------------------------------------
struct Scene {
    HostMap map;
    std::vector<std::int32_t> rows, octave;
    std::vector<std::vector<MapObservation>> obs;
    LoopCorrections corr;
    LoopPoints pts;
    Sim3 T;
};

Scene make_scene(unsigned seed, int nKf, int nMp, int nRows, int meanObs, int nCorr) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    Scene S;
    HostMap &M = S.map;
    for (int k = 0; k < nKf; ++k) {
        const Sim3 r(std::array<double, 4>{U(rng), U(rng), U(rng), U(rng)}, Sim3::Vec3{5 * U(rng), 5 * U(rng), 5 * U(rng)}, 1.0);
        M.pose.push_back(sim3ToSe3(r));
    }
    const int nPool = 4 * nMp;
    M.pool.resize(nPool);
    for (auto &d : M.pool) for (auto &w : d) w = (std::uint32_t)rng();
    M.pos.resize(nMp); M.norm.resize(nMp); M.dmin.assign(nMp, 0.5f); M.dmax.assign(nMp, 20.f); M.desc.resize(nMp);
    for (int i = 0; i < nMp; ++i) {
        M.pos[i] = {8 * U(rng), 8 * U(rng), 8 * U(rng)};
        M.norm[i] = {(float)U(rng), (float)U(rng), (float)U(rng)};
        for (auto &w : M.desc[i]) w = (std::uint32_t)rng();
    }
    std::vector<std::int32_t> perm(nMp);
    for (int i = 0; i < nMp; ++i) perm[i] = i;
    std::shuffle(perm.begin(), perm.end(), rng);
    S.rows.assign(perm.begin(), perm.begin() + nRows);
    for (int r = 0; r < nRows; ++r) {
        const int n = 1 + (int)(rng() % (unsigned)(2 * meanObs - 1));
        std::vector<MapObservation> o;
        for (int i = 0; i < n; ++i) o.push_back({(std::int32_t)(rng() % (unsigned)nKf), rng() % 16 == 0 ? -1 : (std::int32_t)(rng() % (unsigned)nPool)});
        std::sort(o.begin(), o.end(), [](const MapObservation &a, const MapObservation &b) { return a.keyframe < b.keyframe; });
        S.obs.push_back(o);
        S.octave.push_back((std::int32_t)(rng() % 8));
    }
    std::vector<std::int32_t> kperm(nKf);
    for (int i = 0; i < nKf; ++i) kperm[i] = i;
    std::shuffle(kperm.begin(), kperm.end(), rng);
    for (int i = 0; i < nCorr; ++i) {
        S.corr.slot.push_back(kperm[i]);
        S.corr.rigid.push_back(i < nCorr / 4);
        S.corr.lambda.push_back(0.5 * (U(rng) + 1.0));
    }
    if (nCorr > 0)
        for (int r = 0; r < nRows; ++r) { S.pts.row.push_back(S.rows[r]); S.pts.reference.push_back((std::int32_t)(rng() % (unsigned)nCorr)); }
    S.T = Sim3(std::array<double, 4>{0.98, 0.05, -0.12, 0.08}, Sim3::Vec3{0.8, -0.4, 1.7}, 1.07);
    return S;
}

struct Downloaded {
    std::vector<Pose> pose;
    std::vector<Vec3d> pos;
    std::vector<Vec3f> norm;
    std::vector<float> dmin, dmax;
    std::vector<KeyPoint::Descriptor> desc;
};
Downloaded download(Context &ctx, const DeviceMapPoints &t, const DeviceKeyframePoses &p) {
    Downloaded d;
    const std::size_t n = t.size();
    d.pose = p.download();
    d.pos.resize(n); d.norm.resize(n); d.dmin.resize(n); d.dmax.resize(n); d.desc.resize(n);
    ctx.check(ms_dev_download(ctx.get(), d.pos.data(), t.position(), 24 * n), "download");
    ctx.check(ms_dev_download(ctx.get(), d.norm.data(), t.norm(), 12 * n), "download");
    ctx.check(ms_dev_download(ctx.get(), d.dmin.data(), t.minDistance(), 4 * n), "download");
    ctx.check(ms_dev_download(ctx.get(), d.dmax.data(), t.maxDistance(), 4 * n), "download");
    ctx.check(ms_dev_download(ctx.get(), d.desc.data(), t.descriptor(), 32 * n), "download");
    return d;
}
template <class T> bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0); }
bool same(const Downloaded &a, const Downloaded &b, bool poses = true) {
    return (!poses || same_bytes(a.pose, b.pose)) && same_bytes(a.pos, b.pos) && same_bytes(a.norm, b.norm) && same_bytes(a.dmin, b.dmin) && same_bytes(a.dmax, b.dmax) && same_bytes(a.desc, b.desc);
}

// ---- --no-gpu -------------------------------------------------------------------------------------------------------------------------
int no_gpu() {
    if (ms_map_refresh(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 8, nullptr) != MS_ERR_INVALID ||
        ms_loop_correct(nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0) != MS_ERR_INVALID) {
        std::printf("a call without a context must fail with MS_ERR_INVALID\n");
        return 1;
    }
    // the checks read the HOST arrays only: the device arrays are stand-in addresses that are never followed
    double *dpos = reinterpret_cast<double *>(0x1000), *dpose = reinterpret_cast<double *>(0x2000);
    float *dn = reinterpret_cast<float *>(0x3000), *dlo = reinterpret_cast<float *>(0x4000), *dhi = reinterpret_cast<float *>(0x5000);
    std::uint32_t *ddesc = reinterpret_cast<std::uint32_t *>(0x6000), *dpool = reinterpret_cast<std::uint32_t *>(0x7000);
    const float sf[8] = {1, 1.2f, 1.44f, 1.728f, 2.07f, 2.49f, 2.99f, 3.58f};
    struct R { std::vector<std::int32_t> rows{3, 0, 7}, start{0, 2, 3, 6}, kf{0, 1, 4, 1, 2, 3}, od{5, -1, 0, 9, 2, 2}, oct{0, 7, 3}; int nMp = 8, nKf = 5, nPool = 10, nLevels = 8; };
    char why[256];
    int cases = 0;
    auto refresh = [&](const R &r, const double *pos = reinterpret_cast<double *>(0x1000), const std::uint32_t *desc = reinterpret_cast<std::uint32_t *>(0x6000), const float *s = nullptr,
                       bool noRows = false, bool noStart = false, bool noKf = false, bool noOct = false) {
        why[0] = 0;
        return ms_map_refresh_check(pos, dn, dlo, dhi, desc, r.nMp, dpose, r.nKf, dpool, r.nPool, noRows ? nullptr : r.rows.data(), (int)r.rows.size(), noStart ? nullptr : r.start.data(),
                                    noKf ? nullptr : r.kf.data(), r.od.data(), noOct ? nullptr : r.oct.data(), s ? s : sf, r.nLevels, why, sizeof(why));
    };
    auto rejected = [&](int rc, const char *what) {
        ++cases;
        if (rc == MS_ERR_INVALID && why[0]) return true;
        std::printf("%s: returned %d (%s), expected MS_ERR_INVALID with a message\n", what, rc, why);
        return false;
    };
    R ok;
    if (refresh(ok) != MS_OK) { std::printf("a valid refresh was rejected: %s\n", why); return 1; }
    { R r; r.rows.clear(); r.start = {0}; r.oct.clear(); if (refresh(r) != MS_OK) { std::printf("n_rows = 0 was rejected: %s\n", why); return 1; } }
    bool good = true;
    { R r; r.rows[1] = 8; good &= rejected(refresh(r), "row beyond the table"); }
    { R r; r.rows[1] = -1; good &= rejected(refresh(r), "negative row"); }
    { R r; r.rows[2] = 3; good &= rejected(refresh(r), "duplicate row"); }
    { R r; r.kf[4] = 5; good &= rejected(refresh(r), "keyframe slot beyond the poses"); }
    { R r; r.kf[0] = -1; good &= rejected(refresh(r), "negative keyframe slot"); }
    { R r; r.od[3] = 10; good &= rejected(refresh(r), "descriptor beyond the pool"); }
    { R r; r.od[3] = -2; good &= rejected(refresh(r), "descriptor index -2"); }
    { R r; r.start = {0, 3, 2, 6}; good &= rejected(refresh(r), "obs_start decreases"); }
    { R r; r.start = {1, 2, 3, 6}; good &= rejected(refresh(r), "obs_start does not begin at 0"); }
    { R r; r.start = {0, 2, 2, 6}; good &= rejected(refresh(r), "empty observation list"); }
    { R r; r.oct[0] = 8; good &= rejected(refresh(r), "octave beyond the levels"); }
    { R r; r.oct[2] = -1; good &= rejected(refresh(r), "negative octave"); }
    { R r; r.nLevels = 0; good &= rejected(refresh(r), "no levels"); }
    good &= rejected(refresh(ok, nullptr), "missing positions");
    good &= rejected(refresh(ok, dpos, nullptr), "descriptor pool without table descriptors");
    good &= rejected(refresh(ok, dpos, ddesc + 1), "misaligned descriptors");
    good &= rejected(refresh(ok, dpos, ddesc, nullptr, true), "missing rows");
    good &= rejected(refresh(ok, dpos, ddesc, nullptr, false, true), "missing obs_start");
    good &= rejected(refresh(ok, dpos, ddesc, nullptr, false, false, true), "missing obs_kf");
    good &= rejected(refresh(ok, dpos, ddesc, nullptr, false, false, false, true), "missing first_octave");
    why[0] = 0;
    good &= rejected(ms_map_refresh_check(dpos, dn, dlo, dhi, ddesc, 8, dpose, 5, dpool, 10, ok.rows.data(), 3, ok.start.data(), ok.kf.data(), ok.od.data(), ok.oct.data(), nullptr, 8, why, sizeof(why)),
                     "missing scale factors");
    why[0] = 0;
    good &= rejected(ms_map_refresh_check(dpos, nullptr, dlo, dhi, ddesc, 8, dpose, 5, dpool, 10, ok.rows.data(), 3, ok.start.data(), ok.kf.data(), ok.od.data(), ok.oct.data(), sf, 8, why, sizeof(why)),
                     "missing normals");
    why[0] = 0;
    good &= rejected(ms_map_refresh_check(dpos, dn, dlo, dhi, ddesc, 8, nullptr, 5, dpool, 10, ok.rows.data(), 3, ok.start.data(), ok.kf.data(), ok.od.data(), ok.oct.data(), sf, 8, why, sizeof(why)),
                     "missing poses");
    const int refreshCases = cases;
    cases = 0;
    struct L { std::vector<double> T{1, 0, 0, 0, 0.1, 0.2, 0.3, 1.1}, lam{0.0, 0.5, 1.0}; std::vector<std::int32_t> slot{4, 0, 2}, row{7, 1, 3, 0}, ref{0, 2, 2, 1}; std::vector<std::uint8_t> rigid{1, 0, 0}; int nKf = 5, nMp = 8; };
    auto loop = [&](const L &l, bool noT = false, bool noSlot = false, bool noRow = false) {
        why[0] = 0;
        return ms_loop_correct_check(dpose, l.nKf, dpos, l.nMp, noT ? nullptr : l.T.data(), noSlot ? nullptr : l.slot.data(), l.rigid.data(), l.lam.data(), (int)l.slot.size(),
                                     noRow ? nullptr : l.row.data(), l.ref.data(), (int)l.row.size(), why, sizeof(why));
    };
    L lok;
    if (loop(lok) != MS_OK) { std::printf("a valid loop correction was rejected: %s\n", why); return 1; }
    { L l; l.slot[1] = 5; good &= rejected(loop(l), "slot beyond the poses"); }
    { L l; l.slot[1] = -1; good &= rejected(loop(l), "negative slot"); }
    { L l; l.slot[2] = 4; good &= rejected(loop(l), "duplicate slot"); }
    { L l; l.row[0] = 8; good &= rejected(loop(l), "row beyond the table"); }
    { L l; l.row[3] = 7; good &= rejected(loop(l), "duplicate row"); }
    { L l; l.ref[1] = 3; good &= rejected(loop(l), "reference beyond the corrections"); }
    { L l; l.ref[1] = -1; good &= rejected(loop(l), "negative reference"); }
    { L l; l.lam[1] = 1.0000001; good &= rejected(loop(l), "lambda above 1"); }
    { L l; l.lam[2] = -1e-12; good &= rejected(loop(l), "lambda below 0"); }
    { L l; l.lam[1] = std::nan(""); good &= rejected(loop(l), "lambda NaN"); }
    { L l; l.T[7] = INFINITY; good &= rejected(loop(l), "infinite scale"); }
    { L l; l.T[2] = std::nan(""); good &= rejected(loop(l), "NaN quaternion"); }
    good &= rejected(loop(lok, true), "missing T");
    good &= rejected(loop(lok, false, true), "missing slots");
    good &= rejected(loop(lok, false, false, true), "missing rows");
    if (!good) return 1;
    // identity rotation, t = (0, 0, -2): camera centre (0, 0, 2); the point at the origin, octave 1
    Parameters prm;
    StaticSettings st(prm);
    HostMap M;
    M.pose.push_back({1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -2});
    M.pos.push_back({0, 0, 0}); M.norm.push_back({9, 9, 9}); M.dmin.push_back(0); M.dmax.push_back(0); M.desc.resize(1);
    M.pool.resize(1); M.pool[0].fill(0xabcdu);
    const int med = refresh_row(M, 0, {{0, 0}}, 1, st, true);
    const float top = 2.f * st.scaleFactors[1];
    if (med != 0 || M.norm[0] != Vec3f{0.f, 0.f, 1.f} || M.dmax[0] != top || M.dmin[0] != top / st.scaleFactors.back() || M.desc[0] != M.pool[0]) {
        std::printf("restatement: one observation: medoid %d norm (%g, %g, %g) max %g min %g\n", med, M.norm[0][0], M.norm[0][1], M.norm[0][2], M.dmax[0], M.dmin[0]);
        return 1;
    }
    std::printf("no-gpu ok %d refresh cases %d loop cases\n", refreshCases, cases);
    return 0;
}

// ---- --gpu ----------------------------------------------------------------------------------------------------------------------------
int gpu() {
    Context ctx(0);
    Parameters prm;
    StaticSettings st(prm);
    Scene S = make_scene(17, 30, 200, 120, 5, 12);
    const HostMap &M = S.map;
    DeviceDescriptorPool pool(ctx, M.pool);
    RefreshArgs ra;
    ra.rows = S.rows; ra.observations = S.obs; ra.firstOctave = S.octave; ra.pool = &pool;
    // chained through the mirror
    DeviceMapPoints tableA(ctx, M.pos, M.norm, M.dmin, M.dmax, M.desc);
    DeviceKeyframePoses posesA(ctx, M.pose);
    const std::vector<int> medA = correctLoop(ctx, tableA, posesA, S.T, S.corr, S.pts, ra, st);
    // the two calls on their own
    DeviceMapPoints tableB(ctx, M.pos, M.norm, M.dmin, M.dmax, M.desc);
    DeviceKeyframePoses posesB(ctx, M.pose);
    const double t8[8] = {S.T.q[0], S.T.q[1], S.T.q[2], S.T.q[3], S.T.t[0], S.T.t[1], S.T.t[2], S.T.s};
    ctx.check(ms_loop_correct(ctx.get(), posesB.pose(), (int)posesB.size(), tableB.mutablePosition(), (int)tableB.size(), t8, S.corr.slot.data(), S.corr.rigid.data(),
                              S.corr.lambda.data(), (int)S.corr.slot.size(), S.pts.row.data(), S.pts.reference.data(), (int)S.pts.row.size()), "ms_loop_correct");
    const Downloaded afterLoop = download(ctx, tableB, posesB);
    const std::vector<int> medB = tableB.refresh(ctx, posesB, S.rows, S.obs, S.octave, st, &pool);
    const Downloaded A = download(ctx, tableA, posesA), B = download(ctx, tableB, posesB);
    if (!same(A, B) || medA != medB) { std::printf("correctLoop differs from ms_loop_correct followed by refresh\n"); return 2; }
    // the restatement of the refresh on the device's own poses and positions: every bit
    HostMap H = M;
    H.pose = afterLoop.pose; H.pos = afterLoop.pos;
    std::vector<int> medH;
    for (std::size_t r = 0; r < S.rows.size(); ++r) medH.push_back(refresh_row(H, S.rows[r], S.obs[r], S.octave[r], st, true));
    Downloaded Hd{H.pose, H.pos, H.norm, H.dmin, H.dmax, H.desc};
    if (!same(B, Hd) || medB != medH) { std::printf("refresh differs from its restatement\n"); return 3; }
    // the restatement of the correction: rigid members and untouched poses bit for bit; the distance of the interpolated ones and of the points is
    // printed, not judged (acos / sin differ between math libraries; tests/test_gpu_map_refresh.py holds them to a measured tolerance)
    HostMap L = M;
    correct_loop(L, S.T, S.corr, S.pts);
    std::vector<char> corrected(M.pose.size(), 0);
    double worst = 0.0;
    for (std::size_t i = 0; i < S.corr.slot.size(); ++i) {
        corrected[S.corr.slot[i]] = 1;
        const Pose &a = afterLoop.pose[S.corr.slot[i]], &b = L.pose[S.corr.slot[i]];
        if (S.corr.rigid[i] && std::memcmp(a.data(), b.data(), 96) != 0) { std::printf("rigid keyframe entry %zu differs from its restatement\n", i); return 4; }
        for (int k = 0; k < 12; ++k) worst = std::max(worst, std::fabs(a[k] - b[k]));
    }
    for (std::size_t k = 0; k < M.pose.size(); ++k)
        if (!corrected[k] && std::memcmp(afterLoop.pose[k].data(), M.pose[k].data(), 96) != 0) { std::printf("pose %zu was not listed and changed\n", k); return 5; }
    for (std::size_t i = 0; i < M.pos.size(); ++i)
        for (int k = 0; k < 3; ++k) worst = std::max(worst, std::fabs(afterLoop.pos[i][k] - L.pos[i][k]));
    int withDesc = 0;
    for (int m : medB) withDesc += m >= 0;
    std::printf("gpu ok chained %zu rows %d medoids worst %.3g\n", S.rows.size(), withDesc, worst);
    return 0;
}

// ---- --baseline -----------------------------------------------------------------------------------------------------------------------
int baseline(int nKf, int nRows, int meanObs) {
    Context ctx(0);
    Parameters prm;
    StaticSettings st(prm);
    const bool loopShape = nKf > 0;
    Scene S = make_scene(23, loopShape ? nKf : 400, nRows + nRows / 4, nRows, meanObs, loopShape ? nKf : 0);
    HostMap &M = S.map;
    DeviceMapPoints table(ctx, M.pos, M.norm, M.dmin, M.dmax, M.desc);
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    double arith = 1e30, rowsUp = 1e30, wholeUp = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
        HostMap W = M;
        const auto t0 = clk::now();
        if (loopShape) correct_loop(W, S.T, S.corr, S.pts);
        for (std::size_t r = 0; r < S.rows.size(); ++r) refresh_row(W, S.rows[r], S.obs[r], S.octave[r], st, true);
        const auto t1 = clk::now();
        if (!loopShape)                                          // the rows one by one, as a caller of the parent commit uploads them
            for (std::int32_t row : S.rows) table.update((std::size_t)row, 1, nullptr, &W.norm[row], &W.dmin[row], &W.dmax[row], &W.desc[row]);
        ms_ctx_sync(ctx.get());
        const auto t2 = clk::now();
        table.update(0, W.pos.size(), loopShape ? W.pos.data() : nullptr, W.norm.data(), W.dmin.data(), W.dmax.data(), W.desc.data());      // or the whole table at once
        ms_ctx_sync(ctx.get());
        const auto t3 = clk::now();
        arith = std::min(arith, ms(t0, t1)); rowsUp = std::min(rowsUp, ms(t1, t2)); wholeUp = std::min(wholeUp, ms(t2, t3));
    }
    std::printf("baseline %s rows %d arithmetic_ms %.3f update_rows_ms %.3f update_table_ms %.3f\n", loopShape ? "loop" : "keyframe", nRows, arith, loopShape ? -1.0 : rowsUp, wholeUp);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_map_refresh, (const void *)&ms_loop_correct, (const void *)&ms_map_refresh_check, (const void *)&ms_loop_correct_check};
    std::printf("link ok %d\n", syms[0] != nullptr && syms[1] != nullptr && syms[2] != nullptr && syms[3] != nullptr);
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu();
    if (argc > 4 && std::strcmp(argv[1], "--baseline") == 0) return baseline(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
    return 0;
}
