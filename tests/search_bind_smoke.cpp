// search_bind_smoke.cpp -- the host mirror of matchLocalMapPoints (host/mi355slam/map_update.hpp; searchByProjectionOnTables in
// keyframe_matcher.hpp) against a walk over a std::set of local map points and std::map observations written for this test.
//   search_bind_smoke --no-gpu   the mirror compiles and links; the host-only validation turns bad calls away and passes the empty ones
//   search_bind_smoke --gpu      one keyframe among three adjacent ones: the mirror call, every table and the match list compared
// The matches of the std::map walk come from searchByProjection (the sibling that downloads the lists and replays the walk on the host,
// checked by project_gate_smoke), so what is compared here is the device walk with its addObservations against the host's.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

const ms_pinhole kCam{450.0, 450.0, 320.0, 240.0, 640, 480};
constexpr int kPairs = 200, kMp = 2 * kPairs, kKf = 5, kStride = 192, kKp = 150, kCurrent = 1;

// mapDB as the reference holds it
struct Mp { std::map<int, int> observations; std::uint8_t flags = 0; };
struct Graph {
    std::map<int, Mp> mapPoints;
    std::vector<std::vector<int>> keyframes;                 // Keyframe::mapPoints per slot

    // mapper_helpers.cpp:241-261: the usable map points of the adjacent keyframes that the current one does not observe, as a std::set
    std::vector<std::int32_t> localMapPoints(int current, const std::vector<std::int32_t> &adjacent) const {
        std::set<int> local;
        for (int a : adjacent)
            for (int r : keyframes[(std::size_t)a]) {
                if (r == -1) continue;
                const Mp &mp = mapPoints.at(r);
                if (mp.observations.count(current) || !(mp.flags & 2)) continue;
                local.insert(r);
            }
        return std::vector<std::int32_t>(local.begin(), local.end());
    }
    // keyframe_matcher.cpp:388-389 for the matches of one searchByProjection call
    unsigned addObservations(int current, const std::vector<std::int32_t> &list, const std::vector<int> &match) {
        unsigned n = 0;
        for (std::size_t i = 0; i < list.size(); ++i) {
            if (match[i] < 0) continue;
            keyframes[(std::size_t)current][(std::size_t)match[i]] = list[i];
            mapPoints.at(list[i]).observations[current] = match[i];
            ++n;
        }
        return n;
    }
};

struct Scene {
    std::vector<DeviceMapPoints::Vec3d> pos;
    std::vector<DeviceMapPoints::Vec3f> norm;
    std::vector<float> dmin, dmax;
    std::vector<KeyPoint::Descriptor> desc;
    KeyPointVector kps;                                      // of the current keyframe
    double R[9], t[3];
    std::vector<std::vector<std::int32_t>> kfMp;             // [kKf][kStride]
    std::vector<std::uint8_t> flags, live;
};

// pairs of map points a millimetre apart with descriptors a few bits apart, so two queries compete for the keypoint that sits on the pair
void make_scene(std::mt19937 &rng, Scene &S) {
    std::uniform_real_distribution<double> U(0.0, 1.0);
    S.pos.resize(kMp); S.norm.resize(kMp); S.dmin.resize(kMp); S.dmax.resize(kMp); S.desc.resize(kMp);
    for (int i = 0; i < kPairs; ++i) {
        const double z = 2.0 + 7.0 * U(rng), x = (1.2 * U(rng) - 0.6) * z, y = (0.9 * U(rng) - 0.45) * z, d = std::sqrt(x * x + y * y + z * z);
        const float dmax = (float)(d * (1.3 + 2.0 * U(rng)));
        KeyPoint::Descriptor ds;
        for (auto &w : ds) w = (std::uint32_t)rng();
        for (int twin = 0; twin < 2; ++twin) {
            const std::size_t r = (std::size_t)(i + twin * kPairs);
            S.pos[r] = {x + 1e-3 * twin, y, z};
            S.norm[r] = {(float)(-x / d), (float)(-y / d), (float)(-z / d)};
            S.dmax[r] = dmax; S.dmin[r] = dmax / 5.f;
            S.desc[r] = ds;
            if (twin) for (int b = 0; b < 6; ++b) S.desc[r][rng() % 8] ^= 1u << (rng() % 32);
        }
    }
    const double a = 0.03, c = std::cos(a), sn = std::sin(a);
    const double R[9] = {c, -sn, 0, sn, c, 0, 0, 0, 1};
    std::copy(R, R + 9, S.R);
    for (double &v : S.t) v = 0.05 * (U(rng) - 0.5);
    S.kfMp.assign(kKf, std::vector<std::int32_t>(kStride, -1));
    std::vector<int> pairs(kPairs);
    for (int i = 0; i < kPairs; ++i) pairs[(std::size_t)i] = i;
    std::shuffle(pairs.begin(), pairs.end(), rng);
    for (int j = 0; j < kKp; ++j) {                          // keypoint j of the current keyframe sits on pair pairs[j]
        const int p = pairs[(std::size_t)j];
        const double *P = S.pos[(std::size_t)p].data();
        double pc[3];
        for (int i = 0; i < 3; ++i) pc[i] = R[3 * i] * P[0] + R[3 * i + 1] * P[1] + R[3 * i + 2] * P[2] + S.t[i];
        KeyPoint k{};
        k.pt.x = (float)(kCam.fx * pc[0] / pc[2] + kCam.cx + 1.5 * (U(rng) - 0.5)); k.pt.y = (float)(kCam.fy * pc[1] / pc[2] + kCam.cy + 1.5 * (U(rng) - 0.5));
        k.octave = (int)(rng() % 8); k.bearing = {0, 0, 1};
        k.descriptor = S.desc[(std::size_t)p];
        for (int b = 0; b < 8; ++b) k.descriptor[rng() % 8] ^= 1u << (rng() % 32);
        S.kps.push_back(k);
        if (U(rng) < 0.3) S.kfMp[kCurrent][(std::size_t)j] = U(rng) < 0.5 ? p : p + kPairs;      // bound already
    }
    for (int s = 0; s < kKf - 1; ++s) {                      // the adjacent keyframes list rows of their own; the last slot stays empty
        if (s == kCurrent) continue;
        std::vector<int> rows(kMp);
        for (int r = 0; r < kMp; ++r) rows[(std::size_t)r] = r;
        std::shuffle(rows.begin(), rows.end(), rng);
        for (int j = 0; j < kKp; ++j) if (U(rng) < 0.8) S.kfMp[(std::size_t)s][(std::size_t)j] = rows[(std::size_t)j];
    }
    S.flags.resize(kMp); S.live.assign(kMp, 1);
    for (int r = 0; r < kMp; ++r) {
        const double f = U(rng);
        S.flags[(std::size_t)r] = f < 0.06 ? 0 : (f < 0.14 ? 1 : (f < 0.4 ? 2 : 3));
    }
    std::vector<char> listed(kMp, 0);
    for (const auto &row : S.kfMp) for (std::int32_t r : row) if (r >= 0) listed[(std::size_t)r] = 1;
    for (int r = 0; r < kMp; ++r) if (!listed[(std::size_t)r]) S.live[(std::size_t)r] = 0;
}

Graph graph_of(const Scene &S) {
    Graph G;
    G.keyframes.assign(kKf, std::vector<int>(kStride, -1));
    for (int r = 0; r < kMp; ++r) if (S.live[(std::size_t)r]) { Mp m; m.flags = S.flags[(std::size_t)r]; G.mapPoints[r] = m; }
    for (int s = 0; s < kKf; ++s)
        for (int j = 0; j < kStride; ++j) {
            const int r = S.kfMp[(std::size_t)s][(std::size_t)j];
            G.keyframes[(std::size_t)s][(std::size_t)j] = r;
            if (r >= 0) G.mapPoints.at(r).observations[s] = j;
        }
    return G;
}

int no_gpu() {
    std::printf("link ok %d\n", (int)(sizeof(SearchBindResult) > 0 && sizeof(detail::BoundMaskSource) > 0 && sizeof(MapTables) > 0));
    char why[256];
    std::int32_t kf[8] = {-1, 2, -1, -1, -1, -1, 0, -1}, nObs[4] = {1, 0, 1, 0}, idx[4] = {3, 1, 2, 9}, out[8] = {0};
    std::uint8_t live[4] = {1, 1, 1, 1}, skip[4] = {0};
    alignas(16) std::uint32_t lists[64] = {0};
    const float *f = reinterpret_cast<const float *>(lists);
    const std::int32_t *i = reinterpret_cast<const std::int32_t *>(lists);
    const std::uint16_t *h = reinterpret_cast<const std::uint16_t *>(lists);
    int cases = 0;
    auto bind = [&](int nKp, int first, int count, int nKept, int slot, int code, const char *text) {
        const int rc = ms_search_bind_check(kf, 2, 4, live, nObs, 4, i, f, f, f, nullptr, nullptr, lists, i, h, i, i, skip, f, f, i, lists, i, nKp, idx, first, count, nKept, slot,
                                            out, out + 1, why, sizeof(why));
        ++cases;
        if (rc != code || (text && !std::strstr(why, text))) { std::printf("bind case %d: rc %d, %s\n", cases, rc, why); return false; }
        return true;
    };
    if (!bind(4, 0, 3, 2, 1, MS_OK, nullptr) || !bind(4, 0, 0, 0, 1, MS_OK, nullptr) || !bind(0, 1, 2, 0, 0, MS_OK, nullptr)) return 1;
    if (!bind(5, 0, 3, 2, 1, MS_ERR_INVALID, "5 keypoints for a stride of 4") || !bind(4, 0, 3, 4, 1, MS_ERR_INVALID, "n_kept 4 for a slice of 3")) return 1;
    if (!bind(4, 0, 3, 2, 2, MS_ERR_INVALID, "slot 2 outside") || !bind(4, 1, 3, 2, 1, MS_ERR_INVALID, "entry 3 is row 9 outside [0, 4)")) return 1;
    if (!bind(4, -1, 3, 2, 1, MS_ERR_INVALID, "negative size") || !bind(4, MS_GATE_MAX_ENTRIES - 2, 3, 2, 1, MS_ERR_CAPACITY, "cap below")) return 1;
    if (ms_bound_mask_check(kf, 2, 4, 4, 1, 4, skip, why, sizeof(why)) != MS_OK) return 1;
    if (ms_bound_mask_check(kf, 2, 4, 4, 1, 4, nullptr, why, sizeof(why)) != MS_ERR_INVALID || !std::strstr(why, "missing array (skip)")) return 1;
    if (ms_bound_mask_check(kf, 2, 4, 4, -1, 4, skip, why, sizeof(why)) != MS_ERR_INVALID || !std::strstr(why, "slot -1 outside")) return 1;
    cases += 3;
    std::printf("no-gpu ok %d cases\n", cases);
    return 0;
}

int gpu() {
    Context ctx(0);
    Parameters prm;
    StaticSettings st(prm);
    std::mt19937 rng(9);
    Scene S;
    make_scene(rng, S);
    KeyframeFeatures kff;
    kff.keyPoints = &S.kps; kff.usable.assign(S.kps.size(), 1);
    for (int j = 0; j < kKp; ++j) if (S.kfMp[kCurrent][(std::size_t)j] != -1) kff.usable[(std::size_t)j] = 0;
    DeviceKeyframe features(ctx, kff);
    DeviceMapPoints points(ctx, S.pos, S.norm, S.dmin, S.dmax, S.desc);
    DeviceKeyframeMapPoints table(ctx, kKf, kStride, kMp);
    DeviceMapPointFlags flags(ctx, S.flags);
    DeviceMapPointLive live(ctx, S.live);
    DeviceArray<std::int32_t> nObs(ctx, kMp);
    for (int s = 0; s < kKf; ++s) table.update((std::size_t)s, S.kfMp[(std::size_t)s]);
    KeyframeSlots slots;
    slots.id.resize(kKf);
    for (int s = 0; s < kKf; ++s) slots.id[(std::size_t)s] = s < kKf - 1 ? 10 + s : -1;
    MapTables tables{table, slots};
    tables.flags = &flags; tables.points = &points; tables.live = &live; tables.observationCount = nObs.data();
    observationCountsOnDevice(ctx, tables);
    const std::vector<std::int32_t> adjacent{0, 2, 3};
    const float threshold = 10.0f;

    // the std::set / std::map walk: the local list, the host replay of searchByProjection, addObservation
    Graph G = graph_of(S);
    const std::vector<std::int32_t> list = G.localMapPoints(kCurrent, adjacent);
    GateView V;
    std::copy(S.R, S.R + 9, V.R); std::copy(S.t, S.t + 3, V.t);
    V.camera = kCam; V.threshold = threshold; V.cosLimit = 0.5f; V.mode = MS_GATE_SEARCH; V.indices = list;
    std::vector<std::uint8_t> bound(kKp, 0);
    for (int j = 0; j < kKp; ++j) bound[(std::size_t)j] = S.kfMp[kCurrent][(std::size_t)j] != -1;
    const std::vector<int> match = searchByProjection(ctx, features, points, V, bound, st);
    const unsigned wantMatched = G.addObservations(kCurrent, list, match);

    FuseKeyframe current;
    current.slot = kCurrent; current.features = &features; current.camera = kCam;
    std::copy(S.R, S.R + 9, current.R); std::copy(S.t, S.t + 3, current.t);
    const SearchBindResult got = matchLocalMapPoints(ctx, tables, current, adjacent, threshold, st, features.mutableUsable(), true);

    if (got.matched != wantMatched || wantMatched < 30 || list.size() < 100 || got.matchKp != std::vector<std::int32_t>(match.begin(), match.end())) {
        std::printf("matchLocalMapPoints: %u matches against %u over %zu rows\n", got.matched, wantMatched, list.size());
        return 2;
    }
    const std::vector<std::int32_t> kf = ctx.download(table.table(), (std::size_t)kKf * kStride), n = nObs.download();
    for (int s = 0; s < kKf; ++s)
        for (int j = 0; j < kStride; ++j)
            if (kf[(std::size_t)(s * kStride + j)] != G.keyframes[(std::size_t)s][(std::size_t)j]) { std::printf("kf_mp differs at slot %d keypoint %d\n", s, j); return 2; }
    for (int r = 0; r < kMp; ++r) {
        const auto it = G.mapPoints.find(r);
        const int want = it == G.mapPoints.end() ? 0 : (int)it->second.observations.size();
        if (n[(std::size_t)r] != want) { std::printf("row %d: n_obs %d, expected %d\n", r, n[(std::size_t)r], want); return 2; }
    }
    const std::vector<std::uint8_t> usable = ctx.download(features.mutableUsable(), (std::size_t)kKp);
    for (int j = 0; j < kKp; ++j)
        if ((usable[(std::size_t)j] != 0) != (G.keyframes[kCurrent][(std::size_t)j] == -1)) { std::printf("usable differs at keypoint %d\n", j); return 2; }
    // a second call finds the rows bound now excluded from the list and binds nothing twice
    const SearchBindResult again = matchLocalMapPoints(ctx, tables, current, adjacent, threshold, st);
    const std::vector<std::int32_t> kf2 = ctx.download(table.table(), (std::size_t)kKf * kStride);
    for (std::size_t i = 0; i < kf.size(); ++i) if (kf2[i] != kf[i] && kf[i] != -1) { std::printf("the second call moved a bound keypoint\n"); return 3; }
    std::printf("matchLocalMapPoints ok matched %u of %zu rows, rescans %d, then %u\n", got.matched, list.size(), got.counts[5], again.matched);
    // the empty list (:263)
    const SearchBindResult none = matchLocalMapPoints(ctx, tables, current, {4}, threshold, st);
    if (none.matched != 0) return 4;
    std::printf("empty list ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu();
    std::printf("usage: search_bind_smoke --no-gpu | --gpu\n");
    return 64;
}
