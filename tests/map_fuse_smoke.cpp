// map_fuse_smoke.cpp -- the host mirror of the fuse steps (host/mi355slam/map_update.hpp: deduplicateMapPoints, searchAndDeduplicate,
// mergeMatchedMapPoints) against a walk over std::map observations written for this test.
//   map_fuse_smoke --no-gpu   the mirror compiles and links; the host-only validation turns bad calls away and passes the empty ones
//   map_fuse_smoke --gpu      one scene of near-duplicate map point pairs seen by five keyframes: the three mirror calls, every table compared
// The candidates of the std::map walk come from replaceDuplicationCandidates (the downloading sibling, checked by project_gate_smoke), so
// what is compared here is the graph surgery and the chain's re-gating, not the gates.
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
constexpr int kPairs = 160, kMp = 2 * kPairs, kKf = 6, kStride = 192, kKp = 150, kTrackBase = 30, kWindow = 256;

// mapDB as the reference holds it
struct Mp { std::map<int, int> observations; std::uint8_t flags = 0; int track = -1; };
struct Graph {
    std::map<int, Mp> mapPoints;
    std::vector<std::vector<int>> keyframes;                 // Keyframe::mapPoints per slot
    std::map<int, int> trackIdToMapPoint;                    // the window's tracks
    std::vector<int> deadTrack = std::vector<int>(kMp, -1);
    std::vector<int> erasedRows, erasedInto;
    unsigned fused = 0;

    void replaceWith(int self, int other) {                  // map_point.cpp:118-156
        if (self == other) return;
        Mp &a = mapPoints.at(self), &b = mapPoints.at(other);
        if (a.track != -1 && b.track == -1) {
            if (trackIdToMapPoint.count(a.track)) trackIdToMapPoint[a.track] = other;
            b.track = a.track;
        }
        for (const auto &o : a.observations) {
            if (!b.observations.count(o.first)) { keyframes[(std::size_t)o.first][(std::size_t)o.second] = other; b.observations[o.first] = o.second; }
            else keyframes[(std::size_t)o.first][(std::size_t)o.second] = -1;
        }
        deadTrack[(std::size_t)self] = a.track;
        mapPoints.erase(self);
        erasedRows.push_back(self); erasedInto.push_back(other);
    }

    // replaceDuplication (keyframe_matcher.cpp:424-526) behind its gates: cand[i] = the best keypoint of list entry i or -1
    void replaceDuplication(int K, const std::vector<std::int32_t> &list, const std::vector<int> &cand) {
        std::set<int> erased;
        std::vector<int> &kf = keyframes[(std::size_t)K];
        for (std::size_t i = 0; i < list.size(); ++i) {
            const int id = list[i];
            if (erased.count(id) || !mapPoints.count(id)) continue;
            Mp &mp = mapPoints.at(id);
            if (mp.observations.count(K) || !(mp.flags & 2) || cand[i] < 0) continue;
            const int best = cand[i], matched = kf[(std::size_t)best];
            if (matched == -1) { mp.observations[K] = best; kf[(std::size_t)best] = id; }
            else {
                Mp &mm = mapPoints.at(matched);
                if (mp.observations.size() < mm.observations.size()) {
                    if (!(mm.flags & 2)) { mm.observations.erase(K); kf[(std::size_t)best] = id; mp.observations[K] = best; }
                    else replaceWith(id, matched);
                    erased.insert(id);
                } else { replaceWith(matched, id); erased.insert(matched); }
            }
            ++fused;
        }
    }
};

struct Scene {
    std::vector<DeviceMapPoints::Vec3d> pos;
    std::vector<DeviceMapPoints::Vec3f> norm;
    std::vector<float> dmin, dmax;
    std::vector<KeyPoint::Descriptor> desc;
    KeyPointVector kps[kKf];
    double R[kKf][9], t[kKf][3];
    std::vector<std::vector<std::int32_t>> kfMp;             // [kKf][kStride]
    std::vector<std::uint8_t> flags, live;
    std::vector<std::int32_t> track;
};

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
    S.kfMp.assign(kKf, std::vector<std::int32_t>(kStride, -1));
    for (int s = 0; s < kKf - 1; ++s) {                      // the last slot stays empty
        const double a = 0.06 * (U(rng) - 0.5), c = std::cos(a), sn = std::sin(a);
        const double R[9] = {c, -sn, 0, sn, c, 0, 0, 0, 1};
        std::copy(R, R + 9, S.R[s]);
        for (double &v : S.t[s]) v = 0.05 * (U(rng) - 0.5);
        std::vector<int> pairs(kPairs);
        for (int i = 0; i < kPairs; ++i) pairs[(std::size_t)i] = i;
        std::shuffle(pairs.begin(), pairs.end(), rng);
        for (int j = 0; j < kKp; ++j) {                      // keypoint j sits on pair pairs[j]: a slot lists a row once
            const int p = pairs[(std::size_t)j];
            const double *P = S.pos[(std::size_t)p].data();
            double pc[3];
            for (int i = 0; i < 3; ++i) pc[i] = R[3 * i] * P[0] + R[3 * i + 1] * P[1] + R[3 * i + 2] * P[2] + S.t[s][i];
            KeyPoint k{};
            k.pt.x = (float)(kCam.fx * pc[0] / pc[2] + kCam.cx + 1.5 * (U(rng) - 0.5)); k.pt.y = (float)(kCam.fy * pc[1] / pc[2] + kCam.cy + 1.5 * (U(rng) - 0.5));
            k.octave = (int)(rng() % 8); k.bearing = {0, 0, 1};
            k.descriptor = S.desc[(std::size_t)p];
            for (int b = 0; b < 8; ++b) k.descriptor[rng() % 8] ^= 1u << (rng() % 32);
            S.kps[s].push_back(k);
            const double how = U(rng);
            const int mine = s == 0 ? p : p + kPairs, twin = s == 0 ? p + kPairs : p;
            S.kfMp[(std::size_t)s][(std::size_t)j] = how < 0.5 ? mine : (how < 0.72 ? twin : -1);
        }
    }
    S.flags.resize(kMp); S.live.assign(kMp, 1); S.track.assign(kMp, -1);
    std::vector<int> ids(kMp);
    for (int i = 0; i < kMp; ++i) ids[(std::size_t)i] = kTrackBase - 20 + i;                  // some below the window, some above it
    std::shuffle(ids.begin(), ids.end(), rng);
    for (int r = 0; r < kMp; ++r) {
        const double f = U(rng);
        S.flags[(std::size_t)r] = f < 0.06 ? 0 : (f < 0.14 ? 1 : (f < 0.4 ? 2 : 3));
        if (U(rng) < 0.5) S.track[(std::size_t)r] = ids[(std::size_t)r];
    }
    std::vector<char> listed(kMp, 0);
    for (const auto &row : S.kfMp) for (std::int32_t r : row) if (r >= 0) listed[(std::size_t)r] = 1;
    for (int r = 0; r < kMp; ++r) if (!listed[(std::size_t)r] && U(rng) < 0.5) S.live[(std::size_t)r] = 0;
}

Graph graph_of(const Scene &S) {
    Graph G;
    G.keyframes.assign(kKf, std::vector<int>(kStride, -1));
    for (int r = 0; r < kMp; ++r)
        if (S.live[(std::size_t)r]) { Mp m; m.flags = S.flags[(std::size_t)r]; m.track = S.track[(std::size_t)r]; G.mapPoints[r] = m; }
        else G.deadTrack[(std::size_t)r] = S.track[(std::size_t)r];
    for (int s = 0; s < kKf; ++s)
        for (int j = 0; j < kStride; ++j) {
            const int r = S.kfMp[(std::size_t)s][(std::size_t)j];
            G.keyframes[(std::size_t)s][(std::size_t)j] = r;
            if (r >= 0) G.mapPoints.at(r).observations[s] = j;
        }
    for (int i = 0; i < kWindow; ++i) G.trackIdToMapPoint[kTrackBase + i] = -1;
    for (int r = 0; r < kMp; ++r) { const int t = S.track[(std::size_t)r]; if (t >= kTrackBase && t < kTrackBase + kWindow) G.trackIdToMapPoint[t] = r; }
    return G;
}

// the device side of one scene
struct Device {
    Context &ctx;
    DeviceMapPoints points;
    DeviceKeyframeMapPoints table;
    DeviceMapPointFlags flags;
    DeviceMapPointLive live;
    DeviceTrackTable tracks;
    DeviceArray<std::int32_t> nObs;
    KeyframeSlots slots;
    Device(Context &c, const Scene &S) : ctx(c), points(c, S.pos, S.norm, S.dmin, S.dmax, S.desc), table(c, kKf, kStride, kMp), flags(c, S.flags), live(c, S.live),
                                        tracks(c, kMp, kTrackBase, kWindow), nObs(c, kMp) {
        for (int s = 0; s < kKf; ++s) table.update((std::size_t)s, S.kfMp[(std::size_t)s]);
        std::vector<std::int32_t> rows, ids, outside;
        for (int r = 0; r < kMp; ++r) {
            const int t = S.track[(std::size_t)r];
            if (t >= kTrackBase && t < kTrackBase + kWindow) { rows.push_back(r); ids.push_back(t); }
        }
        tracks.bind(rows, ids);
        // the tracks outside the window: mp_track alone (what a narrower window leaves behind)
        for (int r = 0; r < kMp; ++r) {
            const std::int32_t t = S.track[(std::size_t)r];
            if (t != -1 && !(t >= kTrackBase && t < kTrackBase + kWindow)) c.check(ms_dev_upload(c.get(), tracks.mpTrack() + r, &t, 4), "ms_dev_upload");
        }
        slots.id.resize(kKf);
        for (int s = 0; s < kKf; ++s) slots.id[(std::size_t)s] = s < kKf - 1 ? 10 + s : -1;
        observationCountsOnDevice(c, tables());
    }
    MapTables tables() {
        MapTables M{table, slots};
        M.flags = &flags; M.points = &points; M.live = &live; M.tracks = &tracks; M.observationCount = nObs.data();
        return M;
    }
};

bool same_tables(Device &D, const Graph &G, const Scene &S, const char *what) {
    const std::vector<std::int32_t> kf = D.ctx.download(D.table.table(), (std::size_t)kKf * kStride), n = D.nObs.download();
    const std::vector<std::uint8_t> live = D.live.download(), flags = D.ctx.download(D.flags.flags(), (std::size_t)kMp);
    const std::vector<std::int32_t> mpTrack = D.tracks.downloadMapPointTracks(), trackRow = D.tracks.downloadTrackRows();
    for (int s = 0; s < kKf; ++s)
        for (int j = 0; j < kStride; ++j)
            if (kf[(std::size_t)(s * kStride + j)] != G.keyframes[(std::size_t)s][(std::size_t)j]) { std::printf("%s: kf_mp differs at slot %d keypoint %d\n", what, s, j); return false; }
    for (int r = 0; r < kMp; ++r) {
        const auto it = G.mapPoints.find(r);
        const bool alive = it != G.mapPoints.end();
        const std::uint8_t wantFlags = alive ? it->second.flags : (S.live[(std::size_t)r] ? 0 : S.flags[(std::size_t)r]);
        const int wantObs = alive ? (int)it->second.observations.size() : 0, wantTrack = alive ? it->second.track : G.deadTrack[(std::size_t)r];
        if ((live[(std::size_t)r] != 0) != alive || flags[(std::size_t)r] != wantFlags || n[(std::size_t)r] != wantObs || mpTrack[(std::size_t)r] != wantTrack) {
            std::printf("%s: row %d differs (live %d flags %d n_obs %d track %d, expected %d %d %d %d)\n", what, r, live[(std::size_t)r], flags[(std::size_t)r], n[(std::size_t)r],
                        mpTrack[(std::size_t)r], (int)alive, wantFlags, wantObs, wantTrack);
            return false;
        }
    }
    for (int i = 0; i < kWindow; ++i)
        if (trackRow[(std::size_t)i] != G.trackIdToMapPoint.at(kTrackBase + i)) { std::printf("%s: track_row differs at %d\n", what, i); return false; }
    return true;
}

bool same_lists(const FuseResult &got, const Graph &G, std::size_t from, const char *what) {
    const std::vector<int> rows(G.erasedRows.begin() + (std::ptrdiff_t)from, G.erasedRows.end()), into(G.erasedInto.begin() + (std::ptrdiff_t)from, G.erasedInto.end());
    if (std::vector<int>(got.erasedRows.begin(), got.erasedRows.end()) != rows || std::vector<int>(got.erasedInto.begin(), got.erasedInto.end()) != into) {
        std::printf("%s: the erased rows differ (%zu against %zu)\n", what, got.erasedRows.size(), rows.size());
        return false;
    }
    return true;
}

int no_gpu() {
    std::printf("link ok %d\n", (int)(sizeof(MapTables) > 0 && sizeof(FuseResult) > 0 && sizeof(FuseKeyframe) > 0));
    char why[256];
    std::int32_t kf[8] = {-1, -1, -1, -1, -1, -1, -1, -1}, nObs[4] = {0}, idx[4] = {0, 1, 2, 1}, kept[4] = {0}, top[16] = {0}, nKept[1] = {2}, out[10] = {0};
    std::uint8_t flags[4] = {0}, live[4] = {1, 1, 1, 1}, oc[2] = {0};
    std::uint16_t dist[16] = {0};
    ms_fuse_view v{1, 0, 3};
    int cases = 0;
    auto fuse = [&](int nViews, int maxDist, int source, int nEntries, const char *text) {
        const int rc = ms_map_fuse_check(kf, 2, 4, flags, live, nObs, 4, nullptr, nullptr, 0, 0, kept, top, dist, idx, nEntries, &v, nKept, nViews, maxDist, source, out, out + 1,
                                         out + 9, why, sizeof(why));
        ++cases;
        if (text ? (rc != MS_ERR_INVALID || !std::strstr(why, text)) : rc != MS_OK) { std::printf("fuse case %d: rc %d, %s\n", cases, rc, why); return false; }
        return true;
    };
    if (!fuse(1, 50, -1, 4, nullptr) || !fuse(0, 50, -1, 0, nullptr) || !fuse(1, 300, -1, 4, "max_dist") || !fuse(1, 50, 2, 4, "source slot")) return 1;
    v.count = 4;
    if (!fuse(1, 50, -1, 4, "lists row 1 twice")) return 1;
    v.count = 5;
    if (!fuse(1, 50, -1, 4, "slice")) return 1;
    v = ms_fuse_view{2, 0, 3};
    if (!fuse(1, 50, -1, 4, "slot 2 outside")) return 1;
    std::int32_t pairs[4] = {0, 1, 1, 4};
    if (ms_map_replace_pairs_check(kf, 2, 4, flags, live, nObs, 4, nullptr, nullptr, 0, 0, pairs, 2, oc, out, why, sizeof(why)) != MS_ERR_INVALID || !std::strstr(why, "row 4 outside")) return 1;
    pairs[3] = 2;
    if (ms_map_replace_pairs_check(kf, 2, 4, flags, live, nObs, 4, nullptr, nullptr, 0, 0, pairs, 2, oc, out, why, sizeof(why)) != MS_OK) return 1;
    if (ms_map_replace_pairs_check(kf, 2, 4, flags, live, nObs, 4, kf, nullptr, 0, 0, pairs, 2, oc, out, why, sizeof(why)) != MS_ERR_INVALID || !std::strstr(why, "one track table")) return 1;
    cases += 3;
    std::printf("no-gpu ok %d fuse cases\n", cases);
    return 0;
}

int gpu() {
    Context ctx(0);
    Parameters prm;
    StaticSettings st(prm);
    std::mt19937 rng(5);
    Scene S;
    make_scene(rng, S);
    std::vector<DeviceKeyframe> features;
    features.reserve(kKf);
    for (int s = 0; s < kKf - 1; ++s) {                      // the empty slot has no keyframe
        KeyframeFeatures f;
        f.keyPoints = &S.kps[s]; f.usable.assign(f.keyPoints->size(), 1);
        features.emplace_back(ctx, f);
    }
    auto keyframe = [&](int s) {
        FuseKeyframe k;
        k.slot = s; k.features = &features[(std::size_t)s]; k.camera = kCam;
        std::copy(S.R[s], S.R[s] + 9, k.R); std::copy(S.t[s], S.t[s] + 3, k.t);
        return k;
    };
    const float margin = 3.0f;
    // the candidates of one replaceDuplication call of the std::map walk, from the downloading sibling
    Device scratch(ctx, S);
    auto candidates = [&](int K, const std::vector<std::int32_t> &list, float m) {
        GateView V;
        std::copy(S.R[K], S.R[K] + 9, V.R); std::copy(S.t[K], S.t[K] + 3, V.t);
        V.camera = kCam; V.threshold = m; V.mode = MS_GATE_FUSE; V.indices = list;
        return replaceDuplicationCandidates(ctx, scratch.points, {V}, {&features[(std::size_t)K]}, st)[0];
    };
    auto valid_rows = [](const std::vector<int> &row) { std::vector<std::int32_t> r; for (int x : row) if (x >= 0) r.push_back(x); return r; };

    // deduplicateMapPoints: current = slot 0, adjacent = 1 .. 4
    Graph G = graph_of(S);
    int changed = 0;
    std::vector<std::int32_t> before;
    for (int a = 1; a <= 4; ++a) {                           // mapper_helpers.cpp:330-334: the list is read live
        const std::vector<std::int32_t> list = valid_rows(G.keyframes[0]);
        if (a > 1) for (std::int32_t r : list) if (std::find(before.begin(), before.end(), r) == before.end()) { ++changed; break; }
        before = list;
        G.replaceDuplication(a, list, candidates(a, list, margin));
    }
    std::set<int> adjacentSet;
    for (int a = 1; a <= 4; ++a) for (int r : G.keyframes[(std::size_t)a]) if (r != -1) adjacentSet.insert(r);
    const std::vector<std::int32_t> setList(adjacentSet.begin(), adjacentSet.end());
    G.replaceDuplication(0, setList, candidates(0, setList, margin));
    Device D(ctx, S);
    const FuseResult got = deduplicateMapPoints(ctx, D.tables(), keyframe(0), {keyframe(1), keyframe(2), keyframe(3), keyframe(4)}, margin, st);
    if (!same_tables(D, G, S, "deduplicateMapPoints") || !same_lists(got, G, 0, "deduplicateMapPoints")) return 2;
    if (got.fusedCount != G.fused || G.fused < 40 || G.erasedRows.size() < 10 || changed < 1 || got.regates < 1) {
        std::printf("deduplicateMapPoints: fused %u against %u, %zu erased, %d list changes, %u regates\n", got.fusedCount, G.fused, G.erasedRows.size(), changed, got.regates);
        return 2;
    }
    std::printf("deduplicateMapPoints ok fused %u erased %zu regates %u\n", got.fusedCount, G.erasedRows.size(), got.regates);

    // searchAndDeduplicate on the tables as they are now: the usable rows of slots 1 .. 3 against keyframes 4 and 0, margin 4
    {
        std::set<int> loopMapPoints;
        for (int a = 1; a <= 3; ++a) for (int r : G.keyframes[(std::size_t)a]) if (r != -1 && (G.mapPoints.at(r).flags & 2)) loopMapPoints.insert(r);
        const std::vector<std::int32_t> list(loopMapPoints.begin(), loopMapPoints.end());
        const std::size_t from = G.erasedRows.size();
        const unsigned fusedBefore = G.fused;
        // the gates read positions only, which nothing here moves: `scratch` still serves
        for (int k : {4, 0}) G.replaceDuplication(k, list, candidates(k, list, 4.0f));
        const FuseResult r = searchAndDeduplicate(ctx, D.tables(), {1, 2, 3}, {keyframe(4), keyframe(0)}, st);
        if (!same_tables(D, G, S, "searchAndDeduplicate") || !same_lists(r, G, from, "searchAndDeduplicate") || r.fusedCount != G.fused - fusedBefore) return 3;
        std::printf("searchAndDeduplicate ok fused %u\n", r.fusedCount);
    }
    // mergeMatchedMapPoints: a chain, an equal pair, a pair the `merged` rule skips
    {
        std::vector<int> alive;
        for (const auto &m : G.mapPoints) alive.push_back(m.first);
        if (alive.size() < 8) { std::printf("mergeMatchedMapPoints: %zu live rows\n", alive.size()); return 4; }
        const std::vector<std::pair<std::int32_t, std::int32_t>> matches{{alive[0], alive[1]}, {alive[1], alive[2]}, {alive[3], alive[3]}, {alive[0], alive[4]}, {alive[5], alive[1]},
                                                                         {alive[6], alive[7]}};
        const std::size_t from = G.erasedRows.size();
        std::set<int> merged;
        std::vector<std::uint8_t> want;
        for (const auto &m : matches) {                      // loop_closer.cpp:533-545
            if (m.first == m.second) { want.push_back(1); continue; }
            if (merged.count(m.first) || merged.count(m.second)) { want.push_back(2); continue; }
            merged.insert(m.first);
            G.replaceWith(m.first, m.second);
            want.push_back(0);
        }
        std::vector<std::uint8_t> outcome;
        const FuseResult r = mergeMatchedMapPoints(ctx, D.tables(), matches, &outcome);
        if (outcome != want || want != std::vector<std::uint8_t>{0, 0, 1, 2, 2, 0} || !same_tables(D, G, S, "mergeMatchedMapPoints") || !same_lists(r, G, from, "mergeMatchedMapPoints")) {
            std::printf("mergeMatchedMapPoints differs\n");
            return 4;
        }
        std::printf("mergeMatchedMapPoints ok replaced %u\n", r.fusedCount);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu();
    std::printf("usage: map_fuse_smoke --no-gpu | --gpu\n");
    return 64;
}
