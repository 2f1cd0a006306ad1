// Compile + link check of the createNewMapPoints part of the host mirror (mi355slam/map_update.hpp: createNewMapPoints, unboundMasks) against
// libmi355slam.so, and its run on one small map.
//   create_points_smoke --no-gpu   the symbols link; a few calls of the three *_check twins (no context, no device)
//   create_points_smoke            mapper_helpers.cpp:271-318 twice on copies of one seeded map: through mi355slam::createNewMapPoints (nothing
//                                  per match on the host), and through a sequential restatement that keeps Keyframe::mapPoints and
//                                  `std::map<KfId, KpId> observations` on the host, runs matchForTriangulationDBoW, downloads the matches, hands
//                                  host lists to triangulateMapPoints, uploads both keyframes' rows (DeviceKeyframeMapPoints::update), the
//                                  descriptors and the masks.  Per-adjacent results, every table and every mask must agree bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>
#include "mi355slam/keyframe_matcher.hpp"
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

int no_gpu() {
    char why[256] = {0};
    const auto *dev = reinterpret_cast<std::int32_t *>(0x1000);       // never dereferenced by the validation
    const auto *devf = reinterpret_cast<float *>(0x1000);
    const auto *devb = reinterpret_cast<std::uint8_t *>(0x1000);
    const auto *devu = reinterpret_cast<std::uint32_t *>(0x1000);
    std::int32_t kfId[3] = {4, 9, 7}, base[3] = {0, 8, 16}, newRows[3] = {3, 8, 5}, n = 0;
    ms_obs_lists l{};
    l.rows = const_cast<std::int32_t *>(dev); l.obs_start = const_cast<std::int32_t *>(dev);
    auto lists = [&](int cur, int adj, int nKp1, int nNew) {
        return ms_create_points_lists_check(dev, 3, 8, devb, 9, kfId, devf, devf, dev, devf, base, cur, adj, dev, nKp1, 8, newRows, nNew, 8, &l, 4, 8, dev, dev, &n, why, sizeof(why));
    };
    if (lists(1, 2, 8, 3) != MS_OK) { std::printf("a valid lists call was rejected: %s\n", why); return 1; }
    int cases = 0;
    cases += lists(1, 1, 8, 3) == MS_ERR_INVALID && why[0];                               // cur == adj
    cases += lists(3, 2, 8, 3) == MS_ERR_INVALID && why[0];                               // slot out of range
    cases += lists(1, 2, 9, 3) == MS_ERR_INVALID && why[0];                               // n_kp > stride
    kfId[2] = -1;      cases += lists(1, 2, 8, 3) == MS_ERR_INVALID && why[0]; kfId[2] = 7;          // an empty slot
    newRows[2] = 3;    cases += lists(1, 2, 8, 3) == MS_ERR_INVALID && why[0]; newRows[2] = 5;       // a new row twice
    newRows[0] = 9;    cases += lists(1, 2, 8, 3) == MS_ERR_INVALID && why[0]; newRows[0] = 3;       // a new row outside the table
    l.rows = nullptr;  cases += lists(1, 2, 8, 3) == MS_ERR_INVALID && why[0]; l.rows = const_cast<std::int32_t *>(dev);
    auto bind = [&](int adj, int nMatches, const std::uint32_t *desc) {
        return ms_create_points_bind_check(dev, 3, 8, devb, devb, desc, nullptr, nullptr, 9, devu, 64, 1, adj, &l, dev, dev, nMatches, 8, 8, nullptr, nullptr, nullptr, nullptr, nullptr, &n,
                                           why, sizeof(why));
    };
    l.obs_desc = const_cast<std::int32_t *>(dev);
    if (bind(2, 4, devu) != MS_OK) { std::printf("a valid bind call was rejected: %s\n", why); return 1; }
    cases += bind(1, 4, devu) == MS_ERR_INVALID && why[0];
    cases += bind(2, 4, nullptr) == MS_ERR_INVALID && why[0];                             // descriptors asked for, no mp_desc
    cases += bind(2, MS_COVIS_MAX_STRIDE + 1, devu) == MS_ERR_CAPACITY && why[0];
    std::int32_t slots[2] = {0, 2}, counts[2] = {8, 3};
    std::uint8_t *masks[2] = {const_cast<std::uint8_t *>(devb), const_cast<std::uint8_t *>(devb)};
    if (ms_unbound_mask_check(dev, 3, 8, 9, slots, counts, masks, 2, why, sizeof(why)) != MS_OK) { std::printf("a valid mask call was rejected: %s\n", why); return 1; }
    counts[0] = 9;     cases += ms_unbound_mask_check(dev, 3, 8, 9, slots, counts, masks, 2, why, sizeof(why)) == MS_ERR_INVALID && why[0]; counts[0] = 8;
    slots[1] = 3;      cases += ms_unbound_mask_check(dev, 3, 8, 9, slots, counts, masks, 2, why, sizeof(why)) == MS_ERR_INVALID && why[0]; slots[1] = 2;
    if (cases != 12) { std::printf("%d of 12 bad calls were rejected\n", cases); return 1; }
    std::printf("no-gpu ok %d cases\n", cases);
    return 0;
}

struct Rng {                             // a fixed sequence: the same map on every run
    std::uint64_t s = 0x9E3779B97F4A7C15ull;
    std::uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (std::uint32_t)(s >> 33); }
    double unit() { return next() / 2147483648.0; }
    int below(int n) { return (int)(next() % (std::uint32_t)n); }
};

struct Map {
    static constexpr int nKf = 5, stride = 320, nMp = 600, current = 2, nKp = 300, nPoints = 150, nExisting = 20, firstFree = 300;
    std::vector<KeyPointVector> keyPoints;                   // per slot
    std::vector<std::vector<std::int32_t>> mapPoints;        // Keyframe::mapPoints per slot
    std::vector<std::vector<unsigned>> node;
    std::vector<std::vector<float>> depth;
    std::vector<std::int32_t> kfId, descBase, adjacent, freeRows;
    std::vector<DeviceKeyframePoses::Pose> pose;
    KeyframeSlots cams;                      // camera and focalLength; the view's id and descBase are kfId and descBase above
    std::vector<DeviceMapPoints::Vec3d> position;
    std::vector<std::uint8_t> flags, live;
    std::vector<KeyPoint::Descriptor> pool;
};

KeyPoint key_point(const ms_pinhole &c, double u, double v, int octave, const KeyPoint::Descriptor &d) {
    KeyPoint kp{};
    kp.pt = {(float)u, (float)v}; kp.angle = 0.f; kp.octave = octave; kp.descriptor = d;
    const double xn = ((double)kp.pt.x - c.cx) / c.fx, yn = ((double)kp.pt.y - c.cy) / c.fy, nrm = std::sqrt(xn * xn + yn * yn + 1.0);
    kp.bearing = {xn / nrm, yn / nrm, 1.0 / nrm};
    return kp;
}

Map make_map() {
    Map m;
    Rng rng;
    const int K = Map::nKf;
    const int ids[Map::nKf] = {5, 9, 7, 11, 3};              // id order is not slot order; slot 3 is younger than the current keyframe
    m.keyPoints.assign(K, {}); m.mapPoints.assign(K, {}); m.node.assign(K, {}); m.depth.assign(K, {});
    const ms_pinhole cam{500.0, 502.0, 320.0, 240.0, 640, 480};
    for (int k = 0; k < K; ++k) {                            // cameras 0.15 apart along x, looking down +z
        m.pose.push_back({1, 0, 0, -0.15 * k, 0, 1, 0, 0.01 * (k % 3), 0, 0, 1, 0});
        m.cams.camera.push_back(cam);
        m.cams.focalLength.push_back(500);
        m.kfId.push_back(ids[k]);
        m.descBase.push_back(k * Map::stride);
    }
    m.adjacent = {3, 0, Map::current, 4};
    auto random_desc = [&] { KeyPoint::Descriptor d; for (auto &w : d) w = rng.next() * 2u + (rng.next() & 1u); return d; };
    auto add = [&](int k, double u, double v, int octave, const KeyPoint::Descriptor &d, unsigned node, std::int32_t row, float depth) {
        m.keyPoints[k].push_back(key_point(cam, u, v, octave, d));
        m.node[k].push_back(node); m.mapPoints[k].push_back(row); m.depth[k].push_back(depth);
    };
    for (int j = 0; j < Map::nKp; ++j) add(Map::current, 640 * rng.unit(), 480 * rng.unit(), rng.below(8), random_desc(), 50u + (unsigned)rng.below(10), -1, -1.f);
    m.position.assign(Map::nMp, DeviceMapPoints::Vec3d{0, 0, 0});
    m.flags.assign(Map::nMp, 0); m.live.assign(Map::nMp, 0);
    auto project = [&](int k, const DeviceMapPoints::Vec3d &X, double &u, double &v) {
        u = 500.0 * (X[0] - 0.15 * k) / X[2] + 320.0 + 0.02 * rng.unit();
        v = 502.0 * (X[1] + 0.01 * (k % 3)) / X[2] + 240.0 + 0.02 * rng.unit();
    };
    for (int p = 0; p < Map::nPoints + Map::nExisting; ++p) {
        const bool existing = p >= Map::nPoints;
        // far: no baseline is enough | middle: 0.3 is, 0.15 is not | near
        const double z = !existing && p % 5 == 0 ? 80.0 : (!existing && p % 3 == 2 && p % 4 == 0 ? 12.0 : 2.5 + 3.0 * rng.unit());
        const DeviceMapPoints::Vec3d X{0.15 * Map::current + (rng.unit() - 0.5) * 0.5 * z, (rng.unit() - 0.5) * 0.35 * z, z};
        const KeyPoint::Descriptor d = random_desc();
        const int octave = rng.below(8), jc = existing ? 2 * (p - Map::nPoints) + 1 : 2 * p;
        const std::int32_t row = existing ? p - Map::nPoints : -1;
        double u, v;
        project(Map::current, X, u, v);
        m.keyPoints[Map::current][jc] = key_point(cam, u, v, octave, d);
        m.node[Map::current][jc] = (unsigned)(p % 8);
        m.mapPoints[Map::current][jc] = row;
        if (!existing && p % 11 == 3) m.depth[Map::current][jc] = (float)(std::sqrt((X[0] - 0.3) * (X[0] - 0.3) + X[1] * X[1] + z * z) * 1.0005);       // the depth branch of :621
        std::vector<int> seen;
        if (existing) seen = {3, 0};
        else if (p % 3 == 0) seen = {3};
        else if (p % 3 == 1) seen = {0};
        else seen = {3, 4};
        for (int k : seen) {
            project(k, X, u, v);
            add(k, u, v, octave, d, (unsigned)(p % 8), row, -1.f);
        }
        if (existing) { m.position[row] = X; m.flags[row] = 3; m.live[row] = 1; }
    }
    for (int k = 0; k < K; ++k)                              // bystanders in every other keyframe
        while (k != Map::current && (int)m.keyPoints[k].size() < 200) add(k, 640 * rng.unit(), 480 * rng.unit(), rng.below(8), random_desc(), 50u + (unsigned)rng.below(10), -1, -1.f);
    m.pool.assign((std::size_t)K * Map::stride, KeyPoint::Descriptor{});
    for (int k = 0; k < K; ++k)
        for (std::size_t j = 0; j < m.keyPoints[k].size(); ++j) m.pool[(std::size_t)m.descBase[k] + j] = m.keyPoints[k][j].descriptor;
    for (int r = Map::nMp - 1; r >= Map::firstFree; --r) m.freeRows.push_back(r);     // in descending order: not the table's
    return m;
}

struct Tables {
    DeviceMapPoints points;
    DeviceMapPointFlags flags;
    DeviceMapPointLive live;
    DeviceKeyframeMapPoints table;
    std::vector<std::unique_ptr<DeviceKeyframe>> frames;
    std::vector<DeviceKeyframe *> framePtr;
    Tables(Context &ctx, const Map &m)
        : points(ctx, m.position, std::vector<DeviceMapPoints::Vec3f>(Map::nMp, DeviceMapPoints::Vec3f{0, 0, 1}), std::vector<float>(Map::nMp, 1.f), std::vector<float>(Map::nMp, 9.f),
                 std::vector<KeyPoint::Descriptor>(Map::nMp, KeyPoint::Descriptor{})),
          flags(ctx, m.flags), live(ctx, m.live), table(ctx, Map::nKf, Map::stride, Map::nMp) {
        for (int k = 0; k < Map::nKf; ++k) {
            table.update(k, m.mapPoints[k]);
            KeyframeFeatures f;
            f.keyPoints = &m.keyPoints[k];
            for (std::size_t j = 0; j < m.keyPoints[k].size(); ++j) { f.usable.push_back(m.mapPoints[k][j] == -1); f.bowFeatureVec[m.node[k][j]].push_back((unsigned)j); }
            frames.emplace_back(new DeviceKeyframe(ctx, f));
            framePtr.push_back(frames.back().get());
        }
    }
    std::vector<unsigned char> bytes(Context &ctx, const Map &m) {       // every table and mask, one after another
        const std::size_t n = Map::nMp;
        std::vector<std::pair<const void *, std::size_t>> parts = {{points.position(), 24 * n}, {points.descriptor(), 32 * n}, {flags.flags(), n}, {live.live(), n},
                                                                   {table.table(), 4 * (std::size_t)Map::nKf * Map::stride}};
        for (int k = 0; k < Map::nKf; ++k) parts.push_back({frames[k]->mutableUsable(), m.keyPoints[k].size()});
        std::vector<unsigned char> out;
        for (const auto &part : parts) {
            std::vector<unsigned char> b(part.second);
            ctx.check(ms_dev_download(ctx.get(), b.data(), part.first, part.second), "ms_dev_download");
            out.insert(out.end(), b.begin(), b.end());
        }
        return out;
    }
};

int run() {
    const Map m = make_map();
    Parameters p;
    StaticSettings settings(p);
    Context ctx(0);
    DeviceKeyframePoses poses(ctx, m.pose);
    DeviceDescriptorPool pool(ctx, m.pool);
    DeviceKeypointTable keypoints(ctx, Map::nKf, Map::stride);
    for (int k = 0; k < Map::nKf; ++k) {
        std::vector<float> x, y; std::vector<std::int32_t> octave;
        for (const KeyPoint &kp : m.keyPoints[k]) { x.push_back(kp.pt.x); y.push_back(kp.pt.y); octave.push_back(kp.octave); }
        keypoints.update(k, x, y, octave, m.depth[k]);
    }

    // ---- the device path
    Tables dev(ctx, m);
    DeviceObservationLists lists(ctx, 4, 8);                 // small on purpose: it grows
    std::vector<std::int32_t> all;
    for (int k = 0; k < Map::nKf; ++k) all.push_back(k);
    KeyframeSlots slots = m.cams;
    slots.id = m.kfId; slots.descBase = m.descBase; slots.frames = dev.framePtr;
    DeviceArray<std::int32_t> nObs(ctx, Map::nMp);
    DeviceTrackTable tracks(ctx, Map::nMp, 0, 1);
    const std::vector<std::int32_t> track41(Map::nMp, 41);
    nObs.fill(7); ctx.check(ms_dev_upload(ctx.get(), tracks.mpTrack(), track41.data(), 4 * track41.size()), "ms_dev_upload");
    MapTables tables{dev.table, slots};
    tables.flags = &dev.flags; tables.points = &dev.points; tables.live = &dev.live; tables.keypoints = &keypoints; tables.poses = &poses; tables.pool = &pool; tables.lists = &lists;
    tables.observationCount = nObs.data(); tables.tracks = &tracks;
    unboundMasks(ctx, tables, all);                          // rewrites what the constructor uploaded; must give the same masks
    const std::vector<CreatedPoints> got = createNewMapPoints(ctx, tables, Map::current, m.adjacent, m.freeRows, settings, TriangulationMethod::TME, &m.pose);

    // ---- the restatement: Keyframe::mapPoints and std::map observations on the host, one match after the other
    Tables ref(ctx, m);
    std::vector<std::vector<std::int32_t>> mapPoints = m.mapPoints;
    std::vector<std::uint8_t> live = m.live;
    std::vector<std::int32_t> free = m.freeRows, wantObs(Map::nMp, 7), wantTrack(Map::nMp, 41);
    std::map<std::int32_t, std::int32_t> slotOfId;
    for (int k = 0; k < Map::nKf; ++k) slotOfId[m.kfId[k]] = k;
    std::size_t created = 0, angle = 0, other = 0, depthBranch = 0, secondTrip = 0, flipped = 0, emptyOrSkipped = 0, failedThenCreated = 0;
    std::vector<std::uint8_t> failedBefore(Map::nKp, 0);
    for (std::size_t a = 0; a < m.adjacent.size(); ++a) {
        const std::int32_t adj = m.adjacent[a];
        if (adj == Map::current) {                           // :281
            if (!got[a].skipped) { std::printf("the current slot was not skipped\n"); return 3; }
            ++emptyOrSkipped;
            continue;
        }
        auto rt = [&](int k, double R[9], double t[3]) { for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) R[3 * i + j] = m.pose[k][4 * i + j]; t[i] = m.pose[k][4 * i + 3]; } };
        double R1[9], t1[3], R2[9], t2[3], E[9];
        rt(Map::current, R1, t1); rt(adj, R2, t2);
        create_E_21(R2, t2, R1, t1, E);
        const std::vector<std::pair<int, int>> matches = matchForTriangulationDBoW(ctx, *ref.frames[Map::current], *ref.frames[adj], E, settings);
        TriangulateArgs args;
        args.obsStart.push_back(0);
        std::vector<std::map<std::int32_t, std::int32_t>> observations;
        for (std::size_t i = 0; i < matches.size(); ++i) {   // :282-301
            args.rows.push_back(free.at(i));
            args.wasTriangulated.push_back(0);
            observations.push_back({{m.kfId[Map::current], matches[i].first}, {m.kfId[adj], matches[i].second}});
            for (const auto &kv : observations.back()) {     // ascending KfId
                const int k = slotOfId.at(kv.first);
                const KeyPoint &kp = m.keyPoints[k][kv.second];
                args.obsKf.push_back(k); args.obsX.push_back(kp.pt.x); args.obsY.push_back(kp.pt.y); args.obsOctave.push_back(kp.octave); args.obsDepth.push_back(m.depth[k][kv.second]);
            }
            args.obsStart.push_back((std::int32_t)args.obsKf.size());
        }
        const TriangulateResult tri = triangulateMapPoints(ctx, ref.points, &ref.flags, poses, m.cams, args, settings, TriangulationMethod::TME);      // :308
        CreatedPoints want;
        for (std::size_t i = 0; i < matches.size(); ++i) {
            const std::int32_t row = args.rows[i], kp1 = matches[i].first, kp2 = matches[i].second;
            depthBranch += m.depth[Map::current][kp1] > 0;
            if (tri.status[i] == 0) { angle += tri.reason[i] == 2; other += tri.reason[i] != 2; failedBefore[kp1] = 1; continue; }       // :309
            failedThenCreated += failedBefore[kp1];
            mapPoints[Map::current][kp1] = row; mapPoints[adj][kp2] = row;                               // :310-311
            live[row] = 1; wantObs[row] = 2; wantTrack[row] = -1;
            std::vector<std::vector<KeyPoint::Descriptor>> desc(1);                                      // updateDescriptor, the general medoid
            for (const auto &kv : observations[i]) desc[0].push_back(m.keyPoints[slotOfId.at(kv.first)][kv.second].descriptor);
            const int best = updateDescriptors(ctx, desc)[0];
            if (best >= 0) ref.points.update(row, 1, nullptr, nullptr, nullptr, nullptr, &desc[0][best]);
            want.createdRows.push_back(row); want.createdKeyPoints1.push_back(kp1); want.createdKeyPoints2.push_back(kp2);
            secondTrip += kp1 >= 256; flipped += m.kfId[adj] > m.kfId[Map::current];
        }
        created += want.createdRows.size();
        emptyOrSkipped += matches.empty();
        ref.table.update(Map::current, mapPoints[Map::current]); ref.table.update(adj, mapPoints[adj]);      // kfTable.update, twice
        ref.live.update(0, Map::nMp, live.data());
        for (int k : {(int)Map::current, (int)adj}) {        // the masks of both frames
            std::vector<std::uint8_t> usable;
            for (std::int32_t r : mapPoints[k]) usable.push_back(r == -1);
            ctx.check(ms_dev_upload(ctx.get(), ref.frames[k]->mutableUsable(), usable.data(), usable.size()), "ms_dev_upload");
        }
        std::vector<std::int32_t> left;
        for (std::int32_t r : free) if (std::find(want.createdRows.begin(), want.createdRows.end(), r) == want.createdRows.end()) left.push_back(r);
        free.swap(left);
        const CreatedPoints &g = got[a];
        if (g.slot != adj || g.skipped || g.rows != args.rows || g.keyPoints1.size() != matches.size()) { std::printf("adjacent %d: the matches differ\n", adj); return 3; }
        for (std::size_t i = 0; i < matches.size(); ++i)
            if (g.keyPoints1[i] != matches[i].first || g.keyPoints2[i] != matches[i].second) { std::printf("adjacent %d: the matches differ\n", adj); return 3; }
        if (g.status != tri.status || g.reason != tri.reason) { std::printf("adjacent %d: the triangulator's results differ\n", adj); return 4; }
        if (g.createdRows != want.createdRows || g.createdKeyPoints1 != want.createdKeyPoints1 || g.createdKeyPoints2 != want.createdKeyPoints2) {
            std::printf("adjacent %d: the created points differ\n", adj);
            return 4;
        }
    }
    if (dev.bytes(ctx, m) != ref.bytes(ctx, m)) { std::printf("the tables differ\n"); return 5; }
    if (nObs.download() != wantObs || tracks.downloadMapPointTracks() != wantTrack) { std::printf("n_obs or mp_track differ\n"); return 5; }
    if (created < 20 || angle < 5 || depthBranch < 3 || secondTrip < 3 || flipped < 5 || emptyOrSkipped < 1 || failedThenCreated < 1) {
        std::printf("the map exercises too little (%zu %zu %zu %zu %zu %zu %zu %zu)\n", created, angle, other, depthBranch, secondTrip, flipped, emptyOrSkipped, failedThenCreated);
        return 6;
    }
    std::printf("createNewMapPoints ok: %zu created (%zu with the observation order flipped, %zu in the second trip, %zu after a failure), %zu angle and %zu other failures, "
                "%zu on the depth branch, tables bit-equal\n", created, flipped, secondTrip, failedThenCreated, angle, other, depthBranch);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_create_points_lists, (const void *)&ms_create_points_lists_check, (const void *)&ms_create_points_bind,
                                   (const void *)&ms_create_points_bind_check, (const void *)&ms_unbound_mask, (const void *)&ms_unbound_mask_check};
    std::printf("link ok %d\n", syms[0] && syms[1] && syms[2] && syms[3] && syms[4] && syms[5]);
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    try {
        return run();
    } catch (const std::exception &e) {
        std::printf("failed: %s\n", e.what());
        return 2;
    }
}
