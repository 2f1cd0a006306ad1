// Compile + link check of the observation-list part of the host mirror (mi355slam/map_tables.hpp and map_update.hpp: DeviceKeypointTable,
// DeviceObservationLists, updateMapPoints, retriangulateCurrent) against libmi355slam.so, and its run on one small map.
//   obs_lists_smoke --no-gpu    the symbols link; a few calls of ms_observation_lists_check (no context, no device)
//   obs_lists_smoke --baseline MAP K S M SLOT   the one-core baseline tools/obs_lists_probe.py times, on the map file of map_cull_smoke
//                               --baseline (K slots of S entries, M rows): building std::map<KfId, KpId> observations of every map point from
//                               the keyframes, then walking them into the CSR lists of two selections (the usable map points of SLOT; every
//                               observed row of the map).  Best of three each; prints the times and a checksum of the lists.
//   obs_lists_smoke             mapper_helpers.cpp:1062-1092 twice on copies of one seeded map: through updateMapPoints / retriangulateCurrent
//                               (lists built on the device, nothing per point on the host), and through a sequential restatement that keeps
//                               `std::map<KfId, KpId> observations` per map point as the reference does, walks it for every row and hands
//                               the host lists to DeviceMapPoints::refresh / triangulateMapPoints.  The tables must agree bit for bit.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

int no_gpu() {
    char why[256] = {0};
    const std::int32_t kfMp[6] = {0, 1, -1, 2, 0, 5}, kfId[2] = {4, 2}, base[2] = {0, 3};
    const auto *dev = reinterpret_cast<std::int32_t *>(0x1000);       // never dereferenced by the validation
    const auto *devf = reinterpret_cast<float *>(0x1000);
    ms_obs_lists l{};
    l.rows = const_cast<std::int32_t *>(dev); l.obs_start = const_cast<std::int32_t *>(dev);
    std::int32_t nRows = 0, nObs = 0;
    ms_obs_select sel{MS_OBS_FROM_SLOT, MS_OBS_ALL, 0, 1, nullptr, 0};
    auto check = [&](const std::int32_t *ids, int stride) {
        return ms_observation_lists_check(kfMp, 2, stride, 6, ids, nullptr, devf, devf, dev, devf, base, &sel, 8, &l, 4, 4, &nRows, &nObs, why, sizeof(why));
    };
    if (check(kfId, 3) != MS_OK) { std::printf("a valid call was rejected: %s\n", why); return 1; }
    int cases = 0;
    const std::int32_t twice[2] = {4, 4}, empty[2] = {4, -1};
    sel.slot = 2;                       cases += check(kfId, 3) == MS_ERR_INVALID && why[0]; sel.slot = 1;
    cases += check(empty, 3) == MS_ERR_INVALID && why[0];
    cases += check(twice, 3) == MS_ERR_INVALID && why[0];
    cases += check(kfId, 0) == MS_ERR_INVALID && why[0];
    sel.filter = MS_OBS_REFRESH;        cases += check(kfId, 3) == MS_ERR_INVALID && why[0]; sel.filter = MS_OBS_ALL;
    sel.source = 7;                     cases += check(kfId, 3) == MS_ERR_INVALID && why[0];
    if (cases != 6) { std::printf("%d of 6 invalid calls were rejected\n", cases); return 1; }
    std::printf("no-gpu ok %d cases\n", cases);
    return 0;
}

// ---- --baseline -----------------------------------------------------------------------------------------------------------------------
struct Csr {
    std::vector<std::int32_t> rows, start{0}, kf, kp;
    unsigned long long sum() const {                         // order-sensitive, wraps in 64 bits (the probe forms the same sum of the device lists)
        unsigned long long s = 0;
        for (std::size_t i = 0; i < rows.size(); ++i) s += (unsigned long long)(i + 1) * (unsigned long long)(rows[i] + 1);
        for (std::size_t o = 0; o < kf.size(); ++o) s += (unsigned long long)(o + 1) * (unsigned long long)(kf[o] * 8192 + kp[o] + 1);
        return s;
    }
};

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

int baseline(const char *path, int nKf, int stride, int nMp, int slot) {
    std::vector<std::int32_t> kfMp((std::size_t)nKf * stride), kfId(nKf);
    std::vector<std::uint8_t> flags(nMp), live(nMp);
    std::FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(kfMp.data(), 4, kfMp.size(), f) != kfMp.size() || std::fread(flags.data(), 1, flags.size(), f) != flags.size() ||
        std::fread(live.data(), 1, live.size(), f) != live.size() || std::fread(kfId.data(), 4, kfId.size(), f) != kfId.size()) {
        std::printf("cannot read %s\n", path);
        return 2;
    }
    std::fclose(f);
    std::int32_t maxId = 0;
    for (std::int32_t id : kfId) maxId = std::max(maxId, id);
    std::vector<std::int32_t> slotOfId((std::size_t)maxId + 1, -1);
    for (int k = 0; k < nKf; ++k) if (kfId[k] >= 0) slotOfId[kfId[k]] = k;
    std::vector<std::map<std::int32_t, std::int32_t>> observations;
    double buildMs = 1e30, walkMs[2] = {1e30, 1e30};
    Csr lists[2];
    for (int rep = 0; rep < 3; ++rep) {
        auto t0 = std::chrono::steady_clock::now();
        observations.assign(nMp, {});                        // MapPoint::observations of every row, by walking the keyframes (addObservation)
        for (int k = 0; k < nKf; ++k) {
            if (kfId[k] < 0) continue;
            for (int j = 0; j < stride; ++j) {
                const std::int32_t r = kfMp[(std::size_t)k * stride + j];
                if (r >= 0 && r < nMp) observations[r][kfId[k]] = j;
            }
        }
        buildMs = std::min(buildMs, ms_since(t0));
        for (int which = 0; which < 2; ++which) {
            t0 = std::chrono::steady_clock::now();
            Csr c;
            auto take = [&](std::int32_t r) {
                c.rows.push_back(r);
                for (const auto &kv : observations[r]) { c.kf.push_back(slotOfId[kv.first]); c.kp.push_back(kv.second); }
                c.start.push_back((std::int32_t)c.kf.size());
            };
            if (which == 0) {                                // the loop of mapper_helpers.cpp:1062: the slot's usable map points
                for (int j = 0; j < stride; ++j) {
                    const std::int32_t r = kfMp[(std::size_t)slot * stride + j];
                    if (r >= 0 && r < nMp && (flags[r] & 2)) take(r);
                }
            } else {                                         // a whole-map pass: every row somebody observes
                for (std::int32_t r = 0; r < nMp; ++r) if (!observations[r].empty()) take(r);
            }
            walkMs[which] = std::min(walkMs[which], ms_since(t0));
            lists[which] = std::move(c);
        }
    }
    std::printf("baseline build_ms %.3f slot_walk_ms %.3f slot_rows %zu slot_obs %zu slot_sum %llu whole_walk_ms %.3f whole_rows %zu whole_obs %zu whole_sum %llu\n", buildMs,
                walkMs[0], lists[0].rows.size(), lists[0].kf.size(), lists[0].sum(), walkMs[1], lists[1].rows.size(), lists[1].kf.size(), lists[1].sum());
    return 0;
}

struct Rng {                             // a fixed sequence: the same map on every run
    std::uint64_t s = 0x9E3779B97F4A7C15ull;
    std::uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (std::uint32_t)(s >> 33); }
    double unit() { return next() / 2147483648.0; }
    int below(int n) { return (int)(next() % (std::uint32_t)n); }
};

struct Map {
    static constexpr int nKf = 14, stride = 48, nMp = 220, current = 11, emptySlot = 4, noDescSlot = 7;
    std::vector<std::vector<std::int32_t>> mapPoints;        // Keyframe::mapPoints per slot
    std::vector<std::int32_t> kfId, descBase;
    std::vector<std::vector<float>> x, y, depth;
    std::vector<std::vector<std::int32_t>> octave;
    std::vector<DeviceKeyframePoses::Pose> pose;
    KeyframeSlots cams;                      // camera and focalLength; the view's id and descBase are kfId and descBase above
    std::vector<DeviceMapPoints::Vec3d> position;
    std::vector<std::uint8_t> flags;
    std::vector<KeyPoint::Descriptor> pool;
};

Map make_map() {
    Map m;
    Rng rng;
    m.mapPoints.assign(Map::nKf, {}); m.x.assign(Map::nKf, {}); m.y.assign(Map::nKf, {}); m.depth.assign(Map::nKf, {}); m.octave.assign(Map::nKf, {});
    for (int k = 0; k < Map::nKf; ++k) {                     // cameras 0.15 apart along x, looking down +z
        m.pose.push_back({1, 0, 0, -0.15 * k, 0, 1, 0, 0.01 * (k % 3), 0, 0, 1, 0});
        m.cams.camera.push_back(ms_pinhole{500.0, 502.0, 320.0, 240.0, 640, 480});
        m.cams.focalLength.push_back(500);
        m.kfId.push_back(k == Map::emptySlot ? -1 : (k == 2 ? 100 : 3 * k + 1));       // slot 2 holds the NEWEST id: id order is not slot order
        m.descBase.push_back(k == Map::noDescSlot ? -1 : k * Map::stride);
    }
    for (int r = 0; r < Map::nMp; ++r) {
        const DeviceMapPoints::Vec3d X{rng.unit() * 3.0 - 0.5, rng.unit() * 2.0 - 1.0, 4.0 + rng.unit() * 6.0};
        m.position.push_back({X[0] + 0.05 * rng.unit(), X[1], X[2] + 0.2 * rng.unit()});         // what the row holds on entry
        m.flags.push_back((std::uint8_t)rng.below(4));
        if (r >= 200) continue;                              // rows nobody observes
        const int n = 1 + rng.below(6), k0 = rng.below(Map::nKf);
        for (int k = k0; k < std::min(k0 + n, (int)Map::nKf); ++k) {
            if ((int)m.mapPoints[k].size() >= Map::stride - 2) continue;
            if (rng.below(5) == 0) { m.mapPoints[k].push_back(-1); m.x[k].push_back(0); m.y[k].push_back(0); m.depth[k].push_back(-1); m.octave[k].push_back(0); }
            const double xc = X[0] - 0.15 * k, yc = X[1] + 0.01 * (k % 3);
            m.mapPoints[k].push_back(r);
            m.x[k].push_back((float)(500.0 * xc / X[2] + 320.0 + 0.1 * rng.unit()));
            m.y[k].push_back((float)(502.0 * yc / X[2] + 240.0 + 0.1 * rng.unit()));
            m.depth[k].push_back(rng.below(4) == 0 ? (float)std::sqrt(xc * xc + yc * yc + X[2] * X[2]) : -1.0f);
            m.octave[k].push_back(rng.below(8));
        }
    }
    m.pool.resize((std::size_t)Map::nKf * Map::stride);
    for (auto &d : m.pool) for (auto &w : d) w = rng.next() & 0x0F0F0F0Fu;       // close descriptors: the medoids are contested
    return m;
}

struct Tables {
    DeviceMapPoints points;
    DeviceMapPointFlags flags;
    Tables(Context &ctx, const Map &m)
        : points(ctx, m.position, std::vector<DeviceMapPoints::Vec3f>(Map::nMp, DeviceMapPoints::Vec3f{0.f, 0.f, 1.f}), std::vector<float>(Map::nMp, 1.f),
                 std::vector<float>(Map::nMp, 2.f), std::vector<KeyPoint::Descriptor>(Map::nMp, KeyPoint::Descriptor{})),
          flags(ctx, m.flags) {}
    std::vector<unsigned char> bytes(Context &ctx) {         // every table, one after another
        const std::size_t n = Map::nMp, sizes[6] = {24 * n, 12 * n, 4 * n, 4 * n, 32 * n, n};
        const void *src[6] = {points.position(), points.norm(), points.minDistance(), points.maxDistance(), points.descriptor(), flags.flags()};
        std::vector<unsigned char> out;
        for (int i = 0; i < 6; ++i) {
            std::vector<unsigned char> part(sizes[i]);
            ctx.check(ms_dev_download(ctx.get(), part.data(), src[i], sizes[i]), "ms_dev_download");
            out.insert(out.end(), part.begin(), part.end());
        }
        return out;
    }
};

int gpu() {
    const Map m = make_map();
    Parameters p;
    StaticSettings settings(p);
    const int minObservationsForBA = 3;
    Context ctx(0);
    DeviceKeyframePoses poses(ctx, m.pose);
    DeviceDescriptorPool pool(ctx, m.pool);
    DeviceKeyframeMapPoints table(ctx, Map::nKf, Map::stride, Map::nMp);
    DeviceKeypointTable keypoints(ctx, Map::nKf, Map::stride);
    for (int k = 0; k < Map::nKf; ++k) { table.update(k, m.mapPoints[k]); keypoints.update(k, m.x[k], m.y[k], m.octave[k], m.depth[k]); }

    // ---- the device path: no per-point structure on the host
    Tables dev(ctx, m);
    DeviceObservationLists lists(ctx, 4, 8);                 // small on purpose: the first call regrows
    KeyframeSlots slots = m.cams;
    slots.id = m.kfId; slots.descBase = m.descBase;
    MapTables tables{table, slots};
    tables.flags = &dev.flags; tables.points = &dev.points; tables.keypoints = &keypoints; tables.poses = &poses; tables.pool = &pool; tables.lists = &lists;
    const std::size_t refreshed = updateMapPoints(ctx, tables, Map::current, minObservationsForBA, settings);
    const TriangulateResult devTri = retriangulateCurrent(ctx, tables, Map::current, settings, TriangulationMethod::TME);
    const std::vector<std::int32_t> devRows = lists.download(lists.lists().rows, lists.rowCount());

    // ---- the restatement: std::map<KfId, KpId> observations per map point, built by walking the keyframes as addObservation does
    std::vector<std::map<std::int32_t, std::int32_t>> observations(Map::nMp);
    std::map<std::int32_t, std::int32_t> slotOfId;
    for (int k = 0; k < Map::nKf; ++k) {
        if (m.kfId[k] < 0) continue;                         // a removed keyframe: its observations were erased with it
        slotOfId[m.kfId[k]] = k;
        for (std::size_t j = 0; j < m.mapPoints[k].size(); ++j)
            if (m.mapPoints[k][j] != -1) observations[m.mapPoints[k][j]][m.kfId[k]] = (std::int32_t)j;
    }
    Tables ref(ctx, m);
    std::vector<std::uint8_t> status = m.flags;
    {                                                        // :1062-1077
        std::vector<std::int32_t> rows, firstOctave;
        std::vector<std::vector<MapObservation>> obs;
        for (std::int32_t r : m.mapPoints[Map::current]) {
            if (r == -1) continue;
            if (!(status[r] & DeviceMapPointFlags::USABLE)) continue;
            rows.push_back(r);
            obs.emplace_back();
            for (const auto &kv : observations[r]) {
                const std::int32_t k = slotOfId.at(kv.first);
                obs.back().push_back(MapObservation{k, m.descBase[k] < 0 ? -1 : m.descBase[k] + kv.second});
            }
            const auto &first = *observations[r].begin();
            firstOctave.push_back(m.octave[slotOfId.at(first.first)][first.second]);
        }
        if (rows.size() != refreshed) { std::printf("%zu rows refreshed, the restatement has %zu\n", refreshed, rows.size()); return 3; }
        ref.points.refresh(ctx, poses, rows, obs, firstOctave, settings, &pool);
        for (std::int32_t r : rows) status[r] = (int)observations[r].size() >= minObservationsForBA ? 3 : 2;
        ref.flags.update(0, Map::nMp, status.data());
    }
    TriangulateArgs args;                                    // :1085-1092
    args.obsStart.push_back(0);
    for (std::int32_t r : m.mapPoints[Map::current]) {
        if (r == -1) continue;
        if (!((status[r] & DeviceMapPointFlags::TRIANGULATED) == 0 || observations[r].size() >= 2)) continue;
        args.rows.push_back(r);
        args.wasTriangulated.push_back((status[r] & DeviceMapPointFlags::USABLE) != 0);
        for (const auto &kv : observations[r]) {
            const std::int32_t k = slotOfId.at(kv.first);
            args.obsKf.push_back(k); args.obsX.push_back(m.x[k][kv.second]); args.obsY.push_back(m.y[k][kv.second]);
            args.obsOctave.push_back(m.octave[k][kv.second]); args.obsDepth.push_back(m.depth[k][kv.second]);
        }
        args.obsStart.push_back((std::int32_t)args.obsKf.size());
    }
    const TriangulateResult refTri = triangulateMapPoints(ctx, ref.points, &ref.flags, poses, m.cams, args, settings, TriangulationMethod::TME);

    if (devRows != args.rows) { std::printf("the re-triangulated rows differ (%zu against %zu)\n", devRows.size(), args.rows.size()); return 4; }
    if (devTri.status != refTri.status || devTri.reason != refTri.reason || devTri.passCount != refTri.passCount) { std::printf("status, reason or pass count differ\n"); return 4; }
    if (dev.bytes(ctx) != ref.bytes(ctx)) { std::printf("the tables differ\n"); return 5; }
    std::size_t triangulated = 0;
    for (std::uint8_t s : devTri.status) triangulated += s != 0;
    if (refreshed < 5 || args.rows.size() < 5 || triangulated < 2) { std::printf("the map exercises too little (%zu, %zu, %zu)\n", refreshed, args.rows.size(), triangulated); return 6; }
    std::printf("obs lists ok: %zu refreshed, %zu re-triangulated (%zu succeeded), tables bit-equal\n", refreshed, args.rows.size(), triangulated);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_observation_lists, (const void *)&ms_observation_lists_check, (const void *)&ms_triangulate_lists,
                                   (const void *)&ms_map_refresh_lists};
    std::printf("link ok %d\n", syms[0] && syms[1] && syms[2] && syms[3]);
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    if (argc > 6 && std::strcmp(argv[1], "--baseline") == 0) return baseline(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
    try {
        return gpu();
    } catch (const std::exception &e) {
        std::printf("failed: %s\n", e.what());
        return 2;
    }
}
