// Compile + link check of the map-graph queries of the host mirror (DeviceKeyframeMapPoints, getNeighbors, computeAdjacentKeyframes,
// localMapPoints in mi355slam/map_tables.hpp and map_update.hpp) against libmi355slam.so (tests/test_covis_abi.py), their comparison with a sequential
// std::map / std::set restatement of the reference's loops, and the one-core baseline tools/covis_probe.py times the device path against.
//   covis_smoke --no-gpu                 every MS_ERR_INVALID case of ms_covisibility / ms_map_point_union through their _check halves (no
//                                        context, no device), and the restatement below on a hand-computed map
//   covis_smoke --gpu                    each mirror against the restatement (tests/test_gpu_covis.py)
//   covis_smoke --baseline K S M Q U [F] the restatement on one core for K slots of S entries over M rows: Q getNeighbors calls and one
//                                        union of U slots with owners; prints the best of three in milliseconds and a checksum of each result,
//                                        and writes the table (int32 [K * S]) to the file F so that the device path can run on the same map
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

// ---- the reference's map graph and loops, sequentially --------------------------------------------------------------------------------
struct HostMap {
    std::vector<std::vector<std::int32_t>> mapPoints;        // Keyframe::mapPoints per slot (-1 = none)
    std::vector<std::map<std::int32_t, int>> observations;   // MapPoint::observations per row: slot -> keypoint
    std::vector<std::uint8_t> flags;
    KeyframeSlots chain;
    void link() {
        observations.assign(flags.size(), {});
        for (std::size_t k = 0; k < mapPoints.size(); ++k)
            for (std::size_t j = 0; j < mapPoints[k].size(); ++j)
                if (mapPoints[k][j] != -1) observations[mapPoints[k][j]].emplace((std::int32_t)k, (int)j);
    }
};

// Keyframe::getNeighbors, keyframe.cpp:192-230
std::vector<std::int32_t> get_neighbors(const HostMap &M, std::int32_t id, std::int32_t previous, std::int32_t next, int minCovisibilities, bool triangulatedOnly) {
    std::map<std::int32_t, int> covisibilities;
    if (previous != -1) covisibilities.emplace(previous, minCovisibilities);
    if (next != -1) covisibilities.emplace(next, minCovisibilities);
    for (std::int32_t mp : M.mapPoints[id]) {
        if (mp == -1) continue;
        if (triangulatedOnly && !(M.flags[mp] & DeviceMapPointFlags::TRIANGULATED)) continue;
        for (const auto &kfKp : M.observations[mp]) {
            if (covisibilities.count(kfKp.first)) covisibilities[kfKp.first]++;
            else covisibilities[kfKp.first] = 1;
        }
    }
    std::vector<std::int32_t> res;
    for (const auto &kfObs : covisibilities)
        if (kfObs.first != id && kfObs.second >= minCovisibilities) res.push_back(kfObs.first);
    return res;
}

// computeAdjacentKeyframes, mapper_helpers.cpp:144-216
std::vector<std::int32_t> compute_adjacent(const HostMap &M, std::int32_t current, int minCovisibilities, int maxKeyframes) {
    std::set<std::int32_t> adjacentSet, parents;
    int i = 0;
    for (std::int32_t backwards = current; backwards != -1;) {
        adjacentSet.insert(backwards);
        if (i % 2 == 0)
            for (std::int32_t k : get_neighbors(M, backwards, M.chain.previous[backwards], M.chain.next[backwards], minCovisibilities, false)) parents.insert(k);
        if (++i >= maxKeyframes) break;
        backwards = M.chain.previous[backwards];
    }
    for (std::int32_t parent : parents) {
        std::int32_t backwards = parent;
        i = 0;
        while (backwards != -1) {
            adjacentSet.insert(backwards);
            if (++i >= maxKeyframes / 2) break;
            backwards = M.chain.previous[backwards];
        }
        std::int32_t forwards = parent;
        i = 0;
        while (forwards != -1) {
            adjacentSet.insert(forwards);
            if (++i >= maxKeyframes / 2) break;
            forwards = M.chain.next[forwards];
        }
    }
    adjacentSet.erase(current);
    std::vector<std::int32_t> adjacent(adjacentSet.begin(), adjacentSet.end());
    const auto &c = M.chain.cameraCenter[current];
    auto dist2 = [&](std::int32_t k) {
        const auto &p = M.chain.cameraCenter[k];
        const double x = p[0] - c[0], y = p[1] - c[1], z = p[2] - c[2];
        return x * x + (y * y + z * z);
    };
    std::sort(adjacent.begin(), adjacent.end(), [&](std::int32_t a, std::int32_t b) { return dist2(a) < dist2(b); });
    if ((int)adjacent.size() > maxKeyframes) adjacent.erase(adjacent.begin() + maxKeyframes, adjacent.end());
    return adjacent;
}

// localMps of matchLocalMapPoints (mapper_helpers.cpp:241-261) without the frustum test
std::vector<std::int32_t> local_mps(const HostMap &M, const std::vector<std::int32_t> &adjacent, std::int32_t current) {
    std::set<std::int32_t> uniqueMps;
    for (std::int32_t k : adjacent)
        for (std::int32_t mp : M.mapPoints[k]) if (mp != -1) uniqueMps.insert(mp);
    std::vector<std::int32_t> localMps;
    for (std::int32_t mp : uniqueMps)
        if ((M.flags[mp] & DeviceMapPointFlags::USABLE) && !M.observations[mp].count(current)) localMps.push_back(mp);
    return localMps;
}

// localMapPoints of correctLoop (loop_closer.cpp:418-433, :465-469): the first keyframe of the list wins
std::map<std::int32_t, std::int32_t> loop_map_points(const HostMap &M, const std::vector<std::int32_t> &keyframes) {
    std::map<std::int32_t, std::int32_t> localMapPoints;
    for (std::size_t p = 0; p < keyframes.size(); ++p)
        for (std::int32_t mp : M.mapPoints[keyframes[p]]) if (mp != -1) localMapPoints.emplace(mp, (std::int32_t)p);
    return localMapPoints;
}

// a chain of keyframes walking along a line; every row is seen by up to maxObs consecutive keyframes (and, for every 16th row, by a
// keyframe far behind as well: the loop that makes a parent outside the chain's tail)
HostMap make_map(unsigned seed, int nKf, int stride, int nMp, int maxObs) {
    std::mt19937 rng(seed);
    HostMap M;
    M.mapPoints.assign(nKf, {});
    M.flags.resize(nMp);
    for (auto &f : M.flags) f = (std::uint8_t)(rng() % 4);
    for (int r = 0; r < nMp; ++r) {
        const int n = 1 + (int)(rng() % (unsigned)maxObs), k0 = (int)(rng() % (unsigned)nKf);
        for (int k = k0; k < std::min(k0 + n, nKf); ++k)
            if ((int)M.mapPoints[k].size() < stride) M.mapPoints[k].push_back(r);
        const int far = (k0 + nKf / 2) % nKf;
        if (r % 16 == 0 && (far < k0 || far >= k0 + n) && (int)M.mapPoints[far].size() < stride) M.mapPoints[far].push_back(r);
    }
    for (auto &l : M.mapPoints) {
        l.resize(stride, -1);
        std::shuffle(l.begin(), l.end(), rng);
    }
    if (nKf > 13) M.mapPoints[13].assign(stride, -1);
    M.chain.previous.resize(nKf); M.chain.next.resize(nKf); M.chain.cameraCenter.resize(nKf);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    for (int k = 0; k < nKf; ++k) {
        M.chain.previous[k] = k - 1;
        M.chain.next[k] = k + 1 < nKf ? k + 1 : -1;
        M.chain.cameraCenter[k] = {0.3 * k + 0.2 * U(rng), U(rng), 3.0 * std::sin(0.2 * k) + 0.2 * U(rng)};
    }
    M.link();
    return M;
}

// ---- --no-gpu -------------------------------------------------------------------------------------------------------------------------
int no_gpu() {
    if (ms_covisibility(nullptr, nullptr, 0, 1, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr) != MS_ERR_INVALID ||
        ms_map_point_union(nullptr, nullptr, 0, 1, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr) != MS_ERR_INVALID) {
        std::printf("a call without a context must fail with MS_ERR_INVALID\n");
        return 1;
    }
    // the checks read the HOST arrays only: the device arrays are stand-in addresses that are never followed
    const std::int32_t *dtab = reinterpret_cast<const std::int32_t *>(0x1000), *dout = reinterpret_cast<const std::int32_t *>(0x3000);
    const std::uint8_t *dflags = reinterpret_cast<const std::uint8_t *>(0x2000);
    char why[256];
    int cases = 0;
    auto rejected = [&](int rc, const char *what) {
        ++cases;
        if (rc == MS_ERR_INVALID && why[0]) return true;
        std::printf("%s: returned %d (%s), expected MS_ERR_INVALID with a message\n", what, rc, why);
        return false;
    };
    struct C { std::vector<ms_covis_query> q{{2, 1, 3, 5, 0}, {0, -1, 1, -3, 1}, {4, 3, -1, 0, 0}}; int nKf = 5, stride = 8, nMp = 20; std::vector<std::int32_t> n{0, 0, 0}; };
    auto covis = [&](const C &c, const std::int32_t *tab = reinterpret_cast<const std::int32_t *>(0x1000), const std::uint8_t *fl = reinterpret_cast<const std::uint8_t *>(0x2000),
                     const std::int32_t *nb = reinterpret_cast<const std::int32_t *>(0x3000), bool noQ = false, bool noN = false) {
        why[0] = 0;
        return ms_covisibility_check(tab, c.nKf, c.stride, fl, c.nMp, noQ ? nullptr : c.q.data(), (int)c.q.size(), nb, noN ? nullptr : c.n.data(), why, sizeof(why));
    };
    C cok;
    if (covis(cok) != MS_OK) { std::printf("valid queries were rejected: %s\n", why); return 1; }
    { C c; c.q.clear(); c.n.clear(); if (covis(c, nullptr, nullptr, nullptr) != MS_OK) { std::printf("n_q = 0 was rejected: %s\n", why); return 1; } }
    { C c; c.nMp = 0; if (covis(c) != MS_OK) { std::printf("n_mp = 0 was rejected: %s\n", why); return 1; } }
    { C c; c.q[1].require = 0; if (covis(c, dtab, nullptr) != MS_OK) { std::printf("queries without flags were rejected: %s\n", why); return 1; } }
    bool good = true;
    { C c; c.q[0].slot = 5; good &= rejected(covis(c), "slot beyond the table"); }
    { C c; c.q[2].slot = -1; good &= rejected(covis(c), "slot -1"); }
    { C c; c.q[0].force_a = 5; good &= rejected(covis(c), "forced slot beyond the table"); }
    { C c; c.q[1].force_b = -2; good &= rejected(covis(c), "forced slot -2"); }
    { C c; c.q[1].force_a = -2; good &= rejected(covis(c), "first forced slot -2"); }
    { C c; c.stride = 0; good &= rejected(covis(c), "stride 0"); }
    { C c; c.stride = -8; good &= rejected(covis(c), "negative stride"); }
    { C c; c.nMp = -1; good &= rejected(covis(c), "negative n_mp"); }
    { C c; c.nKf = -1; good &= rejected(covis(c), "negative n_kf"); }
    good &= rejected(covis(cok, dtab, nullptr), "require without flags");
    good &= rejected(covis(cok, nullptr), "missing table");
    good &= rejected(covis(cok, dtab, dflags, nullptr), "missing neighbours");
    good &= rejected(covis(cok, dtab, dflags, dout, true), "missing queries");
    good &= rejected(covis(cok, dtab, dflags, dout, false, true), "missing n_neighbours");
    why[0] = 0;
    good &= rejected(ms_covisibility_check(dtab, 5, 8, dflags, 20, cok.q.data(), -1, dout, cok.n.data(), why, sizeof(why)), "negative n_q");
    const int covisCases = cases;
    cases = 0;
    struct U { std::vector<std::int32_t> list{3, 1, 1, 4, 0, 2}; std::vector<ms_union_problem> p{{0, 4, 2, 2}, {4, 2, -1, 0}, {6, 0, 0, 1}}; int nKf = 5, stride = 8, nMp = 20; std::vector<std::int32_t> n{0, 0, 0}; };
    auto uni = [&](const U &u, const std::int32_t *tab = reinterpret_cast<const std::int32_t *>(0x1000), const std::uint8_t *fl = reinterpret_cast<const std::uint8_t *>(0x2000),
                   const std::int32_t *rows = reinterpret_cast<const std::int32_t *>(0x3000), bool noList = false, bool noP = false, bool noN = false) {
        why[0] = 0;
        return ms_map_point_union_check(tab, u.nKf, u.stride, fl, u.nMp, noList ? nullptr : u.list.data(), (int)u.list.size(), noP ? nullptr : u.p.data(), (int)u.p.size(), rows,
                                        noN ? nullptr : u.n.data(), why, sizeof(why));
    };
    U uok;
    if (uni(uok) != MS_OK) { std::printf("valid unions were rejected: %s\n", why); return 1; }
    { U u; u.p.clear(); u.n.clear(); if (uni(u, nullptr, nullptr, nullptr) != MS_OK) { std::printf("n_u = 0 was rejected: %s\n", why); return 1; } }
    { U u; u.nMp = 0; if (uni(u) != MS_OK) { std::printf("n_mp = 0 was rejected: %s\n", why); return 1; } }
    { U u; u.list.clear(); u.p = {{0, 0, -1, 0}}; u.n = {0}; if (uni(u, dtab, dflags, dout, true) != MS_OK) { std::printf("an empty list was rejected: %s\n", why); return 1; } }
    { U u; u.list[1] = 5; good &= rejected(uni(u), "listed slot beyond the table"); }
    { U u; u.list[5] = -1; good &= rejected(uni(u), "listed slot -1"); }
    { U u; u.p[0].count = 7; good &= rejected(uni(u), "slice beyond the list"); }
    { U u; u.p[1].first = -1; good &= rejected(uni(u), "negative slice start"); }
    { U u; u.p[1].count = -1; good &= rejected(uni(u), "negative slice length"); }
    { U u; u.p[2].first = 7; good &= rejected(uni(u), "empty slice beyond the list"); }
    { U u; u.p[1].first = 0x7fffffff; u.p[1].count = 2; good &= rejected(uni(u), "slice whose end overflows"); }
    { U u; u.p[0].exclude_slot = 5; good &= rejected(uni(u), "exclude slot beyond the table"); }
    { U u; u.p[1].exclude_slot = -2; good &= rejected(uni(u), "exclude slot -2"); }
    { U u; u.stride = 0; good &= rejected(uni(u), "stride 0"); }
    { U u; u.nMp = -3; good &= rejected(uni(u), "negative n_mp"); }
    good &= rejected(uni(uok, dtab, nullptr), "require without flags");
    good &= rejected(uni(uok, nullptr), "missing table");
    good &= rejected(uni(uok, dtab, dflags, nullptr), "missing rows");
    good &= rejected(uni(uok, dtab, dflags, dout, true), "missing list");
    good &= rejected(uni(uok, dtab, dflags, dout, false, true), "missing problems");
    good &= rejected(uni(uok, dtab, dflags, dout, false, false, true), "missing n_rows");
    if (!good) return 1;
    // three keyframes in a chain: 0 sees rows {0, 1, 2}, 1 sees {1, 2, 3}, 2 sees {3}; row 2 is not triangulated
    HostMap M;
    M.mapPoints = {{0, -1, 1, 2}, {2, 3, 1, -1}, {-1, -1, 3, -1}};
    M.flags = {3, 3, 2, 3};
    M.chain.previous = {-1, 0, 1}; M.chain.next = {1, 2, -1};
    M.link();
    const bool restated = get_neighbors(M, 0, -1, -1, 2, false) == std::vector<std::int32_t>{1} && get_neighbors(M, 0, -1, -1, 2, true).empty() &&
                          get_neighbors(M, 0, -1, 2, 9, false) == std::vector<std::int32_t>{2} && get_neighbors(M, 1, 0, 2, 1, false) == std::vector<std::int32_t>{0, 2} &&
                          get_neighbors(M, 2, 2, -1, -4, false) == std::vector<std::int32_t>{1} && local_mps(M, {0, 1}, 2) == std::vector<std::int32_t>{0, 1, 2} &&
                          loop_map_points(M, {1, 0, 1}) == std::map<std::int32_t, std::int32_t>{{0, 1}, {1, 0}, {2, 0}, {3, 0}};
    if (!restated) { std::printf("restatement: the hand-computed map differs\n"); return 1; }
    std::printf("no-gpu ok %d covis cases %d union cases\n", covisCases, cases);
    return 0;
}

// ---- --gpu ----------------------------------------------------------------------------------------------------------------------------
int gpu() {
    Context ctx(0);
    const int nKf = 90, stride = 120, nMp = 1500;
    HostMap M = make_map(29, nKf, stride, nMp, 8);
    DeviceKeyframeMapPoints table(ctx, nKf, stride, nMp);
    for (int k = 0; k < nKf; ++k) table.update(k, M.mapPoints[k]);
    DeviceMapPointFlags flags(ctx, M.flags);
    // update() turns away what the kernels would only ignore, and leaves the slot as it was
    int turnedAway = 0;
    for (std::int32_t bad : {-2, nMp, nMp + 1, (std::int32_t)0x7fffffff, (std::int32_t)0x80000000}) {
        try { table.update(5, {1, bad, 2}); } catch (const std::invalid_argument &) { ++turnedAway; }
    }
    try { table.update(nKf, {}); } catch (const std::invalid_argument &) { ++turnedAway; }
    try { table.update(0, std::vector<std::int32_t>(stride + 1, -1)); } catch (const std::invalid_argument &) { ++turnedAway; }
    if (turnedAway != 7) { std::printf("update: %d of 7 bad calls were turned away\n", turnedAway); return 2; }
    // getNeighbors: every slot x thresholds x triangulatedOnly, in one call per combination
    std::size_t lists = 0, longest = 0, empty = 0;
    for (int minCovis : {-3, 0, 1, 5, 15})
        for (bool tri : {false, true}) {
            std::vector<NeighborQuery> q;
            for (int k = 0; k < nKf; ++k) q.push_back({k, k % 3 == 2 ? -1 : M.chain.previous[k], M.chain.next[k], minCovis, tri});
            const auto got = getNeighbors(ctx, table, &flags, q);
            for (int k = 0; k < nKf; ++k) {
                if (got[k] != get_neighbors(M, k, q[k].previous, q[k].next, minCovis, tri)) { std::printf("getNeighbors differs: slot %d minCovis %d tri %d\n", k, minCovis, (int)tri); return 3; }
                ++lists; longest = std::max(longest, got[k].size()); empty += got[k].empty();
            }
        }
    if (longest < 10) { std::printf("getNeighbors: the longest list has %zu entries\n", longest); return 3; }
    std::printf("getNeighbors ok %zu lists longest %zu empty %zu\n", lists, longest, empty);
    // a removed keyframe
    HostMap R = M;
    R.mapPoints[40].assign(stride, -1); R.link();
    table.clear(40);
    {
        std::vector<NeighborQuery> q;
        for (int k = 36; k < 45; ++k) q.push_back({k, -1, -1, 1, false});
        const auto got = getNeighbors(ctx, table, nullptr, q);
        for (std::size_t i = 0; i < q.size(); ++i)
            if (got[i] != get_neighbors(R, q[i].slot, -1, -1, 1, false)) { std::printf("getNeighbors differs after clear(40): slot %d\n", q[i].slot); return 4; }
    }
    table.update(40, M.mapPoints[40]);
    std::printf("update ok %d turned away\n", turnedAway);
    // computeAdjacentKeyframes from several keyframes, thresholds and sizes
    MapTables tables{table, M.chain};
    tables.flags = &flags;
    std::size_t adjacentTotal = 0;
    for (std::int32_t current : {89, 60, 14, 13, 0})
        for (int minCovis : {1, 4})
            for (int maxKeyframes : {20, 7, 1}) {
                const auto got = computeAdjacentKeyframes(ctx, tables, current, minCovis, maxKeyframes);
                if (got != compute_adjacent(M, current, minCovis, maxKeyframes)) { std::printf("computeAdjacentKeyframes differs: current %d minCovis %d max %d\n", current, minCovis, maxKeyframes); return 5; }
                adjacentTotal += got.size();
            }
    if (adjacentTotal < 100) { std::printf("computeAdjacentKeyframes: %zu keyframes in all\n", adjacentTotal); return 5; }
    std::printf("computeAdjacentKeyframes ok %zu keyframes\n", adjacentTotal);
    // localMapPoints: the lists of matchLocalMapPoints and of correctLoop
    const std::int32_t current = 60;
    const auto adjacent = compute_adjacent(M, current, 1, 20);
    const LoopPoints local = localMapPoints(ctx, table, &flags, adjacent, current, DeviceMapPointFlags::USABLE, false);
    if (local.row != local_mps(M, adjacent, current) || !local.reference.empty()) { std::printf("localMapPoints differs from localMps\n"); return 6; }
    std::vector<std::int32_t> loopKfs;
    for (int k = 70; k >= 30; --k) loopKfs.push_back(k);
    loopKfs.push_back(50);
    const LoopPoints loop = localMapPoints(ctx, table, nullptr, loopKfs);
    const auto want = loop_map_points(M, loopKfs);
    std::vector<std::int32_t> wantRow, wantRef;
    for (const auto &e : want) { wantRow.push_back(e.first); wantRef.push_back(e.second); }
    if (loop.row != wantRow || loop.reference != wantRef) { std::printf("localMapPoints differs from localMapPoints of correctLoop\n"); return 7; }
    const LoopPoints none = localMapPoints(ctx, table, nullptr, {});
    if (!none.row.empty()) { std::printf("localMapPoints of no keyframes is not empty\n"); return 8; }
    std::printf("localMapPoints ok %zu local %zu loop rows\n", local.row.size(), loop.row.size());
    return 0;
}

// ---- --baseline -----------------------------------------------------------------------------------------------------------------------
int baseline(int nKf, int stride, int nMp, int nQ, int nUnion, const char *dump) {
    HostMap M = make_map(31, nKf, stride, nMp, 15);
    if (dump) {
        std::FILE *f = std::fopen(dump, "wb");
        if (!f) { std::printf("cannot write %s\n", dump); return 1; }
        for (const auto &l : M.mapPoints) std::fwrite(l.data(), 4, l.size(), f);
        std::fclose(f);
    }
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    double tNb = 1e30, tUnion = 1e30;
    unsigned long long sumNb = 0, sumUnion = 0;
    for (int rep = 0; rep < 3; ++rep) {
        sumNb = sumUnion = 0;
        const auto t0 = clk::now();
        for (int q = 0; q < nQ; ++q) {
            const std::int32_t k = (std::int32_t)((long long)q * nKf / nQ);
            for (std::int32_t n : get_neighbors(M, k, M.chain.previous[k], M.chain.next[k], 5, false)) sumNb += (unsigned)n + 1;
        }
        const auto t1 = clk::now();
        std::vector<std::int32_t> kfs;
        for (int k = 0; k < nUnion; ++k) kfs.push_back(k % nKf);
        for (const auto &e : loop_map_points(M, kfs)) sumUnion += (unsigned long long)e.first * 31 + (unsigned)e.second;
        const auto t2 = clk::now();
        tNb = std::min(tNb, ms(t0, t1)); tUnion = std::min(tUnion, ms(t1, t2));
    }
    std::printf("baseline slots %d stride %d rows %d neighbours_ms %.3f neighbours_sum %llu union_ms %.3f union_sum %llu\n", nKf, stride, nMp, tNb, sumNb, tUnion, sumUnion);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_covisibility, (const void *)&ms_map_point_union, (const void *)&ms_covisibility_check, (const void *)&ms_map_point_union_check};
    std::printf("link ok %d\n", syms[0] != nullptr && syms[1] != nullptr && syms[2] != nullptr && syms[3] != nullptr);
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu();
    if (argc > 6 && std::strcmp(argv[1], "--baseline") == 0) return baseline(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), argc > 7 ? argv[7] : nullptr);
    return 0;
}
