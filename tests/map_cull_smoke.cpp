// Compile + link check of the culling step of the host mirror (DeviceMapPointLive, observationCounts, cullMap in
// mi355slam/map_tables.hpp and map_update.hpp) against libmi355slam.so (tests/test_map_cull_abi.py), its comparison with a sequential std::map
// restatement of the reference's loops (mapper_helpers.cpp:349-482, mapdb.cpp:161-174), and the one-core baseline tools/cull_probe.py times
// the device path against.
//   map_cull_smoke --no-gpu               every MS_ERR_INVALID case of ms_map_cull through ms_map_cull_check (no context, no device), and the
//                                         restatement below on a hand-computed map.  The validation itself (csrc/map_checks.cpp) runs under
//                                         sanitizers in tests/test_map_checks_corpus.py
//   map_cull_smoke --gpu                  observationCounts and cullMap against the restatement, the relinked KeyframeSlots included
//   map_cull_smoke --baseline K S M C [F] the restatement on one core for K slots of S entries over M rows and C candidates: building the
//                                         observation maps (what ms_observation_count replaces) and the two culling passes; prints the best
//                                         of three in milliseconds and checksums, and writes the map to the file F (kf_mp int32 [K * S] |
//                                         flags uint8 [M] | live uint8 [M] | kf_id int32 [K] | kf_t float64 [K] | cand int32 [C]) so that the
//                                         device path can run on the same map
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <set>
#include <vector>
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

// ---- the reference's map and loops, sequentially ---------------------------------------------------------------------------------------
struct HostMap {
    std::vector<std::vector<std::int32_t>> mapPoints;        // Keyframe::mapPoints per slot (-1 = none)
    std::vector<std::map<std::int32_t, int>> observations;   // MapPoint::observations per row: KfId -> entries of that keyframe
    std::vector<std::uint8_t> flags, live;
    std::vector<std::int32_t> cand;
    KeyframeSlots chain;
    std::map<std::int32_t, std::int32_t> slotOf;             // mapDB.keyframes: KfId -> slot
    std::vector<std::int32_t> removedRows, removedKeyframes; // in the order of removal
    std::vector<std::uint8_t> removedWhy;
    void link() {
        observations.assign(flags.size(), {});
        slotOf.clear();
        for (std::size_t k = 0; k < mapPoints.size(); ++k) {
            if (chain.id[k] < 0) continue;
            slotOf[chain.id[k]] = (std::int32_t)k;
            for (std::int32_t r : mapPoints[k]) if (r != -1) ++observations[r][chain.id[k]];
        }
    }
    std::size_t size(std::int32_t r) const {
        std::size_t n = 0;
        for (const auto &o : observations[r]) n += (std::size_t)o.second;
        return n;
    }
};

// MapDB::removeMapPoint, mapdb.cpp:161-174
void remove_map_point(HostMap &M, std::int32_t r, std::uint8_t why) {
    for (const auto &o : M.observations[r])
        for (std::int32_t &e : M.mapPoints[M.slotOf.at(o.first)]) if (e == r) e = -1;
    M.observations[r].clear();
    M.live[r] = 0; M.flags[r] = 0;
    M.removedRows.push_back(r); M.removedWhy.push_back(why);
}

// cullMapPoints, mapper_helpers.cpp:349-373
void cull_map_points(HostMap &M, std::int32_t current, double minAge) {
    for (std::int32_t r = 0; r < (std::int32_t)M.flags.size(); ++r) {
        if (!M.live[r]) continue;
        const auto &obs = M.observations[r];
        if (obs.empty()) { remove_map_point(M, r, 1); continue; }
        const int obsAge = (int)(M.chain.t[current] - M.chain.t[M.slotOf.at(obs.begin()->first)]);
        if (!obs.count(M.chain.id[current]) && obsAge > minAge && !(M.flags[r] & DeviceMapPointFlags::TRIANGULATED)) remove_map_point(M, r, 2);
    }
}

// removeKeyframe, mapper_helpers.cpp:375-431 (what it does to the tables and the links)
void remove_keyframe(HostMap &M, std::int32_t k) {
    std::set<std::int32_t> mapPointsToErase;
    const std::int32_t prev = M.chain.previous[k], next = M.chain.next[k], id = M.chain.id[k];
    for (std::int32_t r : M.mapPoints[k]) {
        if (r == -1) continue;
        auto &obs = M.observations[r];
        if (--obs[id] == 0) obs.erase(id);
        if (obs.empty() && M.live[r]) mapPointsToErase.insert(r);
    }
    for (std::int32_t r : mapPointsToErase) remove_map_point(M, r, 3);
    if (next != -1) M.chain.previous[next] = prev;
    if (prev != -1) M.chain.next[prev] = next;
    M.mapPoints[k].assign(M.mapPoints[k].size(), -1);
    M.slotOf.erase(id);
    M.chain.previous[k] = M.chain.next[k] = -1;
    M.chain.id[k] = -1;
    M.removedKeyframes.push_back(k);
}

// cullKeyframes, mapper_helpers.cpp:433-482
void cull_keyframes(HostMap &M, const std::vector<std::int32_t> &adjacent, const std::vector<std::int32_t> &loopKeyframes, const CullSettings &s) {
    std::vector<std::int32_t> sorted = adjacent;
    std::sort(sorted.begin(), sorted.end(), [&](std::int32_t a, std::int32_t b) { return M.chain.id[a] > M.chain.id[b]; });
    for (std::int32_t k : sorted) {
        if (M.chain.previous[k] < 0) continue;
        if (std::find(loopKeyframes.begin(), loopKeyframes.end(), k) != loopKeyframes.end()) continue;
        unsigned nMapPoints = 0;
        int nCritical = 0;
        for (std::int32_t r : M.mapPoints[k]) {
            if (r == -1) continue;
            nMapPoints++;
            if (M.size(r) <= (std::size_t)s.minObservationsForBA) nCritical++;
        }
        const bool remove = s.ratioFloat32 ? nCritical < nMapPoints * (float)s.keyframeCullMaxCriticalRatio : nCritical < nMapPoints * s.keyframeCullMaxCriticalRatio;
        if (remove) remove_keyframe(M, k);
    }
}

// a chain of keyframes one second apart; every row is seen by a run of up to maxObs consecutive keyframes, every
// 16th row also by the newest keyframe; the last rows are never observed, and every 50th row holds no map point
HostMap make_map(unsigned seed, int nKf, int stride, int nMp, int maxObs, int nCand) {
    std::mt19937 rng(seed);
    HostMap M;
    M.mapPoints.assign(nKf, {});
    M.flags.resize(nMp); M.live.assign(nMp, 1);
    for (auto &f : M.flags) f = (std::uint8_t)(rng() % 4);
    for (int r = 0; r < nMp; ++r) if (r % 50 == 49) M.live[r] = 0;
    const int observed = nMp - nMp / 20;
    for (int r = 0; r < observed; ++r) {
        const int n = 1 + (int)(rng() % (unsigned)maxObs), k0 = (int)(rng() % (unsigned)nKf);
        for (int k = k0; k < std::min(k0 + n, nKf); ++k)
            if ((int)M.mapPoints[k].size() < stride) M.mapPoints[k].push_back(r);
        if (r % 16 == 0 && k0 + n < nKf && (int)M.mapPoints[nKf - 1].size() < stride) M.mapPoints[nKf - 1].push_back(r);
    }
    for (auto &l : M.mapPoints) {
        l.resize(stride, -1);
        std::shuffle(l.begin(), l.end(), rng);
    }
    M.chain.previous.resize(nKf); M.chain.next.resize(nKf); M.chain.cameraCenter.resize(nKf); M.chain.id.resize(nKf); M.chain.t.resize(nKf);
    std::uniform_real_distribution<double> U(0.0, 0.5);
    for (int k = 0; k < nKf; ++k) {
        M.chain.previous[k] = k - 1;
        M.chain.next[k] = k + 1 < nKf ? k + 1 : -1;
        M.chain.cameraCenter[k] = {0.3 * k, 0.0, 0.0};
        M.chain.id[k] = 2 * k + 5;
        M.chain.t[k] = (double)k + U(rng);
    }
    // the newest keyframes but the current one, in shuffled order
    for (int k = nKf - 2; k >= 0 && (int)M.cand.size() < nCand; --k) M.cand.push_back(k);
    std::shuffle(M.cand.begin(), M.cand.end(), rng);
    M.link();
    return M;
}

CullSettings smoke_settings() {
    CullSettings s;
    s.minMapPointCullingAge = 12.0; s.minObservationsForBA = 2; s.keyframeCullMaxCriticalRatio = 0.3;
    return s;
}

unsigned long long checksum_rows(const std::vector<std::int32_t> &rows, const std::vector<std::uint8_t> &why) {
    unsigned long long sum = 0;
    for (std::size_t i = 0; i < rows.size(); ++i) sum += (unsigned long long)rows[i] * 31 + why[i];
    return sum;
}

// ---- --no-gpu -------------------------------------------------------------------------------------------------------------------------
int no_gpu() {
    if (ms_map_cull(nullptr, nullptr, 0, 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != MS_ERR_INVALID ||
        ms_observation_count(nullptr, nullptr, 0, 1, 0, nullptr, nullptr, nullptr, nullptr) != MS_ERR_INVALID) {
        std::printf("a call without a context must fail with MS_ERR_INVALID\n");
        return 1;
    }
    // the check reads the HOST arrays only: the device arrays are stand-in addresses that are never followed
    const std::int32_t *dtab = reinterpret_cast<const std::int32_t *>(0x1000), *drows = reinterpret_cast<const std::int32_t *>(0x4000);
    const std::uint8_t *dflags = reinterpret_cast<const std::uint8_t *>(0x2000), *dlive = reinterpret_cast<const std::uint8_t *>(0x3000);
    char why[256];
    int cases = 0;
    struct C {
        int nKf = 5, stride = 8, nMp = 20;
        std::vector<std::int32_t> id{4, 9, -1, 2, 7};
        std::vector<double> t{1.0, 2.5, 0.0, 0.5, 2.0};
        std::vector<std::int32_t> cand{0, 4, 3};
        std::vector<std::uint8_t> keep{0, 0, 1}, removed{0, 0, 0};
        ms_cull_settings s{1, 1, 10.0, 2, 0.5, 0};
        std::int32_t nRows = 0, nKfs = 0;
    };
    struct Missing { bool tab = false, flags = false, live = false, id = false, t = false, cand = false, keep = false, s = false, rows = false, removed = false, nRows = false, nKfs = false; };
    auto check = [&](C &c, const Missing &m = Missing()) {
        why[0] = 0;
        return ms_map_cull_check(m.tab ? nullptr : dtab, c.nKf, c.stride, m.flags ? nullptr : dflags, m.live ? nullptr : dlive, c.nMp, m.id ? nullptr : c.id.data(),
                                 m.t ? nullptr : c.t.data(), m.cand ? nullptr : c.cand.data(), m.keep ? nullptr : c.keep.data(), (int)c.cand.size(), m.s ? nullptr : &c.s,
                                 m.rows ? nullptr : drows, m.removed ? nullptr : c.removed.data(), m.nRows ? nullptr : &c.nRows, m.nKfs ? nullptr : &c.nKfs, why, sizeof(why));
    };
    auto accepted = [&](int rc, const char *what) {
        if (rc == MS_OK) return true;
        std::printf("%s was rejected: %s\n", what, why);
        return false;
    };
    auto rejected = [&](int rc, const char *what) {
        ++cases;
        if (rc == MS_ERR_INVALID && why[0]) return true;
        std::printf("%s: returned %d (%s), expected MS_ERR_INVALID with a message\n", what, rc, why);
        return false;
    };
    bool good = true;
    { C c; good &= accepted(check(c), "a valid call"); }
    { C c; c.cand.clear(); c.keep.clear(); c.removed.clear(); Missing m; m.cand = m.keep = m.removed = true; good &= accepted(check(c, m), "n_cand = 0"); }
    { C c; c.nMp = 0; Missing m; m.live = m.rows = true; good &= accepted(check(c, m), "n_mp = 0"); }
    { C c; c.s.cull_points = 0; Missing m; m.flags = true; good &= accepted(check(c, m), "cull_points = 0 without flags"); }
    { C c; Missing m; m.keep = true; good &= accepted(check(c, m), "no cand_keep"); }
    { C c; c.t[2] = std::nan(""); good &= accepted(check(c), "a time that is not finite in an empty slot"); }
    { C c; c.s.min_age = -3.0; c.s.max_critical_ratio = -1.0; c.s.min_obs_for_ba = 0; good &= accepted(check(c), "negative min_age and ratio"); }
    if (!good) return 1;
    { C c; c.s.current_slot = 5; good &= rejected(check(c), "current slot beyond the table"); }
    { C c; c.s.current_slot = -1; good &= rejected(check(c), "current slot -1"); }
    { C c; c.cand[1] = 5; good &= rejected(check(c), "candidate beyond the table"); }
    { C c; c.cand[0] = -1; good &= rejected(check(c), "candidate -1"); }
    { C c; c.cand[2] = 0; good &= rejected(check(c), "candidate listed twice"); }
    { C c; c.cand[1] = 1; good &= rejected(check(c), "candidate equal to the current slot"); }
    { C c; c.s.current_slot = 2; good &= rejected(check(c), "empty current slot"); }
    { C c; c.cand[1] = 2; good &= rejected(check(c), "empty candidate slot"); }
    { C c; c.id[3] = 9; good &= rejected(check(c), "kf_id listed twice"); }
    { C c; c.t[0] = std::numeric_limits<double>::infinity(); good &= rejected(check(c), "kf_t not finite"); }
    { C c; c.t[1] = std::nan(""); good &= rejected(check(c), "kf_t of the current slot not finite"); }
    { C c; c.t[3] = -3.0e9; good &= rejected(check(c), "age outside int32"); }
    { C c; c.t[4] = 2147483651.0; good &= rejected(check(c), "negative age outside int32"); }
    { C c; c.s.min_age = std::nan(""); good &= rejected(check(c), "min_age not finite"); }
    { C c; c.s.max_critical_ratio = std::numeric_limits<double>::infinity(); good &= rejected(check(c), "max_critical_ratio not finite"); }
    { C c; c.s.min_obs_for_ba = -1; good &= rejected(check(c), "negative min_obs_for_ba"); }
    { C c; c.stride = 0; good &= rejected(check(c), "stride 0"); }
    { C c; c.nMp = -1; good &= rejected(check(c), "negative n_mp"); }
    { C c; c.nKf = -1; good &= rejected(check(c), "negative n_kf"); }
    {
        C c;
        why[0] = 0;
        good &= rejected(ms_map_cull_check(dtab, c.nKf, c.stride, dflags, dlive, c.nMp, c.id.data(), c.t.data(), c.cand.data(), c.keep.data(), -1, &c.s, drows, c.removed.data(),
                                           &c.nRows, &c.nKfs, why, sizeof(why)), "negative n_cand");
    }
    { C c; Missing m; m.flags = true; good &= rejected(check(c, m), "cull_points without flags"); }
    { C c; Missing m; m.tab = true; good &= rejected(check(c, m), "missing table"); }
    { C c; Missing m; m.live = true; good &= rejected(check(c, m), "missing mp_live"); }
    { C c; Missing m; m.id = true; good &= rejected(check(c, m), "missing kf_id"); }
    { C c; Missing m; m.t = true; good &= rejected(check(c, m), "missing kf_t"); }
    { C c; Missing m; m.cand = true; good &= rejected(check(c, m), "missing cand"); }
    { C c; Missing m; m.s = true; good &= rejected(check(c, m), "missing settings"); }
    { C c; Missing m; m.rows = true; good &= rejected(check(c, m), "missing removed_rows"); }
    { C c; Missing m; m.removed = true; good &= rejected(check(c, m), "missing cand_removed"); }
    { C c; Missing m; m.nRows = true; good &= rejected(check(c, m), "missing n_removed_rows"); }
    { C c; Missing m; m.nKfs = true; good &= rejected(check(c, m), "missing n_removed_kf"); }
    if (!good) return 1;
    // four keyframes in a chain, ids 10, 20, 30, 40 one second apart; rows: 0 seen by {0}, 1 by {0, 1}, 2 by {1, 2}, 3 by {2, 3}, 4 by {2},
    // 5 by nobody, 6 by {1} and triangulated.  current = 3, min age 1.5: rows 0, 1 (age 3) and 2 (age 2) go as aged, row 5 as empty; row 3 is
    // listed by the current keyframe, row 4 is young (age 1), row 6 is triangulated.  Then slot 2 {3, 4}: counts 2 and 1, critical 2 of 2, kept
    // at ratio 0.5; slot 1 {6}: critical 1 of 1, kept; slot 0 has no previous keyframe.  With ratio 1.5 both go, newest first: slot 2 orphans
    // row 4 (row 3 keeps the current keyframe), slot 1 orphans row 6.
    HostMap M;
    M.mapPoints = {{0, 1, -1}, {1, 2, 6}, {2, 3, 4}, {3, -1, -1}};
    M.flags = {0, 2, 0, 0, 2, 0, 3}; M.live.assign(7, 1);
    M.chain.previous = {-1, 0, 1, 2}; M.chain.next = {1, 2, 3, -1}; M.chain.id = {10, 20, 30, 40}; M.chain.t = {0.0, 1.0, 2.0, 3.0};
    M.chain.cameraCenter.resize(4);
    M.link();
    HostMap A = M;
    CullSettings s;
    s.minMapPointCullingAge = 1.5; s.minObservationsForBA = 2; s.keyframeCullMaxCriticalRatio = 0.5;
    cull_map_points(A, 3, s.minMapPointCullingAge);
    cull_keyframes(A, {1, 2, 0}, {}, s);
    bool restated = A.removedRows == std::vector<std::int32_t>{0, 1, 2, 5} && A.removedWhy == std::vector<std::uint8_t>{2, 2, 2, 1} && A.removedKeyframes.empty() &&
                    A.mapPoints[1] == std::vector<std::int32_t>{-1, -1, 6} && A.mapPoints[2] == std::vector<std::int32_t>{-1, 3, 4};
    HostMap B = M;
    s.keyframeCullMaxCriticalRatio = 1.5;
    cull_map_points(B, 3, s.minMapPointCullingAge);
    cull_keyframes(B, {1, 2, 0}, {}, s);
    restated = restated && B.removedRows == std::vector<std::int32_t>{0, 1, 2, 5, 4, 6} && B.removedWhy == std::vector<std::uint8_t>{2, 2, 2, 1, 3, 3} &&
               B.removedKeyframes == std::vector<std::int32_t>{2, 1} && B.chain.next[0] == 3 && B.chain.previous[3] == 0 && B.size(3) == 1 && B.live[3] == 1;
    if (!restated) { std::printf("restatement: the hand-computed map differs\n"); return 1; }
    std::printf("no-gpu ok %d cull cases\n", cases);
    return 0;
}

// ---- --gpu ----------------------------------------------------------------------------------------------------------------------------
int gpu() {
    Context ctx(0);
    const int nKf = 40, stride = 70, nMp = 700;
    for (bool f32 : {false, true}) {
        HostMap M = make_map(7, nKf, stride, nMp, 6, 16);
        DeviceKeyframeMapPoints table(ctx, nKf, stride, nMp);
        for (int k = 0; k < nKf; ++k) table.update(k, M.mapPoints[k]);
        DeviceMapPointFlags flags(ctx, M.flags);
        DeviceMapPointLive live(ctx, M.live);
        const ObservationCounts counts = observationCounts(ctx, table, M.chain.id);
        for (int r = 0; r < nMp; ++r) {
            const auto &obs = M.observations[r];
            const std::int32_t first = obs.empty() ? -1 : M.slotOf.at(obs.begin()->first), last = obs.empty() ? -1 : M.slotOf.at(obs.rbegin()->first);
            if (counts.count[r] != (std::int32_t)M.size(r) || counts.first[r] != first || counts.last[r] != last) { std::printf("observationCounts differs: row %d\n", r); return 2; }
        }
        CullSettings s = smoke_settings();
        s.ratioFloat32 = f32;
        const std::int32_t current = nKf - 1;
        const std::vector<std::int32_t> loopKeyframes{M.cand[1], 3};
        KeyframeSlots chain = M.chain;
        MapTables tables{table, chain};
        tables.flags = &flags; tables.live = &live;
        const CullResult got = cullMap(ctx, tables, current, M.cand, loopKeyframes, s);
        cull_map_points(M, current, s.minMapPointCullingAge);
        cull_keyframes(M, M.cand, loopKeyframes, s);
        // the restatement lists the rows in the order of removal, the device in row order
        std::vector<std::pair<std::int32_t, std::uint8_t>> want, have;
        for (std::size_t i = 0; i < M.removedRows.size(); ++i) want.emplace_back(M.removedRows[i], M.removedWhy[i]);
        for (std::size_t i = 0; i < got.removedRows.size(); ++i) have.emplace_back(got.removedRows[i], got.removedWhy[i]);
        std::sort(want.begin(), want.end());
        if (have != want) { std::printf("cullMap: removed rows differ (%zu, expected %zu)\n", have.size(), want.size()); return 3; }
        if (got.removedKeyframes != M.removedKeyframes) { std::printf("cullMap: removed keyframes differ (%zu, expected %zu)\n", got.removedKeyframes.size(), M.removedKeyframes.size()); return 3; }
        int reasons[4] = {0, 0, 0, 0};
        for (std::uint8_t w : got.removedWhy) ++reasons[w & 3];
        if (!reasons[1] || !reasons[2] || !reasons[3] || got.removedKeyframes.empty() || got.removedKeyframes.size() + 2 > M.cand.size()) {
            std::printf("cullMap: the map exercises too little (%d / %d / %d rows, %zu keyframes)\n", reasons[1], reasons[2], reasons[3], got.removedKeyframes.size());
            return 3;
        }
        if (live.download() != M.live) { std::printf("cullMap: live bytes differ\n"); return 3; }
        const ObservationCounts after = observationCounts(ctx, table, chain.id);
        for (int r = 0; r < nMp; ++r)
            if (after.count[r] != (std::int32_t)M.size(r)) { std::printf("cullMap: the table differs at row %d\n", r); return 3; }
        std::printf("cullMap ok ratioFloat32 %d: %d empty %d aged %d orphaned rows, %zu keyframes\n", (int)f32, reasons[1], reasons[2], reasons[3], got.removedKeyframes.size());
        if (chain.previous != M.chain.previous || chain.next != M.chain.next || chain.id != M.chain.id) { std::printf("cullMap: the relinked chain differs\n"); return 4; }
        for (std::size_t i = 0; i < got.removedKeyframes.size(); ++i)
            if (got.removedPrevious[i] < 0) { std::printf("cullMap: the first keyframe was removed\n"); return 4; }
        std::printf("chain ok ratioFloat32 %d\n", (int)f32);
    }
    std::printf("observationCounts ok\n");
    return 0;
}

// ---- --baseline -----------------------------------------------------------------------------------------------------------------------
int baseline(int nKf, int stride, int nMp, int nCand, const char *dump) {
    const HostMap M0 = make_map(31, nKf, stride, nMp, 15, nCand);
    if (dump) {
        std::FILE *f = std::fopen(dump, "wb");
        if (!f) { std::printf("cannot write %s\n", dump); return 1; }
        for (const auto &l : M0.mapPoints) std::fwrite(l.data(), 4, l.size(), f);
        std::fwrite(M0.flags.data(), 1, M0.flags.size(), f);
        std::fwrite(M0.live.data(), 1, M0.live.size(), f);
        std::fwrite(M0.chain.id.data(), 4, M0.chain.id.size(), f);
        std::fwrite(M0.chain.t.data(), 8, M0.chain.t.size(), f);
        std::fwrite(M0.cand.data(), 4, M0.cand.size(), f);
        std::fclose(f);
    }
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const CullSettings s = smoke_settings();
    double tLink = 1e30, tCull = 1e30;
    unsigned long long sumObs = 0, sumRows = 0, sumKfs = 0;
    for (int rep = 0; rep < 3; ++rep) {
        HostMap M = M0;
        const auto t0 = clk::now();
        M.link();                                            // the observation maps: what the host keeps today to answer "how many" and "which is oldest"
        sumObs = 0;
        for (int r = 0; r < nMp; ++r) sumObs += M.size(r) * 7 + (unsigned)(M.observations[r].empty() ? 0 : M.slotOf.at(M.observations[r].begin()->first) + 1);
        const auto t1 = clk::now();
        cull_map_points(M, nKf - 1, s.minMapPointCullingAge);
        cull_keyframes(M, M.cand, {}, s);
        const auto t2 = clk::now();
        tLink = std::min(tLink, ms(t0, t1)); tCull = std::min(tCull, ms(t1, t2));
        sumRows = checksum_rows(M.removedRows, M.removedWhy);
        sumKfs = 0;
        for (std::int32_t k : M.removedKeyframes) sumKfs += (unsigned)k + 1;
    }
    std::printf("baseline slots %d stride %d rows %d candidates %d count_ms %.3f count_sum %llu cull_ms %.3f rows_sum %llu keyframes_sum %llu\n", nKf, stride, nMp, nCand, tLink,
                sumObs, tCull, sumRows, sumKfs);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_observation_count, (const void *)&ms_map_cull, (const void *)&ms_map_cull_check};
    std::printf("link ok %d\n", syms[0] != nullptr && syms[1] != nullptr && syms[2] != nullptr);
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) return gpu();
    if (argc > 5 && std::strcmp(argv[1], "--baseline") == 0) return baseline(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), argc > 6 ? argv[6] : nullptr);
    return 0;
}
