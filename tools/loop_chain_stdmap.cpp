// loop_chain_stdmap.cpp -- the host side of tools/loop_chain_probe.py: the walks ms_loop_usable_mask, ms_loop_pairs and ms_loop_sim3_lists
// replace (keyframe_matcher.cpp:79-84, loop_closer.cpp:203-213 with loop_ransac.cpp:17-41, optimize_transform.cpp:101-142), restated over
// std::map<MpId, MapPoint> / std::map<KfId, Keyframe> with MapPoint::observations a std::map<KfId, KpId>, on one core.  Given the scene file
// the probe writes (its device tables and matched arrays: the SAME input the device calls get) it builds the map from it; without one it
// builds a map of the probe's shape itself.  It prints the median time of the three walks for the candidates in milliseconds.
//   g++ -O2 -std=c++17 loop_chain_stdmap.cpp -o loop_chain_stdmap && ./loop_chain_stdmap [reps] [scene file]
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

struct MapPoint {
    std::array<double, 3> position;
    int status;                                  // 3 = TRIANGULATED
    std::map<int, int> observations;             // KfId -> KpId
};
struct Keyframe {
    std::vector<int> mapPoints;                  // per keypoint, -1 for none
    std::array<double, 12> poseCW;
    std::vector<int> octave;
    std::vector<float> x, y;
};

static std::array<double, 3> camPoint(const std::array<double, 12> &P, const std::array<double, 3> &p) {
    std::array<double, 3> o;
    for (int i = 0; i < 3; ++i) o[i] = ((P[4 * i] * p[0] + P[4 * i + 1] * p[1]) + P[4 * i + 2] * p[2]) + P[4 * i + 3];
    return o;
}

int main(int argc, char **argv) {
    const int reps = argc > 1 ? std::atoi(argv[1]) : 15;
    int n_kf = 40, n_kp = 2000, n_mp = 200000, n_cand = 11, n_levels = 8, curSlot = 0;
    std::mt19937 rng(9);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::map<int, MapPoint> mapPoints;
    std::map<int, Keyframe> keyframes;
    std::vector<int> candIds;
    std::vector<std::vector<int>> matched;
    std::vector<float> sigma;
    if (argc > 2) {                                          // the probe's scene: header, then the tables as the device holds them
        FILE *f = std::fopen(argv[2], "rb");
        if (!f) { std::printf("cannot open %s\n", argv[2]); return 1; }
        bool ok = true;
        auto rd = [&](void *p, size_t bytes) { if (bytes && std::fread(p, 1, bytes, f) != bytes) ok = false; };
        int h[6];
        rd(h, sizeof h);
        if (!ok) return 1;
        n_kf = h[0]; n_kp = h[1]; n_mp = h[2]; n_cand = h[3]; n_levels = h[4]; curSlot = h[5];
        const size_t nk = (size_t)n_kf * n_kp;
        std::vector<int> kfMp(nk), oct(nk), cand(n_cand), mt((size_t)n_cand * n_kp);
        std::vector<float> x(nk), y(nk);
        std::vector<double> pose((size_t)n_kf * 12), pos((size_t)n_mp * 3);
        std::vector<unsigned char> live(n_mp), flags(n_mp);
        sigma.resize(n_levels);
        rd(kfMp.data(), 4 * nk); rd(oct.data(), 4 * nk); rd(x.data(), 4 * nk); rd(y.data(), 4 * nk); rd(pose.data(), 8 * pose.size()); rd(pos.data(), 8 * pos.size());
        rd(live.data(), live.size()); rd(flags.data(), flags.size()); rd(cand.data(), 4 * cand.size()); rd(mt.data(), 4 * mt.size()); rd(sigma.data(), 4 * sigma.size());
        std::fclose(f);
        if (!ok) { std::printf("short scene file\n"); return 1; }
        for (int r = 0; r < n_mp; ++r)
            if (live[r]) mapPoints[r] = MapPoint{{pos[3 * (size_t)r], pos[3 * (size_t)r + 1], pos[3 * (size_t)r + 2]}, (flags[r] & 1) ? 3 : 2, {}};
        for (int k = 0; k < n_kf; ++k) {
            Keyframe kf;
            kf.mapPoints.assign(n_kp, -1);
            kf.octave.assign(oct.begin() + (size_t)k * n_kp, oct.begin() + (size_t)(k + 1) * n_kp);
            kf.x.assign(x.begin() + (size_t)k * n_kp, x.begin() + (size_t)(k + 1) * n_kp); kf.y.assign(y.begin() + (size_t)k * n_kp, y.begin() + (size_t)(k + 1) * n_kp);
            std::memcpy(kf.poseCW.data(), pose.data() + 12 * (size_t)k, 96);
            for (int i = 0; i < n_kp; ++i) {
                const int r = kfMp[(size_t)k * n_kp + i];
                if (r < 0 || r >= n_mp || !live[r]) continue;           // a culled point's observation is gone from the map
                kf.mapPoints[i] = r;
                mapPoints.at(r).observations[100 + 3 * k] = i;
            }
            keyframes[100 + 3 * k] = std::move(kf);
        }
        for (int c = 0; c < n_cand; ++c) {
            candIds.push_back(100 + 3 * cand[c]);
            matched.emplace_back(mt.begin() + (size_t)c * n_kp, mt.begin() + (size_t)(c + 1) * n_kp);
        }
    } else {
        for (int r = 0; r < n_mp; ++r) mapPoints[r] = MapPoint{{40 * U(rng) - 20, 40 * U(rng) - 20, 40 * U(rng) - 20}, U(rng) < 0.5 ? 3 : 2, {}};
        for (int k = 0; k < n_kf; ++k) {
            Keyframe kf;
            kf.mapPoints.assign(n_kp, -1); kf.octave.resize(n_kp); kf.x.resize(n_kp); kf.y.resize(n_kp);
            for (int i = 0; i < 12; ++i) kf.poseCW[i] = 2 * U(rng) - 1;
            for (int i = 0; i < n_kp; ++i) {
                kf.octave[i] = (int)(rng() % n_levels); kf.x[i] = (float)(640 * U(rng)); kf.y[i] = (float)(480 * U(rng));
                if (U(rng) >= 0.8) continue;
                int r = (int)(rng() % n_mp);
                while (mapPoints[r].observations.count(100 + 3 * k)) r = (int)(rng() % n_mp);
                kf.mapPoints[i] = r;
                mapPoints[r].observations[100 + 3 * k] = i;
            }
            keyframes[100 + 3 * k] = std::move(kf);
        }
        for (int c = 0; c < n_cand; ++c) candIds.push_back(100 + 3 * (3 * c + 2));
        matched.assign(n_cand, std::vector<int>(n_kp));
        for (auto &m : matched) {
            for (int i = 0; i < n_kp; ++i) m[i] = i;
            std::shuffle(m.begin(), m.end(), rng);
            for (int i = 0; i < n_kp; ++i) if (U(rng) < 0.4) m[i] = -1;
        }
        sigma.assign(n_levels, 1.f);
        for (int l = 1; l < n_levels; ++l) sigma[l] = sigma[l - 1] * 1.44f;
    }
    const int curId = 100 + 3 * curSlot;
    const float CHI_SQ_2D = 9.21034f;
    std::vector<double> times;
    double sink = 0;
    size_t n_pairs = 0, n_listed = 0;
    for (int rep = 0; rep < reps + 2; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        const Keyframe &cur = keyframes.at(curId);
        // keyframe_matcher.cpp:79-84, :94-96: the usable masks of the current keyframe and of every candidate
        std::vector<std::vector<unsigned char>> usable;
        for (int s = -1; s < n_cand; ++s) {
            const Keyframe &kf = s < 0 ? cur : keyframes.at(candIds[s]);
            std::vector<unsigned char> u(kf.mapPoints.size(), 0);
            for (size_t i = 0; i < u.size(); ++i)
                if (kf.mapPoints[i] != -1) u[i] = s < 0 || mapPoints.at(kf.mapPoints[i]).status == 3;
            usable.push_back(std::move(u));
        }
        n_pairs = n_listed = 0;
        for (int c = 0; c < n_cand; ++c) {
            const Keyframe &cand = keyframes.at(candIds[c]);
            std::vector<std::pair<int, int>> matches;                            // loop_closer.cpp:203-213
            for (int i = 0; i < n_kp; ++i) {
                const int m = matched[c][i];
                if (m < 0) continue;
                const int id1 = cur.mapPoints.at(i), id2 = cand.mapPoints.at(m);
                if (id1 != -1 && id2 != -1 && id1 != id2) matches.emplace_back(id1, id2);
            }
            std::vector<std::array<double, 3>> p1, p2;                           // loop_ransac.cpp:17-41
            std::vector<float> thr1, thr2;
            p1.reserve(matches.size()); p2.reserve(matches.size()); thr1.reserve(matches.size()); thr2.reserve(matches.size());
            for (const auto &mt : matches) {
                const MapPoint &mp1 = mapPoints.at(mt.first), &mp2 = mapPoints.at(mt.second);
                p1.push_back(camPoint(cur.poseCW, mp1.position)); p2.push_back(camPoint(cand.poseCW, mp2.position));
                thr1.push_back(CHI_SQ_2D * sigma.at(cur.octave.at(mp1.observations.at(curId))));
                thr2.push_back(CHI_SQ_2D * sigma.at(cand.octave.at(mp2.observations.at(candIds[c]))));
            }
            n_pairs += matches.size();
            std::vector<std::array<double, 3>> q1, q2;                           // optimize_transform.cpp:101-142 for every other pair
            std::vector<std::array<double, 2>> o1, o2;
            std::vector<float> i1, i2;
            for (size_t e = 0; e < matches.size(); e += 2) {
                const MapPoint &mp1 = mapPoints.at(matches[e].first), &mp2 = mapPoints.at(matches[e].second);
                const int k1 = mp1.observations.at(curId), k2 = mp2.observations.at(candIds[c]);
                q1.push_back(camPoint(cur.poseCW, mp1.position)); q2.push_back(camPoint(cand.poseCW, mp2.position));
                o1.push_back({((double)cur.x[k1] - 320.0) / 500.0, ((double)cur.y[k1] - 240.0) / 500.0});
                o2.push_back({((double)cand.x[k2] - 320.0) / 500.0, ((double)cand.y[k2] - 240.0) / 500.0});
                i1.push_back(sigma.at(cur.octave.at(k1))); i2.push_back(sigma.at(cand.octave.at(k2)));
            }
            n_listed += q1.size();
            if (!p1.empty()) sink += p1.back()[0] + thr2.back() + (q1.empty() ? 0 : o2.back()[1] + i1.back()) + usable[c + 1][0];
        }
        const auto t1 = std::chrono::steady_clock::now();
        if (rep >= 2) times.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::sort(times.begin(), times.end());
    std::printf("{\"std_map_one_core_ms\": %.4f, \"n_pairs\": %zu, \"n_listed\": %zu, \"sink\": %g}\n", times[times.size() / 2], n_pairs, n_listed, sink);
    return 0;
}
