// Compile + link check of the keyframe database in the host mirror (mi355slam::BowIndex add / remove / getBowSimilar) against
// libmi355slam.so; with a GPU it also runs a mapper-like sequence of adds, removals and queries and compares every query with the
// small restatement below (tests/test_bow_db_abi.py, tests/test_gpu_bow_db.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>
#include "mi355slam/bow_index.hpp"

using namespace mi355slam;

namespace {

// what the reference does with its inverted index: count shared words per id, threshold, L1 score, order, cut
std::vector<BowSimilar> restated(const std::map<MapKf, BowVector> &db, const BowVector &q, MapKf self, float minRatio, float scoreRatio) {
    std::map<MapKf, unsigned> common;
    for (const auto &e : db) {
        if (e.first == self) continue;
        unsigned c = 0;
        for (const auto &kv : q) c += e.second.count(kv.first) ? 1u : 0u;
        if (c > 0) common[e.first] = c;
    }
    if (common.empty()) return {};
    unsigned maxc = 0;
    for (const auto &c : common) maxc = std::max(maxc, c.second);
    const unsigned minc = (unsigned)(minRatio * (float)maxc);
    std::vector<BowSimilar> out;
    for (const auto &c : common) {
        if (c.second <= minc) continue;
        const BowVector &w = db.at(c.first);
        double s = 0.0;
        for (const auto &kv : q) {
            auto it = w.find(kv.first);
            if (it != w.end()) s += std::fabs(kv.second - it->second) - std::fabs(kv.second) - std::fabs(it->second);
        }
        out.push_back(BowSimilar{c.first, (float)(-s / 2.0)});
    }
    std::stable_sort(out.begin(), out.end(), [](const BowSimilar &a, const BowSimilar &b) { return a.score > b.score; });
    const float minScore = out[0].score * scoreRatio;
    std::size_t keep = 0;
    while (keep < out.size() && !(out[keep].score < minScore)) ++keep;
    out.resize(keep);
    return out;
}

BowVector random_vector(std::mt19937 &rng, const std::vector<unsigned> &place, int n_words) {
    BowVector v;
    std::uniform_real_distribution<double> u(0.01, 2.0), keep(0.0, 1.0);
    for (unsigned w : place) if (keep(rng) < 0.8) v[w] = u(rng);
    for (int k = 0; k < 20; ++k) v[(unsigned)(rng() % (unsigned)n_words)] = u(rng);
    double norm = 0.0;
    for (const auto &kv : v) norm += std::fabs(kv.second);
    for (auto &kv : v) kv.second /= norm;
    return v;
}

}  // namespace

int main(int argc, char **argv) {
    // a two-level vocabulary: 16 inner nodes of 64 leaves each (the database only needs the word count)
    VocabularyTree tree;
    tree.branchingFactor = 16; tree.depthLevels = 2;
    tree.parent.push_back(0); tree.wordId.push_back(-1); tree.weight.push_back(0.0);
    for (int i = 0; i < 16; ++i) { tree.parent.push_back(0); tree.wordId.push_back(-1); tree.weight.push_back(0.0); }
    int words = 0;
    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 64; ++k) { tree.parent.push_back(1 + i); tree.wordId.push_back(words++); tree.weight.push_back(1.0); }
    tree.descriptor.assign(8 * tree.parent.size(), 0u);
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) {
        // reference every new mirror entry point so that the link resolves them
        void (BowIndex::*a)(const BowVector &, MapKf) = &BowIndex::add;
        void (BowIndex::*r)(MapKf) = &BowIndex::remove;
        std::vector<BowSimilar> (BowIndex::*g)(const BowVector &, MapKf, float, float) = &BowIndex::getBowSimilar;
        std::printf("link ok %d %d %d\n", a != nullptr, r != nullptr, g != nullptr);
        return 0;
    }
    Context ctx(0);
    BowIndex index(ctx, tree);
    std::mt19937 rng(7);
    std::vector<std::vector<unsigned>> places(12);
    for (auto &p : places) {
        std::set<unsigned> s;
        while (s.size() < 150) s.insert((unsigned)(rng() % (unsigned)words));
        p.assign(s.begin(), s.end());
    }
    const std::int32_t CURRENT = 1000;
    std::map<MapKf, BowVector> db;
    int queries = 0, results = 0, bad = 0;
    // atlas maps first (mapper_helpers.cpp:979), then the mapper's order per keyframe: query (loop_closer.cpp:132), add (:1099), cull (:387)
    for (int m = 0; m < 2; ++m)
        for (int k = 0; k < 40; ++k) {
            BowVector v = random_vector(rng, places[(std::size_t)(rng() % places.size())], words);
            index.add(v, MapKf{m, k}); db[MapKf{m, k}] = v;
        }
    for (int kf = 0; kf < 300; ++kf) {
        BowVector v = random_vector(rng, places[(std::size_t)(rng() % places.size())], words);
        const MapKf self{CURRENT, kf};
        for (float mr : {0.8f, 0.0f}) {
            const std::vector<BowSimilar> got = index.getBowSimilar(v, self, mr, 0.75f), want = restated(db, v, self, mr, 0.75f);
            ++queries; results += (int)want.size();
            bool same = got.size() == want.size();
            for (std::size_t i = 0; same && i < got.size(); ++i)
                same = got[i].mapKf == want[i].mapKf && std::memcmp(&got[i].score, &want[i].score, 4) == 0;
            if (!same) ++bad;
        }
        index.add(v, self); db[self] = v;
        if (kf >= 60 && kf % 3 != 0) { const MapKf old{CURRENT, kf - 60}; index.remove(old); db.erase(old); }
    }
    index.remove(MapKf{CURRENT, 123456});                                     // absent: nothing happens
    std::printf("%d queries, %d results, %d mismatches\n", queries, results, bad);
    if (bad || results == 0) return 1;
    std::printf("bow db ok\n");
    return 0;
}
