// bow_index.hpp -- host mirror of BowIndex::transform (bow_index.hpp:36-64, bow_index.cpp:59-93).
//
// The reference's BowIndex owns a DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> loaded from a file and calls its batch
// transform with levelsUp = 4.  DBoW2 is an external library (not in the reference tree); the mirror keeps the vocabulary as
// the flat arrays DBoW2 holds per node, sends the tree descent to the device (ms_bow_transform) and assembles the two ordered
// maps on the host in feature order, exactly as DBoW2's batch transform does: v[word] += weight and fv[node].push_back(i) for
// weight > 0, then BowVector::normalize(L1).  add / remove / getBowSimilar (bow_index.cpp:44-57, :95-176) go to the device
// keyframe database (ms_bow_db), created on the first add: the reference's inverted index std::vector<std::list<MapKf>> and
// DBoW2's L1 scoring are replaced, and the results are the reference's (ties in score in (mapId, kfId) order).  A keyframe whose
// descent lies on the device (ms_keyframe_admit) enters the database without a host vector: addAdmitted / addWords have the device
// do assembleVector's sums in assembleVector's order (ms_bow_db_add_words), bowVector brings an entry back.
#pragma once
#include <cmath>
#include <fstream>
#include <map>
#include <sstream>
#include <utility>
#include "common.hpp"

namespace mi355slam {

using BowVector = std::map<unsigned, double>;                        // DBoW2::BowVector: WordId -> WordValue
using FeatureVector = std::map<unsigned, std::vector<unsigned>>;     // DBoW2::FeatureVector: NodeId -> feature indices

// The vocabulary as DBoW2 stores it (TemplatedVocabulary::m_nodes): node 0 is the root.
struct VocabularyTree {
    int branchingFactor = 0, depthLevels = 0;                        // m_k, m_L
    int scoring = 0, weighting = 0;                                  // m_scoring (0 = L1_NORM), m_weighting (0 = TF_IDF), as in the file header
    std::vector<std::int32_t> parent, wordId;                        // wordId = -1 for inner nodes
    std::vector<std::uint32_t> descriptor;                           // 8 words per node
    std::vector<double> weight;
    std::size_t size() const { return parent.size(); }

    // DBoW2's text vocabulary format (the one ORB-SLAM's vocabularies ship in; TemplatedVocabulary::loadFromTextFile): a
    // header line "k L scoring weighting", then one line per node "parent isLeaf b0 .. b31 weight" with the descriptor as 32
    // decimal bytes.  Nodes get ids in file order starting at 1, words get ids in the order their leaves appear.
    static VocabularyTree loadFromTextFile(const std::string &path) {
        std::ifstream f(path);
        if (!f) throw std::runtime_error("mi355slam: cannot open vocabulary " + path);
        VocabularyTree v;
        std::string line;
        std::getline(f, line);
        int scoring = 0, weighting = 0;
        { std::stringstream ss(line); ss >> v.branchingFactor >> v.depthLevels >> scoring >> weighting; }
        v.scoring = scoring; v.weighting = weighting;
        if (v.branchingFactor < 0 || v.branchingFactor > 20 || v.depthLevels < 1 || v.depthLevels > 10 || scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3)
            throw std::runtime_error("mi355slam: vocabulary header out of range in " + path);
        v.parent.push_back(0); v.wordId.push_back(-1); v.weight.push_back(0.0); v.descriptor.resize(8, 0u);
        int words = 0;
        while (std::getline(f, line)) {
            if (line.empty()) continue;
            std::stringstream ss(line);
            int pid = 0, leaf = 0;
            ss >> pid >> leaf;
            std::uint8_t bytes[32];
            for (int k = 0; k < 32; ++k) { int b = 0; ss >> b; bytes[k] = (std::uint8_t)b; }
            double w = 0.0;
            ss >> w;
            if (!ss) throw std::runtime_error("mi355slam: malformed vocabulary line in " + path);
            v.parent.push_back(pid); v.weight.push_back(w); v.wordId.push_back(leaf > 0 ? words++ : -1);
            for (int k = 0; k < 8; ++k)
                v.descriptor.push_back((std::uint32_t)bytes[4 * k] | ((std::uint32_t)bytes[4 * k + 1] << 8) | ((std::uint32_t)bytes[4 * k + 2] << 16) | ((std::uint32_t)bytes[4 * k + 3] << 24));
        }
        return v;
    }
};

// bow_index.hpp:21-30 (MapId / KfId are plain integers here)
struct MapKf {
    std::int32_t mapId, kfId;
};
inline bool operator==(const MapKf &a, const MapKf &b) { return a.mapId == b.mapId && a.kfId == b.kfId; }
inline bool operator<(const MapKf &a, const MapKf &b) { return a.mapId == b.mapId ? a.kfId < b.kfId : a.mapId < b.mapId; }

struct BowSimilar {
    MapKf mapKf;
    float score;
};

class BowIndex {
public:
    BowIndex(Context &ctx, const VocabularyTree &tree) : ctx_(ctx), scoring_(tree.scoring) {
        for (std::int32_t w : tree.wordId) nWords_ = std::max(nWords_, w + 1);
        ctx_.check(ms_bow_vocab_create(ctx_.get(), (int)tree.size(), tree.parent.data(), tree.descriptor.data(), tree.weight.data(), tree.wordId.data(),
                                       tree.depthLevels, &vocab_), "ms_bow_vocab_create");
    }
    ~BowIndex() { ms_bow_db_destroy(db_); ms_bow_vocab_destroy(vocab_); }
    BowIndex(const BowIndex &) = delete;

    // bow_index.cpp:59-93
    void transform(const KeyPointVector &keypoints, BowVector &bowVector, FeatureVector &bowFeatureVector) {
        const int levelsUp = 4;                                                   // bow_index.cpp:85
        const std::size_t n = keypoints.size();
        bowVector.clear(); bowFeatureVector.clear();
        if (n == 0) return;
        reserve(n);
        host_desc_.resize(8 * n);
        for (std::size_t i = 0; i < n; ++i) for (int k = 0; k < 8; ++k) host_desc_[8 * i + k] = keypoints[i].descriptor[k];
        d_desc_.upload(0, 8 * n, host_desc_.data());
        ctx_.check(ms_bow_transform(ctx_.get(), vocab_, d_desc_.data(), (int)n, levelsUp, d_word_.data(), d_weight_.data(), d_node_.data()), "ms_bow_transform");
        word_.resize(n); weight_.resize(n); node_.resize(n);                      // host buffers reused across calls
        ctx_.check(ms_dev_download(ctx_.get(), word_.data(), d_word_.data(), 4 * n), "ms_dev_download");
        ctx_.check(ms_dev_download(ctx_.get(), weight_.data(), d_weight_.data(), 8 * n), "ms_dev_download");
        ctx_.check(ms_dev_download(ctx_.get(), node_.data(), d_node_.data(), 4 * n), "ms_dev_download");
        assemble(word_, weight_, node_, bowVector, bowFeatureVector);
    }

    // DBoW2's batch transform after the per-feature descents (TF_IDF / TF weighting, L1 scoring): host only
    static void assemble(const std::vector<std::int32_t> &word, const std::vector<double> &weight, const std::vector<std::int32_t> &node,
                         BowVector &v, FeatureVector &fv) {
        for (std::size_t i = 0; i < word.size(); ++i) {
            if (!(weight[i] > 0)) continue;                                       // stop words
            v[(unsigned)word[i]] += weight[i];                                    // BowVector::addWeight
            fv[(unsigned)node[i]].push_back((unsigned)i);                         // FeatureVector::addFeature
        }
        double norm = 0.0;
        for (const auto &kv : v) norm += std::fabs(kv.second);                    // BowVector::normalize(L1)
        if (norm > 0.0) for (auto &kv : v) kv.second /= norm;
    }

    // assemble without the FeatureVector, for a keyframe whose node lists ms_keyframe_admit built on the device (admitKeyframe): the
    // same sums in the same feature order, so the same bits
    static void assembleVector(const std::vector<std::int32_t> &word, const std::vector<double> &weight, BowVector &v) {
        for (std::size_t i = 0; i < word.size(); ++i) {
            if (!(weight[i] > 0)) continue;
            v[(unsigned)word[i]] += weight[i];
        }
        double norm = 0.0;
        for (const auto &kv : v) norm += std::fabs(kv.second);
        if (norm > 0.0) for (auto &kv : v) kv.second /= norm;
    }
    const ms_bow_vocab *vocabulary() const { return vocab_; }                     // the device tree, for ms_keyframe_admit

    // bow_index.cpp:44-48: the reference passes the keyframe (its shared->bowVec and id) and the map id
    void add(const BowVector &bowVec, MapKf mapKf) {
        requireL1();
        if (!db_) ctx_.check(ms_bow_db_create(ctx_.get(), std::max(nWords_, 1), 1024, 1024ll * 500, &db_), "ms_bow_db_create");
        flatten(bowVec);
        ctx_.check(ms_bow_db_add(db_, mapKf.mapId, mapKf.kfId, (int)qWords_.size(), qWords_.data(), qValues_.data()), "ms_bow_db_add");
    }

    // add for a keyframe whose descent lies on the DEVICE (ms_bow_db_add_words): wordDev / weightDev [n] as ms_bow_transform and
    // ms_keyframe_admit write them.  The device does assembleVector's sums in assembleVector's order and packs the vector into the
    // database's pool; no host vector exists.  Returns the entry's number of words.
    int addWords(const std::int32_t *wordDev, const double *weightDev, int n, MapKf mapKf) {
        requireL1();
        ensureDatabase();
        std::int32_t nWords = 0;
        ctx_.check(ms_bow_db_add_words(db_, mapKf.mapId, mapKf.kfId, wordDev, weightDev, n, &nWords), "ms_bow_db_add_words");
        return (int)nWords;
    }

    // add for the keyframe the context's latest ms_keyframe_admit admitted (admitKeyframe, or a direct call that passed NULL for the
    // admission's host word / weight): the descent is taken where that call left it (ms_keyframe_admit_words)
    int addAdmitted(MapKf mapKf) {
        const std::int32_t *word = nullptr;
        const double *weight = nullptr;
        std::int32_t n = 0;
        ctx_.check(ms_keyframe_admit_words(ctx_.get(), &word, &weight, &n), "ms_keyframe_admit_words");
        return addWords(word, weight, (int)n, mapKf);
    }

    // a live entry's BowVector, downloaded (ms_bow_db_entry): what keyframe.shared->bowVec held, e.g. for serialization
    BowVector bowVector(MapKf mapKf) {
        ensureDatabase();
        int n = 0;
        for (;;) {
            entryWords_.resize(entryCap_); entryValues_.resize(entryCap_);
            const int rc = ms_bow_db_entry(db_, mapKf.mapId, mapKf.kfId, (int)entryCap_, entryWords_.data(), entryValues_.data(), &n);
            if (rc != MS_ERR_CAPACITY) { ctx_.check(rc, "ms_bow_db_entry"); break; }
            entryCap_ = (std::size_t)n;
        }
        BowVector v;
        for (int i = 0; i < n; ++i) v.emplace_hint(v.end(), (unsigned)entryWords_[(std::size_t)i], entryValues_[(std::size_t)i]);
        return v;
    }

    // bow_index.cpp:50-57
    void remove(MapKf mapKf) {
        if (db_) ctx_.check(ms_bow_db_remove(db_, mapKf.mapId, mapKf.kfId), "ms_bow_db_remove");
    }

    // bow_index.cpp:95-176: `current` is the query keyframe's own id ({CURRENT_MAP_ID, kf.id}, :100); the ratios are the
    // reference's parameters.bowMinInCommonRatio and parameters.bowScoreRatio
    std::vector<BowSimilar> getBowSimilar(const BowVector &query, MapKf current, float minInCommonRatio, float scoreRatio) {
        requireL1();
        if (!db_) return {};
        flatten(query);
        int total = 0;
        for (;;) {
            outMap_.resize(outCap_); outKf_.resize(outCap_); outScore_.resize(outCap_);
            ctx_.check(ms_bow_db_query(db_, (int)qWords_.size(), qWords_.data(), qValues_.data(), current.mapId, current.kfId, minInCommonRatio, scoreRatio,
                                       (int)outCap_, outMap_.data(), outKf_.data(), outScore_.data(), &total), "ms_bow_db_query");
            if ((std::size_t)total <= outCap_) break;
            outCap_ = (std::size_t)total;
        }
        std::vector<BowSimilar> similar((std::size_t)total);
        for (int i = 0; i < total; ++i) similar[(std::size_t)i] = BowSimilar{MapKf{outMap_[(std::size_t)i], outKf_[(std::size_t)i]}, outScore_[(std::size_t)i]};
        return similar;
    }

private:
    void requireL1() const {
        if (scoring_ != 0)
            throw std::runtime_error("mi355slam: BowIndex add / getBowSimilar support L1 scoring only (vocabulary scoring type " + std::to_string(scoring_) + ")");
    }
    void ensureDatabase() {                                                       // the sizes add() creates it with
        if (!db_) ctx_.check(ms_bow_db_create(ctx_.get(), std::max(nWords_, 1), 1024, 1024ll * 500, &db_), "ms_bow_db_create");
    }
    void flatten(const BowVector &v) {
        qWords_.clear(); qValues_.clear();
        for (const auto &kv : v) { qWords_.push_back((std::int32_t)kv.first); qValues_.push_back(kv.second); }
    }
    void reserve(std::size_t n) {
        if (n <= cap_) return;
        // free, forget the capacity, allocate, and only then record it (the order of Context::workspace): a failed allocation leaves no buffers and capacity 0
        d_desc_.reset(); d_word_.reset(); d_weight_.reset(); d_node_.reset();
        cap_ = 0;
        const std::size_t cap = n + n / 2 + 64;
        DeviceArray<std::uint32_t> desc(ctx_, 8 * cap);
        DeviceArray<std::int32_t> word(ctx_, cap);
        DeviceArray<double> weight(ctx_, cap);
        DeviceArray<std::int32_t> node(ctx_, cap);
        d_desc_ = std::move(desc); d_word_ = std::move(word); d_weight_ = std::move(weight); d_node_ = std::move(node);
        cap_ = cap;
    }
    Context &ctx_;
    int scoring_ = 0, nWords_ = 0;
    ms_bow_vocab *vocab_ = nullptr;
    ms_bow_db *db_ = nullptr;                                                     // created on the first add
    std::vector<std::int32_t> qWords_, outMap_, outKf_;
    std::vector<double> qValues_;
    std::vector<float> outScore_;
    std::size_t outCap_ = 64;
    std::vector<std::int32_t> entryWords_;                                        // bowVector's download
    std::vector<double> entryValues_;
    std::size_t entryCap_ = 512;
    DeviceArray<std::uint32_t> d_desc_;
    DeviceArray<std::int32_t> d_word_, d_node_;
    DeviceArray<double> d_weight_;
    std::size_t cap_ = 0;                                                         // keypoints the four buffers hold
    std::vector<std::uint32_t> host_desc_;
    std::vector<std::int32_t> word_, node_;
    std::vector<double> weight_;
};

}  // namespace mi355slam
