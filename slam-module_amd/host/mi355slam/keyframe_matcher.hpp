// keyframe_matcher.hpp -- host mirror of the free functions of keyframe_matcher.hpp:33-91.
//
// The reference's Keyframe / MapDB carry the graph; the device only needs flat per-keyframe arrays, so a
// KeyframeFeatures view is built once per keyframe (INTEGRATION.md shows the 15 lines that fill it from
// kf.shared->keyPoints, kf.mapPoints and kf.shared->bowFeatureVec) and uploaded by DeviceKeyframe.
#pragma once
#include <algorithm>
#include <cstring>
#include <array>
#include <map>
#include <stdexcept>
#include <utility>
#include "common.hpp"
#include "optimize_transform.hpp"

namespace mi355slam {

constexpr unsigned HAMMING_DIST_THR_LOW = MS_HAMMING_THR_LOW, HAMMING_DIST_THR_HIGH = MS_HAMMING_THR_HIGH, MAX_HAMMING_DIST = MS_HAMMING_MAX;

struct KeyframeFeatures {
    const KeyPointVector *keyPoints = nullptr;                              // kf.shared->keyPoints
    std::vector<std::uint8_t> usable;                                        // per keypoint: the matcher-specific map-point gate
    std::map<unsigned, std::vector<unsigned>> bowFeatureVec;                  // DBoW2::FeatureVector (ordered node -> keypoint indices)
};

// Device-resident copy of one keyframe's matcher inputs.
class DeviceKeyframe {
public:
    DeviceKeyframe(Context &ctx, const KeyframeFeatures &kf) : ctx_(ctx) {
        const auto &kps = *kf.keyPoints;
        const std::size_t n = kps.size();
        std::vector<std::uint32_t> desc(8 * n); std::vector<float> ang(n); std::vector<std::int32_t> oct(n); std::vector<double> bear(3 * n);
        for (std::size_t i = 0; i < n; ++i) {
            for (int k = 0; k < 8; ++k) desc[8 * i + k] = kps[i].descriptor[k];
            ang[i] = kps[i].angle; oct[i] = kps[i].octave;
            for (int k = 0; k < 3; ++k) bear[3 * i + k] = kps[i].bearing[k];
        }
        std::vector<std::int32_t> node_id, node_start{0}, kp_idx;
        for (const auto &kv : kf.bowFeatureVec) {                             // std::map iterates node ids ascending
            node_id.push_back((std::int32_t)kv.first);
            for (unsigned i : kv.second) kp_idx.push_back((std::int32_t)i);
            node_start.push_back((std::int32_t)kp_idx.size());
        }
        f_.n = (std::int32_t)n;
        f_.desc = up(desc); f_.angle = up(ang); f_.octave = up(oct); f_.bearing = up(bear); f_.usable = up(kf.usable);
        f_.bow.n_nodes = (std::int32_t)node_id.size(); f_.bow.node_id = up(node_id); f_.bow.node_start = up(node_start); f_.bow.kp_idx = up(kp_idx);
        // FeatureSearch::create (feature_search.cpp:22-30): the keypoints sorted by y, for the radius queries of M3-M5
        std::vector<float> x(n), y(n), sx(n), sy(n); std::vector<std::int32_t> si(n);
        for (std::size_t i = 0; i < n; ++i) { x[i] = kps[i].pt.x; y[i] = kps[i].pt.y; }
        ctx_.check(ms_feature_search_sort(x.data(), y.data(), (int)n, sx.data(), sy.data(), si.data()), "ms_feature_search_sort");
        sx_ = up(sx); sy_ = up(sy); si_ = up(si);
        // host copies of what a single query's scan needs (searchByProjectionCore settles the rare query whose top-4 list ran out right here,
        // instead of a round trip to the device): 48 bytes per keypoint
        hsx_ = std::move(sx); hsy_ = std::move(sy); hsi_ = std::move(si); hdesc_ = std::move(desc); hoct_ = std::move(oct);
    }
    const std::vector<float> &hostSortedX() const { return hsx_; }
    const std::vector<float> &hostSortedY() const { return hsy_; }
    const std::vector<std::int32_t> &hostSortedIndex() const { return hsi_; }
    const std::uint32_t *hostDescriptor(std::size_t i) const { return hdesc_.data() + 8 * i; }
    int hostOctave(std::size_t i) const { return hoct_[i]; }
    const float *sortedX() const { return sx_; }
    const float *sortedY() const { return sy_; }
    const std::int32_t *sortedIndex() const { return si_; }
    ~DeviceKeyframe() { for (void *p : owned_) ms_dev_free(ctx_.get(), p); }
    DeviceKeyframe(const DeviceKeyframe &) = delete;
    const ms_match_frame &frame() const { return f_; }
private:
    template <typename T> const T *up(const std::vector<T> &v) {
        void *d = nullptr;
        ctx_.check(ms_dev_alloc(ctx_.get(), v.size() * sizeof(T) + 16, &d), "ms_dev_alloc");
        owned_.push_back(d);
        if (!v.empty()) ctx_.check(ms_dev_upload(ctx_.get(), d, v.data(), v.size() * sizeof(T)), "ms_dev_upload");
        return static_cast<const T *>(d);
    }
    Context &ctx_;
    ms_match_frame f_{};
    const float *sx_ = nullptr, *sy_ = nullptr;
    const std::int32_t *si_ = nullptr;
    std::vector<float> hsx_, hsy_;
    std::vector<std::int32_t> hsi_, hoct_;
    std::vector<std::uint32_t> hdesc_;
    std::vector<void *> owned_;
};

namespace detail {
inline std::size_t pad16(std::size_t n) { return (n + 15) / 16 * 16; }

inline unsigned run_greedy(Context &ctx, bool triangulation, const DeviceKeyframe &kf1, const DeviceKeyframe &kf2, std::vector<int> &out,
                           float ratio, const double *E12, const std::vector<float> *scaleFactors, float thrDeg) {
    // one workspace block: [match count (16 B)][matched: n1 ints][E: 9 doubles][scale factors]; one upload (M2 only), one call, one download
    const std::size_t n1 = (std::size_t)kf1.frame().n;
    const std::size_t oM = 16, oE = oM + pad16(4 * n1), oS = oE + 80, total = oS + pad16(4 * (scaleFactors ? scaleFactors->size() : 0));
    unsigned char *ws = ctx.workspace(total);
    std::int32_t *mptr = reinterpret_cast<std::int32_t *>(ws + oM);
    ms_match_frame f1 = kf1.frame(), f2 = kf2.frame();
    int rc;
    if (triangulation) {
        std::vector<unsigned char> &st = ctx.staging();
        st.assign(total - oE, 0);
        std::memcpy(st.data(), E12, 72);
        std::memcpy(st.data() + 80, scaleFactors->data(), 4 * scaleFactors->size());
        ctx.check(ms_dev_upload(ctx.get(), ws + oE, st.data(), st.size()), "ms_dev_upload");
        rc = ms_match_triangulation(ctx.get(), &f1, &f2, 1, reinterpret_cast<const double *>(ws + oE), reinterpret_cast<const float *>(ws + oS), thrDeg, 1, &mptr,
                                    reinterpret_cast<std::int32_t *>(ws));
    } else {
        rc = ms_match_loop_closure(ctx.get(), &f1, &f2, 1, ratio, 1, &mptr, reinterpret_cast<std::int32_t *>(ws));
    }
    ctx.check(rc, "greedy matcher");
    std::vector<unsigned char> &st = ctx.staging();
    st.resize(oM + 4 * n1);
    ctx.check(ms_dev_download(ctx.get(), st.data(), ws, st.size()), "ms_dev_download");
    std::int32_t num = 0;
    std::memcpy(&num, st.data(), 4);
    out.assign(n1, -1);
    if (n1) std::memcpy(out.data(), st.data() + oM, 4 * n1);
    return (unsigned)num;
}
}  // namespace detail

// matchForLoopClosures (keyframe_matcher.hpp:33-40, keyframe_matcher.cpp:50-158).
// usable1 = keypoint has a map point (and it is TRIANGULATED when requireTringulationForLoopClosures, :79-84);
// usable2 = keypoint has a TRIANGULATED map point (:94-96).
inline unsigned matchForLoopClosures(Context &ctx, const DeviceKeyframe &kf1, const DeviceKeyframe &kf2,
                                     std::vector<int> &matchedMapPoints, const Parameters &parameters) {
    return detail::run_greedy(ctx, false, kf1, kf2, matchedMapPoints, parameters.loopClosureFeatureMatchLoweRatio, nullptr, nullptr, 0.f);
}

// matchForTriangulationDBoW (keyframe_matcher.hpp:53, keyframe_matcher.cpp:160-293).  usable = keypoint has NO map point.
// E12 = create_E_21(kf2.R, kf2.t, kf1.R, kf1.t) (keyframe_matcher.cpp:171-175), row-major.
inline std::vector<std::pair<int, int>> matchForTriangulationDBoW(Context &ctx, const DeviceKeyframe &kf1, const DeviceKeyframe &kf2,
                                                                  const double E12[9], const StaticSettings &settings) {
    std::vector<int> m;
    detail::run_greedy(ctx, true, kf1, kf2, m, 0.f, E12, &settings.scaleFactors, settings.parameters.epipolarCheckThresholdDegrees);
    std::vector<std::pair<int, int>> matches;                               // ascending idx_1 (:279-292)
    for (std::size_t i = 0; i < m.size(); ++i) if (m[i] >= 0) matches.emplace_back((int)i, m[i]);
    return matches;
}

// ---- projection-guided matchers (M3-M5) ---------------------------------------------------------------------------
// The caller keeps what touches the map graph: reprojection, distance / viewing-angle gates, predictScaleLevel, the
// radius query Keyframe::getFeaturesAround and all map mutation.  What it hands over per surviving map point is its
// descriptor and the candidate keypoint indices; the Hamming scoring runs on the GPU for all map points at once.
struct ProjectionQuery {
    KeyPoint::Descriptor descriptor;            // mp.descriptor
    std::vector<std::int32_t> candidates;       // indices from kf.getFeaturesAround(...) (keyframe_matcher.cpp:340-344, :473, :596)
};

// The same scan with the radius query done on the device: the reprojected position and the search radius instead of a candidate list
// (kf.getFeaturesAround(reprojection, radius, indices), keyframe_matcher.cpp:340-344 / :470-473 / :596).
struct RadiusQuery {
    KeyPoint::Descriptor descriptor;
    float x = 0, y = 0, radius = 0;
    std::int32_t minOctave = -0x7fffffff, maxOctave = 0x7fffffff;      // findMatchesTranformedMps keeps [pred - 1, pred] (:611)
};

// Per query the four best candidates in (distance, scan position) order -- ms_hamming_candidates_topk / ms_projection_topk -- and how many candidates
// were scored in all: with nScored <= 4 the list IS the candidate set.
struct CandidateLists {
    std::vector<std::int32_t> idx, octave, nScored;      // [4 n], [4 n], [n]
    std::vector<std::uint16_t> dist;                     // [4 n]
};

namespace detail {
// uploads the queries (one block), runs the scan, downloads the lists (one block)
inline CandidateLists score_candidates(Context &ctx, const DeviceKeyframe &kf, const std::vector<ProjectionQuery> &qs,
                                       const std::vector<std::uint8_t> *skip, std::size_t first = 0, std::size_t count = ~std::size_t(0)) {
    count = std::min(count, qs.size() - first);
    CandidateLists out;
    out.idx.assign(4 * count, -1); out.octave.assign(4 * count, -1); out.nScored.assign(count, 0); out.dist.assign(4 * count, MS_HAMMING_MAX);
    if (count == 0) return out;
    std::size_t nc = 0;
    for (std::size_t i = 0; i < count; ++i) nc += qs[first + i].candidates.size();
    const std::size_t nk = skip ? skip->size() : 0;
    const std::size_t oD = 0, oS = oD + 32 * count, oI = oS + pad16(4 * (count + 1)), oK = oI + pad16(4 * nc), inBytes = oK + pad16(nk);
    const std::size_t oTi = inBytes, oTo = oTi + 16 * count, oN = oTo + 16 * count, oTd = oN + pad16(4 * count), total = oTd + pad16(8 * count);
    std::vector<unsigned char> &st = ctx.staging();
    st.assign(inBytes, 0);
    std::int32_t *start = reinterpret_cast<std::int32_t *>(st.data() + oS), *idx = reinterpret_cast<std::int32_t *>(st.data() + oI);
    std::size_t at = 0;
    for (std::size_t i = 0; i < count; ++i) {
        const ProjectionQuery &q = qs[first + i];
        std::memcpy(st.data() + oD + 32 * i, q.descriptor.data(), 32);
        start[i] = (std::int32_t)at;
        if (!q.candidates.empty()) std::memcpy(idx + at, q.candidates.data(), 4 * q.candidates.size());
        at += q.candidates.size();
    }
    start[count] = (std::int32_t)at;
    if (nk) std::memcpy(st.data() + oK, skip->data(), nk);
    unsigned char *ws = ctx.workspace(total);
    ctx.check(ms_dev_upload(ctx.get(), ws, st.data(), inBytes), "ms_dev_upload");
    const ms_match_frame &f = kf.frame();
    ctx.check(ms_hamming_candidates_topk(ctx.get(), reinterpret_cast<const std::uint32_t *>(ws + oD), (int)count, f.desc, reinterpret_cast<const std::int32_t *>(ws + oS),
                                         reinterpret_cast<const std::int32_t *>(ws + oI), nk ? ws + oK : nullptr, f.octave, reinterpret_cast<std::int32_t *>(ws + oTi),
                                         reinterpret_cast<std::uint16_t *>(ws + oTd), reinterpret_cast<std::int32_t *>(ws + oTo), reinterpret_cast<std::int32_t *>(ws + oN)),
              "ms_hamming_candidates_topk");
    st.resize(total - oTi);
    ctx.check(ms_dev_download(ctx.get(), st.data(), ws + oTi, total - oTi), "ms_dev_download");
    std::memcpy(out.idx.data(), st.data(), 16 * count); std::memcpy(out.octave.data(), st.data() + (oTo - oTi), 16 * count);
    std::memcpy(out.nScored.data(), st.data() + (oN - oTi), 4 * count); std::memcpy(out.dist.data(), st.data() + (oTd - oTi), 8 * count);
    return out;
}

inline CandidateLists score_candidates(Context &ctx, const DeviceKeyframe &kf, const std::vector<RadiusQuery> &qs,
                                       const std::vector<std::uint8_t> *skip, std::size_t first = 0, std::size_t count = ~std::size_t(0)) {
    count = std::min(count, qs.size() - first);
    CandidateLists out;
    out.idx.assign(4 * count, -1); out.octave.assign(4 * count, -1); out.nScored.assign(count, 0); out.dist.assign(4 * count, MS_HAMMING_MAX);
    if (count == 0) return out;
    const std::size_t nk = skip ? skip->size() : 0, sec = pad16(4 * count);
    const std::size_t oD = 0, oX = 32 * count, oY = oX + sec, oR = oY + sec, oLo = oR + sec, oHi = oLo + sec, oK = oHi + sec, inBytes = oK + pad16(nk);
    const std::size_t oTi = inBytes, oTo = oTi + 16 * count, oN = oTo + 16 * count, oTd = oN + sec, total = oTd + pad16(8 * count);
    std::vector<unsigned char> &st = ctx.staging();
    st.assign(inBytes, 0);
    float *x = reinterpret_cast<float *>(st.data() + oX), *y = reinterpret_cast<float *>(st.data() + oY), *r = reinterpret_cast<float *>(st.data() + oR);
    std::int32_t *lo = reinterpret_cast<std::int32_t *>(st.data() + oLo), *hi = reinterpret_cast<std::int32_t *>(st.data() + oHi);
    for (std::size_t i = 0; i < count; ++i) {
        const RadiusQuery &q = qs[first + i];
        std::memcpy(st.data() + oD + 32 * i, q.descriptor.data(), 32);
        x[i] = q.x; y[i] = q.y; r[i] = q.radius; lo[i] = q.minOctave; hi[i] = q.maxOctave;
    }
    if (nk) std::memcpy(st.data() + oK, skip->data(), nk);
    unsigned char *ws = ctx.workspace(total);
    ctx.check(ms_dev_upload(ctx.get(), ws, st.data(), inBytes), "ms_dev_upload");
    const ms_match_frame &f = kf.frame();
    ctx.check(ms_projection_topk(ctx.get(), kf.sortedX(), kf.sortedY(), kf.sortedIndex(), f.n, f.desc, f.octave, nk ? ws + oK : nullptr,
                                 reinterpret_cast<const float *>(ws + oX), reinterpret_cast<const float *>(ws + oY), reinterpret_cast<const float *>(ws + oR),
                                 reinterpret_cast<const std::int32_t *>(ws + oLo), reinterpret_cast<const std::int32_t *>(ws + oHi),
                                 reinterpret_cast<const std::uint32_t *>(ws + oD), (int)count, reinterpret_cast<std::int32_t *>(ws + oTi),
                                 reinterpret_cast<std::uint16_t *>(ws + oTd), reinterpret_cast<std::int32_t *>(ws + oTo), reinterpret_cast<std::int32_t *>(ws + oN), nullptr),
              "ms_projection_topk");
    st.resize(total - oTi);
    ctx.check(ms_dev_download(ctx.get(), st.data(), ws + oTi, total - oTi), "ms_dev_download");
    std::memcpy(out.idx.data(), st.data(), 16 * count); std::memcpy(out.octave.data(), st.data() + (oTo - oTi), 16 * count);
    std::memcpy(out.nScored.data(), st.data() + (oN - oTi), 4 * count); std::memcpy(out.dist.data(), st.data() + (oTd - oTi), 8 * count);
    return out;
}
}  // namespace detail

namespace detail {
struct Best2 { int best = -1, bestDist = 256, bestDist2 = 256, bestLevel = -1, bestLevel2 = -1; };
inline int hamming256(const std::uint32_t *a, const std::uint32_t *b) { int d = 0; for (int k = 0; k < 8; ++k) d += __builtin_popcount(a[k] ^ b[k]); return d; }
inline void best2_update(Best2 &b, int idx, int dist, int level) {                        // keyframe_matcher.cpp:369-377
    if (dist < b.bestDist) { b.bestDist2 = b.bestDist; b.bestDist = dist; b.bestLevel2 = b.bestLevel; b.bestLevel = level; b.best = idx; }
    else if (dist < b.bestDist2) { b.bestLevel2 = level; b.bestDist2 = dist; }
}
// one query's whole scan on the host, against the CURRENT mask (the reference's loop :356-378 as it stands); a handful of queries per keyframe get here
inline Best2 rescan_on_host(const DeviceKeyframe &kf, const ProjectionQuery &q, const std::vector<std::uint8_t> &bound) {
    Best2 b;
    for (std::int32_t j : q.candidates)
        if (!bound[(std::size_t)j]) best2_update(b, j, hamming256(q.descriptor.data(), kf.hostDescriptor((std::size_t)j)), kf.hostOctave((std::size_t)j));
    return b;
}
inline Best2 rescan_on_host(const DeviceKeyframe &kf, const RadiusQuery &q, const std::vector<std::uint8_t> &bound) {
    // FeatureSearch::getFeaturesAround (feature_search.cpp:33-48) in float32, every operation rounded on its own (a product or sum formed in double and
    // rounded to float IS the float32 result, so the compiler's contraction setting cannot change it) -- the same arithmetic as k_projection_candidates
    const std::vector<float> &sx = kf.hostSortedX(), &sy = kf.hostSortedY();
    const float ylo = q.y - q.radius, yhi = q.y + q.radius, r2 = (float)((double)q.radius * (double)q.radius);
    Best2 b;
    for (std::size_t pos = (std::size_t)(std::lower_bound(sy.begin(), sy.end(), ylo) - sy.begin()); pos < sy.size() && sy[pos] <= yhi; ++pos) {
        const float dx = q.x - sx[pos], dy = q.y - sy[pos];
        const float dx2 = (float)((double)dx * (double)dx), dy2 = (float)((double)dy * (double)dy);
        if (!((float)((double)dx2 + (double)dy2) < r2)) continue;
        const std::size_t j = (std::size_t)kf.hostSortedIndex()[pos];
        if (bound[j] || kf.hostOctave(j) < q.minOctave || kf.hostOctave(j) > q.maxOctave) continue;
        best2_update(b, (int)j, hamming256(q.descriptor.data(), kf.hostDescriptor(j)), kf.hostOctave(j));
    }
    return b;
}

// The greedy replay of searchByProjection (keyframe_matcher.cpp:356-389) over the top-4 lists of queries [first, first + count) of `l`: per query
// the first two list entries that no earlier query of this call has bound are the reference's best and second best; a query whose list ran
// out before its candidate set did (fewer than two free entries, more than four scored) is settled by rescan(q) -> Best2 against the CURRENT
// mask.  accepted(q, keypoint) is called for every match, in walk order; `bound` is updated.  Returns the number of rescans.
template <class Rescan, class Accepted>
inline unsigned replay_search(const CandidateLists &l, std::size_t first, std::size_t count, std::vector<std::uint8_t> &bound, Rescan rescan, Accepted accepted) {
    std::vector<std::uint8_t> taken(bound.size(), 0);            // bound during this call
    unsigned again = 0;
    for (std::size_t q = first; q < first + count; ++q) {
        Best2 b;
        int found = 0;
        for (int e = 0; e < 4 && found < 2; ++e) {
            const int j = l.idx[4 * q + e];
            if (j < 0) break;
            if (taken[(std::size_t)j]) continue;
            if (found == 0) { b.best = j; b.bestDist = l.dist[4 * q + e]; b.bestLevel = l.octave[4 * q + e]; }
            else { b.bestDist2 = l.dist[4 * q + e]; b.bestLevel2 = l.octave[4 * q + e]; }
            ++found;
        }
        if (found < 2 && l.nScored[q] > 4) { b = rescan(q); ++again; }                         // `bound` = initial mask + everything taken so far
        if (b.best == -1) continue;                                                          // :380
        if (b.bestDist <= (int)HAMMING_DIST_THR_HIGH) {                                        // :382-383
            if (b.bestLevel == b.bestLevel2 && b.bestDist > 0.8 * b.bestDist2) continue;       // :385-386
            accepted(q, b.best); bound[(std::size_t)b.best] = 1; taken[(std::size_t)b.best] = 1;
        }
    }
    return again;
}

// replaceDuplication (:479-499) / findMatchesTranformedMps (:600-627): the best candidate of query q when it is close enough, else -1
inline int best_candidate(const CandidateLists &l, std::size_t q, unsigned maxDist) {
    return l.idx[4 * q] >= 0 && l.dist[4 * q] <= maxDist ? l.idx[4 * q] : -1;
}
}  // namespace detail

// Scoring + accept rule of searchByProjection (keyframe_matcher.cpp:349-389).  `bound[k]` != 0 marks keypoints that already
// carry an observed map point (:358-360); it is updated as matches are accepted, in query order, exactly like the
// reference's loop.  ONE launch scores every query against the initial mask and returns its four best candidates; the replay below
// walks the queries in order and takes, per query, the first two list entries that no earlier query of this call has bound -- the
// best and second best of the reference's scan over the keypoints still free (the scan order is the list's tie-break).  A query whose
// list is too short for that (more than four candidates in all, and fewer than two of its four best still free: three of its four best
// went to earlier map points of the same call) is scanned again on the host against the current mask (detail::rescan_on_host).
// Returns, per query, the matched keypoint index or -1; the caller performs addObservation (:388-389).
// `Query` is ProjectionQuery (candidate lists from the host's getFeaturesAround) or RadiusQuery (radius query on the device).
template <class Query>
inline std::vector<int> searchByProjectionCore(Context &ctx, const DeviceKeyframe &kf, const std::vector<Query> &queries,
                                               std::vector<std::uint8_t> &bound, unsigned *rescored = nullptr) {
    std::vector<int> match(queries.size(), -1);
    const CandidateLists s = detail::score_candidates(ctx, kf, queries, &bound);
    const unsigned again = detail::replay_search(s, 0, queries.size(), bound, [&](std::size_t q) { return detail::rescan_on_host(kf, queries[q], bound); },
                                                 [&](std::size_t q, int best) { match[q] = best; });
    if (rescored) *rescored = again;
    return match;
}

// Scoring of replaceDuplication (keyframe_matcher.cpp:479-499: best only, accept <= 50) and findMatchesTranformedMps
// (:600-627: accept <= 100; the caller pre-filters candidates by octave, :611).  No greedy state in the scoring itself.
template <class Query>
inline std::vector<int> bestCandidateCore(Context &ctx, const DeviceKeyframe &kf, const std::vector<Query> &queries, unsigned maxDist) {
    const CandidateLists s = detail::score_candidates(ctx, kf, queries, nullptr);
    std::vector<int> match(queries.size(), -1);
    for (std::size_t i = 0; i < queries.size(); ++i) match[i] = detail::best_candidate(s, i, maxDist);
    return match;
}

// MapPoint::updateDescriptor (map_point.cpp:75-116) for many map points in one launch.  observations[p] lists, for map
// point p, the descriptors of its observing keypoints (the caller gathers kf.shared->keyPoints.at(obs.second.v).descriptor
// for keyframes with hasFeatureDescriptors(), :78-84, in the order of the observations map).  Returns the position of the
// chosen descriptor in that list, or -1 for an empty list (the reference then leaves `descriptor` untouched, :86).
inline std::vector<int> updateDescriptors(Context &ctx, const std::vector<std::vector<KeyPoint::Descriptor>> &observations) {
    const std::size_t n = observations.size();
    std::vector<int> best(n, -1);
    if (n == 0) return best;
    std::vector<std::uint32_t> pool;
    std::vector<std::int32_t> start(n + 1, 0), idx;
    std::size_t longest = 0;
    for (std::size_t p = 0; p < n; ++p) {
        for (const KeyPoint::Descriptor &d : observations[p]) { idx.push_back((std::int32_t)(pool.size() / 8)); pool.insert(pool.end(), d.begin(), d.end()); }
        start[p + 1] = (std::int32_t)idx.size();
        longest = std::max(longest, observations[p].size());
    }
    std::vector<void *> bufs;
    auto up = [&](const void *src, std::size_t bytes) { void *d = nullptr; ctx.check(ms_dev_alloc(ctx.get(), bytes + 32, &d), "ms_dev_alloc"); bufs.push_back(d);
                                                         if (bytes && src) { ctx.check(ms_dev_upload(ctx.get(), d, src, bytes), "ms_dev_upload"); }
                                                         return d; };
    void *dp = up(pool.data(), pool.size() * 4), *ds = up(start.data(), start.size() * 4), *di = up(idx.data(), idx.size() * 4);
    void *out = up(nullptr, 4 * n);
    const int rc = ms_descriptor_medoid(ctx.get(), static_cast<const std::uint32_t *>(dp), static_cast<const std::int32_t *>(ds),
                                        static_cast<const std::int32_t *>(di), (int)n, (int)longest, static_cast<std::int32_t *>(out), nullptr);
    if (rc == MS_OK) ctx.check(ms_dev_download(ctx.get(), best.data(), out, 4 * n), "download");
    for (void *p : bufs) ms_dev_free(ctx.get(), p);
    ctx.check(rc, "ms_descriptor_medoid");
    return best;
}

// ---- M5: findMatchesTranformedMps + matchMapPointsSim3 (keyframe_matcher.cpp:552-686) ------------------------------------
// One map point of keyframe A as findMatchesTranformedMps sees it after the part that needs the map graph and the camera model
// (:572-596): `usable` = has a map point (mpId != -1), TRIANGULATED, reprojectToImage succeeded, the viewing distance |R X + t| lies in
// [minViewingDistance, maxViewingDistance]; (x, y) = the reprojection into keyframe B; predScaleLevel = mp.predictScaleLevel(...).
struct Sim3Projection {
    bool usable = false;
    KeyPoint::Descriptor descriptor{};          // mp.descriptor
    float x = 0, y = 0;
    int predScaleLevel = 0;
};

// findMatchesTranformedMps (:552-631): matches[iA] = index of the best keypoint of kfB (radius margin * scaleFactors[pred], octave in
// [pred - 1, pred], strictly smaller distance wins = first of the radius query's order, accepted at <= HAMMING_DIST_THR_HIGH) or -1.
inline std::vector<int> findMatchesTranformedMps(Context &ctx, const std::vector<Sim3Projection> &mpsA, const std::vector<bool> &alreadyMatchedInA,
                                                 const DeviceKeyframe &kfB, float margin, const StaticSettings &settings) {
    std::vector<int> matchesAtoB(mpsA.size(), -1);
    std::vector<RadiusQuery> qs;
    std::vector<std::size_t> owner;
    for (std::size_t indA = 0; indA < mpsA.size(); ++indA) {
        if (alreadyMatchedInA.at(indA) || !mpsA[indA].usable) continue;                        // :566-590
        const Sim3Projection &m = mpsA[indA];
        RadiusQuery q;
        q.descriptor = m.descriptor; q.x = m.x; q.y = m.y;
        q.radius = margin * settings.scaleFactors.at((std::size_t)m.predScaleLevel);           // :596
        q.minOctave = m.predScaleLevel - 1; q.maxOctave = m.predScaleLevel;                    // :611
        qs.push_back(q); owner.push_back(indA);
    }
    const std::vector<int> best = bestCandidateCore(ctx, kfB, qs, HAMMING_DIST_THR_HIGH);     // :600-627
    for (std::size_t i = 0; i < qs.size(); ++i) matchesAtoB[owner[i]] = best[i];
    return matchesAtoB;
}

// matchMapPointsSim3 (:633-686) on keypoint indices: `matches` holds (index in kf1, index in kf2) pairs -- the reference keeps
// (MpId, MpId) and looks the indices up through mapPoints.at(id).observations.at(kf.id) (:645-648); the caller does that lookup and the
// reverse one (kf.mapPoints.at(index)) for the pairs appended here.  mps1in2 = kf1's map points projected into kf2 with
// transform12^-1 * kf1.poseCW (:650), mps2in1 = kf2's into kf1 with transform12 * kf2.poseCW (:661).  Returns the number added.
inline unsigned matchMapPointsSim3(Context &ctx, const DeviceKeyframe &kf1, const DeviceKeyframe &kf2, const std::vector<Sim3Projection> &mps1in2,
                                   const std::vector<Sim3Projection> &mps2in1, std::vector<std::pair<int, int>> &matches, const StaticSettings &settings) {
    constexpr float margin = 7.5;                                                              // :641
    // keypoints that already carry a match are left out of both searches (:645-648)
    std::vector<bool> taken1(mps1in2.size(), false), taken2(mps2in1.size(), false);
    for (const std::pair<int, int> &m : matches) { taken1.at((std::size_t)m.first) = true; taken2.at((std::size_t)m.second) = true; }
    const std::vector<int> fwd = findMatchesTranformedMps(ctx, mps1in2, taken1, kf2, margin, settings);      // kf1 keypoint -> kf2 keypoint or -1
    const std::vector<int> bwd = findMatchesTranformedMps(ctx, mps2in1, taken2, kf1, margin, settings);      // kf2 keypoint -> kf1 keypoint or -1
    // a pair is kept when each side names the other (:672-685), in ascending kf1 index
    const std::size_t before = matches.size();
    for (std::size_t i1 = 0; i1 < fwd.size(); ++i1)
        if (fwd[i1] >= 0 && bwd.at((std::size_t)fwd[i1]) == (int)i1) matches.emplace_back((int)i1, fwd[i1]);
    return (unsigned)(matches.size() - before);
}

// ---- M3-M5 with the gates on the device (ms_project_gate) ------------------------------------------------------------------------
// The per-map-point loop in front of the three matchers (reprojection, viewing distance, viewing angle, predictScaleLevel, radius;
// keyframe_matcher.cpp:313-345, :442-471, :573-596) runs on the device over a table of map points that lives there, and its output IS the
// query block of ms_projection_topk: no query array is built or uploaded by the host.  What reads the map graph stays with the caller
// (observations.count, the BAD / NOT_TRIANGULATED test, erasedMapPointIds): it passes the rows that survive those filters, in walk order.

// Keyframe poses on the device, one slot per keyframe: rows 0-2 of poseCW, row-major (12 doubles).  What ms_map_refresh reads the camera
// centres from and ms_loop_correct corrects in place.  update() re-uploads a range after the host changed poses (bundle adjustment).
class DeviceKeyframePoses {
public:
    using Pose = std::array<double, 12>;
    DeviceKeyframePoses(Context &ctx, const std::vector<Pose> &poseCW) : ctx_(ctx), n_(poseCW.size()) {
        ctx_.check(ms_dev_alloc(ctx_.get(), 96 * n_ + 16, &pose_), "ms_dev_alloc");
        update(0, n_, poseCW.data());
    }
    ~DeviceKeyframePoses() { ms_dev_free(ctx_.get(), pose_); }
    DeviceKeyframePoses(const DeviceKeyframePoses &) = delete;
    void update(std::size_t first, std::size_t count, const Pose *poseCW) {
        if (first + count > n_) throw std::runtime_error("DeviceKeyframePoses::update: range outside the table");
        if (count) ctx_.check(ms_dev_upload(ctx_.get(), static_cast<double *>(pose_) + 12 * first, poseCW, 96 * count), "ms_dev_upload");
    }
    std::vector<Pose> download() const {
        std::vector<Pose> out(n_);
        if (n_) ctx_.check(ms_dev_download(ctx_.get(), out.data(), pose_, 96 * n_), "ms_dev_download");
        return out;
    }
    std::size_t size() const { return n_; }
    double *pose() const { return static_cast<double *>(pose_); }
private:
    Context &ctx_;
    std::size_t n_;
    void *pose_ = nullptr;
};

// Keypoint descriptors on the device, the pool MapObservation::descriptor indexes (the descriptors of the keyframes' keypoints, uploaded as the
// keyframes arrive).
class DeviceDescriptorPool {
public:
    DeviceDescriptorPool(Context &ctx, const std::vector<KeyPoint::Descriptor> &descriptors) : ctx_(ctx), n_(descriptors.size()) {
        ctx_.check(ms_dev_alloc(ctx_.get(), 32 * n_ + 16, &desc_), "ms_dev_alloc");
        if (n_) ctx_.check(ms_dev_upload(ctx_.get(), desc_, descriptors.data(), 32 * n_), "ms_dev_upload");
    }
    ~DeviceDescriptorPool() { ms_dev_free(ctx_.get(), desc_); }
    DeviceDescriptorPool(const DeviceDescriptorPool &) = delete;
    std::size_t size() const { return n_; }
    const std::uint32_t *descriptor() const { return static_cast<const std::uint32_t *>(desc_); }
private:
    Context &ctx_;
    std::size_t n_;
    void *desc_ = nullptr;
};

// One entry of MapPoint::observations as the refresh reads it: the observing keyframe's slot in DeviceKeyframePoses and the observing
// keypoint's descriptor in the pool (-1: the keyframe has no descriptors, map_point.cpp:80).
struct MapObservation {
    std::int32_t keyframe = 0;
    std::int32_t descriptor = -1;
};

// The map points the gates read, structure-of-arrays on the device.  Row i = one MapPoint: position, norm, minViewingDistance,
// maxViewingDistance, descriptor.  update() uploads a range the host computed; refresh() recomputes rows where they lie (MapPoint::updateDistanceAndNorm /
// updateDescriptor on the device), and mi355slam::correctLoop moves positions there.
class DeviceMapPoints {
public:
    using Vec3d = std::array<double, 3>;
    using Vec3f = std::array<float, 3>;
    DeviceMapPoints(Context &ctx, const std::vector<Vec3d> &position, const std::vector<Vec3f> &norm, const std::vector<float> &minDistance,
                    const std::vector<float> &maxDistance, const std::vector<KeyPoint::Descriptor> &descriptor) : ctx_(ctx), n_(position.size()) {
        if (norm.size() != n_ || minDistance.size() != n_ || maxDistance.size() != n_ || descriptor.size() != n_)
            throw std::runtime_error("DeviceMapPoints: the arrays describe different numbers of map points");
        pos_ = alloc<double>(3 * n_); norm_ = alloc<float>(3 * n_); min_ = alloc<float>(n_); max_ = alloc<float>(n_); desc_ = alloc<std::uint32_t>(8 * n_);
        update(0, n_, position.data(), norm.data(), minDistance.data(), maxDistance.data(), descriptor.data());
    }
    ~DeviceMapPoints() { for (void *p : owned_) ms_dev_free(ctx_.get(), p); }
    DeviceMapPoints(const DeviceMapPoints &) = delete;
    // rows [first, first + count) of the fields that are not nullptr
    void update(std::size_t first, std::size_t count, const Vec3d *position, const Vec3f *norm, const float *minDistance, const float *maxDistance,
                const KeyPoint::Descriptor *descriptor) {
        if (first + count > n_) throw std::runtime_error("DeviceMapPoints::update: range outside the table");
        if (count == 0) return;
        if (position) up(pos_ + 3 * first, position, 24 * count);
        if (norm) up(norm_ + 3 * first, norm, 12 * count);
        if (minDistance) up(min_ + first, minDistance, 4 * count);
        if (maxDistance) up(max_ + first, maxDistance, 4 * count);
        if (descriptor) up(desc_ + 8 * first, descriptor, 32 * count);
    }
    // MapPoint::updateDescriptor + MapPoint::updateDistanceAndNorm (map_point.cpp:75-116, :158-172) for the rows `rows`, computed and written on the
    // device (ms_map_refresh).  observations[i] = row rows[i]'s observations in the order of the observations map (ascending KfId, so the first is
    // getFirstObservation()); firstOctave[i] = the octave of that first observation's keypoint (:168).  Without a pool the descriptors stay as
    // they are.  Returns, per row, the position of the chosen descriptor's observation in its list (-1 / -2: the row kept its descriptor).
    std::vector<int> refresh(Context &ctx, const DeviceKeyframePoses &poses, const std::vector<std::int32_t> &rows,
                             const std::vector<std::vector<MapObservation>> &observations, const std::vector<std::int32_t> &firstOctave,
                             const StaticSettings &settings, const DeviceDescriptorPool *pool = nullptr) {
        if (observations.size() != rows.size() || firstOctave.size() != rows.size())
            throw std::invalid_argument("DeviceMapPoints::refresh: one observation list and one octave per row");
        std::vector<std::int32_t> start(rows.size() + 1, 0), kf, desc;
        for (std::size_t i = 0; i < rows.size(); ++i) {
            for (const MapObservation &o : observations[i]) { kf.push_back(o.keyframe); desc.push_back(o.descriptor); }
            start[i + 1] = (std::int32_t)kf.size();
        }
        std::vector<std::int32_t> medoid(rows.size(), -1);
        ctx.check(ms_map_refresh(ctx.get(), pos_, norm_, min_, max_, desc_, (int)n_, poses.pose(), (int)poses.size(), pool ? pool->descriptor() : nullptr,
                                 pool ? (int)pool->size() : 0, rows.data(), (int)rows.size(), start.data(), kf.data(), pool ? desc.data() : nullptr,
                                 firstOctave.data(), settings.scaleFactors.data(), (int)settings.scaleFactors.size(), medoid.data()), "ms_map_refresh");
        return std::vector<int>(medoid.begin(), medoid.end());
    }
    double *mutablePosition() { return pos_; }
    float *mutableNorm() { return norm_; }                   // what updateMapPoints writes, with the two distances and the descriptors
    float *mutableMinDistance() { return min_; }
    float *mutableMaxDistance() { return max_; }
    std::uint32_t *mutableDescriptor() { return desc_; }
    std::size_t size() const { return n_; }
    const double *position() const { return pos_; }
    const float *norm() const { return norm_; }
    const float *minDistance() const { return min_; }
    const float *maxDistance() const { return max_; }
    const std::uint32_t *descriptor() const { return desc_; }
private:
    template <typename T> T *alloc(std::size_t n) {
        void *d = nullptr;
        ctx_.check(ms_dev_alloc(ctx_.get(), n * sizeof(T) + 16, &d), "ms_dev_alloc");
        owned_.push_back(d);
        return static_cast<T *>(d);
    }
    void up(void *dst, const void *src, std::size_t bytes) { ctx_.check(ms_dev_upload(ctx_.get(), dst, src, bytes), "ms_dev_upload"); }
    Context &ctx_;
    std::size_t n_;
    double *pos_ = nullptr;
    float *norm_ = nullptr, *min_ = nullptr, *max_ = nullptr;
    std::uint32_t *desc_ = nullptr;
    std::vector<void *> owned_;
};

// The keyframes LoopCloser::correctLoop moves (loop_closer.cpp:420-470), as slots of DeviceKeyframePoses: rigid = a member of
// rigidlyTransformedKfIds (:427, T itself), otherwise lambda = (t - t0) / (t1 - t0) of :458.
struct LoopCorrections {
    std::vector<std::int32_t> slot;
    std::vector<std::uint8_t> rigid;
    std::vector<double> lambda;
};
// localMapPoints (:418, :429-433, :465-469) as table rows: row[j] moves with the keyframe at position reference[j] of LoopCorrections::slot.
struct LoopPoints {
    std::vector<std::int32_t> row, reference;
};
// What DeviceMapPoints::refresh takes for the moved points (:504-505).
struct RefreshArgs {
    std::vector<std::int32_t> rows;
    std::vector<std::vector<MapObservation>> observations;
    std::vector<std::int32_t> firstOctave;
    const DeviceDescriptorPool *pool = nullptr;
};

// LoopCloser::correctLoop from the pose correction to the refresh of the moved map points (loop_closer.cpp:398-506) on the device tables:
// ms_loop_correct (poses, then points), then DeviceMapPoints::refresh of refreshArgs.rows.  T = the Sim3 of :405.  Re-triangulation (:508-523)
// stays with the caller.  Returns refresh's medoids.
inline std::vector<int> correctLoop(Context &ctx, DeviceMapPoints &table, DeviceKeyframePoses &poses, const Sim3 &T, const LoopCorrections &corrections,
                                    const LoopPoints &points, const RefreshArgs &refreshArgs, const StaticSettings &settings) {
    if (corrections.rigid.size() != corrections.slot.size() || corrections.lambda.size() != corrections.slot.size() || points.reference.size() != points.row.size())
        throw std::invalid_argument("correctLoop: the correction lists have different lengths");
    const double t8[8] = {T.q[0], T.q[1], T.q[2], T.q[3], T.t[0], T.t[1], T.t[2], T.s};
    ctx.check(ms_loop_correct(ctx.get(), poses.pose(), (int)poses.size(), table.mutablePosition(), (int)table.size(), t8, corrections.slot.data(),
                              corrections.rigid.data(), corrections.lambda.data(), (int)corrections.slot.size(), points.row.data(), points.reference.data(),
                              (int)points.row.size()), "ms_loop_correct");
    return table.refresh(ctx, poses, refreshArgs.rows, refreshArgs.observations, refreshArgs.firstOctave, settings, refreshArgs.pool);
}

// ---- set queries over the map graph (ms_covisibility, ms_map_point_union) ---------------------------------------------------------
// Keyframe::mapPoints of every keyframe on the device, one slot per keyframe: entry j of a slot = the DeviceMapPoints row bound to keypoint j,
// -1 for none.  What getNeighbors and the map-point unions read; the lists those produce are what GateView::indices / LoopPoints take.
class DeviceKeyframeMapPoints {
public:
    DeviceKeyframeMapPoints(Context &ctx, std::size_t slots, std::size_t stride, std::size_t mapPoints) : ctx_(ctx), n_(slots), stride_(stride), nMp_(mapPoints) {
        if (stride_ < 1) throw std::invalid_argument("DeviceKeyframeMapPoints: stride < 1");
        ctx_.check(ms_dev_alloc(ctx_.get(), 4 * n_ * stride_ + 16, &table_), "ms_dev_alloc");
        const std::vector<std::int32_t> none(n_ * stride_, -1);
        if (n_) ctx_.check(ms_dev_upload(ctx_.get(), table_, none.data(), 4 * none.size()), "ms_dev_upload");
    }
    ~DeviceKeyframeMapPoints() { ms_dev_free(ctx_.get(), table_); }
    DeviceKeyframeMapPoints(const DeviceKeyframeMapPoints &) = delete;
    // Keyframe::mapPoints of the keyframe in `slot` (shorter than the stride: padded with -1).  The host still holds the data here, so this is
    // where an entry outside [-1, mapPoints) is turned away; the kernels treat whatever they find outside [0, mapPoints) as "none".
    void update(std::size_t slot, const std::vector<std::int32_t> &mapPoints) {
        if (slot >= n_ || mapPoints.size() > stride_) throw std::invalid_argument("DeviceKeyframeMapPoints::update: slot or length outside the table");
        for (std::int32_t r : mapPoints)
            if (r < -1 || r >= (std::int64_t)nMp_) throw std::invalid_argument("DeviceKeyframeMapPoints::update: entry " + std::to_string(r) + " outside [-1, " + std::to_string(nMp_) + ")");
        std::vector<std::int32_t> row(stride_, -1);
        std::copy(mapPoints.begin(), mapPoints.end(), row.begin());
        ctx_.check(ms_dev_upload(ctx_.get(), static_cast<std::int32_t *>(table_) + slot * stride_, row.data(), 4 * stride_), "ms_dev_upload");
    }
    void clear(std::size_t slot) { update(slot, {}); }      // a removed keyframe
    std::size_t size() const { return n_; }
    std::size_t stride() const { return stride_; }
    std::size_t mapPointCount() const { return nMp_; }
    const std::int32_t *table() const { return static_cast<const std::int32_t *>(table_); }
    std::int32_t *mutableTable() { return static_cast<std::int32_t *>(table_); }            // what cullMap writes
private:
    Context &ctx_;
    std::size_t n_, stride_, nMp_;
    void *table_ = nullptr;
};

// MapPoint::status of every table row as the queries read it: bit 0 = TRIANGULATED, bit 1 = neither NOT_TRIANGULATED nor BAD.
class DeviceMapPointFlags {
public:
    static constexpr std::uint8_t TRIANGULATED = 1, USABLE = 2;
    DeviceMapPointFlags(Context &ctx, const std::vector<std::uint8_t> &flags) : ctx_(ctx), n_(flags.size()) {
        ctx_.check(ms_dev_alloc(ctx_.get(), n_ + 16, &flags_), "ms_dev_alloc");
        update(0, n_, flags.data());
    }
    ~DeviceMapPointFlags() { ms_dev_free(ctx_.get(), flags_); }
    DeviceMapPointFlags(const DeviceMapPointFlags &) = delete;
    void update(std::size_t first, std::size_t count, const std::uint8_t *flags) {
        if (first + count > n_) throw std::runtime_error("DeviceMapPointFlags::update: range outside the table");
        if (count) ctx_.check(ms_dev_upload(ctx_.get(), static_cast<std::uint8_t *>(flags_) + first, flags, count), "ms_dev_upload");
    }
    std::size_t size() const { return n_; }
    const std::uint8_t *flags() const { return static_cast<const std::uint8_t *>(flags_); }
    std::uint8_t *mutableFlags() { return static_cast<std::uint8_t *>(flags_); }          // what triangulateMapPoints writes
private:
    Context &ctx_;
    std::size_t n_;
    void *flags_ = nullptr;
};

// ---- the map-point triangulator (ms_triangulate) ------------------------------------------------------------------------------------
// TriangulationMethod of mapper_helpers.hpp plus the first / last variant (triangulateMapPointFirstLastObs).
enum class TriangulationMethod { TME = MS_TRI_TME, MIDPOINT = MS_TRI_MIDPOINT, FIRST_LAST = MS_TRI_FIRST_LAST };
// Per keyframe slot of DeviceKeyframePoses: the pinhole stand-in of kf.shared->camera and its getFocalLength().
struct KeyframeCameras {
    std::vector<ms_pinhole> camera;
    std::vector<std::int32_t> focalLength;
};
// The map points to triangulate and MapPoint::observations of each, flattened in the reference's iteration order (ascending KfId):
// row r's observations are [obsStart[r], obsStart[r + 1]); obsKf = the keyframe's slot, obsX / obsY / obsOctave = kp.pt and kp.octave,
// obsDepth = keyPointDepth (empty: no depth anywhere); wasTriangulated = status != NOT_TRIANGULATED on entry (mapper_helpers.cpp:607).
struct TriangulateArgs {
    std::vector<std::int32_t> rows;
    std::vector<std::uint8_t> wasTriangulated;
    std::vector<std::int32_t> obsStart, obsKf, obsOctave;
    std::vector<float> obsX, obsY, obsDepth;
};
// Per entry of TriangulateArgs::rows: status (0 NOT_TRIANGULATED, 1 UNSURE, 2 TRIANGULATED), the first gate that stopped the point (the reason
// codes of ms_triangulate) and nNew of triangulateMapPointFirstLastObs.
struct TriangulateResult {
    std::vector<std::uint8_t> status, reason;
    std::vector<std::int32_t> passCount;
};

// triangulateMapPoint / triangulateMapPointFirstLastObs (mapper_helpers.cpp:600-812) for args.rows, on the device: positions are written into
// `table`, the status flags (DeviceMapPointFlags encoding) into `flags` when given.  The debug counters of loop_closer.cpp:516-521 follow from
// the result and the entry state: `failed` = the entry status was TRIANGULATED and status != 2; `changed` (a comparison of position values in
// the reference) = the position was written: status != 0, or the depth branch of :621 ran (not wasTriangulated, a positive depth, reason != 1).
inline TriangulateResult triangulateMapPoints(Context &ctx, DeviceMapPoints &table, DeviceMapPointFlags *flags, const DeviceKeyframePoses &poses,
                                              const KeyframeCameras &cams, const TriangulateArgs &args, const StaticSettings &settings, TriangulationMethod method) {
    const std::size_t n = args.rows.size();
    if (args.wasTriangulated.size() != n || args.obsStart.size() != n + 1) throw std::invalid_argument("triangulateMapPoints: one flag and one list per row");
    const std::size_t nObs = (std::size_t)std::max<std::int32_t>(args.obsStart.back(), 0);
    if (args.obsKf.size() < nObs || args.obsOctave.size() < nObs || args.obsX.size() < nObs || args.obsY.size() < nObs || (!args.obsDepth.empty() && args.obsDepth.size() < nObs))
        throw std::invalid_argument("triangulateMapPoints: the observation arrays are shorter than obsStart says");
    if (cams.camera.size() != poses.size() || cams.focalLength.size() != poses.size()) throw std::invalid_argument("triangulateMapPoints: one camera per keyframe slot");
    if (flags && flags->size() < table.size()) throw std::invalid_argument("triangulateMapPoints: fewer flags than map points");
    const Parameters &p = settings.parameters;
    const ms_tri_settings s{settings.levelSigmaSq.data(), (std::int32_t)settings.levelSigmaSq.size(), p.minTriangulationAngleTwoObs, p.minTriangulationAngleMultipleObs,
                            p.relativeReprojectionErrorThreshold, p.computeDenseStereoDepth ? 1 : 0};
    TriangulateResult out;
    out.status.assign(n, 0); out.reason.assign(n, 0); out.passCount.assign(n, 0);
    ctx.check(ms_triangulate(ctx.get(), table.mutablePosition(), flags ? flags->mutableFlags() : nullptr, (int)table.size(), poses.pose(), (int)poses.size(),
                             cams.camera.data(), cams.focalLength.data(), args.rows.data(), args.wasTriangulated.data(), (int)n, args.obsStart.data(), args.obsKf.data(),
                             args.obsX.data(), args.obsY.data(), args.obsOctave.data(), args.obsDepth.empty() ? nullptr : args.obsDepth.data(), &s, (int)method,
                             out.status.data(), out.reason.data(), out.passCount.data()), "ms_triangulate");
    return out;
}

// One call of Keyframe::getNeighbors (keyframe.cpp:192-230): the keyframe's slot, its previousKfId / nextKfId as slots (-1 for none).
struct NeighborQuery {
    std::int32_t slot = 0, previous = -1, next = -1;
    int minCovisibilities = 1;
    bool triangulatedOnly = false;
};

// getNeighbors for every query in one device call: per query the neighbour slots, ascending (the order of the reference's std::map walk).
inline std::vector<std::vector<std::int32_t>> getNeighbors(Context &ctx, const DeviceKeyframeMapPoints &table, const DeviceMapPointFlags *flags,
                                                           const std::vector<NeighborQuery> &queries) {
    std::vector<std::vector<std::int32_t>> out(queries.size());
    if (queries.empty()) return out;
    if (flags && flags->size() < table.mapPointCount()) throw std::invalid_argument("getNeighbors: fewer flags than map points");
    std::vector<ms_covis_query> q(queries.size());
    for (std::size_t i = 0; i < queries.size(); ++i)
        q[i] = ms_covis_query{queries[i].slot, queries[i].previous, queries[i].next, (std::int32_t)queries[i].minCovisibilities,
                              (std::uint8_t)(queries[i].triangulatedOnly ? DeviceMapPointFlags::TRIANGULATED : 0)};
    const std::size_t nKf = table.size(), bytes = 4 * queries.size() * nKf;
    std::int32_t *packed = reinterpret_cast<std::int32_t *>(ctx.workspace(bytes));
    std::vector<std::int32_t> n(queries.size(), 0);
    ctx.check(ms_covisibility(ctx.get(), table.table(), (int)nKf, (int)table.stride(), flags ? flags->flags() : nullptr, (int)table.mapPointCount(), q.data(), (int)q.size(),
                              nullptr, packed, n.data()), "ms_covisibility");
    std::vector<std::int32_t> host(queries.size() * nKf);
    ctx.check(ms_dev_download(ctx.get(), host.data(), packed, bytes), "ms_dev_download");
    for (std::size_t i = 0; i < queries.size(); ++i) out[i].assign(host.begin() + i * nKf, host.begin() + i * nKf + n[i]);
    return out;
}

// What computeAdjacentKeyframes reads of the map besides the covisibilities: per slot the previousKfId / nextKfId links (as slots, -1 for
// none) and Keyframe::cameraCenter().
struct KeyframeChain {
    std::vector<std::int32_t> previous, next;
    std::vector<std::array<double, 3>> cameraCenter;
    // what observationCounts and cullMap read in addition: per slot the KfId (-1 for an empty slot) and Keyframe::t
    std::vector<std::int32_t> id;
    std::vector<double> t;
};

// computeAdjacentKeyframes (mapper_helpers.cpp:144-229): the getNeighbors calls of every second keyframe of the chain behind `current`
// (:160-176) are ONE ms_covisibility call; the chain walks from the parents and the squared-distance sort (:178-216) stay on the host.
inline std::vector<std::int32_t> computeAdjacentKeyframes(Context &ctx, const DeviceKeyframeMapPoints &table, const DeviceMapPointFlags *flags, std::int32_t current,
                                                          int minCovisibilities, int maxKeyframes, const KeyframeChain &chain) {
    if (chain.previous.size() != table.size() || chain.next.size() != table.size() || chain.cameraCenter.size() != table.size())
        throw std::invalid_argument("computeAdjacentKeyframes: one link pair and one camera centre per slot");
    auto inTable = [&](std::int32_t s) { return s >= 0 && (std::size_t)s < table.size(); };
    if (!inTable(current)) throw std::invalid_argument("computeAdjacentKeyframes: current keyframe outside the table");
    std::vector<char> adjacentSet(table.size(), 0);          // std::set<KfId> over slots: walked in ascending order below
    std::vector<NeighborQuery> queries;
    int i = 0;
    for (std::int32_t backwards = current; backwards != -1; backwards = chain.previous[backwards]) {
        if (!inTable(backwards)) throw std::invalid_argument("computeAdjacentKeyframes: a link leaves the table");
        adjacentSet[backwards] = 1;
        if (i % 2 == 0) queries.push_back({backwards, chain.previous[backwards], chain.next[backwards], minCovisibilities, false});
        if (++i >= maxKeyframes) break;
    }
    std::vector<char> parents(table.size(), 0);
    for (const std::vector<std::int32_t> &nb : getNeighbors(ctx, table, flags, queries))
        for (std::int32_t k : nb) parents[k] = 1;
    for (std::size_t parent = 0; parent < parents.size(); ++parent) {
        if (!parents[parent]) continue;
        for (const std::vector<std::int32_t> *link : {&chain.previous, &chain.next}) {
            i = 0;
            for (std::int32_t at = (std::int32_t)parent; at != -1; at = (*link)[at]) {
                if (!inTable(at)) throw std::invalid_argument("computeAdjacentKeyframes: a link leaves the table");
                adjacentSet[at] = 1;
                if (++i >= maxKeyframes / 2) break;
            }
        }
    }
    adjacentSet[current] = 0;
    std::vector<std::int32_t> adjacent;
    for (std::size_t k = 0; k < adjacentSet.size(); ++k) if (adjacentSet[k]) adjacent.push_back((std::int32_t)k);
    const std::array<double, 3> &c = chain.cameraCenter[current];
    auto dist2 = [&](std::int32_t k) {                       // squaredNorm of a 3-vector, Eigen's unrolled redux: x^2 + (y^2 + z^2)
        const std::array<double, 3> &p = chain.cameraCenter[k];
        const double x = p[0] - c[0], y = p[1] - c[1], z = p[2] - c[2];
        return x * x + (y * y + z * z);
    };
    std::sort(adjacent.begin(), adjacent.end(), [&](std::int32_t a, std::int32_t b) { return dist2(a) < dist2(b); });
    if ((int)adjacent.size() > maxKeyframes) adjacent.erase(adjacent.begin() + maxKeyframes, adjacent.end());
    return adjacent;
}

// The ordered union of the map points of a list of keyframes: rows ascending (the std::set / std::map walk) and, for each, the first
// position of the list whose keyframe lists it (localMapPoints.emplace of loop_closer.cpp:430-432) -- LoopPoints as it stands.
//   matchLocalMapPoints (mapper_helpers.cpp:241-261)   localMapPoints(ctx, table, &flags, adjacentSlots, currentSlot, DeviceMapPointFlags::USABLE).row
//                                                      is GateView::indices in front of isInFrustum
//   deduplicateMapPoints (:337-345), searchAndDeduplicate (loop_closer.cpp:569-584)   exclude = -1, require = 0
//   correctLoop (:418-433, :465-469)                   keyframes = LoopCorrections::slot; the result is its LoopPoints
inline LoopPoints localMapPoints(Context &ctx, const DeviceKeyframeMapPoints &table, const DeviceMapPointFlags *flags, const std::vector<std::int32_t> &keyframes,
                                 std::int32_t excludeSlot = -1, std::uint8_t require = 0, bool withOwner = true) {
    LoopPoints out;
    const std::size_t nMp = table.mapPointCount();
    if (flags && flags->size() < nMp) throw std::invalid_argument("localMapPoints: fewer flags than map points");
    const ms_union_problem problem{0, (std::int32_t)keyframes.size(), excludeSlot, require};
    std::int32_t *rows = reinterpret_cast<std::int32_t *>(ctx.workspace(8 * nMp + 256)), *owner = rows + (nMp + 63) / 64 * 64;
    std::int32_t n = 0;
    ctx.check(ms_map_point_union(ctx.get(), table.table(), (int)table.size(), (int)table.stride(), flags ? flags->flags() : nullptr, (int)nMp, keyframes.data(),
                                 (int)keyframes.size(), &problem, 1, rows, withOwner ? owner : nullptr, &n), "ms_map_point_union");
    out.row.resize((std::size_t)n);
    if (withOwner) out.reference.resize((std::size_t)n);
    if (n) {
        ctx.check(ms_dev_download(ctx.get(), out.row.data(), rows, 4 * (std::size_t)n), "ms_dev_download");
        if (withOwner) ctx.check(ms_dev_download(ctx.get(), out.reference.data(), owner, 4 * (std::size_t)n), "ms_dev_download");
    }
    return out;
}

// ---- observation counts and culling on the map tables (ms_observation_count, ms_map_cull) -----------------------------------------
// Non-zero = the table row holds a map point of mapDB.mapPoints.  A free row and a point whose observations are all gone both have zero
// observations, and triangulateMapPoints overwrites the flags, so this is an array of its own.
class DeviceMapPointLive {
public:
    DeviceMapPointLive(Context &ctx, const std::vector<std::uint8_t> &live) : ctx_(ctx), n_(live.size()) {
        ctx_.check(ms_dev_alloc(ctx_.get(), n_ + 16, &live_), "ms_dev_alloc");
        update(0, n_, live.data());
    }
    ~DeviceMapPointLive() { ms_dev_free(ctx_.get(), live_); }
    DeviceMapPointLive(const DeviceMapPointLive &) = delete;
    void update(std::size_t first, std::size_t count, const std::uint8_t *live) {
        if (first + count > n_) throw std::runtime_error("DeviceMapPointLive::update: range outside the table");
        if (count) ctx_.check(ms_dev_upload(ctx_.get(), static_cast<std::uint8_t *>(live_) + first, live, count), "ms_dev_upload");
    }
    std::vector<std::uint8_t> download() const {
        std::vector<std::uint8_t> out(n_);
        if (n_) ctx_.check(ms_dev_download(ctx_.get(), out.data(), live_, n_), "ms_dev_download");
        return out;
    }
    std::size_t size() const { return n_; }
    const std::uint8_t *live() const { return static_cast<const std::uint8_t *>(live_); }
    std::uint8_t *mutableLive() { return static_cast<std::uint8_t *>(live_); }              // what cullMap writes
private:
    Context &ctx_;
    std::size_t n_;
    void *live_ = nullptr;
};

// Per table row: mp.observations.size(), getFirstObservation() and getLastObservation() as slots (-1 for a row nobody observes).
struct ObservationCounts {
    std::vector<std::int32_t> count, first, last;
};

// The transpose of the keyframe table, computed where it lies: what the status promotion of mapper_helpers.cpp:1072 and the row selection of
// :1088 read, without a std::map of observations per point on the host.  kfIds: per slot the KfId, -1 for an empty slot.
inline ObservationCounts observationCounts(Context &ctx, const DeviceKeyframeMapPoints &table, const std::vector<std::int32_t> &kfIds) {
    if (kfIds.size() != table.size()) throw std::invalid_argument("observationCounts: one KfId per slot");
    const std::size_t nMp = table.mapPointCount(), pitch = (nMp + 63) / 64 * 64;
    ObservationCounts out;
    out.count.resize(nMp); out.first.resize(nMp); out.last.resize(nMp);
    std::int32_t *dev = reinterpret_cast<std::int32_t *>(ctx.workspace(12 * pitch + 256));
    ctx.check(ms_observation_count(ctx.get(), table.table(), (int)table.size(), (int)table.stride(), (int)nMp, kfIds.data(), dev, dev + pitch, dev + 2 * pitch),
              "ms_observation_count");
    if (nMp) {
        ctx.check(ms_dev_download(ctx.get(), out.count.data(), dev, 4 * nMp), "ms_dev_download");
        ctx.check(ms_dev_download(ctx.get(), out.first.data(), dev + pitch, 4 * nMp), "ms_dev_download");
        ctx.check(ms_dev_download(ctx.get(), out.last.data(), dev + 2 * pitch, 4 * nMp), "ms_dev_download");
    }
    return out;
}

// The three ParametersSlam fields the culling step reads.  Their types are not in the reference tree: ratioFloat32 says whether
// keyframeCullMaxCriticalRatio is a float there (the product of :476 is then rounded to float32); see INTEGRATION.md.
struct CullSettings {
    double minMapPointCullingAge = 0.0;
    int minObservationsForBA = 0;
    double keyframeCullMaxCriticalRatio = 0.0;
    bool cullPoints = true;             // false: cullKeyframes alone
    bool ratioFloat32 = false;
};

// What the host side of the map still has to do after a cull: the removed rows (ascending) with the reason of each (1 no observation left,
// 2 aged and not triangulated, 3 orphaned by a removed keyframe) -- trackIdToMapPoint.erase and the host copies of those points -- and the
// removed keyframes as slots, in the order of removal (descending KfId) -- bowIndex->remove, the `uncertainty` accumulation onto the next
// keyframe and re-pointing referenceKeyframe to the previous one (mapper_helpers.cpp:384, :408-426), with the links as they were before.
struct CullResult {
    std::vector<std::int32_t> removedRows;
    std::vector<std::uint8_t> removedWhy;
    std::vector<std::int32_t> removedKeyframes, removedPrevious, removedNext;
};

// cullMapPoints + cullKeyframes (mapper_helpers.cpp:1095-1096) in ONE device call on the tables in place.  `current` and adjacentKfIds /
// loopClosureKeyframes are slots; a candidate without a previous keyframe (:453) or named by a loop-closure edge (:455-464) is kept.  The
// previous / next links of `chain` are relinked as removeKeyframe does (:414-420) and a removed slot's id becomes -1.
inline CullResult cullMap(Context &ctx, DeviceKeyframeMapPoints &table, DeviceMapPointFlags *flags, DeviceMapPointLive &live, KeyframeChain &chain, std::int32_t current,
                          const std::vector<std::int32_t> &adjacentKfIds, const std::vector<std::int32_t> &loopClosureKeyframes, const CullSettings &settings) {
    const std::size_t nKf = table.size(), nMp = table.mapPointCount();
    if (chain.previous.size() != nKf || chain.next.size() != nKf || chain.id.size() != nKf || chain.t.size() != nKf)
        throw std::invalid_argument("cullMap: one link pair, one KfId and one time per slot");
    if (live.size() < nMp || (flags && flags->size() < nMp)) throw std::invalid_argument("cullMap: fewer live bytes or flags than map points");
    if (settings.cullPoints && !flags) throw std::invalid_argument("cullMap: cullMapPoints reads the flags");
    std::vector<std::uint8_t> keep(adjacentKfIds.size(), 0), removed(adjacentKfIds.size(), 0);
    for (std::size_t i = 0; i < adjacentKfIds.size(); ++i) {
        const std::int32_t k = adjacentKfIds[i];
        if (k < 0 || (std::size_t)k >= nKf) throw std::invalid_argument("cullMap: adjacent keyframe outside the table");
        keep[i] = chain.previous[k] < 0 || std::find(loopClosureKeyframes.begin(), loopClosureKeyframes.end(), k) != loopClosureKeyframes.end();
    }
    const ms_cull_settings s{current, settings.cullPoints ? 1 : 0, settings.minMapPointCullingAge, (std::int32_t)settings.minObservationsForBA,
                             settings.keyframeCullMaxCriticalRatio, settings.ratioFloat32 ? 1 : 0};
    const std::size_t pitch = (nMp + 63) / 64 * 64;
    std::int32_t *rows = reinterpret_cast<std::int32_t *>(ctx.workspace(5 * pitch + 256));
    std::uint8_t *why = reinterpret_cast<std::uint8_t *>(rows + pitch);
    std::int32_t nRows = 0, nKfs = 0;
    ctx.check(ms_map_cull(ctx.get(), table.mutableTable(), (int)nKf, (int)table.stride(), flags ? flags->mutableFlags() : nullptr, live.mutableLive(), (int)nMp, chain.id.data(),
                          chain.t.data(), adjacentKfIds.data(), keep.data(), (int)adjacentKfIds.size(), &s, nullptr, rows, why, removed.data(), &nRows, &nKfs), "ms_map_cull");
    CullResult out;
    out.removedRows.resize((std::size_t)nRows); out.removedWhy.resize((std::size_t)nRows);
    if (nRows) {
        ctx.check(ms_dev_download(ctx.get(), out.removedRows.data(), rows, 4 * (std::size_t)nRows), "ms_dev_download");
        ctx.check(ms_dev_download(ctx.get(), out.removedWhy.data(), why, (std::size_t)nRows), "ms_dev_download");
    }
    for (std::size_t i = 0; i < adjacentKfIds.size(); ++i) if (removed[i]) out.removedKeyframes.push_back(adjacentKfIds[i]);
    std::sort(out.removedKeyframes.begin(), out.removedKeyframes.end(), [&](std::int32_t a, std::int32_t b) { return chain.id[a] > chain.id[b]; });
    for (std::int32_t k : out.removedKeyframes) {            // :414-420, in the order of removal
        const std::int32_t prev = chain.previous[k], next = chain.next[k];
        out.removedPrevious.push_back(prev); out.removedNext.push_back(next);
        if (next != -1) chain.previous[next] = prev;
        if (prev != -1) chain.next[prev] = next;
        chain.previous[k] = chain.next[k] = -1;
        chain.id[k] = -1;
    }
    return out;
}

// ---- observation lists on the device (ms_observation_lists, ms_map_refresh_lists, ms_triangulate_lists) -------------------------------
// The keypoints of every keyframe on the device, parallel to DeviceKeyframeMapPoints: kp.pt.x / kp.pt.y, kp.octave and keyPointDepth of
// keypoint j of the keyframe in a slot (a depth <= 0 is "none", as the triangulator reads it).  update() uploads one slot when its keyframe arrives.
class DeviceKeypointTable {
public:
    DeviceKeypointTable(Context &ctx, std::size_t slots, std::size_t stride) : ctx_(ctx), n_(slots), stride_(stride) {
        if (stride_ < 1) throw std::invalid_argument("DeviceKeypointTable: stride < 1");
        for (void **p : {&x_, &y_, &octave_, &depth_}) ctx_.check(ms_dev_alloc(ctx_.get(), 4 * n_ * stride_ + 16, p), "ms_dev_alloc");
        const std::vector<float> zero(n_ * stride_, 0.0f);   // all-zero bits: x = y = 0, octave 0, no depth
        for (void *p : {x_, y_, octave_, depth_})
            if (n_) ctx_.check(ms_dev_upload(ctx_.get(), p, zero.data(), 4 * zero.size()), "ms_dev_upload");
    }
    ~DeviceKeypointTable() { for (void *p : {x_, y_, octave_, depth_}) ms_dev_free(ctx_.get(), p); }
    DeviceKeypointTable(const DeviceKeypointTable &) = delete;
    // the keypoints of the keyframe in `slot` (shorter than the stride: the rest keeps what it held; no map point is bound there).  depth may be empty
    void update(std::size_t slot, const std::vector<float> &x, const std::vector<float> &y, const std::vector<std::int32_t> &octave, const std::vector<float> &depth) {
        const std::size_t n = x.size();
        if (slot >= n_ || n > stride_ || y.size() != n || octave.size() != n || (!depth.empty() && depth.size() != n))
            throw std::invalid_argument("DeviceKeypointTable::update: slot or lengths outside the table");
        if (n == 0) return;
        const std::vector<float> none(n, -1.0f);
        const void *src[4] = {x.data(), y.data(), octave.data(), depth.empty() ? none.data() : depth.data()};
        void *dst[4] = {x_, y_, octave_, depth_};
        for (int i = 0; i < 4; ++i) ctx_.check(ms_dev_upload(ctx_.get(), static_cast<char *>(dst[i]) + 4 * slot * stride_, src[i], 4 * n), "ms_dev_upload");
    }
    std::size_t size() const { return n_; }
    std::size_t stride() const { return stride_; }
    const float *x() const { return static_cast<const float *>(x_); }
    const float *y() const { return static_cast<const float *>(y_); }
    const std::int32_t *octave() const { return static_cast<const std::int32_t *>(octave_); }
    const float *depth() const { return static_cast<const float *>(depth_); }
private:
    Context &ctx_;
    std::size_t n_, stride_;
    void *x_ = nullptr, *y_ = nullptr, *octave_ = nullptr, *depth_ = nullptr;
};

// Which rows an observation-list call takes: the map points of one keyframe slot (the loops of mapper_helpers.cpp:1062 / :1085), or rows
// that already lie on the device (the output of a map-point union, removed rows), and the filter of the loop (MS_OBS_*).
struct ObservationSelection {
    std::int32_t slot = -1;                  // >= 0: MS_OBS_FROM_SLOT
    const std::int32_t *deviceRows = nullptr;   // otherwise MS_OBS_FROM_ROWS: DEVICE [rowCount]
    std::size_t rowCount = 0;
    int filter = MS_OBS_ALL;
    bool dropEmpty = false;
};

// MapPoint::observations of chosen rows as CSR lists in device memory (ms_observation_lists): owns the buffers of ms_obs_lists and regrows
// them when a call reports MS_ERR_CAPACITY.  Nothing of the lists is on the host; rows() and friends are DEVICE pointers for the next call.
class DeviceObservationLists {
public:
    explicit DeviceObservationLists(Context &ctx, std::size_t rows = 256, std::size_t observations = 2048) : ctx_(ctx) { reserve(rows, observations); }
    ~DeviceObservationLists() { release(); }
    DeviceObservationLists(const DeviceObservationLists &) = delete;
    // kfIds: per slot the KfId, -1 for an empty slot; descBase: per slot the DeviceDescriptorPool index of its keypoint 0, -1 for none
    // (empty: no descriptor indices); levels: octaves outside [0, levels) are an error (0: not looked at).
    void build(const DeviceKeyframeMapPoints &table, const DeviceKeypointTable &keypoints, const DeviceMapPointFlags *flags, const std::vector<std::int32_t> &kfIds,
               const std::vector<std::int32_t> &descBase, const ObservationSelection &selection, int levels) {
        if (kfIds.size() != table.size() || (!descBase.empty() && descBase.size() != table.size())) throw std::invalid_argument("DeviceObservationLists::build: one KfId and one base per slot");
        if (keypoints.size() != table.size() || keypoints.stride() != table.stride()) throw std::invalid_argument("DeviceObservationLists::build: the keypoint table does not match the keyframe table");
        if (flags && flags->size() < table.mapPointCount()) throw std::invalid_argument("DeviceObservationLists::build: fewer flags than map points");
        const ms_obs_select sel{selection.slot >= 0 ? MS_OBS_FROM_SLOT : MS_OBS_FROM_ROWS, selection.filter, selection.dropEmpty ? 1 : 0, selection.slot, selection.deviceRows,
                                (std::int32_t)selection.rowCount};
        for (int attempt = 0;; ++attempt) {
            ms_obs_lists l = lists();
            if (descBase.empty()) l.obs_desc = nullptr;
            if (!flags) l.was_triangulated = nullptr;
            std::int32_t nRows = 0, nObs = 0;
            const int rc = ms_observation_lists(ctx_.get(), table.table(), (int)table.size(), (int)table.stride(), (int)table.mapPointCount(), kfIds.data(),
                                                flags ? flags->flags() : nullptr, keypoints.x(), keypoints.y(), keypoints.octave(), keypoints.depth(),
                                                descBase.empty() ? nullptr : descBase.data(), &sel, levels, &l, (int)capRows_, (int)capObs_, &nRows, &nObs);
            if (rc == MS_ERR_CAPACITY && attempt == 0 && ((std::size_t)nRows > capRows_ || (std::size_t)nObs > capObs_)) {
                reserve(std::max<std::size_t>(nRows, capRows_), std::max<std::size_t>(nObs, capObs_));      // the needed counts came back: once is enough
                continue;
            }
            ctx_.check(rc, "ms_observation_lists");
            nRows_ = (std::size_t)nRows; nObs_ = (std::size_t)nObs;
            hasDesc_ = !descBase.empty();
            return;
        }
    }
    std::size_t rowCount() const { return nRows_; }
    std::size_t observationCount() const { return nObs_; }
    bool hasDescriptors() const { return hasDesc_; }
    ms_obs_lists lists() const {
        return ms_obs_lists{i32(0), i32(1), i32(2), i32(3), static_cast<std::uint8_t *>(buf_[4]), i32(5), i32(6), i32(7), i32(8), f32(9), f32(10), f32(11)};
    }
    // a copy for the host (tests, debugging): `count` int32 from a row array (rows, obs_start, n_obs_row, first_octave) or an observation array
    std::vector<std::int32_t> download(const std::int32_t *deviceArray, std::size_t count) const {
        std::vector<std::int32_t> out(count);
        if (count) ctx_.check(ms_dev_download(ctx_.get(), out.data(), deviceArray, 4 * count), "ms_dev_download");
        return out;
    }
private:
    std::int32_t *i32(int i) const { return static_cast<std::int32_t *>(buf_[i]); }
    float *f32(int i) const { return static_cast<float *>(buf_[i]); }
    void release() { for (void *&p : buf_) { if (p) ms_dev_free(ctx_.get(), p); p = nullptr; } }
    void reserve(std::size_t rows, std::size_t observations) {
        release();
        capRows_ = rows + rows / 2; capObs_ = observations + observations / 2;
        for (int i = 0; i < 12; ++i) ctx_.check(ms_dev_alloc(ctx_.get(), 4 * ((i < 5 ? capRows_ + 1 : capObs_)) + 16, &buf_[i]), "ms_dev_alloc");
    }
    Context &ctx_;
    void *buf_[12] = {nullptr};              // in the order of ms_obs_lists' fields
    std::size_t capRows_ = 0, capObs_ = 0, nRows_ = 0, nObs_ = 0;
    bool hasDesc_ = false;
};

// The map-point update of a new keyframe, mapper_helpers.cpp:1062-1077, without a per-point host structure: the observation lists of the
// current keyframe's usable map points (status neither NOT_TRIANGULATED nor BAD, :1066) are built on the device, then updateDescriptor +
// updateDistanceAndNorm (:1069-1070) and the status promotion of :1072-1076 run on them where they lie.  `pool` may be null (descriptors stay).
// Returns the number of refreshed map points; `lists` holds them afterwards.
inline std::size_t updateMapPoints(Context &ctx, DeviceObservationLists &lists, DeviceMapPoints &mapPoints, DeviceMapPointFlags &flags, const DeviceKeyframeMapPoints &table,
                                   const DeviceKeypointTable &keypoints, const DeviceKeyframePoses &poses, const std::vector<std::int32_t> &kfIds,
                                   const std::vector<std::int32_t> &descBase, const DeviceDescriptorPool *pool, std::int32_t currentSlot, int minObservationsForBA,
                                   const StaticSettings &settings) {
    ObservationSelection sel;
    sel.slot = currentSlot; sel.filter = MS_OBS_REFRESH; sel.dropEmpty = true;
    const int levels = (int)settings.scaleFactors.size();
    lists.build(table, keypoints, &flags, kfIds, pool ? descBase : std::vector<std::int32_t>(), sel, levels);
    const ms_obs_lists l = lists.lists();
    ctx.check(ms_map_refresh_lists(ctx.get(), mapPoints.position(), mapPoints.mutableNorm(), mapPoints.mutableMinDistance(), mapPoints.mutableMaxDistance(),
                                   mapPoints.mutableDescriptor(), (int)mapPoints.size(), poses.pose(),
                                   (int)poses.size(), pool ? pool->descriptor() : nullptr, pool ? (int)pool->size() : 0, &l, (int)lists.rowCount(), (int)lists.observationCount(),
                                   settings.scaleFactors.data(), levels, std::max(minObservationsForBA, 1), flags.mutableFlags(), nullptr), "ms_map_refresh_lists");
    return lists.rowCount();
}

// The re-triangulation after local BA, mapper_helpers.cpp:1085-1092: the current keyframe's map points that are not TRIANGULATED or have at
// least two observations (:1088), triangulated from device lists.  The per-point results come back as from triangulateMapPoints, in the
// order of the keyframe's keypoints.
inline TriangulateResult retriangulateCurrent(Context &ctx, DeviceObservationLists &lists, DeviceMapPoints &mapPoints, DeviceMapPointFlags &flags,
                                              const DeviceKeyframeMapPoints &table, const DeviceKeypointTable &keypoints, const DeviceKeyframePoses &poses,
                                              const KeyframeCameras &cams, const std::vector<std::int32_t> &kfIds, std::int32_t currentSlot, const StaticSettings &settings,
                                              TriangulationMethod method) {
    if (cams.camera.size() != poses.size() || cams.focalLength.size() != poses.size()) throw std::invalid_argument("retriangulateCurrent: one camera per keyframe slot");
    ObservationSelection sel;
    sel.slot = currentSlot; sel.filter = MS_OBS_RETRIANGULATE;
    lists.build(table, keypoints, &flags, kfIds, {}, sel, (int)settings.levelSigmaSq.size());
    const Parameters &p = settings.parameters;
    const ms_tri_settings s{settings.levelSigmaSq.data(), (std::int32_t)settings.levelSigmaSq.size(), p.minTriangulationAngleTwoObs, p.minTriangulationAngleMultipleObs,
                            p.relativeReprojectionErrorThreshold, p.computeDenseStereoDepth ? 1 : 0};
    const std::size_t n = lists.rowCount();
    TriangulateResult out;
    out.status.assign(n, 0); out.reason.assign(n, 0); out.passCount.assign(n, 0);
    const ms_obs_lists l = lists.lists();
    ctx.check(ms_triangulate_lists(ctx.get(), mapPoints.mutablePosition(), flags.mutableFlags(), (int)mapPoints.size(), poses.pose(), (int)poses.size(), cams.camera.data(),
                                   cams.focalLength.data(), &l, (int)n, (int)lists.observationCount(), &s, (int)method, out.status.data(), out.reason.data(),
                                   out.passCount.data()), "ms_triangulate_lists");
    return out;
}

// ---- matchTrackedFeatures on the device tables (ms_match_tracked, ms_match_tracked_finish) ----------------------------------------------
// MapPoint::trackId of every table row and mapDB.trackIdToMapPoint as a window of track ids on the device.  A track counts as present only
// while its row is live and carries the id back, so cullMap and the reuse of a row need no write here: the entries go stale and are read
// as erased.  Grow-only: ensureTrack() widens the window (the contents move through the host; rare).
class DeviceTrackTable {
public:
    DeviceTrackTable(Context &ctx, std::size_t mapPoints, std::int32_t trackBase = 0, std::size_t window = 4096) : ctx_(ctx), nMp_(mapPoints), base_(trackBase) {
        ctx_.check(ms_dev_alloc(ctx_.get(), 4 * nMp_ + 16, &mpTrack_), "ms_dev_alloc");
        const std::vector<std::int32_t> none(nMp_, -1);
        if (nMp_) ctx_.check(ms_dev_upload(ctx_.get(), mpTrack_, none.data(), 4 * nMp_), "ms_dev_upload");
        reserve(window);
    }
    ~DeviceTrackTable() { ms_dev_free(ctx_.get(), mpTrack_); if (trackRow_) ms_dev_free(ctx_.get(), trackRow_); }
    DeviceTrackTable(const DeviceTrackTable &) = delete;
    // the window holds at least [trackBase, trackId]
    void ensureTrack(std::int32_t trackId) {
        if (trackId < base_) throw std::invalid_argument("DeviceTrackTable::ensureTrack: track id below the window base");
        const std::size_t need = (std::size_t)(trackId - base_) + 1;
        if (need > window_) reserve(std::max(need, 2 * window_));
    }
    // rows that already hold points of known tracks (a map loaded from the host): mp_track[row] = trackId and track_row[trackId] = row
    void bind(const std::vector<std::int32_t> &rows, const std::vector<std::int32_t> &trackIds) {
        if (rows.size() != trackIds.size()) throw std::invalid_argument("DeviceTrackTable::bind: one track id per row");
        for (std::size_t i = 0; i < rows.size(); ++i) {
            if (rows[i] < 0 || (std::size_t)rows[i] >= nMp_) throw std::invalid_argument("DeviceTrackTable::bind: row outside the table");
            ensureTrack(trackIds[i]);
        }
        for (std::size_t i = 0; i < rows.size(); ++i) {
            ctx_.check(ms_dev_upload(ctx_.get(), mpTrack() + rows[i], &trackIds[i], 4), "ms_dev_upload");
            ctx_.check(ms_dev_upload(ctx_.get(), trackRow() + (trackIds[i] - base_), &rows[i], 4), "ms_dev_upload");
        }
    }
    std::vector<std::int32_t> downloadMapPointTracks() const { return download(mpTrack_, nMp_); }
    std::vector<std::int32_t> downloadTrackRows() const { return download(trackRow_, window_); }
    std::size_t mapPointCount() const { return nMp_; }
    std::size_t window() const { return window_; }
    std::int32_t trackBase() const { return base_; }
    std::int32_t *mpTrack() const { return static_cast<std::int32_t *>(mpTrack_); }
    std::int32_t *trackRow() const { return static_cast<std::int32_t *>(trackRow_); }
private:
    std::vector<std::int32_t> download(const void *p, std::size_t n) const {
        std::vector<std::int32_t> out(n);
        if (n) ctx_.check(ms_dev_download(ctx_.get(), out.data(), p, 4 * n), "ms_dev_download");
        return out;
    }
    void reserve(std::size_t window) {
        std::vector<std::int32_t> rows = trackRow_ ? downloadTrackRows() : std::vector<std::int32_t>();
        rows.resize(std::max<std::size_t>(window, 1), -1);
        void *grown = nullptr;
        ctx_.check(ms_dev_alloc(ctx_.get(), 4 * rows.size() + 16, &grown), "ms_dev_alloc");
        ctx_.check(ms_dev_upload(ctx_.get(), grown, rows.data(), 4 * rows.size()), "ms_dev_upload");
        if (trackRow_) ms_dev_free(ctx_.get(), trackRow_);
        trackRow_ = grown; window_ = rows.size();
    }
    Context &ctx_;
    std::size_t nMp_, window_ = 0;
    std::int32_t base_;
    void *mpTrack_ = nullptr, *trackRow_ = nullptr;
};

// The current frame as matchTrackedFeatures reads it: its keyframe slot (the keypoints are in DeviceKeypointTable, the pose in
// DeviceKeyframePoses; poseCW is the same pose on the host) and keyPointToTrackId per keypoint, -1 for none.
struct TrackedFrame {
    std::int32_t slot = 0;
    DeviceKeyframePoses::Pose poseCW{};
    std::vector<std::int32_t> keyPointToTrackId;
};
// Per keypoint the outcome (0 no track | 1 created | 2 just tracked | 3 bound after isInFrustum and checkReprojectionError | 4 outside the
// frustum | 5 reprojection error | 6 absent track, no descriptors), the rows of the created map points with their keypoints (in keypoint
// order: what nextMpId, the host MapPoint objects and their colours are derived from), the reference's debug counters, and FIRST_LAST's
// result per just-tracked point.
struct MatchTrackedResult {
    std::vector<std::uint8_t> outcome;
    std::vector<std::int32_t> createdRows, createdKeyPoints;
    std::size_t newPoints = 0, justTriangulated = 0, checked = 0, frustumFail = 0, reproFail = 0, success = 0;
    TriangulateResult firstLast;
};

// matchTrackedFeatures (mapper_helpers.cpp:67-142) for one frame on the device tables, nothing per keypoint on the host:
//   ms_match_tracked (the walk: bind, gate, create) -> ms_observation_lists of the just-tracked rows -> ms_triangulate_lists FIRST_LAST (:90)
//   -> ms_match_tracked_finish (the descriptor of the points that are now UNSURE, :811; the rows of :121) -> the refresh of :121-124: one pass
//   when the frame has descriptors, otherwise the just-tracked TRIANGULATED rows with the descriptor half and the checked rows without it.
// freeRows: table rows the caller offers to new map points, at least as many as the frame can create (the k-th created point takes the
// k-th); `pool` must hold the frame's descriptors at descBase[slot] when that is >= 0.  `lists` is scratch and holds the last refresh's rows.
inline MatchTrackedResult matchTrackedFeatures(Context &ctx, DeviceObservationLists &lists, DeviceKeyframeMapPoints &table, DeviceMapPoints &mapPoints, DeviceMapPointFlags &flags,
                                               DeviceMapPointLive &live, DeviceTrackTable &tracks, const DeviceKeypointTable &keypoints, const DeviceKeyframePoses &poses,
                                               const KeyframeCameras &cams, const std::vector<std::int32_t> &kfIds, const std::vector<std::int32_t> &descBase,
                                               const DeviceDescriptorPool *pool, const TrackedFrame &frame, const std::vector<std::int32_t> &freeRows,
                                               const StaticSettings &settings, float viewAngleLimitCos = 0.5f) {
    const std::size_t nKf = table.size(), nMp = table.mapPointCount(), nKp = frame.keyPointToTrackId.size(), nNew = freeRows.size();
    if (frame.slot < 0 || (std::size_t)frame.slot >= nKf) throw std::invalid_argument("matchTrackedFeatures: slot outside the table");
    if (cams.camera.size() != nKf || cams.focalLength.size() != nKf || kfIds.size() != nKf || descBase.size() != nKf || poses.size() != nKf)
        throw std::invalid_argument("matchTrackedFeatures: one camera, focal length, KfId, descriptor base and pose per slot");
    if (mapPoints.size() != nMp || flags.size() < nMp || live.size() < nMp || tracks.mapPointCount() != nMp) throw std::invalid_argument("matchTrackedFeatures: the map-point tables differ in size");
    if (keypoints.size() != nKf || keypoints.stride() != table.stride()) throw std::invalid_argument("matchTrackedFeatures: the keypoint table does not match the keyframe table");
    const bool hasDescriptors = descBase[frame.slot] >= 0;
    if (hasDescriptors && !pool) throw std::invalid_argument("matchTrackedFeatures: the frame has descriptors and there is no pool");
    for (std::int32_t t : frame.keyPointToTrackId) if (t >= 0) tracks.ensureTrack(t);
    const int levels = (int)settings.levelSigmaSq.size();
    const Parameters &p = settings.parameters;
    ms_tracked_frame f{};
    f.slot = frame.slot;
    std::copy(frame.poseCW.begin(), frame.poseCW.end(), f.pose);
    f.cam = cams.camera[frame.slot]; f.focal = cams.focalLength[frame.slot];
    f.desc_base = descBase[frame.slot]; f.track_base = tracks.trackBase();
    f.level_sigma_sq = settings.levelSigmaSq.data(); f.n_levels = levels;
    f.rel_reprojection_threshold = p.relativeReprojectionErrorThreshold; f.view_cos_limit = viewAngleLimitCos;
    // device scratch: created rows | created keypoints | just-tracked rows | checked rows | refresh rows | outcomes
    const std::size_t pitchKp = (nKp + 63) / 64 * 64 + 64, pitchNew = (nNew + 63) / 64 * 64 + 64;
    std::int32_t *createdRows = reinterpret_cast<std::int32_t *>(ctx.workspace(4 * (2 * pitchNew + 4 * pitchKp) + pitchKp + 256));
    std::int32_t *createdKp = createdRows + pitchNew, *trackedRows = createdKp + pitchNew, *checkedRows = trackedRows + pitchKp, *refreshRows = checkedRows + pitchKp;
    std::uint8_t *outcome = reinterpret_cast<std::uint8_t *>(refreshRows + 2 * pitchKp);
    std::int32_t counts[5] = {0, 0, 0, 0, 0};
    ctx.check(ms_match_tracked(ctx.get(), table.mutableTable(), (int)nKf, (int)table.stride(), flags.mutableFlags(), live.mutableLive(), mapPoints.position(), mapPoints.norm(),
                               mapPoints.minDistance(), mapPoints.maxDistance(), mapPoints.mutableDescriptor(), tracks.mpTrack(), (int)nMp, keypoints.x(), keypoints.y(),
                               keypoints.octave(), pool ? pool->descriptor() : nullptr, pool ? (int)pool->size() : 0, tracks.trackRow(), (int)tracks.window(), &f,
                               frame.keyPointToTrackId.data(), (int)nKp, freeRows.data(), (int)nNew, outcome, createdRows, createdKp, trackedRows, checkedRows, counts),
              "ms_match_tracked");
    MatchTrackedResult out;
    out.newPoints = (std::size_t)counts[0]; out.justTriangulated = (std::size_t)counts[1]; out.checked = (std::size_t)counts[2];
    out.frustumFail = (std::size_t)counts[3]; out.reproFail = (std::size_t)counts[4];
    out.outcome.resize(nKp); out.createdRows.resize(out.newPoints); out.createdKeyPoints.resize(out.newPoints);
    if (nKp) ctx.check(ms_dev_download(ctx.get(), out.outcome.data(), outcome, nKp), "ms_dev_download");
    if (out.newPoints) {
        ctx.check(ms_dev_download(ctx.get(), out.createdRows.data(), createdRows, 4 * out.newPoints), "ms_dev_download");
        ctx.check(ms_dev_download(ctx.get(), out.createdKeyPoints.data(), createdKp, 4 * out.newPoints), "ms_dev_download");
    }
    const std::vector<std::int32_t> noBase;
    auto listsOf = [&](const std::int32_t *rows, std::size_t n, bool dropEmpty) {
        ObservationSelection sel;
        sel.deviceRows = rows; sel.rowCount = n; sel.dropEmpty = dropEmpty;
        lists.build(table, keypoints, &flags, kfIds, pool ? descBase : noBase, sel, levels);
    };
    std::size_t nTracked = 0;
    if (out.justTriangulated) {                              // :90
        listsOf(trackedRows, out.justTriangulated, false);
        nTracked = lists.rowCount();
        const ms_tri_settings s{settings.levelSigmaSq.data(), (std::int32_t)levels, p.minTriangulationAngleTwoObs, p.minTriangulationAngleMultipleObs,
                                p.relativeReprojectionErrorThreshold, p.computeDenseStereoDepth ? 1 : 0};
        out.firstLast.status.assign(nTracked, 0); out.firstLast.reason.assign(nTracked, 0); out.firstLast.passCount.assign(nTracked, 0);
        const ms_obs_lists l = lists.lists();
        ctx.check(ms_triangulate_lists(ctx.get(), mapPoints.mutablePosition(), flags.mutableFlags(), (int)nMp, poses.pose(), (int)nKf, cams.camera.data(), cams.focalLength.data(), &l,
                                       (int)nTracked, (int)lists.observationCount(), &s, MS_TRI_FIRST_LAST, out.firstLast.status.data(), out.firstLast.reason.data(),
                                       out.firstLast.passCount.data()), "ms_triangulate_lists");
    }
    ms_obs_lists l = lists.lists();
    if (!pool) l.obs_desc = nullptr;
    std::int32_t nRefresh = 0;
    ctx.check(ms_match_tracked_finish(ctx.get(), &l, (int)nTracked, flags.flags(), pool ? pool->descriptor() : nullptr, mapPoints.mutableDescriptor(), (int)nMp, checkedRows,
                                      (int)out.checked, hasDescriptors ? 1 : 0, refreshRows, (int)(2 * pitchKp), &nRefresh), "ms_match_tracked_finish");
    auto refresh = [&](const std::int32_t *rows, std::size_t n, bool descriptors) {                      // :121-124
        if (n == 0) return;
        listsOf(rows, n, true);
        const ms_obs_lists r = lists.lists();
        const bool withPool = descriptors && pool;
        ctx.check(ms_map_refresh_lists(ctx.get(), mapPoints.position(), mapPoints.mutableNorm(), mapPoints.mutableMinDistance(), mapPoints.mutableMaxDistance(),
                                       mapPoints.mutableDescriptor(), (int)nMp, poses.pose(), (int)nKf, withPool ? pool->descriptor() : nullptr, withPool ? (int)pool->size() : 0, &r,
                                       (int)lists.rowCount(), (int)lists.observationCount(), settings.scaleFactors.data(), (int)settings.scaleFactors.size(), 0, nullptr, nullptr),
                  "ms_map_refresh_lists");
    };
    refresh(refreshRows, (std::size_t)nRefresh, true);
    if (!hasDescriptors) refresh(checkedRows, out.checked, false);
    out.success = (std::size_t)nRefresh + (hasDescriptors ? 0 : out.checked);
    return out;
}

// One view of a gate call: a pose (p_c = R p + t, row-major; for MS_GATE_SIM3 rotBAW / transBAW, which may carry a scale), a pinhole camera
// (the stand-in of ms_pinhole), the loop's threshold / margin, and the table rows to walk, in the reference's order.
struct GateView {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    ms_pinhole camera{};
    float threshold = 0.f;              // searchByProjection: threshold; replaceDuplication / findMatchesTranformedMps: margin
    float cosLimit = 0.5f;              // searchByProjection's viewAngleLimitCos (:304) / isInFrustum's argument
    int mode = MS_GATE_SEARCH;
    std::vector<std::int32_t> indices;
};

namespace detail {
// the result of gate + scoring for a list of views: view v's kept entries are slice positions [first[v], first[v] + nKept[v]) of the lists
struct GatedLists {
    std::vector<std::int32_t> first, nKept, keptEntry;       // keptEntry: position in the views' concatenated index lists
    CandidateLists lists;
    const unsigned char *ws = nullptr;                       // the device block (query arrays), for the rare host rescan
    std::size_t oX = 0, oY = 0, oR = 0, oD = 0;
};

inline void pack_views(const std::vector<GateView> &views, std::vector<ms_gate_view> &V, std::vector<std::int32_t> &index) {
    V.clear(); index.clear();
    for (const GateView &g : views) {
        ms_gate_view v{};
        std::memcpy(v.R_cw, g.R, sizeof(v.R_cw)); std::memcpy(v.t_cw, g.t, sizeof(v.t_cw));
        v.cam = g.camera; v.threshold = g.threshold; v.view_cos_limit = g.cosLimit; v.mode = g.mode;
        v.first = (std::int32_t)index.size(); v.count = (std::int32_t)g.indices.size();
        index.insert(index.end(), g.indices.begin(), g.indices.end());
        V.push_back(v);
    }
}

// ms_project_gate over all views, then ms_projection_topk per view against kfs[v] on the packed slices where they lie; one download of the lists.
// skip (optional) = searchByProjection's bound mask, uploaded for every view's keyframe alike (used with one view).
inline GatedLists gate_and_score(Context &ctx, const DeviceMapPoints &table, const std::vector<GateView> &views, const std::vector<const DeviceKeyframe *> &kfs,
                                 const StaticSettings &settings, const std::vector<std::uint8_t> *skip) {
    std::vector<ms_gate_view> V;
    std::vector<std::int32_t> index;
    pack_views(views, V, index);
    const std::size_t ne = index.size(), sec = pad16(4 * ne), nk = skip ? skip->size() : 0;
    GatedLists g;
    g.nKept.assign(views.size(), 0);
    for (const ms_gate_view &v : V) g.first.push_back(v.first);
    const std::size_t oX = 0, oY = oX + sec, oR = oY + sec, oLo = oR + sec, oHi = oLo + sec, oD = oHi + sec, oK = oD + 32 * ne;
    const std::size_t oE = oK + pad16(nk), oTi = oE + sec, oTo = oTi + 16 * ne, oN = oTo + 16 * ne, oTd = oN + sec, total = oTd + pad16(8 * ne);
    unsigned char *ws = ctx.workspace(total + 16);
    g.ws = ws; g.oX = oX; g.oY = oY; g.oR = oR; g.oD = oD;
    auto F = [&](std::size_t o) { return reinterpret_cast<float *>(ws + o); };
    auto I = [&](std::size_t o) { return reinterpret_cast<std::int32_t *>(ws + o); };
    ctx.check(ms_project_gate(ctx.get(), table.position(), table.norm(), table.minDistance(), table.maxDistance(), table.descriptor(), (int)table.size(),
                              index.data(), (int)ne, V.data(), (int)V.size(), settings.scaleFactors.data(), (int)settings.scaleFactors.size(),
                              settings.parameters.orbScaleFactor, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, I(oE), F(oX), F(oY), F(oR), I(oLo), I(oHi),
                              reinterpret_cast<std::uint32_t *>(ws + oD), g.nKept.data()), "ms_project_gate");
    g.keptEntry.assign(ne, -1);
    g.lists.idx.assign(4 * ne, -1); g.lists.octave.assign(4 * ne, -1); g.lists.nScored.assign(ne, 0); g.lists.dist.assign(4 * ne, MS_HAMMING_MAX);
    if (ne == 0) return g;
    if (nk) ctx.check(ms_dev_upload(ctx.get(), ws + oK, skip->data(), nk), "ms_dev_upload");
    for (std::size_t v = 0; v < V.size(); ++v) {
        const std::size_t f = (std::size_t)V[v].first;
        const ms_match_frame &fr = kfs[v]->frame();
        ctx.check(ms_projection_topk(ctx.get(), kfs[v]->sortedX(), kfs[v]->sortedY(), kfs[v]->sortedIndex(), fr.n, fr.desc, fr.octave, nk ? ws + oK : nullptr,
                                     F(oX) + f, F(oY) + f, F(oR) + f, I(oLo) + f, I(oHi) + f, reinterpret_cast<const std::uint32_t *>(ws + oD) + 8 * f, g.nKept[v],
                                     I(oTi) + 4 * f, reinterpret_cast<std::uint16_t *>(ws + oTd) + 4 * f, I(oTo) + 4 * f, I(oN) + f, nullptr), "ms_projection_topk");
    }
    std::vector<unsigned char> &st = ctx.staging();
    st.resize(total - oE);
    ctx.check(ms_dev_download(ctx.get(), st.data(), ws + oE, total - oE), "ms_dev_download");
    for (std::size_t v = 0; v < V.size(); ++v) {              // only the kept part of every slice was written
        const std::size_t f = (std::size_t)V[v].first, k = (std::size_t)g.nKept[v];
        if (k == 0) continue;
        std::memcpy(g.keptEntry.data() + f, st.data() + 4 * f, 4 * k);
        std::memcpy(g.lists.idx.data() + 4 * f, st.data() + (oTi - oE) + 16 * f, 16 * k);
        std::memcpy(g.lists.octave.data() + 4 * f, st.data() + (oTo - oE) + 16 * f, 16 * k);
        std::memcpy(g.lists.nScored.data() + f, st.data() + (oN - oE) + 4 * f, 4 * k);
        std::memcpy(g.lists.dist.data() + 4 * f, st.data() + (oTd - oE) + 8 * f, 8 * k);
    }
    return g;
}
}  // namespace detail

// Keyframe::isInFrustum (keyframe.cpp:247-262) for many map points at once: reprojection, viewing distance and viewing angle of the table rows
// `indices` against one pose and camera.
inline std::vector<bool> isInFrustum(Context &ctx, const DeviceMapPoints &table, const std::vector<std::int32_t> &indices, const double R[9], const double t[3],
                                     const ms_pinhole &camera, float cosLimit, const StaticSettings &settings) {
    ms_gate_view v{};
    std::memcpy(v.R_cw, R, sizeof(v.R_cw)); std::memcpy(v.t_cw, t, sizeof(v.t_cw));
    v.cam = camera; v.view_cos_limit = cosLimit; v.mode = MS_GATE_SEARCH; v.first = 0; v.count = (std::int32_t)indices.size();
    std::vector<bool> in(indices.size(), false);
    if (indices.empty()) return in;
    unsigned char *ws = ctx.workspace(indices.size() + 16);
    std::int32_t kept = 0;
    ctx.check(ms_project_gate(ctx.get(), table.position(), table.norm(), table.minDistance(), table.maxDistance(), table.descriptor(), (int)table.size(),
                              indices.data(), (int)indices.size(), &v, 1, settings.scaleFactors.data(), (int)settings.scaleFactors.size(),
                              settings.parameters.orbScaleFactor, ws, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr, &kept), "ms_project_gate");
    std::vector<unsigned char> &st = ctx.staging();
    st.resize(indices.size());
    ctx.check(ms_dev_download(ctx.get(), st.data(), ws, indices.size()), "ms_dev_download");
    for (std::size_t i = 0; i < indices.size(); ++i) in[i] = st[i] == 0;
    return in;
}

// searchByProjection (keyframe_matcher.cpp:295-414) over table rows: view.indices = the map points `mps` in the caller's order, view.mode =
// MS_GATE_SEARCH, view.threshold = threshold.  Gates, radius query and scoring run on the device; the replay is the one searchByProjectionCore runs
// (detail::replay_search; a list that ran out is settled by one host scan of that query, for which the kept queries are read back once).  Returns, per entry of view.indices, the matched keypoint or -1; `bound` is updated.
inline std::vector<int> searchByProjection(Context &ctx, const DeviceKeyframe &kf, const DeviceMapPoints &table, const GateView &view,
                                           std::vector<std::uint8_t> &bound, const StaticSettings &settings, unsigned *rescored = nullptr) {
    std::vector<int> match(view.indices.size(), -1);
    const detail::GatedLists g = detail::gate_and_score(ctx, table, {view}, {&kf}, settings, &bound);
    // the kept queries' position, radius and descriptor, read back once and only if a list ran out.  g.ws points into Context::workspace, which a
    // larger request would free: nothing between gate_and_score and the end of this function asks the context for workspace.
    const std::size_t nq = (std::size_t)g.nKept[0];
    std::vector<float> qx, qy, qr;
    std::vector<std::uint32_t> qd;
    auto rescan = [&](std::size_t q) {
        if (qx.empty()) {
            qx.resize(nq); qy.resize(nq); qr.resize(nq); qd.resize(8 * nq);
            ctx.check(ms_dev_download(ctx.get(), qx.data(), g.ws + g.oX, 4 * nq), "ms_dev_download");
            ctx.check(ms_dev_download(ctx.get(), qy.data(), g.ws + g.oY, 4 * nq), "ms_dev_download");
            ctx.check(ms_dev_download(ctx.get(), qr.data(), g.ws + g.oR, 4 * nq), "ms_dev_download");
            ctx.check(ms_dev_download(ctx.get(), qd.data(), g.ws + g.oD, 32 * nq), "ms_dev_download");
        }
        RadiusQuery rq;
        rq.x = qx[q]; rq.y = qy[q]; rq.radius = qr[q];
        std::memcpy(rq.descriptor.data(), qd.data() + 8 * q, 32);
        return detail::rescan_on_host(kf, rq, bound);
    };
    const unsigned again = detail::replay_search(g.lists, 0, nq, bound, rescan, [&](std::size_t q, int best) { match[(std::size_t)g.keptEntry[q]] = best; });
    if (rescored) *rescored = again;
    return match;
}

// The candidate search of replaceDuplication (keyframe_matcher.cpp:442-499) for ALL adjacent keyframes of a fuse step in one gate call:
// views[v] (MS_GATE_FUSE, threshold = margin, indices = the rows that pass the graph filters of :429-440 for keyframe v) against kfs[v].
// Returns, per view and entry, the best keypoint inside the radius at Hamming distance <= HAMMING_DIST_THR_LOW, or -1 (:495-499); the
// caller walks them in order and performs the graph surgery of :501-525 (a point erased on the way is skipped there, :429).
inline std::vector<std::vector<int>> replaceDuplicationCandidates(Context &ctx, const DeviceMapPoints &table, const std::vector<GateView> &views,
                                                                  const std::vector<const DeviceKeyframe *> &kfs, const StaticSettings &settings) {
    const detail::GatedLists g = detail::gate_and_score(ctx, table, views, kfs, settings, nullptr);
    std::vector<std::vector<int>> out(views.size());
    for (std::size_t v = 0; v < views.size(); ++v) {
        out[v].assign(views[v].indices.size(), -1);
        const std::size_t f = (std::size_t)g.first[v];
        for (std::size_t q = f; q < f + (std::size_t)g.nKept[v]; ++q)
            out[v][(std::size_t)g.keptEntry[q] - f] = detail::best_candidate(g.lists, q, HAMMING_DIST_THR_LOW);
    }
    return out;
}

// matchMapPointsSim3 (keyframe_matcher.cpp:633-686) over table rows instead of the caller's `project` lambda: mps1[i] / mps2[i] = the table row
// of the TRIANGULATED map point of keypoint i of kf1 / kf2, or -1 (:568-571).  (R1in2, t1in2) = transform12^-1 * kf1.poseCW takes world points
// into kf2 (:650), (R2in1, t2in1) = transform12 * kf2.poseCW into kf1 (:661); both may carry the Sim3's scale.  One gate call, two scoring launches.
inline unsigned matchMapPointsSim3(Context &ctx, const DeviceKeyframe &kf1, const DeviceKeyframe &kf2, const DeviceMapPoints &table,
                                   const std::vector<std::int32_t> &mps1, const std::vector<std::int32_t> &mps2, const double R1in2[9], const double t1in2[3],
                                   const double R2in1[9], const double t2in1[3], const ms_pinhole &camera1, const ms_pinhole &camera2,
                                   std::vector<std::pair<int, int>> &matches, const StaticSettings &settings) {
    constexpr float margin = 7.5;                                                              // :641
    std::vector<bool> taken1(mps1.size(), false), taken2(mps2.size(), false);                  // :645-648
    for (const std::pair<int, int> &m : matches) { taken1.at((std::size_t)m.first) = true; taken2.at((std::size_t)m.second) = true; }
    std::vector<GateView> views(2);
    std::vector<std::size_t> owner[2];
    auto fill = [&](int v, const std::vector<std::int32_t> &mps, const std::vector<bool> &taken, const double *R, const double *t, const ms_pinhole &cam) {
        std::memcpy(views[v].R, R, 72); std::memcpy(views[v].t, t, 24);
        views[v].camera = cam; views[v].threshold = margin; views[v].mode = MS_GATE_SIM3;
        for (std::size_t i = 0; i < mps.size(); ++i)
            if (!taken[i] && mps[i] >= 0) { views[v].indices.push_back(mps[i]); owner[v].push_back(i); }
    };
    fill(0, mps1, taken1, R1in2, t1in2, camera2);
    fill(1, mps2, taken2, R2in1, t2in1, camera1);
    const detail::GatedLists g = detail::gate_and_score(ctx, table, views, {&kf2, &kf1}, settings, nullptr);
    std::vector<int> fwd(mps1.size(), -1), bwd(mps2.size(), -1);
    for (int v = 0; v < 2; ++v) {
        std::vector<int> &dst = v == 0 ? fwd : bwd;
        const std::size_t f = (std::size_t)g.first[v];
        for (std::size_t q = f; q < f + (std::size_t)g.nKept[v]; ++q)
            dst[owner[v][(std::size_t)g.keptEntry[q] - f]] = detail::best_candidate(g.lists, q, HAMMING_DIST_THR_HIGH);   // :625-627
    }
    const std::size_t before = matches.size();
    for (std::size_t i1 = 0; i1 < fwd.size(); ++i1)                                            // :672-685
        if (fwd[i1] >= 0 && bwd.at((std::size_t)fwd[i1]) == (int)i1) matches.emplace_back((int)i1, fwd[i1]);
    return (unsigned)(matches.size() - before);
}

// create_E_21 (openvslam/essential_solver.cc:157-162), row-major 3x3
inline void create_E_21(const double R1w[9], const double t1w[3], const double R2w[9], const double t2w[3], double E[9]) {
    double R21[9], t21[3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += R2w[3 * i + k] * R1w[3 * j + k]; R21[3 * i + j] = s; }
    for (int i = 0; i < 3; ++i) { double s = 0; for (int k = 0; k < 3; ++k) s += -R21[3 * i + k] * t1w[k]; t21[i] = s + t2w[i]; }
    const double S[9] = {0, -t21[2], t21[1], t21[2], 0, -t21[0], -t21[1], t21[0], 0};
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += S[3 * i + k] * R21[3 * k + j]; E[3 * i + j] = s; }
}

}  // namespace mi355slam
