// keyframe_matcher.hpp -- host mirror of the free functions of keyframe_matcher.hpp:33-91.
//
// The reference's Keyframe / MapDB carry the graph; the device only needs flat per-keyframe arrays, so a
// KeyframeFeatures view is built once per keyframe (INTEGRATION.md shows the 15 lines that fill it from
// kf.shared->keyPoints, kf.mapPoints and kf.shared->bowFeatureVec) and uploaded by DeviceKeyframe.  The gate-based overloads at the end read
// the map points from DeviceMapPoints (map_tables.hpp); the operations on the map itself are in map_update.hpp.
#pragma once
#include <algorithm>
#include <cstring>
#include <array>
#include <map>
#include <stdexcept>
#include <utility>
#include "common.hpp"
#include "map_tables.hpp"

namespace mi355slam {

constexpr unsigned HAMMING_DIST_THR_LOW = MS_HAMMING_THR_LOW, HAMMING_DIST_THR_HIGH = MS_HAMMING_THR_HIGH, MAX_HAMMING_DIST = MS_HAMMING_MAX;

struct KeyframeFeatures {
    const KeyPointVector *keyPoints = nullptr;                              // kf.shared->keyPoints
    std::vector<std::uint8_t> usable;                                        // per keypoint: the matcher-specific map-point gate
    std::map<unsigned, std::vector<unsigned>> bowFeatureVec;                  // DBoW2::FeatureVector (ordered node -> keypoint indices)
};

namespace detail {
// a host vector's copy on the device
template <typename T> DeviceArray<T> uploaded(Context &ctx, const std::vector<T> &v) {
    DeviceArray<T> d(ctx, v.size());
    d.upload(0, v.size(), v.data());
    return d;
}
}  // namespace detail

// Device-resident copy of one keyframe's matcher inputs.
class DeviceKeyframe {
public:
    DeviceKeyframe(Context &ctx, const KeyframeFeatures &kf) {
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
        using detail::uploaded;
        desc_ = uploaded(ctx, desc); angle_ = uploaded(ctx, ang); octave_ = uploaded(ctx, oct); bearing_ = uploaded(ctx, bear); usable_ = uploaded(ctx, kf.usable);
        nodeId_ = uploaded(ctx, node_id); nodeStart_ = uploaded(ctx, node_start); kpIdx_ = uploaded(ctx, kp_idx);
        f_.n = (std::int32_t)n;
        f_.desc = desc_.data(); f_.angle = angle_.data(); f_.octave = octave_.data(); f_.bearing = bearing_.data(); f_.usable = usable_.data();
        f_.bow.n_nodes = (std::int32_t)node_id.size(); f_.bow.node_id = nodeId_.data(); f_.bow.node_start = nodeStart_.data(); f_.bow.kp_idx = kpIdx_.data();
        // FeatureSearch::create (feature_search.cpp:22-30): the keypoints sorted by y, for the radius queries of M3-M5
        std::vector<float> x(n), y(n), sx(n), sy(n); std::vector<std::int32_t> si(n);
        for (std::size_t i = 0; i < n; ++i) { x[i] = kps[i].pt.x; y[i] = kps[i].pt.y; }
        ctx.check(ms_feature_search_sort(x.data(), y.data(), (int)n, sx.data(), sy.data(), si.data()), "ms_feature_search_sort");
        sx_ = uploaded(ctx, sx); sy_ = uploaded(ctx, sy); si_ = uploaded(ctx, si);
        // host copies of what a single query's scan needs (searchByProjectionCore settles the rare query whose top-4 list ran out right here,
        // instead of a round trip to the device): 48 bytes per keypoint
        hsx_ = std::move(sx); hsy_ = std::move(sy); hsi_ = std::move(si); hdesc_ = std::move(desc); hoct_ = std::move(oct);
    }
    // Empty arrays for up to `capacity` keypoints that ms_keyframe_admit completes on the device (admitKeyframe, map_update.hpp): nothing is
    // uploaded, now or later.  Until admitted() the keyframe has no keypoints.
    DeviceKeyframe(Context &ctx, std::size_t capacity)
        : desc_(ctx, 8 * capacity), angle_(ctx, capacity), sx_(ctx, capacity), sy_(ctx, capacity), octave_(ctx, capacity), nodeId_(ctx, capacity),
          nodeStart_(ctx, capacity + 1), kpIdx_(ctx, capacity), si_(ctx, capacity), bearing_(ctx, 3 * capacity), usable_(ctx, capacity), cap_(capacity) {}
    std::size_t capacity() const { return cap_; }            // 0 for a keyframe built from host features
    // what ms_keyframe_admit writes on the device, and the host copies it fills from its one download
    ms_admit_frame admitFrame() {
        return ms_admit_frame{(std::int32_t)cap_, desc_.data(), angle_.data(), octave_.data(), bearing_.data(), usable_.data(), sx_.data(), sy_.data(), si_.data(), nodeId_.data(),
                              nodeStart_.data(), kpIdx_.data()};
    }
    ms_admit_host admitHost(std::int32_t *keyPointTrackIds, std::int32_t *word, double *weight) {
        hsx_.resize(cap_); hsy_.resize(cap_); hsi_.resize(cap_); hoct_.resize(cap_); hdesc_.resize(8 * cap_);      // a keyframe admitted again: the vectors keep their storage
        return ms_admit_host{keyPointTrackIds, word, weight, hsx_.data(), hsy_.data(), hsi_.data(), hoct_.data(), hdesc_.data()};
    }
    // completes the ms_match_frame from the call's counts (n, n_nodes, keypoints in the node lists)
    void admitted(const std::int32_t counts[3]) {
        const std::size_t n = (std::size_t)counts[0];
        f_ = ms_match_frame{};
        f_.n = counts[0];
        f_.desc = desc_.data(); f_.angle = angle_.data(); f_.octave = octave_.data(); f_.bearing = bearing_.data(); f_.usable = usable_.data();
        f_.bow.n_nodes = counts[1]; f_.bow.node_id = nodeId_.data(); f_.bow.node_start = nodeStart_.data(); f_.bow.kp_idx = kpIdx_.data();
        hsx_.resize(n); hsy_.resize(n); hsi_.resize(n); hoct_.resize(n); hdesc_.resize(8 * n);
    }
    const std::vector<float> &hostSortedX() const { return hsx_; }
    const std::vector<float> &hostSortedY() const { return hsy_; }
    const std::vector<std::int32_t> &hostSortedIndex() const { return hsi_; }
    const std::uint32_t *hostDescriptor(std::size_t i) const { return hdesc_.data() + 8 * i; }
    int hostOctave(std::size_t i) const { return hoct_[i]; }
    const float *sortedX() const { return sx_.data(); }
    const float *sortedY() const { return sy_.data(); }
    const std::int32_t *sortedIndex() const { return si_.data(); }
    const ms_match_frame &frame() const { return f_; }
    // the DEVICE `usable` mask [keypoints]: what createNewMapPoints clears as it binds keypoints, and unboundMasks rewrites from the keyframe table
    std::uint8_t *mutableUsable() { return usable_.data(); }
    std::size_t keyPointCount() const { return (std::size_t)f_.n; }
private:
    ms_match_frame f_{};                     // pointers into the arrays below
    DeviceArray<std::uint32_t> desc_;
    DeviceArray<float> angle_, sx_, sy_;
    DeviceArray<std::int32_t> octave_, nodeId_, nodeStart_, kpIdx_, si_;
    DeviceArray<double> bearing_;
    DeviceArray<std::uint8_t> usable_;
    std::vector<float> hsx_, hsy_;
    std::vector<std::int32_t> hsi_, hoct_;
    std::vector<std::uint32_t> hdesc_;
    std::size_t cap_ = 0;
};

namespace detail {
inline std::size_t pad16(std::size_t n) { return (n + 15) / 16 * 16; }
inline std::size_t padded(std::size_t n) { return (n + 63) / 64 * 64 + 64; }      // the pitch of a scratch array of n entries

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
    const DeviceArray<std::uint32_t> dp = detail::uploaded(ctx, pool);
    const DeviceArray<std::int32_t> ds = detail::uploaded(ctx, start), di = detail::uploaded(ctx, idx);
    DeviceArray<std::int32_t> out(ctx, n);
    ctx.check(ms_descriptor_medoid(ctx.get(), dp.data(), ds.data(), di.data(), (int)n, (int)longest, out.data(), nullptr), "ms_descriptor_medoid");
    const std::vector<std::int32_t> chosen = out.download();
    return std::vector<int>(chosen.begin(), chosen.end());
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

// gate_and_score's sibling for ms_map_fuse (map_update.hpp): the same gate and the same scoring per view, but the lists stay where the kernels
// left them -- nothing but nKept comes back.  keptEntry / topIdx / topDist are DEVICE pointers into Context::workspace, packed per view at
// first[v]; `extra` = extraBytesPerEntry bytes per entry behind them for the caller's own device outputs.  The pointers hold until the next
// request for workspace.
struct DeviceGatedLists {
    std::vector<std::int32_t> index, first, count, nKept;    // index: mp_index as ms_project_gate got it
    const std::int32_t *keptEntry = nullptr, *topIdx = nullptr;
    const std::uint16_t *topDist = nullptr;
    unsigned char *extra = nullptr;
    // the rest of what the two kernels left, for ms_search_bind (searchByProjectionOnTables)
    const float *qX = nullptr, *qY = nullptr, *qRadius = nullptr;
    const std::int32_t *qMinOctave = nullptr, *qMaxOctave = nullptr, *topOctave = nullptr, *nScored = nullptr;
    const std::uint32_t *qDesc = nullptr;
    const std::uint8_t *skip = nullptr;                      // the mask the scoring used (BoundMaskSource), or null
};
// searchByProjection's bound mask taken from the DEVICE keyframe table: slot's row of kfMp [nKf x stride] over nMp map points (ms_bound_mask)
struct BoundMaskSource {
    const std::int32_t *kfMp = nullptr;
    std::size_t nKf = 0, stride = 0, nMp = 0;
    std::int32_t slot = 0;
};

// bound (optional) = where searchByProjection's skip mask comes from: it is written into the same block by ms_bound_mask, in stream order in
// front of the scoring, and the scoring of every view reads it (used with one view, whose keyframe sits in bound->slot).
inline DeviceGatedLists gate_and_score_device(Context &ctx, const DeviceMapPoints &table, const std::vector<GateView> &views, const std::vector<const DeviceKeyframe *> &kfs,
                                              const StaticSettings &settings, std::size_t extraBytesPerEntry, const BoundMaskSource *bound = nullptr) {
    std::vector<ms_gate_view> V;
    DeviceGatedLists g;
    pack_views(views, V, g.index);
    const std::size_t ne = g.index.size(), sec = pad16(4 * ne);
    g.nKept.assign(views.size(), 0);
    for (const ms_gate_view &v : V) { g.first.push_back(v.first); g.count.push_back(v.count); }
    const std::size_t oX = 0, oY = oX + sec, oR = oY + sec, oLo = oR + sec, oHi = oLo + sec, oD = oHi + sec, oE = oD + 32 * ne;
    const std::size_t oTi = oE + sec, oTo = oTi + 16 * ne, oN = oTo + 16 * ne, oTd = oN + sec, oX2 = oTd + pad16(8 * ne);
    const std::size_t nSkip = bound && !kfs.empty() ? (std::size_t)kfs[0]->frame().n : 0, oK = oX2 + pad16(extraBytesPerEntry * ne), total = oK + pad16(nSkip);
    unsigned char *ws = ctx.workspace(total + 16);
    auto F = [&](std::size_t o) { return reinterpret_cast<float *>(ws + o); };
    auto I = [&](std::size_t o) { return reinterpret_cast<std::int32_t *>(ws + o); };
    g.keptEntry = I(oE); g.topIdx = I(oTi); g.topDist = reinterpret_cast<const std::uint16_t *>(ws + oTd); g.extra = ws + oX2;
    g.qX = F(oX); g.qY = F(oY); g.qRadius = F(oR); g.qMinOctave = I(oLo); g.qMaxOctave = I(oHi); g.qDesc = reinterpret_cast<const std::uint32_t *>(ws + oD);
    g.topOctave = I(oTo); g.nScored = I(oN);
    if (bound) {
        g.skip = ws + oK;
        ctx.check(ms_bound_mask(ctx.get(), bound->kfMp, (int)bound->nKf, (int)bound->stride, (int)bound->nMp, bound->slot, (int)nSkip, ws + oK), "ms_bound_mask");
    }
    ctx.check(ms_project_gate(ctx.get(), table.position(), table.norm(), table.minDistance(), table.maxDistance(), table.descriptor(), (int)table.size(),
                              g.index.data(), (int)ne, V.data(), (int)V.size(), settings.scaleFactors.data(), (int)settings.scaleFactors.size(),
                              settings.parameters.orbScaleFactor, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, I(oE), F(oX), F(oY), F(oR), I(oLo), I(oHi),
                              reinterpret_cast<std::uint32_t *>(ws + oD), g.nKept.data()), "ms_project_gate");
    for (std::size_t v = 0; v < V.size() && ne; ++v) {
        const std::size_t f = (std::size_t)V[v].first;
        const ms_match_frame &fr = kfs[v]->frame();
        ctx.check(ms_projection_topk(ctx.get(), kfs[v]->sortedX(), kfs[v]->sortedY(), kfs[v]->sortedIndex(), fr.n, fr.desc, fr.octave, g.skip,
                                     F(oX) + f, F(oY) + f, F(oR) + f, I(oLo) + f, I(oHi) + f, reinterpret_cast<const std::uint32_t *>(ws + oD) + 8 * f, g.nKept[v],
                                     I(oTi) + 4 * f, reinterpret_cast<std::uint16_t *>(ws + oTd) + 4 * f, I(oTo) + 4 * f, I(oN) + f, nullptr), "ms_projection_topk");
    }
    return g;
}
}  // namespace detail

// What searchByProjectionOnTables returns: the match count, the queries per outcome code of ms_search_bind (counts[5] = the rescans) and, on
// request, per entry of view.indices the matched keypoint or -1.
struct SearchBindResult {
    unsigned matched = 0;
    std::array<std::int32_t, 6> counts{};
    std::vector<std::int32_t> matchKp;
};

// searchByProjection (keyframe_matcher.cpp:295-414) over table rows with the walk and both addObservations (:388-389) on the device tables:
// ms_bound_mask (slot's row of M.keyframes -> the scoring's skip mask) -> gates -> scoring -> ms_search_bind on the lists where they lie.  Writes
// M.keyframes and M.observationCount, reads M.points and M.live; kf is the keyframe in `slot`; usable (optional) = its DEVICE matcher mask
// (DeviceKeyframe::mutableUsable), cleared at each bound keypoint.  view as for searchByProjection.  Nothing comes down but the gate's n_kept
// and the result block (and match_kp when asked for).
inline SearchBindResult searchByProjectionOnTables(Context &ctx, MapTables M, const DeviceKeyframe &kf, const GateView &view, std::int32_t slot, const StaticSettings &settings,
                                                   std::uint8_t *usable = nullptr, bool wantMatches = false) {
    M.require("searchByProjectionOnTables", M.POINTS | M.FLAGS | M.LIVE | M.COUNTS);
    SearchBindResult out;
    std::int32_t *kfMp = M.keyframes.mutableTable();
    const std::size_t nKp = (std::size_t)kf.frame().n, ne = view.indices.size(), nKf = M.keyframes.size(), stride = M.keyframes.stride(), nMp = M.keyframes.mapPointCount();
    const detail::BoundMaskSource bound{kfMp, nKf, stride, nMp, slot};
    const detail::DeviceGatedLists g = detail::gate_and_score_device(ctx, *M.points, {view}, {&kf}, settings, wantMatches ? 4 : 0, &bound);
    std::int32_t *matchKp = wantMatches && ne ? reinterpret_cast<std::int32_t *>(g.extra) : nullptr;
    std::int32_t n = 0;
    const ms_match_frame &f = kf.frame();
    ctx.check(ms_search_bind(ctx.get(), kfMp, (int)nKf, (int)stride, M.live->live(), M.observationCount, (int)nMp, g.keptEntry, g.qX, g.qY, g.qRadius, g.qMinOctave, g.qMaxOctave,
                             g.qDesc, g.topIdx, g.topDist, g.topOctave, g.nScored, g.skip, kf.sortedX(), kf.sortedY(), kf.sortedIndex(), f.desc, f.octave, (int)nKp, g.index.data(),
                             g.first[0], g.count[0], g.nKept[0], slot, matchKp, nullptr, usable, &n, out.counts.data()), "ms_search_bind");
    out.matched = (unsigned)n;
    if (matchKp) out.matchKp = ctx.download(matchKp, ne);
    return out;
}

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
