// map_tables.hpp -- the device-resident map of the host mirror: what MapDB, Keyframe::mapPoints and MapPoint hold, as flat tables.
// Every class here is DeviceArray members (common.hpp) plus the checks of its update(): the host keeps the map graph, the device keeps
// these tables, and the operations of map_update.hpp and the gates of keyframe_matcher.hpp run on them where they lie.
#pragma once
#include <algorithm>
#include <array>
#include <stdexcept>
#include <string>
#include <utility>
#include "common.hpp"

namespace mi355slam {

class DeviceKeyframe;                        // keyframe_matcher.hpp

// Keyframe poses on the device, one slot per keyframe: rows 0-2 of poseCW, row-major (12 doubles).  What ms_map_refresh reads the camera
// centres from and ms_loop_correct corrects in place.  update() re-uploads a range after the host changed poses (bundle adjustment).
class DeviceKeyframePoses {
public:
    using Pose = std::array<double, 12>;
    DeviceKeyframePoses(Context &ctx, const std::vector<Pose> &poseCW) : pose_(ctx, poseCW.size()) { update(0, size(), poseCW.data()); }
    void update(std::size_t first, std::size_t count, const Pose *poseCW) { pose_.upload(first, count, poseCW); }
    std::vector<Pose> download() const { return pose_.download(); }
    std::size_t size() const { return pose_.size(); }
    double *pose() const { return reinterpret_cast<double *>(pose_.data()); }
private:
    mutable DeviceArray<Pose> pose_;         // pose() const hands out the pointer the kernels write through
};

// Keypoint descriptors on the device, the pool MapObservation::descriptor indexes (the descriptors of the keyframes' keypoints, uploaded as the
// keyframes arrive).
class DeviceDescriptorPool {
public:
    DeviceDescriptorPool(Context &ctx, const std::vector<KeyPoint::Descriptor> &descriptors) : desc_(ctx, descriptors.size()), used_(descriptors.size()) {
        desc_.upload(0, size(), descriptors.data());
    }
    // An empty pool of `capacity` descriptors that keyframes are admitted into (admitKeyframe, map_update.hpp): append only.  Space is not
    // reused when keyframes leave.
    DeviceDescriptorPool(Context &ctx, std::size_t capacity) : desc_(ctx, capacity) {}
    // room for n more descriptors: the index of the first.  Throws when the pool is full; nothing is reserved then.
    std::size_t reserve(std::size_t n) {
        if (n > size() - used_) throw std::length_error("DeviceDescriptorPool::reserve: " + std::to_string(n) + " descriptors, " + std::to_string(size() - used_) + " free");
        const std::size_t base = used_;
        used_ += n;
        return base;
    }
    // the last n descriptors of the latest reservation were not needed (admitKeyframe reserves before the device has counted the keypoints)
    void release(std::size_t n) {
        if (n > used_) throw std::length_error("DeviceDescriptorPool::release: more than is reserved");
        used_ -= n;
    }
    std::size_t used() const { return used_; }
    std::size_t size() const { return desc_.size(); }
    const std::uint32_t *descriptor() const { return reinterpret_cast<const std::uint32_t *>(desc_.data()); }
    std::uint32_t *mutableDescriptor() { return reinterpret_cast<std::uint32_t *>(desc_.data()); }      // what admitKeyframe writes
private:
    DeviceArray<KeyPoint::Descriptor> desc_;
    std::size_t used_ = 0;
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
                    const std::vector<float> &maxDistance, const std::vector<KeyPoint::Descriptor> &descriptor) : n_(position.size()) {
        if (norm.size() != n_ || minDistance.size() != n_ || maxDistance.size() != n_ || descriptor.size() != n_)
            throw std::runtime_error("DeviceMapPoints: the arrays describe different numbers of map points");
        pos_ = DeviceArray<double>(ctx, 3 * n_); norm_ = DeviceArray<float>(ctx, 3 * n_); min_ = DeviceArray<float>(ctx, n_); max_ = DeviceArray<float>(ctx, n_);
        desc_ = DeviceArray<std::uint32_t>(ctx, 8 * n_);
        update(0, n_, position.data(), norm.data(), minDistance.data(), maxDistance.data(), descriptor.data());
    }
    // rows [first, first + count) of the fields that are not nullptr
    void update(std::size_t first, std::size_t count, const Vec3d *position, const Vec3f *norm, const float *minDistance, const float *maxDistance,
                const KeyPoint::Descriptor *descriptor) {
        if (first + count > n_) throw std::runtime_error("DeviceMapPoints::update: range outside the table");
        if (count == 0) return;
        if (position) pos_.upload(3 * first, 3 * count, position->data());
        if (norm) norm_.upload(3 * first, 3 * count, norm->data());
        if (minDistance) min_.upload(first, count, minDistance);
        if (maxDistance) max_.upload(first, count, maxDistance);
        if (descriptor) desc_.upload(8 * first, 8 * count, descriptor->data());
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
        ctx.check(ms_map_refresh(ctx.get(), pos_.data(), norm_.data(), min_.data(), max_.data(), desc_.data(), (int)n_, poses.pose(), (int)poses.size(),
                                 pool ? pool->descriptor() : nullptr, pool ? (int)pool->size() : 0, rows.data(), (int)rows.size(), start.data(), kf.data(), pool ? desc.data() : nullptr,
                                 firstOctave.data(), settings.scaleFactors.data(), (int)settings.scaleFactors.size(), medoid.data()), "ms_map_refresh");
        return std::vector<int>(medoid.begin(), medoid.end());
    }
    double *mutablePosition() { return pos_.data(); }
    float *mutableNorm() { return norm_.data(); }            // what updateMapPoints writes, with the two distances and the descriptors
    float *mutableMinDistance() { return min_.data(); }
    float *mutableMaxDistance() { return max_.data(); }
    std::uint32_t *mutableDescriptor() { return desc_.data(); }
    std::size_t size() const { return n_; }
    const double *position() const { return pos_.data(); }
    const float *norm() const { return norm_.data(); }
    const float *minDistance() const { return min_.data(); }
    const float *maxDistance() const { return max_.data(); }
    const std::uint32_t *descriptor() const { return desc_.data(); }
private:
    std::size_t n_;
    DeviceArray<double> pos_;
    DeviceArray<float> norm_, min_, max_;
    DeviceArray<std::uint32_t> desc_;
};

// Keyframe::mapPoints of every keyframe on the device, one slot per keyframe: entry j of a slot = the DeviceMapPoints row bound to keypoint j,
// -1 for none.  What getNeighbors and the map-point unions read; the lists those produce are what GateView::indices / LoopPoints take.
class DeviceKeyframeMapPoints {
public:
    DeviceKeyframeMapPoints(Context &ctx, std::size_t slots, std::size_t stride, std::size_t mapPoints) : n_(slots), stride_(stride), nMp_(mapPoints) {
        if (stride_ < 1) throw std::invalid_argument("DeviceKeyframeMapPoints: stride < 1");
        table_ = DeviceArray<std::int32_t>(ctx, n_ * stride_);
        table_.fill(-1);
    }
    // Keyframe::mapPoints of the keyframe in `slot` (shorter than the stride: padded with -1).  The host still holds the data here, so this is
    // where an entry outside [-1, mapPoints) is turned away; the kernels treat whatever they find outside [0, mapPoints) as "none".
    void update(std::size_t slot, const std::vector<std::int32_t> &mapPoints) {
        if (slot >= n_ || mapPoints.size() > stride_) throw std::invalid_argument("DeviceKeyframeMapPoints::update: slot or length outside the table");
        for (std::int32_t r : mapPoints)
            if (r < -1 || r >= (std::int64_t)nMp_) throw std::invalid_argument("DeviceKeyframeMapPoints::update: entry " + std::to_string(r) + " outside [-1, " + std::to_string(nMp_) + ")");
        std::vector<std::int32_t> row(stride_, -1);
        std::copy(mapPoints.begin(), mapPoints.end(), row.begin());
        table_.upload(slot * stride_, stride_, row.data());
    }
    void clear(std::size_t slot) { update(slot, {}); }      // a removed keyframe
    std::size_t size() const { return n_; }
    std::size_t stride() const { return stride_; }
    std::size_t mapPointCount() const { return nMp_; }
    const std::int32_t *table() const { return table_.data(); }
    std::int32_t *mutableTable() { return table_.data(); }            // what cullMap writes
private:
    std::size_t n_, stride_, nMp_;
    DeviceArray<std::int32_t> table_;
};

// MapPoint::status of every table row as the queries read it: bit 0 = TRIANGULATED, bit 1 = neither NOT_TRIANGULATED nor BAD.
class DeviceMapPointFlags {
public:
    static constexpr std::uint8_t TRIANGULATED = 1, USABLE = 2;
    DeviceMapPointFlags(Context &ctx, const std::vector<std::uint8_t> &flags) : flags_(ctx, flags.size()) { update(0, size(), flags.data()); }
    void update(std::size_t first, std::size_t count, const std::uint8_t *flags) { flags_.upload(first, count, flags); }
    std::size_t size() const { return flags_.size(); }
    const std::uint8_t *flags() const { return flags_.data(); }
    std::uint8_t *mutableFlags() { return flags_.data(); }          // what triangulateMapPoints writes
private:
    DeviceArray<std::uint8_t> flags_;
};

// Non-zero = the table row holds a map point of mapDB.mapPoints.  A free row and a point whose observations are all gone both have zero
// observations, and triangulateMapPoints overwrites the flags, so this is an array of its own.
class DeviceMapPointLive {
public:
    DeviceMapPointLive(Context &ctx, const std::vector<std::uint8_t> &live) : live_(ctx, live.size()) { update(0, size(), live.data()); }
    void update(std::size_t first, std::size_t count, const std::uint8_t *live) { live_.upload(first, count, live); }
    std::vector<std::uint8_t> download() const { return live_.download(); }
    std::size_t size() const { return live_.size(); }
    const std::uint8_t *live() const { return live_.data(); }
    std::uint8_t *mutableLive() { return live_.data(); }              // what cullMap writes
private:
    DeviceArray<std::uint8_t> live_;
};

// ---- observation lists on the device (ms_observation_lists, ms_map_refresh_lists, ms_triangulate_lists) -------------------------------
// The keypoints of every keyframe on the device, parallel to DeviceKeyframeMapPoints: kp.pt.x / kp.pt.y, kp.octave and keyPointDepth of
// keypoint j of the keyframe in a slot (a depth <= 0 is "none", as the triangulator reads it).  update() uploads one slot when its keyframe arrives.
class DeviceKeypointTable {
public:
    DeviceKeypointTable(Context &ctx, std::size_t slots, std::size_t stride) : n_(slots), stride_(stride) {
        if (stride_ < 1) throw std::invalid_argument("DeviceKeypointTable: stride < 1");
        x_ = DeviceArray<float>(ctx, n_ * stride_); y_ = DeviceArray<float>(ctx, n_ * stride_);
        octave_ = DeviceArray<std::int32_t>(ctx, n_ * stride_); depth_ = DeviceArray<float>(ctx, n_ * stride_);
        x_.fill(0.0f); y_.fill(0.0f); octave_.fill(0); depth_.fill(0.0f);       // x = y = 0, octave 0, no depth
    }
    // the keypoints of the keyframe in `slot` (shorter than the stride: the rest keeps what it held; no map point is bound there).  depth may be empty
    void update(std::size_t slot, const std::vector<float> &x, const std::vector<float> &y, const std::vector<std::int32_t> &octave, const std::vector<float> &depth) {
        const std::size_t n = x.size();
        if (slot >= n_ || n > stride_ || y.size() != n || octave.size() != n || (!depth.empty() && depth.size() != n))
            throw std::invalid_argument("DeviceKeypointTable::update: slot or lengths outside the table");
        if (n == 0) return;
        const std::vector<float> none(n, -1.0f);
        x_.upload(slot * stride_, n, x.data()); y_.upload(slot * stride_, n, y.data()); octave_.upload(slot * stride_, n, octave.data());
        depth_.upload(slot * stride_, n, depth.empty() ? none.data() : depth.data());
    }
    std::size_t size() const { return n_; }
    std::size_t stride() const { return stride_; }
    const float *x() const { return x_.data(); }
    const float *y() const { return y_.data(); }
    const std::int32_t *octave() const { return octave_.data(); }
    const float *depth() const { return depth_.data(); }
    float *mutableX() { return x_.data(); }                  // what admitKeyframe writes, with the three below
    float *mutableY() { return y_.data(); }
    std::int32_t *mutableOctave() { return octave_.data(); }
    float *mutableDepth() { return depth_.data(); }
private:
    std::size_t n_, stride_;
    DeviceArray<float> x_, y_;
    DeviceArray<std::int32_t> octave_;
    DeviceArray<float> depth_;
};

struct MapTables;

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
    // The lists of `selection` over M.keyframes / M.keypoints / M.flags (may be null) with M.slots.id (per slot the KfId, -1 for an empty slot);
    // withDescriptors: M.slots.descBase gives the descriptor indices; levels: octaves outside [0, levels) are an error (0: not looked at).
    void build(const MapTables &M, bool withDescriptors, const ObservationSelection &selection, int levels);
    // room for at least `rows` rows and `observations` observations (the contents are not kept when the buffers grow), and the counts a
    // caller that filled the lists itself (createNewMapPoints) found
    void ensure(std::size_t rows, std::size_t observations) {
        if (rows > capRows_ || observations > capObs_ || !buf_.obsStart.data()) reserve(std::max(rows, capRows_), std::max(observations, capObs_));
    }
    void setCounts(std::size_t rows, std::size_t observations, bool hasDescriptors) { nRows_ = rows; nObs_ = observations; hasDesc_ = hasDescriptors; }
    std::size_t rowCapacity() const { return capRows_; }
    std::size_t observationCapacity() const { return capObs_; }
    std::size_t rowCount() const { return nRows_; }
    std::size_t observationCount() const { return nObs_; }
    bool hasDescriptors() const { return hasDesc_; }
    ms_obs_lists lists(bool withDescriptors = true) const {                   // false: obs_desc = nullptr, for a call without a pool
        Buffers &b = buf_;
        return ms_obs_lists{b.rows.data(), b.obsStart.data(), b.nObsRow.data(), b.firstOctave.data(), b.wasTriangulated.data(), b.obsKf.data(), b.obsKp.data(),
                            b.obsOctave.data(), withDescriptors ? b.obsDesc.data() : nullptr, b.obsX.data(), b.obsY.data(), b.obsDepth.data()};
    }
    // a copy for the host (tests, debugging): `count` int32 from a row array (rows, obs_start, n_obs_row, first_octave) or an observation array
    std::vector<std::int32_t> download(const std::int32_t *deviceArray, std::size_t count) const { return ctx_.download(deviceArray, count); }
private:
    struct Buffers {                         // in the order of ms_obs_lists' fields
        DeviceArray<std::int32_t> rows, obsStart, nObsRow, firstOctave;
        DeviceArray<std::uint8_t> wasTriangulated;
        DeviceArray<std::int32_t> obsKf, obsKp, obsOctave, obsDesc;
        DeviceArray<float> obsX, obsY, obsDepth;
    };
    // free, forget the capacity, allocate, then record the capacity (Context::workspace's order): one set of buffers at the peak, and a failed allocation leaves none and capacity 0
    void reserve(std::size_t rows, std::size_t observations) {
        buf_ = Buffers{};
        capRows_ = capObs_ = 0;
        const std::size_t capRows = rows + rows / 2, capObs = observations + observations / 2;
        Buffers b;
        b.rows = DeviceArray<std::int32_t>(ctx_, capRows + 1); b.obsStart = DeviceArray<std::int32_t>(ctx_, capRows + 1);
        b.nObsRow = DeviceArray<std::int32_t>(ctx_, capRows + 1); b.firstOctave = DeviceArray<std::int32_t>(ctx_, capRows + 1);
        b.wasTriangulated = DeviceArray<std::uint8_t>(ctx_, 4 * (capRows + 1));                // four bytes a row, as the other row arrays
        b.obsKf = DeviceArray<std::int32_t>(ctx_, capObs); b.obsKp = DeviceArray<std::int32_t>(ctx_, capObs);
        b.obsOctave = DeviceArray<std::int32_t>(ctx_, capObs); b.obsDesc = DeviceArray<std::int32_t>(ctx_, capObs);
        b.obsX = DeviceArray<float>(ctx_, capObs); b.obsY = DeviceArray<float>(ctx_, capObs); b.obsDepth = DeviceArray<float>(ctx_, capObs);
        buf_ = std::move(b);
        capRows_ = capRows; capObs_ = capObs;
    }
    Context &ctx_;
    mutable Buffers buf_;                    // lists() const hands out the pointers the kernels write through
    std::size_t capRows_ = 0, capObs_ = 0, nRows_ = 0, nObs_ = 0;
    bool hasDesc_ = false;
};

// MapPoint::trackId of every table row and mapDB.trackIdToMapPoint as a window of track ids on the device.  A track counts as present only
// while its row is live and carries the id back, so cullMap and the reuse of a row need no write here: the entries go stale and are read
// as erased.  Grow-only: ensureTrack() widens the window (the contents move through the host; rare).
class DeviceTrackTable {
public:
    DeviceTrackTable(Context &ctx, std::size_t mapPoints, std::int32_t trackBase = 0, std::size_t window = 4096) : ctx_(ctx), base_(trackBase), mpTrack_(ctx, mapPoints) {
        mpTrack_.fill(-1);
        reserve(window);
    }
    // the window holds at least [trackBase, trackId]
    void ensureTrack(std::int32_t trackId) {
        if (trackId < base_) throw std::invalid_argument("DeviceTrackTable::ensureTrack: track id below the window base");
        const std::size_t need = (std::size_t)(trackId - base_) + 1;
        if (need > window()) reserve(std::max(need, 2 * window()));
    }
    // rows that already hold points of known tracks (a map loaded from the host): mp_track[row] = trackId and track_row[trackId] = row
    void bind(const std::vector<std::int32_t> &rows, const std::vector<std::int32_t> &trackIds) {
        if (rows.size() != trackIds.size()) throw std::invalid_argument("DeviceTrackTable::bind: one track id per row");
        for (std::size_t i = 0; i < rows.size(); ++i) {
            if (rows[i] < 0 || (std::size_t)rows[i] >= mapPointCount()) throw std::invalid_argument("DeviceTrackTable::bind: row outside the table");
            ensureTrack(trackIds[i]);
        }
        for (std::size_t i = 0; i < rows.size(); ++i) {
            mpTrack_.upload((std::size_t)rows[i], 1, &trackIds[i]);
            trackRow_.upload((std::size_t)(trackIds[i] - base_), 1, &rows[i]);
        }
    }
    std::vector<std::int32_t> downloadMapPointTracks() const { return mpTrack_.download(); }
    std::vector<std::int32_t> downloadTrackRows() const { return trackRow_.download(); }
    std::size_t mapPointCount() const { return mpTrack_.size(); }
    std::size_t window() const { return trackRow_.size(); }
    std::int32_t trackBase() const { return base_; }
    std::int32_t *mpTrack() const { return mpTrack_.data(); }
    std::int32_t *trackRow() const { return trackRow_.data(); }
private:
    // allocate and fill the new window, then drop the old one: a failure on the way leaves the old window as it was
    void reserve(std::size_t window) {
        std::vector<std::int32_t> rows = downloadTrackRows();
        rows.resize(std::max<std::size_t>(window, 1), -1);
        DeviceArray<std::int32_t> grown(ctx_, rows.size());
        grown.upload(0, rows.size(), rows.data());
        trackRow_ = std::move(grown);
    }
    Context &ctx_;
    std::int32_t base_;
    mutable DeviceArray<std::int32_t> mpTrack_, trackRow_;      // mpTrack() / trackRow() const hand out the pointers the kernels write through
};

// ---- the view every map-table entry point takes ------------------------------------------------------------------------------------------
// What the host keeps per keyframe slot, one entry per slot of DeviceKeyframeMapPoints in each vector a step reads (MapTables::require).
struct KeyframeSlots {
    std::vector<std::int32_t> id;                            // KfId, -1 for an empty slot
    std::vector<double> t;                                   // Keyframe::t
    std::vector<std::int32_t> previous, next;                // previousKfId / nextKfId as slots, -1 for none
    std::vector<std::array<double, 3>> cameraCenter;         // Keyframe::cameraCenter()
    std::vector<ms_pinhole> camera;                          // the pinhole stand-in of kf.shared->camera
    std::vector<std::int32_t> focalLength;                   // its getFocalLength()
    std::vector<std::int32_t> descBase;                      // DeviceDescriptorPool index of the slot's keypoint 0, -1 for none
    std::vector<DeviceKeyframe *> frames;                    // the slot's matcher inputs on the device, null for none
};

// The map tables as one non-owning view: references for what every step reads, pointers for what only some do.  Built once and passed down a
// chain of steps; each step names the parts it needs in one require() line and says in its comment which tables it writes.
struct MapTables {
    enum Part : unsigned { POINTS = 1, FLAGS = 2, LIVE = 4, KEYPOINTS = 8, POSES = 16, TRACKS = 32, COUNTS = 64, LISTS = 128, CAMERAS = 256, FOCALS = 512, IDS = 1024,
                           TIMES = 2048, LINKS = 4096, CENTRES = 8192, DESC_BASES = 16384, FRAMES = 32768 };
    DeviceKeyframeMapPoints &keyframes;
    KeyframeSlots &slots;
    DeviceMapPoints *points = nullptr;
    DeviceMapPointFlags *flags = nullptr;
    DeviceMapPointLive *live = nullptr;
    DeviceKeypointTable *keypoints = nullptr;
    DeviceKeyframePoses *poses = nullptr;
    DeviceTrackTable *tracks = nullptr;
    DeviceDescriptorPool *pool = nullptr;
    std::int32_t *observationCount = nullptr;                // DEVICE [mapPointCount]: mp.observations.size() of every row (observationCountsOnDevice)
    DeviceObservationLists *lists = nullptr;                 // scratch of the steps that build observation lists

    // Throws std::invalid_argument(who + ": ...") when a part of `parts` is absent, when a table that is present disagrees in size with the
    // keyframe table, or when a per-slot vector of `parts` does not have one entry per slot.
    void require(const char *who, unsigned parts) const {
        const std::size_t nKf = keyframes.size(), nMp = keyframes.mapPointCount();
        auto fail = [&](const std::string &what) { throw std::invalid_argument(std::string(who) + ": " + what); };
        const void *const present[] = {points, flags, live, keypoints, poses, tracks, observationCount, lists};
        const std::size_t perSlot[] = {slots.camera.size(), slots.focalLength.size(), slots.id.size(), slots.t.size(), std::min(slots.previous.size(), slots.next.size()),
                                       slots.cameraCenter.size(), slots.descBase.size(), slots.frames.size()};
        static const char *const name[] = {"map points", "flags", "live bytes", "keypoint table", "poses", "track table", "observation counts", "observation lists", "camera", "focal length",
                                           "KfId", "time", "link pair", "camera centre", "descriptor base", "frame"};
        for (unsigned i = 0; i < 8; ++i) if ((parts >> i & 1) && !present[i]) fail(std::string("no ") + name[i]);
        if ((points && points->size() != nMp) || (flags && flags->size() < nMp) || (live && live->size() < nMp) || (tracks && tracks->mapPointCount() != nMp))
            fail("the map-point tables differ in size");
        if (keypoints && (keypoints->size() != nKf || keypoints->stride() != keyframes.stride())) fail("the keypoint table does not match the keyframe table");
        if (poses && poses->size() != nKf) fail("one pose per slot");
        for (unsigned i = 8; i < 16; ++i) if ((parts >> i & 1) && perSlot[i - 8] != nKf) fail(std::string("one ") + name[i] + " per slot");
        if ((parts & LINKS) && slots.previous.size() != slots.next.size()) fail("one link pair per slot");
    }
    const std::uint32_t *poolDescriptor() const { return pool ? pool->descriptor() : nullptr; }
    int poolSize() const { return pool ? (int)pool->size() : 0; }
    // the four track arguments of ms_map_fuse / ms_map_replace_pairs (nulls and zeros without a track table)
    struct TrackWindow { std::int32_t *mpTrack, *trackRow, base; int window; };
    TrackWindow trackWindow() const { return tracks ? TrackWindow{tracks->mpTrack(), tracks->trackRow(), tracks->trackBase(), (int)tracks->window()} : TrackWindow{nullptr, nullptr, 0, 0}; }
};

inline void DeviceObservationLists::build(const MapTables &M, bool withDescriptors, const ObservationSelection &selection, int levels) {
    M.require("DeviceObservationLists::build", M.KEYPOINTS | M.IDS | (withDescriptors ? M.DESC_BASES : 0u));
    const DeviceKeyframeMapPoints &table = M.keyframes;
    const ms_obs_select sel{selection.slot >= 0 ? MS_OBS_FROM_SLOT : MS_OBS_FROM_ROWS, selection.filter, selection.dropEmpty ? 1 : 0, selection.slot, selection.deviceRows,
                            (std::int32_t)selection.rowCount};
    if (!buf_.obsStart.data()) reserve(0, 0);                // a regrow that failed left nothing behind: start again from the smallest buffers
    for (int attempt = 0;; ++attempt) {
        ms_obs_lists l = lists(withDescriptors);
        if (!M.flags) l.was_triangulated = nullptr;
        std::int32_t nRows = 0, nObs = 0;
        const int rc = ms_observation_lists(ctx_.get(), table.table(), (int)table.size(), (int)table.stride(), (int)table.mapPointCount(), M.slots.id.data(),
                                            M.flags ? M.flags->flags() : nullptr, M.keypoints->x(), M.keypoints->y(), M.keypoints->octave(), M.keypoints->depth(),
                                            withDescriptors ? M.slots.descBase.data() : nullptr, &sel, levels, &l, (int)capRows_, (int)capObs_, &nRows, &nObs);
        if (rc == MS_ERR_CAPACITY && attempt == 0 && ((std::size_t)nRows > capRows_ || (std::size_t)nObs > capObs_)) {
            reserve(std::max<std::size_t>(nRows, capRows_), std::max<std::size_t>(nObs, capObs_));      // the needed counts came back: once is enough
            continue;
        }
        ctx_.check(rc, "ms_observation_lists");
        nRows_ = (std::size_t)nRows; nObs_ = (std::size_t)nObs;
        hasDesc_ = withDescriptors;
        return;
    }
}

}  // namespace mi355slam
