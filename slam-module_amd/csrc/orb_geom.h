// orb_geom.h -- everything ms_orb_create (orb.hip) works out on the host before it touches the device: the pyramid geometry the kernels
// trust (orb_geometry), the constant tables (orb_resize_tables, orb_describe_tables) and the layout of the extractor's one device block
// (ORB_BLOCK_* / orb_block_layout).  Plain C++17, no HIP: tests/orb_geom_check.cpp compiles it alone with geometry.cpp and compares it with a
// record of the arithmetic it was lifted from (tests/golden/orb_geom_cases.txt).
//
// The declarations live in an anonymous namespace because the structs are kernel arguments of orb.hip, whose kernels are declared in one:
// the namespace is part of the kernels' mangled names.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include "ms_check.h"
#include "ms_geometry.h"
#include "ms_layout.h"
#include "fast_tiles.h"
#include "describe_order.h"
#include "describe_lanes.h"
#include "resize_plan.h"

#if defined(__HIPCC__)
typedef uint2 orb_u2; typedef uint4 orb_u4; typedef float4 orb_f4;
#else       // the same bytes for a host compiler (only their sizes matter to the layout)
struct alignas(8) orb_u2 { uint32_t x, y; };
struct alignas(16) orb_u4 { uint32_t x, y, z, w; };
struct alignas(16) orb_f4 { float x, y, z, w; };
#endif

namespace {

constexpr int kPatchRadius = MS_ORB_PATCH_RADIUS;   // 19
constexpr int kMaxQuota = 4096;                      // per-level selection capacity (LDS sort)
constexpr int kResizeRows = 5;   // destination rows per lane: the table fetch is paid once and 10 source windows (30 dwords) are in flight per lane
constexpr int kFastPruneMinBlocks = 2 * 4 * 256;   // launches with more workgroups than this learn a raised threshold (k_fast)
constexpr int kBlurSeg = 248;   // outputs per wave row segment
constexpr int kBlurRows = 18;   // output rows per wave (+ 6 halo rows loaded).  Measured in one session: 8 -> 0.61 ms, 14 -> 0.53, 16 -> 0.67 (64-row tiles: row starts collide), 18 -> 0.51, 28 -> 0.51
// (8 pixels per lane with 8-byte loads and stores -- half the memory instructions per pixel -- was built and measured: 0.60 ms against 0.51, at 6..10 rows per wave)

struct LevelGeom {
    int32_t w, h, pitch, quota;
    int32_t min_dist;                 // per-level minimum keypoint distance (0/1 = none), feature_detector.cpp:79-82
    int32_t det_base;                 // first slot of this level in det arrays (prefix of quotas)
    int32_t cand_cap;                 // capacity of this level's candidate list (entries)
    int32_t btiles_x, btile_base;     // k_blur tile table (248 x 72 tiles: 4 waves x kBlurRows rows)
    uint32_t btiles_inv;              // ceil(2^32 / tiles_x): row of a tile = mulhi(t, inv), exact for t < 2^16
    uint64_t img_off, blur_off;       // byte offsets inside a frame slab
    uint64_t cand_off;                // entry offset inside a frame's candidate buffer
    float scale;                      // scaleFactors[l] (float32 chain)
};

struct PyrGeom {
    int32_t levels, lk_level, fast_threshold, max_kpts, max_tracks, capacity;
    int32_t det_stride;               // per-frame stride of the det arrays = max(max_kpts, sum of the level quotas): the quotas are rounded per level
                                      // (static_settings.cpp:52) and can add up to more than max_kpts (e.g. 15 levels / 160 keypoints -> 161)
    int32_t width, height, btiles_total, ftiles_total;      // ftiles_total: entries of k_fast's tile table (fast_tiles.h)
    uint64_t slab_stride, cand_stride;     // per frame: bytes / entries
    int32_t umax[16];
    LevelGeom L[MS_MAX_LEVELS];
};

// first tile id of every level, passed BY VALUE (kernel-argument SGPRs): finding a block's level must not be a chain of
// dependent loads from the geometry table (that chain was a third of k_fast's wave time)
struct TileMap { int32_t base[MS_MAX_LEVELS + 1]; };

// What the tiled kernels (k_blur, k_fast) need about a level, also BY VALUE in the kernel arguments: one batch of scalar loads from the
// kernel-argument segment once the block knows its level, instead of a chain of dependent loads from the geometry table behind branches.
struct TileLevel { int32_t w, h, pitch, btiles_x, cand_cap; uint32_t btiles_inv; uint64_t img_off, blur_off, cand_off; float scale; int32_t det_base;
                   int32_t sel_k; };     // sel_k: how many of the level's strongest candidates k_select looks at (its `want`)
struct TileLevels { TileLevel L[MS_MAX_LEVELS]; uint64_t slab_stride, cand_stride; int32_t levels, fast_threshold; };

// ------------------------------------------------------------------------------------------------ geometry
struct OrbGeom {
    PyrGeom geom;
    TileLevels tile_levels;
    TileMap blur_tiles;
    std::vector<uint32_t> ftile_tab;     // k_fast's tile table (the cover of fast_tiles.h), two dwords per tile: level | S << 4,  X0 | Y0 << 16
    int32_t ftiles_level0;               // its first entries are level 0's tiles (the table is level-major): how many
    uint64_t lvl0_off;                   // where a caller's level 0 goes when it cannot be used in place
    int32_t lvl0_pitch;
};

#define ORB_GEOM_FAIL(code, ...) return ms_why(code, why, why_bytes, __VA_ARGS__)

// Checks a configuration and derives its geometry.  MS_OK, or MS_ERR_INVALID / MS_ERR_CAPACITY with the reason in `why` (R is then half filled
// and not to be used).  The first failing statement decides the message.
inline int orb_geometry(const ms_orb_config &cfg, OrbGeom &R, char *why, size_t why_bytes) {
    if (cfg.levels < 1 || cfg.levels > MS_MAX_LEVELS || cfg.max_kpts < 1 || cfg.max_batch < 1 || cfg.max_tracks < 0 ||
        cfg.lk_track_level < 0 || cfg.lk_track_level >= cfg.levels || cfg.fast_threshold < 1 || cfg.fast_threshold > 254 ||
        !(cfg.scale_factor > 1.0f) || !(cfg.min_distance >= 0.f) || cfg.width > 32767 || cfg.height > 32767 ||
        (int64_t)cfg.width * cfg.height >= (1 << 24))
        ORB_GEOM_FAIL(MS_ERR_INVALID, "unsupported configuration");
    R = OrbGeom{};
    PyrGeom &G = R.geom;
    G.levels = cfg.levels; G.lk_level = cfg.lk_track_level; G.fast_threshold = cfg.fast_threshold;
    G.max_kpts = cfg.max_kpts; G.max_tracks = cfg.max_tracks;
    G.width = cfg.width; G.height = cfg.height;
    int32_t w[MS_MAX_LEVELS], h[MS_MAX_LEVELS], quota[MS_MAX_LEVELS];
    float sf[MS_MAX_LEVELS];
    msgeo::level_sizes(cfg.levels, cfg.scale_factor, cfg.width, cfg.height, w, h);
    msgeo::level_quotas(cfg.levels, cfg.scale_factor, cfg.max_kpts, quota);
    msgeo::scale_factors(cfg.levels, cfg.scale_factor, sf);
    msgeo::umax(G.umax);
    uint64_t off = 0, coff = 0;
    int det_base = 0, bt = 0;
    for (int l = 0; l < cfg.levels; ++l) {
        if (w[l] < 2 * kPatchRadius + 2 || h[l] < 2 * kPatchRadius + 2 || quota[l] > kMaxQuota)
            ORB_GEOM_FAIL(MS_ERR_INVALID, "level %d is %dx%d (min 40x40) / quota %d (max %d)", l, w[l], h[l], quota[l], kMaxQuota);
        // k_blur's mulhi tile division is exact below 2^16 tiles per level.  Out of reach under the limits above: a level is at most 32767 pixels
        // either way, which is 133 x 456 = 60648 tiles of 248 x 72 outputs (and 65536 tiles hold more than the 2^24 pixels a frame may have).
        if ((int64_t)ms_div_up(w[l], kBlurSeg) * ms_div_up(h[l], 4 * kBlurRows) >= 65536)
            ORB_GEOM_FAIL(MS_ERR_CAPACITY, "level %d (%dx%d) needs more than 65535 blur tiles", l, w[l], h[l]);
        LevelGeom &L = G.L[l];
        L.w = w[l]; L.h = h[l]; L.pitch = (int)ms_align_up(w[l], 64); L.quota = quota[l]; L.scale = sf[l];
        {   // feature_detector.cpp:79-82: minDist = floor(gfttMinDistance * (min(w,h) / 720 * 0.8) + 0.5)
            const double su = std::min(w[l], h[l]) / 720.0 * 0.8;
            L.min_dist = (int)std::floor(cfg.min_distance * su + 0.5);
        }
        L.det_base = det_base; det_base += quota[l];
        L.img_off = off; off += (uint64_t)L.pitch * L.h;
        L.blur_off = off; off += (uint64_t)L.pitch * L.h;
        L.cand_cap = (int32_t)ms_align_up((size_t)(((w[l] + 1) / 2) * ((h[l] + 1) / 2) + 256), 4);   // strict 3x3 maxima: <= one per 2x2 block; a multiple of 4 so that every level's list starts 16-byte aligned (k_select reads it as uint4)
        L.cand_off = coff; coff += L.cand_cap;
        L.btiles_x = ms_div_up(w[l], kBlurSeg); L.btile_base = bt; bt += L.btiles_x * ms_div_up(h[l], 4 * kBlurRows);
        L.btiles_inv = (uint32_t)(((1ull << 32) + L.btiles_x - 1) / L.btiles_x);
    }
    G.btiles_total = bt;
    {
        std::vector<fast_tiles::Tile> cover;
        for (int l = 0; l < cfg.levels; ++l) {
            cover.clear();
            fast_tiles::cover(w[l], h[l], cover);
            for (const fast_tiles::Tile &t : cover) {
                R.ftile_tab.push_back((uint32_t)l | ((uint32_t)t.S << 4));
                R.ftile_tab.push_back((uint32_t)t.X0 | ((uint32_t)t.Y0 << 16));
            }
            if (l == 0) R.ftiles_level0 = (int32_t)(R.ftile_tab.size() / 2);
            // 16 bits each in the entry; the last tile of a level has the largest of both.  Out of reach: a level is at most 32767 pixels either way.
            if (!cover.empty() && (cover.back().X0 > 0xFFFF || cover.back().Y0 > 0xFFFF))
                ORB_GEOM_FAIL(MS_ERR_CAPACITY, "level %d (%dx%d) is beyond the detector's tile table (65535 px)", l, w[l], h[l]);
        }
    }
    const size_t ftiles = R.ftile_tab.size() / 2;
    G.ftiles_total = (int)ftiles;
    // the tile index is k_fast's grid y.  Out of reach: a tile holds about 7000 outputs, so a level of under 2^24 pixels has a few thousand tiles
    // (under 2500 in the shapes tried, thin ones included) and 16 levels stay below the limit
    if (ftiles > 65535) ORB_GEOM_FAIL(MS_ERR_CAPACITY, "%zu detector tiles per frame (max 65535)", ftiles);
    G.det_stride = std::max(cfg.max_kpts, det_base);       // the reference keeps per-level vectors, so a frame can hold sum(quota) > maxKeypoints points
    G.capacity = G.det_stride + cfg.max_tracks;
    // a slot-table entry holds the output slot beside the level.  In reach only through max_tracks (the quotas add up to 16 x 4096 at most)
    if (G.capacity >= (1 << (32 - describe_order::kSlotShift)))
        ORB_GEOM_FAIL(MS_ERR_CAPACITY, "%d output slots per frame (max %d)", G.capacity, (1 << (32 - describe_order::kSlotShift)) - 1);
    for (int l = 0; l < cfg.levels; ++l) {
        const LevelGeom &L = G.L[l];
        const int sel_k = (cfg.min_distance > 0.f && L.min_dist >= 2) ? std::min(4 * L.quota, kMaxQuota) : L.quota;     // k_select's `want`
        R.tile_levels.L[l] = TileLevel{L.w, L.h, L.pitch, L.btiles_x, L.cand_cap, L.btiles_inv, L.img_off, L.blur_off, L.cand_off, L.scale, L.det_base, sel_k};
    }
    for (int l = 0; l <= MS_MAX_LEVELS; ++l) R.blur_tiles.base[l] = l < cfg.levels ? G.L[l].btile_base : bt;
    G.slab_stride = ms_align_up(off, 256); G.cand_stride = coff;
    R.tile_levels.slab_stride = G.slab_stride; R.tile_levels.cand_stride = G.cand_stride; R.tile_levels.levels = G.levels; R.tile_levels.fast_threshold = G.fast_threshold;
    R.lvl0_off = G.L[0].img_off; R.lvl0_pitch = G.L[0].pitch;
    return MS_OK;
}
#undef ORB_GEOM_FAIL

// Whether a call over nf frames runs k_fast as two launches -- level 0's tiles beside the resize chain, the other levels' behind it
// (orb_enqueue_kernels): only when each part alone is a launch that learns a raised threshold, i.e. has more than kFastPruneMinBlocks
// workgroups.  A smaller call (a frame, a few frames) keeps its single launch and pays for no event pair; a pyramid of one level has no
// second part.
inline bool orb_fast_split_auto(int nf, int ftiles_level0, int ftiles_total) {
    return (long long)nf * std::min(ftiles_level0, ftiles_total - ftiles_level0) > kFastPruneMinBlocks;
}

// ------------------------------------------------------------------------------------------------ constant tables
// The tables of the resize from level l - 1 to level l >= 1: xt [w padded to 4][4] = sx, a0, a1, 0 and yt [h padded to kResizeRows][4] = sy0, sy1
// (clamped rows), b0, b1 for k_resize, padded to whole groups with the last entry repeated; `wide` when the taps of four pixels can lie beyond an
// 8-byte window (scale factor > 2); x8 = k_resize8's column table when the level's real tables pass both of its tests (resize_plan.h), else empty.
struct OrbResizeTables { std::vector<int16_t> xt, yt; std::vector<uint32_t> x8; bool wide = false; };

inline void orb_resize_tables(const PyrGeom &G, int l, OrbResizeTables &T) {
    const int sw = G.L[l - 1].w, sh = G.L[l - 1].h, dw = G.L[l].w, dh = G.L[l].h;
    std::vector<int16_t> xo, xc, yo, yc;
    msgeo::resize_tables(sw, dw, true, xo, xc);
    msgeo::resize_tables(sh, dh, false, yo, yc);
    const int wpad = ms_div_up(dw, 4) * 4, hpad = ms_div_up(dh, kResizeRows) * kResizeRows;     // whole groups, last entry repeated
    std::vector<int16_t> xt(4 * (size_t)wpad), yt(4 * (size_t)hpad);
    for (int d = 0; d < dw; ++d) { xt[4 * d] = xo[d]; xt[4 * d + 1] = xc[2 * d]; xt[4 * d + 2] = xc[2 * d + 1]; xt[4 * d + 3] = 0; }
    for (int d = 0; d < dh; ++d) {      // clip(sy, 0, ssize.height) applied to both tap rows
        yt[4 * d] = (int16_t)std::min(std::max((int)yo[d], 0), sh - 1);
        yt[4 * d + 1] = (int16_t)std::min(std::max((int)yo[d] + 1, 0), sh - 1);
        yt[4 * d + 2] = yc[2 * d]; yt[4 * d + 3] = yc[2 * d + 1];
    }
    for (int d = dw; d < wpad; ++d) for (int k = 0; k < 4; ++k) xt[4 * d + k] = xt[4 * (dw - 1) + k];
    for (int d = dh; d < hpad; ++d) for (int k = 0; k < 4; ++k) yt[4 * d + k] = yt[4 * (dh - 1) + k];
    T.wide = false;
    for (int d = 0; d + 3 < dw; d += 4) if (xo[d + 3] + 1 - xo[d] > 7) T.wide = true;   // taps beyond an 8-byte window
    T.x8.clear();                                        // the 8-pixel kernel takes the level iff its real tables pass both tests
    if (T.wide || !resize_plan::rows_shared(yt.data(), dh, sh) || !resize_plan::build_columns(xo.data(), xc.data(), sw, dw, T.x8)) T.x8.clear();
    T.xt.swap(xt); T.yt.swap(yt);
}

// k_describe's lane tables (mt) and the 256 BRIEF point pairs as floats (pf)
inline void orb_describe_tables(const int32_t *umax, std::vector<uint32_t> &mt, std::vector<float> &pf) {
    static const int8_t pattern[1024] = {
#include "orb_pattern.inc"
    };
    // disc mask of the 31 x 31 orientation patch as k_describe's lanes hold it: dword i = lane + 64 t (the t-th of the lane) covers columns 4 (i & 7) .. + 3 of row
    // i >> 3; a byte is kept when |u| <= u_max[|v|] (orb_extractor.cpp:174-186, :259-271), the 32nd column and row are cleared
    mt.assign(64 * 4 + 32 * 4 + 64 + 64 * 2, 0u);
    for (int lane = 0; lane < 64; ++lane)
        for (int t = 0; t < 4; ++t) mt[lane * 4 + t] = describe_lanes::disc_mask(lane, t, umax);
    // behind it, pass 1 of k_describe's blur as matrix operands (B of v_mfma_i32_16x16x64_i8: lane (n, kg) holds rows k = 16 kg .. + 15 of column 16 t + n, one byte each):
    // the taps 18 34 48 56 48 34 18 by patch column x -- window byte k contributes to x when 0 <= k - x - 1 <= 6.  Only dt = kg - t = 0 and 1 can be non-zero, and the
    // pattern depends on (dt, n) alone: [dt][n][4 dwords], the horizontal half of describe_lanes::tap_table (entry [1][0] is all zero and serves as the zero operand);
    // behind that the packed (row, byte) of every lane's first three window pieces, and the lane's two dwords of pass 2's A operand (the vertical taps)
    uint32_t taps[64 * 4];
    describe_lanes::tap_table(taps);
    std::copy(taps, taps + 32 * 4, &mt[64 * 4]);
    for (int lane = 0; lane < 64; ++lane) {
        mt[64 * 4 + 32 * 4 + lane] = describe_lanes::win_pack(lane);
        for (int dm = 0; dm < 2; ++dm) mt[64 * 4 + 32 * 4 + 64 + 2 * lane + dm] = describe_lanes::vert_operand(lane, dm);
    }
    pf.resize(1024);
    for (int i = 0; i < 1024; ++i) pf[i] = (float)pattern[i];
}

struct OrbTables {
    OrbResizeTables level[MS_MAX_LEVELS];       // [0] stays empty
    std::vector<uint32_t> moment;
    std::vector<float> pattern;
};
inline void orb_tables(const PyrGeom &G, OrbTables &C) {
    for (int l = 1; l < G.levels; ++l) orb_resize_tables(G, l, C.level[l]);
    orb_describe_tables(G.umax, C.moment, C.pattern);
}

// ------------------------------------------------------------------------------------------------ the device block
// Every array of the extractor's one device block, once, in block order: X(element type, name, elements) and XL(...) for an array per pyramid
// level l.  ms_orb declares its d_<name> pointers from these lists and orb_block_layout places them (MsLayout: every array starts on a 256-byte
// boundary -- k_select reads candidates as uint4, the describe outputs are written in wide stores -- and an array of no elements still has a
// byte), so a new array is one more line here.  In the counts: G = the PyrGeom, R = the OrbGeom, C = the OrbTables, B = max_batch,
// T = max(max_tracks, 1), cap = G.capacity.
//
// The constants come first and go up in one copy; a per-level array may be empty (level 0; x8 on a level k_resize8 may not take) and its pointer is then null.
#define ORB_BLOCK_CONSTANTS(X, XL)                                                                                                   \
    X (PyrGeom,  geom,       1)                                                                                                       \
    XL(int16_t,  xtab,       C.level[l].xt.size())        /* k_resize: [dw][4] */                                                     \
    XL(int16_t,  ytab,       C.level[l].yt.size())        /* k_resize, k_resize8: [dh][4] */                                          \
    XL(uint32_t, xtab8,      C.level[l].x8.size())        /* k_resize8's column table, on the levels it may take (resize_plan.h) */   \
    X (orb_u2,   ftile_tab,  R.ftile_tab.size() / 2 + 2)  /* k_fast: (level | S << 4, X0 | Y0 << 16) of every tile, + 16 bytes */      \
    X (orb_u4,   moment_tab, C.moment.size() / 4)         /* k_describe: disc mask of the orientation patch and the blur operands */   \
    X (orb_f4,   pattern_f,  C.pattern.size() / 4)        /* k_describe: the 256 BRIEF point pairs as floats */
// The working arrays, zeroed once at create time.
#define ORB_BLOCK_WORK(X)                                                                                                             \
    X(uint8_t,  slab,       B * G.slab_stride + 256)      /* + slack (round 1's k_describe could touch one byte past the last plane; today's window loads stay inside the level) */ \
    X(uint32_t, cand,       B * G.cand_stride)                                                                                        \
    X(int32_t,  cand_count, B * MS_MAX_LEVELS)                                                                                        \
    X(uint32_t, score_hist, B * MS_MAX_LEVELS * 256)      /* k_fast: 256 score bins per (frame, level) of the candidates found so far in the launch; zero between calls */ \
    X(int32_t,  last_count, B * MS_MAX_LEVELS)            /* candidates k_fast appended per (frame, level) in the last call (ms_orb_last_candidate_counts) */ \
    X(int32_t,  det_count,  B * MS_MAX_LEVELS)                                                                                        \
    X(int32_t,  trk_count,  B)                                                                                                        \
    X(int16_t,  det_x,      B * (size_t)G.det_stride)                                                                                 \
    X(int16_t,  det_y,      B * (size_t)G.det_stride)                                                                                 \
    X(uint8_t,  det_score,  B * (size_t)G.det_stride)                                                                                 \
    X(int16_t,  trk_x,      B * T)                                                                                                    \
    X(int16_t,  trk_y,      B * T)                                                                                                    \
    X(float,    trk_px,     B * T)                                                                                                    \
    X(float,    trk_py,     B * T)                                                                                                    \
    X(int32_t,  trk_id,     B * T)                                                                                                    \
    X(float,    track_xy,   B * T * 2)                                                                                                \
    X(int32_t,  track_id,   B * T)                                                                                                    \
    X(int32_t,  n_tracks,   B)                                                                                                        \
    X(float,    x,          B * cap)                      /* outputs */                                                               \
    X(float,    y,          B * cap)                                                                                                  \
    X(float,    angle,      B * cap)                                                                                                  \
    X(int32_t,  octave,     B * cap)                                                                                                  \
    X(int32_t,  track,      B * cap)                                                                                                  \
    X(int32_t,  count,      B)                                                                                                        \
    X(orb_u2,   slot_tab,   B * cap)                      /* k_slots: output slot -> (x | y << 16, level) */                          \
    X(uint32_t, desc,       B * cap * 8)

#define ORB_X_ARRAY(T, name, count) MsArray<T> name;
#define ORB_XL_ARRAY(T, name, count) MsArray<T> name[MS_MAX_LEVELS];
struct OrbBlock {
    ORB_BLOCK_CONSTANTS(ORB_X_ARRAY, ORB_XL_ARRAY)
    size_t const_end = 0;               // the constants are bytes [0, const_end) ...
    ORB_BLOCK_WORK(ORB_X_ARRAY)
    size_t end = 0;                     // ... and the working arrays [const_end, end)
};
#undef ORB_X_ARRAY
#undef ORB_XL_ARRAY

inline OrbBlock orb_block_layout(const ms_orb_config &cfg, const OrbGeom &R, const OrbTables &C) {
    const PyrGeom &G = R.geom;
    const size_t B = (size_t)cfg.max_batch, T = (size_t)std::max(cfg.max_tracks, 1), cap = (size_t)G.capacity;
    OrbBlock K;
    MsLayout lay;
#define ORB_X_PLACE(E, name, count) K.name = lay.array<E>(std::max<size_t>((count), 1));
#define ORB_XL_PLACE(E, name, count) for (int l = 0; l < MS_MAX_LEVELS; ++l) K.name[l] = lay.array<E>(count);
    ORB_BLOCK_CONSTANTS(ORB_X_PLACE, ORB_XL_PLACE)
    K.const_end = lay.end;
    ORB_BLOCK_WORK(ORB_X_PLACE)
    K.end = lay.end;
#undef ORB_X_PLACE
#undef ORB_XL_PLACE
    return K;
}

// the constants of a block as the device gets them: `stage` = bytes [0, const_end) of the block
inline void orb_stage_constants(const OrbBlock &K, const OrbGeom &R, const OrbTables &C, std::vector<uint8_t> &stage) {
    stage.assign(K.const_end, 0);
    void *s = stage.data();
    K.geom.fill(s, &R.geom);
    for (int l = 0; l < MS_MAX_LEVELS; ++l) {
        K.xtab[l].fill(s, C.level[l].xt.data());
        K.ytab[l].fill(s, C.level[l].yt.data());
        K.xtab8[l].fill(s, C.level[l].x8.data());
    }
    K.ftile_tab.put(s, 0, reinterpret_cast<const orb_u2 *>(R.ftile_tab.data()), R.ftile_tab.size() / 2);
    K.moment_tab.fill(s, reinterpret_cast<const orb_u4 *>(C.moment.data()));
    K.pattern_f.fill(s, reinterpret_cast<const orb_f4 *>(C.pattern.data()));
}

}  // namespace
