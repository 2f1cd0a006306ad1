// The host side of ms_orb_create (slam-module_amd/csrc/orb_geom.h with geometry.cpp) on the CPU, against tests/golden/orb_geom_cases.txt:
//   - the record holds, per configuration, every field of PyrGeom, TileLevels and TileMap, the length and an FNV-1a hash of k_fast's tile table, the
//     level-0 offset and pitch, per level the `wide` flag and the lengths and hashes of the resize tables (an 8-pixel table of length 0 = the level
//     stays on the 4-pixel kernel), and the describe tables' hashes; for a rejected configuration the status and the message.  It was written by the
//     arithmetic of ms_orb_create before that moved into orb_geom.h, and is compared line by line, field by field;
//   - invariants of every accepted case: image and blur planes disjoint and inside slab_stride, candidate lists disjoint inside cand_stride with
//     offsets and capacities that are multiples of 4, det_base the prefix sum of the quotas, TileMap::base non-decreasing and ending at btiles_total,
//     btiles_inv dividing exactly for every tile id of its level;
//   - the device block of every accepted case at max_batch 1 and 3: arrays disjoint and 256-aligned, each at least as large as the allocation it
//     replaces (kSeparate below: the counts the separate hipMallocs had), constants a prefix, slacks present, no table on a level without one;
//   - the staged constants hold the tables where the layout says.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "orb_geom.h"

static long long g_checks = 0;
#define CHECK(c, ...) do { ++g_checks; if (!(c)) { std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); return false; } } while (0)

// ---- record ----------------------------------------------------------------------------------------------------------------------------------
static uint64_t fnv1a(const void *p, size_t bytes) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; ++i) { h ^= static_cast<const uint8_t *>(p)[i]; h *= 0x100000001b3ull; }
    return h;
}
static std::string fmt(const char *f, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof(buf), f, ap);
    va_end(ap);
    return buf;
}
static uint32_t f32_bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }
struct LevelRecord { bool wide; size_t xt_n, yt_n, x8_n; uint64_t xt_h, yt_h, x8_h; };

// the lines of an accepted configuration; templated on the struct types so that the program that wrote the record could use it on its own copies
template <class PG, class TLS, class TM>
static std::vector<std::string> record_lines(const PG &G, const TLS &TL, const TM &tm, const uint32_t *ftab, size_t ftab_dwords, uint64_t lvl0_off, int lvl0_pitch,
                                             const LevelRecord *lr, const std::vector<uint32_t> &mt, const std::vector<float> &pf) {
    std::vector<std::string> out;
    out.push_back(fmt("pyr levels %d lk_level %d fast_threshold %d max_kpts %d max_tracks %d capacity %d det_stride %d width %d height %d btiles_total %d ftiles_total %d slab_stride %" PRIu64 " cand_stride %" PRIu64,
                      G.levels, G.lk_level, G.fast_threshold, G.max_kpts, G.max_tracks, G.capacity, G.det_stride, G.width, G.height, G.btiles_total, G.ftiles_total, (uint64_t)G.slab_stride, (uint64_t)G.cand_stride));
    std::string u = "umax";
    for (int i = 0; i < 16; ++i) u += fmt(" %d", G.umax[i]);
    out.push_back(u);
    for (int l = 0; l < MS_MAX_LEVELS; ++l) {       // all 16: the levels a configuration does not use stay zero
        const auto &L = G.L[l];
        out.push_back(fmt("level %d w %d h %d pitch %d quota %d min_dist %d det_base %d cand_cap %d btiles_x %d btile_base %d btiles_inv %u img_off %" PRIu64 " blur_off %" PRIu64 " cand_off %" PRIu64 " scale 0x%08x",
                          l, L.w, L.h, L.pitch, L.quota, L.min_dist, L.det_base, L.cand_cap, L.btiles_x, L.btile_base, L.btiles_inv, (uint64_t)L.img_off, (uint64_t)L.blur_off, (uint64_t)L.cand_off, f32_bits(L.scale)));
        const auto &T = TL.L[l];
        out.push_back(fmt("tile_level %d w %d h %d pitch %d btiles_x %d cand_cap %d btiles_inv %u img_off %" PRIu64 " blur_off %" PRIu64 " cand_off %" PRIu64 " scale 0x%08x det_base %d sel_k %d",
                          l, T.w, T.h, T.pitch, T.btiles_x, T.cand_cap, T.btiles_inv, (uint64_t)T.img_off, (uint64_t)T.blur_off, (uint64_t)T.cand_off, f32_bits(T.scale), T.det_base, T.sel_k));
    }
    out.push_back(fmt("tile_levels slab_stride %" PRIu64 " cand_stride %" PRIu64 " levels %d fast_threshold %d", (uint64_t)TL.slab_stride, (uint64_t)TL.cand_stride, TL.levels, TL.fast_threshold));
    std::string b = "tile_map";
    for (int i = 0; i <= MS_MAX_LEVELS; ++i) b += fmt(" %d", tm.base[i]);
    out.push_back(b);
    out.push_back(fmt("ftile_tab tiles %zu fnv %016" PRIx64, ftab_dwords / 2, fnv1a(ftab, 4 * ftab_dwords)));
    out.push_back(fmt("lvl0 off %" PRIu64 " pitch %d", lvl0_off, lvl0_pitch));
    for (int l = 1; l < G.levels; ++l)
        out.push_back(fmt("resize %d wide %d xt %zu %016" PRIx64 " yt %zu %016" PRIx64 " x8 %zu %016" PRIx64, l, (int)lr[l].wide, lr[l].xt_n, lr[l].xt_h, lr[l].yt_n, lr[l].yt_h, lr[l].x8_n, lr[l].x8_h));
    out.push_back(fmt("describe moment %zu %016" PRIx64 " pattern %zu %016" PRIx64, mt.size(), fnv1a(mt.data(), 4 * mt.size()), pf.size(), fnv1a(pf.data(), 4 * pf.size())));
    return out;
}
static std::string config_line(const ms_orb_config &c) {
    return fmt("case width %d height %d levels %d scale_factor %.9g max_kpts %d lk_track_level %d fast_threshold %d max_tracks %d max_batch %d min_distance %.9g",
               c.width, c.height, c.levels, c.scale_factor, c.max_kpts, c.lk_track_level, c.fast_threshold, c.max_tracks, c.max_batch, c.min_distance);
}
// ---- end of record -----------------------------------------------------------------------------------------------------------------------------

static bool parse_config(const std::string &line, ms_orb_config &c) {
    char sf[64], md[64];
    if (std::sscanf(line.c_str(), "case width %d height %d levels %d scale_factor %63s max_kpts %d lk_track_level %d fast_threshold %d max_tracks %d max_batch %d min_distance %63s",
                    &c.width, &c.height, &c.levels, sf, &c.max_kpts, &c.lk_track_level, &c.fast_threshold, &c.max_tracks, &c.max_batch, md) != 10) return false;
    c.scale_factor = std::strtof(sf, nullptr); c.min_distance = std::strtof(md, nullptr);
    return true;
}

// line against line, and where they differ, the first field that does
static bool same_line(const std::string &want, const std::string &got, const std::string &which) {
    if (want == got) { ++g_checks; return true; }
    std::istringstream a(want), b(got);
    std::string x, y, name;
    while (a >> x && b >> y) { if (x != y) break; name = x; }
    std::printf("FAIL %s\n  field after '%s': recorded %s, computed %s\n  recorded: %s\n  computed: %s\n", which.c_str(), name.c_str(), x.c_str(), y.c_str(), want.c_str(), got.c_str());
    return false;
}

struct Span { uint64_t lo, hi; };
static bool disjoint_inside(std::vector<Span> v, uint64_t limit) {
    std::sort(v.begin(), v.end(), [](const Span &a, const Span &b) { return a.lo < b.lo; });
    for (size_t i = 0; i < v.size(); ++i) {
        if (v[i].hi < v[i].lo || v[i].hi > limit) return false;
        if (i && v[i].lo < v[i - 1].hi) return false;
    }
    return true;
}

static bool check_invariants(const OrbGeom &R) {
    const PyrGeom &G = R.geom;
    std::vector<Span> planes, lists;
    int quota_sum = 0;
    for (int l = 0; l < G.levels; ++l) {
        const LevelGeom &L = G.L[l];
        CHECK(L.pitch >= L.w && L.pitch % 64 == 0, "level %d pitch %d", l, L.pitch);
        planes.push_back(Span{L.img_off, L.img_off + (uint64_t)L.pitch * L.h});
        planes.push_back(Span{L.blur_off, L.blur_off + (uint64_t)L.pitch * L.h});
        lists.push_back(Span{L.cand_off, L.cand_off + (uint64_t)L.cand_cap});
        CHECK(L.cand_off % 4 == 0 && L.cand_cap % 4 == 0, "level %d candidate list at %" PRIu64 " of %d entries", l, L.cand_off, L.cand_cap);
        CHECK(L.cand_cap >= ((L.w + 1) / 2) * ((L.h + 1) / 2), "level %d capacity %d", l, L.cand_cap);
        CHECK(L.det_base == quota_sum, "level %d det_base %d, quotas before it %d", l, L.det_base, quota_sum);
        quota_sum += L.quota;
        CHECK(R.blur_tiles.base[l] == L.btile_base && R.blur_tiles.base[l + 1] >= R.blur_tiles.base[l], "level %d tile base", l);
        const int tiles = L.btiles_x * ms_div_up(L.h, 4 * kBlurRows);
        CHECK(R.blur_tiles.base[l] + tiles == (l + 1 < G.levels ? G.L[l + 1].btile_base : G.btiles_total), "level %d has %d tiles", l, tiles);
        CHECK(L.btiles_x * kBlurSeg >= L.w, "level %d tiles across", l);
        for (int t = 0; t < tiles; ++t) {       // as k_blur finds a tile's row: one tile across is the tile id itself (2^32 / 1 does not fit btiles_inv)
            const int row = L.btiles_x == 1 ? t : (int)(((uint64_t)(uint32_t)t * L.btiles_inv) >> 32);
            if (row != t / L.btiles_x) CHECK(false, "level %d tile %d: mulhi row %d, division %d", l, t, row, t / L.btiles_x);
        }
        g_checks += tiles;
    }
    for (int l = G.levels; l <= MS_MAX_LEVELS; ++l) CHECK(R.blur_tiles.base[l] == G.btiles_total, "tile base %d", l);
    CHECK(disjoint_inside(planes, G.slab_stride), "planes overlap or pass slab_stride %" PRIu64, G.slab_stride);
    CHECK(disjoint_inside(lists, G.cand_stride), "candidate lists overlap or pass cand_stride %" PRIu64, G.cand_stride);
    CHECK(G.slab_stride % 256 == 0, "slab_stride %" PRIu64, G.slab_stride);
    CHECK(G.det_stride >= quota_sum && G.det_stride >= G.max_kpts && G.capacity == G.det_stride + G.max_tracks, "det_stride %d capacity %d", G.det_stride, G.capacity);
    CHECK((size_t)G.ftiles_total * 2 == R.ftile_tab.size(), "ftiles_total %d", G.ftiles_total);
    return true;
}

// What ms_orb_create allocated array by array before the block, in bytes: the counts of its hipMalloc calls.  B = max_batch, T = max(max_tracks, 1).
struct Separate { const char *name; size_t bytes; };
static std::vector<Separate> separate_allocations(const ms_orb_config &cfg, const OrbGeom &R, const OrbTables &C) {
    const PyrGeom &G = R.geom;
    const size_t B = (size_t)cfg.max_batch, T = (size_t)std::max(cfg.max_tracks, 1), cap = (size_t)G.capacity, det = (size_t)G.det_stride, ML = MS_MAX_LEVELS;
    std::vector<Separate> v = {
        {"geom", sizeof(PyrGeom)}, {"slab", B * G.slab_stride + 256}, {"cand", 4 * B * G.cand_stride}, {"cand_count", 4 * B * ML}, {"score_hist", 4 * B * ML * 256},
        {"last_count", 4 * B * ML}, {"det_count", 4 * B * ML}, {"trk_count", 4 * B}, {"det_x", 2 * B * det}, {"det_y", 2 * B * det}, {"det_score", B * det},
        {"trk_x", 2 * B * T}, {"trk_y", 2 * B * T}, {"trk_px", 4 * B * T}, {"trk_py", 4 * B * T}, {"trk_id", 4 * B * T}, {"track_xy", 4 * B * T * 2}, {"track_id", 4 * B * T},
        {"n_tracks", 4 * B}, {"x", 4 * B * cap}, {"y", 4 * B * cap}, {"angle", 4 * B * cap}, {"octave", 4 * B * cap}, {"track", 4 * B * cap}, {"count", 4 * B},
        {"slot_tab", 8 * B * cap}, {"desc", 4 * B * cap * 8},
        {"ftile_tab", 8 * (size_t)G.ftiles_total + 16}, {"moment_tab", 4 * (size_t)(64 * 4 + 32 * 4 + 64 + 64 * 2)}, {"pattern_f", 4 * 1024},
    };
    static char names[3 * MS_MAX_LEVELS][16];
    for (int l = 0; l < MS_MAX_LEVELS; ++l) {        // per level l >= 1: 4 int16 per column / row, padded to whole groups; 8 dwords per chunk of 8 columns where the level has the table
        const bool used = l >= 1 && l < G.levels;
        const size_t wpad = used ? (size_t)(G.L[l].w + 3) / 4 * 4 : 0, hpad = used ? (size_t)(G.L[l].h + kResizeRows - 1) / kResizeRows * kResizeRows : 0;
        const size_t chunks = used && !C.level[l].x8.empty() ? (size_t)(G.L[l].w + 7) / 8 : 0;
        std::snprintf(names[3 * l], 16, "xtab[%d]", l); std::snprintf(names[3 * l + 1], 16, "ytab[%d]", l); std::snprintf(names[3 * l + 2], 16, "xtab8[%d]", l);
        v.push_back({names[3 * l], 2 * 4 * wpad}); v.push_back({names[3 * l + 1], 2 * 4 * hpad}); v.push_back({names[3 * l + 2], 4 * 8 * chunks});
    }
    return v;
}

struct Placed { std::string name; size_t off, bytes; bool constant; };
static std::vector<Placed> placed_arrays(const OrbBlock &K) {
    std::vector<Placed> v;
    bool constant = true;
#define PLACED(T, name, n) v.push_back(Placed{#name, K.name.off, K.name.bytes(), constant});
#define PLACED_L(T, name, n) for (int l = 0; l < MS_MAX_LEVELS; ++l) v.push_back(Placed{fmt(#name "[%d]", l), K.name[l].off, K.name[l].bytes(), constant});
    ORB_BLOCK_CONSTANTS(PLACED, PLACED_L)
    constant = false;
    ORB_BLOCK_WORK(PLACED)
#undef PLACED
#undef PLACED_L
    return v;
}

static bool check_block(ms_orb_config cfg, const OrbGeom &R, const OrbTables &C, int max_batch) {
    cfg.max_batch = max_batch;
    const OrbBlock K = orb_block_layout(cfg, R, C);
    const std::vector<Placed> arrays = placed_arrays(K);
    const std::vector<Separate> before = separate_allocations(cfg, R, C);
    CHECK(arrays.size() == before.size(), "%zu arrays in the block, %zu separate allocations", arrays.size(), before.size());
    std::vector<Span> spans;
    bool in_constants = true;
    for (const Placed &a : arrays) {
        const Separate *s = nullptr;
        for (const Separate &b : before) if (a.name == b.name) s = &b;
        CHECK(s, "array %s has no entry in the table of separate allocations", a.name.c_str());
        CHECK(a.off % 256 == 0, "%s at %zu", a.name.c_str(), a.off);
        CHECK(a.bytes >= s->bytes, "%s: %zu bytes in the block, %zu as an allocation of its own", a.name.c_str(), a.bytes, s->bytes);
        if (s->bytes == 0) CHECK(a.bytes == 0, "%s: %zu bytes where the level has no table", a.name.c_str(), a.bytes);
        else CHECK(a.bytes >= 1, "%s is empty", a.name.c_str());
        if (a.bytes) spans.push_back(Span{a.off, a.off + a.bytes});
        CHECK(a.constant == (a.off + a.bytes <= K.const_end) && (a.constant || a.off >= K.const_end), "%s at %zu + %zu, constants end at %zu", a.name.c_str(), a.off, a.bytes, K.const_end);
        CHECK(in_constants || !a.constant, "%s: a constant behind a working array", a.name.c_str());
        in_constants = a.constant;
    }
    CHECK(disjoint_inside(spans, K.end), "arrays overlap or pass the block's %zu bytes", K.end);
    CHECK(K.const_end % 256 == 0 && K.const_end <= K.end, "constants end at %zu", K.const_end);
    // the slacks: 256 bytes behind the last frame's slab, 16 behind the last tile
    CHECK(K.slab.bytes() >= (size_t)max_batch * R.geom.slab_stride + 256, "slab of %zu bytes", K.slab.bytes());
    CHECK(K.ftile_tab.bytes() >= 4 * R.ftile_tab.size() + 16, "tile table of %zu bytes", K.ftile_tab.bytes());
    for (int l = 0; l < MS_MAX_LEVELS; ++l) {
        const bool used = l >= 1 && l < R.geom.levels;
        CHECK((K.xtab[l].count != 0) == used && (K.ytab[l].count != 0) == used, "level %d tables", l);
        CHECK((K.xtab8[l].count != 0) == (used && !C.level[l].x8.empty()), "level %d 8-pixel table", l);
    }
    // the staged constants, read back through the layout
    std::vector<uint8_t> stage;
    orb_stage_constants(K, R, C, stage);
    CHECK(stage.size() == K.const_end, "%zu staged bytes", stage.size());
    CHECK(std::memcmp(K.geom.at(stage.data()), &R.geom, sizeof(PyrGeom)) == 0, "staged geometry");
    CHECK(std::memcmp(K.ftile_tab.at(stage.data()), R.ftile_tab.data(), 4 * R.ftile_tab.size()) == 0, "staged tile table");
    CHECK(std::memcmp(K.moment_tab.at(stage.data()), C.moment.data(), 4 * C.moment.size()) == 0 && K.moment_tab.bytes() == 4 * C.moment.size(), "staged lane tables");
    CHECK(std::memcmp(K.pattern_f.at(stage.data()), C.pattern.data(), 4 * C.pattern.size()) == 0 && K.pattern_f.bytes() == 4 * C.pattern.size(), "staged pattern");
    for (int l = 1; l < R.geom.levels; ++l) {
        const OrbResizeTables &T = C.level[l];
        CHECK(K.xtab[l].count == T.xt.size() && std::memcmp(K.xtab[l].at(stage.data()), T.xt.data(), 2 * T.xt.size()) == 0, "staged xtab %d", l);
        CHECK(K.ytab[l].count == T.yt.size() && std::memcmp(K.ytab[l].at(stage.data()), T.yt.data(), 2 * T.yt.size()) == 0, "staged ytab %d", l);
        CHECK(K.xtab8[l].count == T.x8.size() && (T.x8.empty() || std::memcmp(K.xtab8[l].at(stage.data()), T.x8.data(), 4 * T.x8.size()) == 0), "staged xtab8 %d", l);
    }
    return true;
}

struct Seen { int accepted = 0, rejected = 0, spaced = 0, spaced_capped = 0, tracks = 0, no_tracks = 0, overflow = 0, wide = 0, no_x8 = 0; };

static bool check_case(const ms_orb_config &cfg, const std::vector<std::string> &want, Seen &seen) {
    const std::string which = config_line(cfg);
    OrbGeom R;
    char why[256] = "";
    const int rc = orb_geometry(cfg, R, why, sizeof(why));
    std::vector<std::string> got = {fmt("status %d", rc)};
    OrbTables C;
    if (rc != MS_OK) got.push_back(std::string("message ") + why);
    else {
        orb_tables(R.geom, C);
        LevelRecord lr[MS_MAX_LEVELS] = {};
        for (int l = 1; l < cfg.levels; ++l) {
            const OrbResizeTables &T = C.level[l];
            lr[l] = LevelRecord{T.wide, T.xt.size(), T.yt.size(), T.x8.size(), fnv1a(T.xt.data(), 2 * T.xt.size()), fnv1a(T.yt.data(), 2 * T.yt.size()), fnv1a(T.x8.data(), 4 * T.x8.size())};
        }
        const std::vector<std::string> rec = record_lines(R.geom, R.tile_levels, R.blur_tiles, R.ftile_tab.data(), R.ftile_tab.size(), R.lvl0_off, R.lvl0_pitch, lr, C.moment, C.pattern);
        got.insert(got.end(), rec.begin(), rec.end());
    }
    CHECK(want.size() == got.size(), "%s: %zu recorded lines, %zu computed", which.c_str(), want.size(), got.size());
    for (size_t i = 0; i < want.size(); ++i) if (!same_line(want[i], got[i], which)) return false;
    if (rc != MS_OK) { ++seen.rejected; return true; }
    ++seen.accepted;
    if (!check_invariants(R)) { std::printf("  in %s\n", which.c_str()); return false; }
    for (int B : {1, 3}) if (!check_block(cfg, R, C, B)) { std::printf("  in %s at max_batch %d\n", which.c_str(), B); return false; }
    for (int l = 0; l < cfg.levels; ++l) {
        if (cfg.min_distance > 0.f && R.tile_levels.L[l].sel_k > R.geom.L[l].quota) ++seen.spaced;
        if (cfg.min_distance > 0.f && R.tile_levels.L[l].sel_k == kMaxQuota && 4 * R.geom.L[l].quota > kMaxQuota) ++seen.spaced_capped;
        if (l && C.level[l].wide) ++seen.wide;
        if (l && C.level[l].x8.empty()) ++seen.no_x8;
    }
    seen.tracks += cfg.max_tracks > 0; seen.no_tracks += cfg.max_tracks == 0;
    seen.overflow += R.geom.det_stride > cfg.max_kpts;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) { std::printf("usage: orb_geom_check tests/golden/orb_geom_cases.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::printf("FAIL cannot read %s\n", argv[1]); return 1; }
    std::string line;
    ms_orb_config cfg{};
    std::vector<std::string> lines;
    bool open = false;
    Seen seen;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        if (line.compare(0, 5, "case ") == 0) {
            if (open || !parse_config(line, cfg)) { std::printf("FAIL bad record near: %s\n", line.c_str()); return 1; }
            if (config_line(cfg) != line) { std::printf("FAIL the configuration does not survive a round trip: %s\n", line.c_str()); return 1; }
            open = true; lines.clear();
        } else if (line == "end") {
            if (!open || !check_case(cfg, lines, seen)) return 1;
            open = false;
        } else lines.push_back(line);
    }
    if (open) { std::printf("FAIL the record ends inside a case\n"); return 1; }
    // the record must hold what it is there for
    if (seen.accepted < 9 || seen.rejected != 9 || !seen.spaced || !seen.spaced_capped || !seen.tracks || !seen.no_tracks || !seen.overflow || !seen.wide || !seen.no_x8) {
        std::printf("FAIL the record lacks cases: %d accepted, %d rejected, spaced levels %d (capped %d), with tracks %d, without %d, quota overflow %d, wide levels %d, levels without an 8-pixel table %d\n",
                    seen.accepted, seen.rejected, seen.spaced, seen.spaced_capped, seen.tracks, seen.no_tracks, seen.overflow, seen.wide, seen.no_x8);
        return 1;
    }
    std::printf("orb geom ok: %d accepted and %d rejected configurations, %lld checks\n", seen.accepted, seen.rejected, g_checks);
    return 0;
}
