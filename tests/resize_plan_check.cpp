// k_resize8's plan (slam-module_amd/csrc/resize_plan.h) on the CPU, with the library's own table formula restated (geometry.cpp):
//   - the eligibility predicate (build_columns, rows_shared) against a brute-force walk of the tables, for source sizes 40 .. 1400 and ratios
//     1.0 .. 2.0; ratio 1.5 is never eligible, and every level of 1280x720, 640x480, 752x480 and 333x119 at 1.2 and of 200x150 at 1.1 is;
//   - a model of a lane's window extraction -- 16 bytes from the aligned offset, the edge wave's shift, three funnels, the selectors -- delivers
//     exactly row[sx] and row[sx + 1] for all 8 columns of every chunk, wave by wave of 64 chunks, on rows allocated to end
//     at last + 4 so that a load beyond it is an out-of-bounds read under AddressSanitizer as well as a failed check; the pixel the vertical
//     pass makes of those bytes equals the reference form;
//   - the table's padding columns keep the window rule and hold the taps build_columns promises;
//   - both grid mappings cover every (frame, row group, chunk) exactly once, for 1 .. 33 frames; by frame, a frame's tiles all carry one XCD label;
//   - decode's multiply-high division equals the division, and a level beyond the grid's y limit stays on the plain mapping.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "resize_plan.h"

namespace rp = resize_plan;

static long long g_checks = 0;
#define CHECK(c, ...) do { ++g_checks; if (!(c)) { std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); return false; } } while (0)

// msgeo::resize_tables and the row table of ms_orb_create
static int16_t coef_q11(float c) { long r = std::lrintf(c * 2048.f); return (int16_t)(r > 32767 ? 32767 : r < -32768 ? -32768 : r); }
static void tables(int src_n, int dst_n, bool is_x, std::vector<int16_t> &ofs, std::vector<int16_t> &coef) {
    ofs.resize(dst_n); coef.resize(2 * (size_t)dst_n);
    const double scale = 1.0 / ((double)dst_n / src_n);
    for (int d = 0; d < dst_n; ++d) {
        float frac = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(frac);
        frac -= (float)s;
        if (is_x) { if (s < 0) { s = 0; frac = 0.f; } if (s >= src_n - 1) { s = src_n - 1; frac = 0.f; } }
        ofs[d] = (int16_t)s; coef[2 * d] = coef_q11(1.f - frac); coef[2 * d + 1] = coef_q11(frac);
    }
}
static std::vector<int16_t> row_table(int sh, int dh) {
    std::vector<int16_t> yo, yc;
    tables(sh, dh, false, yo, yc);
    const int hpad = (dh + rp::kRows - 1) / rp::kRows * rp::kRows;
    std::vector<int16_t> yt(4 * (size_t)hpad);
    for (int d = 0; d < hpad; ++d) {
        const int e = d < dh ? d : dh - 1;
        yt[4 * d] = (int16_t)std::min(std::max((int)yo[e], 0), sh - 1); yt[4 * d + 1] = (int16_t)std::min(std::max((int)yo[e] + 1, 0), sh - 1);
        yt[4 * d + 2] = yc[2 * e]; yt[4 * d + 3] = yc[2 * e + 1];
    }
    return yt;
}
static void level_sizes(int levels, float f, int w0, int h0, std::vector<int> &w, std::vector<int> &h) {
    float s = 1.f;
    w.assign(1, w0); h.assign(1, h0);
    for (int l = 1; l < levels; ++l) { s = f * s; w.push_back((int)std::round(w0 * 1.0 / (double)s)); h.push_back((int)std::round(h0 * 1.0 / (double)s)); }
}

// brute force: which source bytes can each half of a chunk reach, and does every tap of every real column lie among them?
static bool columns_brute(const std::vector<int16_t> &sx, int sw, int dw) {
    if (sw < 16 || sw > 65536) return false;
    for (int c = 0; c * 8 < dw; ++c)
        for (int j = 0; j < 8 && c * 8 + j < dw; ++j) {
            const int first = sx[c * 8] + (j < 4 ? 0 : 4);                // the half's 8 bytes: two funnel results
            for (int tap = 0; tap < 2; ++tap) { const int b = sx[c * 8 + j] + tap; if (b < first || b >= first + 8) return false; }
        }
    return true;
}
static bool rows_brute(int sh, int dh) {
    std::vector<int16_t> yo, yc;
    tables(sh, dh, false, yo, yc);
    for (int g = 0; g < dh; g += 5) {
        const int s0 = std::min(std::max((int)yo[g], 0), sh - 1);
        for (int r = 0; r < 5 && g + r < dh; ++r) {
            const int y0 = std::min(std::max((int)yo[g + r], 0), sh - 1), y1 = std::min(std::max((int)yo[g + r] + 1, 0), sh - 1), d = y0 - s0;
            if ((d != r && d != r + 1) || y1 != std::min(y0 + 1, sh - 1)) return false;
        }
    }
    return true;
}

static uint32_t dot2(uint32_t x, uint32_t a) { return (x & 0xFFFFu) * (a & 0xFFFFu) + (x >> 16) * (a >> 16); }      // v_dot2_u32_u16

// the lanes of every wave of `seg` chunks over one source row
static bool check_windows(int sw, int dw, const std::vector<int16_t> &sx, const std::vector<int16_t> &coef, const std::vector<uint32_t> &tab, uint32_t &rng) {
    const int last = (sw - 1) & ~3, nchunks = (dw + 7) / 8, dw4 = (dw + 3) / 4 * 4;
    CHECK((int)tab.size() == nchunks * 8, "%d entries for %d chunks", (int)tab.size(), nchunks);
    std::vector<uint8_t> row0((size_t)last + 4), row1((size_t)last + 4);     // exactly the bytes a kernel may read
    for (auto *row : {&row0, &row1}) for (auto &b : *row) { rng = rng * 1664525u + 1013904223u; b = (uint8_t)(rng >> 24); }
    for (int c = 0; c < nchunks; ++c) {
        const uint32_t *e = &tab[(size_t)c * 8];
        CHECK((int)rp::chunk_sx0(e[0], e[1], e[2], e[3]) == sx[c * 8], "sw %d dw %d chunk %d: sx0 %u", sw, dw, c, rp::chunk_sx0(e[0], e[1], e[2], e[3]));
        for (int j = 0; j < 8; ++j) {
            const int d = c * 8 + j, k = (int)(e[j] & 7u), src = d < dw ? d : dw - 1;
            CHECK(k <= rp::kMaxK, "k %d", k);
            if (d < dw4) {
                CHECK(rp::entry_taps(e[j]) == resize_vpass::preshift_taps((uint32_t)coef[2 * src] | ((uint32_t)coef[2 * src + 1] << 16)), "sw %d dw %d column %d taps", sw, dw, d);
                CHECK(k == sx[src] - sx[c * 8] - (j < 4 ? 0 : 4), "sw %d dw %d column %d k %d", sw, dw, d, k);
            } else CHECK(rp::entry_taps(e[j]) == 0 && k == 0, "sw %d dw %d padding column %d", sw, dw, d);
        }
    }
    const int seg = 64;                                  // lanes of a wave: the edge form is the wave's choice
    for (int c0 = 0; c0 < nchunks; c0 += seg) {
        bool edge = false;
        for (int c = c0; c < std::min(c0 + seg, nchunks); ++c) edge = edge || rp::lane_is_edge(sx[c * 8] & ~3, last);
        for (int c = c0; c < std::min(c0 + seg, nchunks); ++c) {
            const uint32_t *e = &tab[(size_t)c * 8];
            const uint32_t sx0 = rp::chunk_sx0(e[0], e[1], e[2], e[3]);
            const int base = (int)(sx0 & ~3u);
            const rp::Fetch ft = rp::fetch(base, last, edge);
            CHECK(ft.from >= 0 && ft.from % 4 == 0 && ft.from + rp::kWindow <= last + 4, "sw %d dw %d chunk %d: load at %d, last %d", sw, dw, c, ft.from, last);
            CHECK(ft.shift >= 0 && ft.shift <= 12 && ft.shift % 4 == 0 && (edge || ft.shift == 0), "shift %d", ft.shift);
            uint32_t F[2][8];
            for (int t = 0; t < 2; ++t) {
                const std::vector<uint8_t> &row = t ? row1 : row0;
                rp::Window W;
                std::memcpy(&W, row.data() + ft.from, 16);
                if (edge) W = rp::shift_down(W.d0, W.d1, W.d2, W.d3, ft.shift);
                const rp::Funnels fn = rp::funnels(W, sx0);
                for (int j = 0; j < 8; ++j) {
                    const uint32_t pair = rp::tap_pair(fn, j, rp::entry_sel(e[j]));
                    F[t][j] = resize_vpass::f8(dot2(pair, rp::entry_taps(e[j])));
                    const int d = c * 8 + j;
                    if (d >= dw) continue;
                    CHECK((pair & 0xFF00FF00u) == 0 && (pair & 255u) == row[sx[d]], "sw %d dw %d seg %d column %d: left tap", sw, dw, seg, d);
                    if (sx[d] + 1 < last + 4) CHECK((pair >> 16) == row[sx[d] + 1], "sw %d dw %d seg %d column %d: right tap", sw, dw, seg, d);
                    else CHECK(coef[2 * d + 1] == 0, "sw %d dw %d column %d: a tap beyond the row has weight %d", sw, dw, d, coef[2 * d + 1]);
                    if (sx[d] + 1 > sw - 1) CHECK(coef[2 * d + 1] == 0, "sw %d dw %d column %d: a tap beyond the row has weight %d", sw, dw, d, coef[2 * d + 1]);
                }
            }
            // one destination row with row taps (1300, 748): the kernel's arithmetic on those bytes against the form it replaces
            const int b0 = 1300, b1 = 748;
            uint32_t v[8];
            for (int j = 0; j < 8; ++j) v[j] = resize_vpass::vsum(resize_vpass::row_tap(b0), F[0][j], resize_vpass::row_tap(b1), F[1][j]);
            const uint32_t out[2] = {resize_vpass::pack4(v[0], v[1], v[2], v[3]), resize_vpass::pack4(v[4], v[5], v[6], v[7])};
            for (int j = 0; j < 8; ++j) {
                const int d = c * 8 + j, got = (int)((out[j >> 2] >> (8 * (j & 3))) & 255u);
                if (d >= dw4) { CHECK(got == 0, "sw %d dw %d padding column %d holds %d", sw, dw, d, got); continue; }
                const int s = d < dw ? d : dw - 1, a0 = coef[2 * s], a1 = coef[2 * s + 1], x1 = a1 ? sx[s] + 1 : sx[s];
                const int r0 = row0[sx[s]] * a0 + row0[x1] * a1, r1 = row1[sx[s]] * a0 + row1[x1] * a1;
                CHECK(got == ((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2), "sw %d dw %d column %d pixel %d", sw, dw, d, got);
            }
        }
    }
    return true;
}

static bool check_level(int sw, int dw, int sh, int dh, int want, uint32_t &rng, long long &eligible) {      // want: 1 eligible, 0 not, -1 either
    std::vector<int16_t> sx, coef;
    tables(sw, dw, true, sx, coef);
    std::vector<uint32_t> tab;
    const bool cols = rp::build_columns(sx.data(), coef.data(), sw, dw, tab);
    CHECK(cols == columns_brute(sx, sw, dw), "columns %d -> %d: predicate %d", sw, dw, (int)cols);
    CHECK(cols || tab.empty(), "a refused level left a table");
    const std::vector<int16_t> yt = row_table(sh, dh);
    const bool rows = rp::rows_shared(yt.data(), dh, sh);
    CHECK(rows == rows_brute(sh, dh), "rows %d -> %d: predicate %d", sh, dh, (int)rows);
    if (want >= 0) CHECK((cols && rows) == (want == 1), "%dx%d -> %dx%d: columns %d rows %d", sw, sh, dw, dh, (int)cols, (int)rows);
    if (cols) { ++eligible; if (!check_windows(sw, dw, sx, coef, tab, rng)) return false; }
    return true;
}

static bool check_cover(int nchunks, int dh, int nf, int map) {
    const rp::Launch L = rp::launch(nchunks * 8 - 3, dh, nf, map);
    CHECK(L.nchunks == nchunks && L.nf == nf && L.gx == (uint32_t)((nchunks + 63) / 64) && L.gy == (uint32_t)((dh + 19) / 20), "launch record");
    const bool by_frame = map == rp::kMapByFrame || (map == rp::kMapAuto && nf >= rp::kByFrameMinFrames);
    CHECK((L.by_frame != 0) == by_frame, "%d frames map %d: by_frame %d", nf, map, L.by_frame);
    if (by_frame) CHECK(L.grid_x == 8 && L.grid_y == L.gx * L.gy && L.grid_z == (uint32_t)((nf + 7) / 8), "grid %u %u %u", L.grid_x, L.grid_y, L.grid_z);
    else CHECK(L.grid_x == L.gx && L.grid_y == L.gy && L.grid_z == (uint32_t)nf, "grid %u %u %u", L.grid_x, L.grid_y, L.grid_z);
    CHECK(L.grid_y <= rp::kGridYLimit && L.grid_z <= 65535u, "grid limits");
    const int groups = (dh + rp::kRows - 1) / rp::kRows;
    std::vector<int> seen((size_t)nf * groups * nchunks, 0);
    for (uint32_t bz = 0; bz < L.grid_z; ++bz) for (uint32_t by = 0; by < L.grid_y; ++by) for (uint32_t bx = 0; bx < L.grid_x; ++bx) {
        const rp::Tile tl = rp::decode(L, bx, by, bz);
        CHECK(tl.tx >= 0 && tl.tx < (int)L.gx && tl.ty >= 0 && tl.ty < (int)L.gy && tl.frame >= 0, "block (%u, %u, %u): tile (%d, %d) frame %d", bx, by, bz, tl.tx, tl.ty, tl.frame);
        if (by_frame) CHECK(tl.frame % 8 == (int)bx, "frame %d on XCD label %u", tl.frame, bx);       // a frame's tiles all carry one label
        for (int wv = 0; wv < 4; ++wv) for (int lane = 0; lane < 64; ++lane) {
            const int dy0 = (tl.ty * 4 + wv) * rp::kRows, chunk = tl.tx * 64 + lane;
            if (tl.frame >= L.nf || dy0 >= dh || chunk >= L.nchunks) continue;
            ++seen[((size_t)tl.frame * groups + dy0 / rp::kRows) * nchunks + chunk];
        }
    }
    CHECK(rp::fills_device(L) == ((int64_t)L.gx * L.gy * nf >= 1280), "the launch-size gate at %u x %u x %d blocks", L.gx, L.gy, nf);
    for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "%d chunks dh %d nf %d map %d: item %zu visited %d times", nchunks, dh, nf, map, i, seen[i]);
    return true;
}

// the multiply-high division of decode against the division, for every divisor a grid can have and block indices up to the grid's limit
static bool check_division() {
    for (uint32_t gx = 1; gx <= 1100; ++gx) {
        rp::Launch L{};
        L.by_frame = 1; L.gx = gx; L.gy = 1; L.inv_gx = 0xFFFFFFFFu / gx;
        for (uint32_t t = 0; t <= rp::kGridYLimit; t += (t < 3000 ? 1 : 61)) {
            const rp::Tile tl = rp::decode(L, 3, t, 5);
            CHECK((uint32_t)tl.tx == t % gx && (uint32_t)tl.ty == t / gx && tl.frame == 43, "gx %u t %u: (%d, %d) frame %d", gx, t, tl.tx, tl.ty, tl.frame);
        }
    }
    // the gate: one 720p frame and a 64-frame piece of the smallest 720p level stay on the 4-pixel kernel, every level of 256 frames of 720p or VGA does not
    CHECK(!rp::fills_device(rp::launch(1067, 600, 1, 0)) && !rp::fills_device(rp::launch(357, 201, 64, 0)), "a small launch passes the gate");
    CHECK(rp::fills_device(rp::launch(357, 201, 256, 0)) && rp::fills_device(rp::launch(179, 134, 256, 0)) && rp::fills_device(rp::launch(1067, 600, 64, 0)), "a large launch fails the gate");
    // a level too large for the y limit of the grid stays on the plain mapping
    const rp::Launch big = rp::launch(8 * 64 * 300, 20 * 300, 64, rp::kMapByFrame);
    CHECK(!big.by_frame && big.grid_x == 300 && big.grid_y == 300 && big.grid_z == 64, "a grid beyond the y limit");
    return true;
}

int main() {
    uint32_t rng = 12345u;
    long long eligible = 0, levels = 0;
    const float ratios[] = {1.0f, 1.05f, 1.1f, 1.15f, 1.2f, 1.25f, 1.3f, 1.4f, 1.5f, 1.6f, 1.8f, 2.0f};
    for (float f : ratios)
        for (int s = 40; s <= 1400; ++s) {
            const int d = (int)std::round(s * 1.0 / (double)f);
            // the same pair of sizes on both axes: columns s -> d and rows s -> d
            if (!check_level(s, d, s, d, f == 1.5f ? 0 : -1, rng, eligible)) return 1;
            ++levels;
        }
    const struct { int w, h; float f; } named[] = {{1280, 720, 1.2f}, {640, 480, 1.2f}, {752, 480, 1.2f}, {333, 119, 1.2f}, {200, 150, 1.1f}};
    for (const auto &n : named) {
        std::vector<int> w, h;
        level_sizes(8, n.f, n.w, n.h, w, h);
        for (int l = 1; l < 8 && w[l] >= 40 && h[l] >= 40; ++l) { if (!check_level(w[l - 1], w[l], h[l - 1], h[l], 1, rng, eligible)) return 1; ++levels; }
    }
    {   // 200x150 at 1.5 (the GPU test's ineligible case)
        std::vector<int> w, h;
        level_sizes(4, 1.5f, 200, 150, w, h);
        for (int l = 1; l < 4; ++l) { if (!check_level(w[l - 1], w[l], h[l - 1], h[l], 0, rng, eligible)) return 1; ++levels; }
    }
    for (int w = 41; w <= 120; ++w) {      // every w mod 8 as the last chunk, narrow levels
        if (!check_level((int)std::round(w * 1.2), w, 60, 50, -1, rng, eligible)) return 1;
        ++levels;
    }
    const int chunk_counts[] = {1, 7, 63, 64, 65, 67, 129, 134};
    const int heights[] = {3, 5, 19, 20, 21, 99};
    for (int nc : chunk_counts) for (int dh : heights) for (int nf : {1, 2, 3, 5, 7, 8, 9, 31, 32, 33}) for (int map : {rp::kMapAuto, rp::kMapPlain, rp::kMapByFrame})
        if (!check_cover(nc, dh, nf, map)) return 1;
    if (!check_division()) return 1;
    std::printf("resize plan ok: %lld levels (%lld with eligible columns), %lld checks\n", levels, eligible, g_checks);
    return 0;
}
