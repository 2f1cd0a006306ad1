// The launch plan of k_resize8 (orb.hip): which levels the 8-pixel kernel takes, its compact column table, which workgroup takes which tile, and what a
// lane does with its 16-byte window.  Plain C++, host- and device-callable: the library builds tables and launches from it, the kernel decodes its
// lane and extracts its tap bytes with it, and tests/resize_plan_check.cpp checks all of it on the CPU.
//
// A lane owns a CHUNK of 8 consecutive destination pixels and kRows destination rows.  Per source row it loads 16 bytes from the dword-aligned
// offset base = sx0 & ~3 (sx0 = the first column's left tap) and funnels them into three dwords lo / mid / hi = source bytes sx0 .. sx0 + 11:
// columns 0 .. 3 pick their tap pair (bytes k, k + 1) from (lo, mid) with k = sx - sx0, columns 4 .. 7 from (mid, hi) with k = sx - sx0 - 4,
// 0 <= k <= 6 in both halves.  A level is ELIGIBLE when every chunk keeps that rule and every group of kRows destination rows reads 6 or 7
// consecutive source rows (the shared-row test of k_resize); every other level stays on the 4-pixel kernel.
//
// The grid comes in two mappings (below): tile by tile across the device, or every frame through the L2 of one XCD.
#pragma once
#include <cstdint>
#include <vector>
#include "resize_vpass.h"

#if defined(__HIPCC__)
#define RPLAN_HD __host__ __device__ __forceinline__
#else
#define RPLAN_HD inline
#endif

namespace resize_plan {

constexpr int kPx = 8;                 // destination pixels per lane
constexpr int kRows = 5;               // destination rows per lane (kResizeRows)
constexpr int kWindow = 16;            // bytes a lane loads per source row
constexpr int kMaxK = 6;               // a column's selector takes bytes k, k + 1 of an 8-byte pair of funnel results
constexpr int kMaxSrcWidth = 65536;    // sx0 travels in 16 spare bits of a chunk's entries

// ---- column table: one dword per destination column, 8 per chunk (32 bytes per lane) --------------------------------------------------------
// bits 4 .. 15 and 20 .. 31: the taps as the horizontal pass takes them (resize_vpass::preshift_taps: a0 << 4 | a1 << 20, each a <= 2048);
// bits 0 .. 2: k;  bits 16 .. 19 of a chunk's entries 0 .. 3: the nibbles of sx0, low first.
constexpr uint32_t kTapMask = 0xFFF0FFF0u;
RPLAN_HD uint32_t entry(int a0, int a1, int k, int nibble) {
    return resize_vpass::preshift_taps((uint32_t)a0 | ((uint32_t)a1 << 16)) | (uint32_t)k | ((uint32_t)nibble << 16);
}
RPLAN_HD uint32_t entry_taps(uint32_t e) { return e & kTapMask; }
RPLAN_HD uint32_t entry_sel(uint32_t e) { return 0x0C010C00u + (e & 7u) * 0x00010001u; }     // v_perm_b32: bytes k, k + 1 into the two 16-bit halves
RPLAN_HD uint32_t chunk_sx0(uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3) {
    return ((e0 >> 16) & 15u) | (((e1 >> 16) & 15u) << 4) | (((e2 >> 16) & 15u) << 8) | (((e3 >> 16) & 15u) << 12);
}

// The table of a level from the column taps (sx[d], coef[2 d], coef[2 d + 1]: msgeo::resize_tables).  False when a chunk breaks the window
// rule (tab is then left empty).  The last chunk is padded: columns dw .. (dw rounded up to 4) - 1 repeat column dw - 1, as the 4-pixel kernel's
// table does, and the columns behind them have both taps zero (k = 0), which makes their pixels 0: the pitch padding holds after this kernel
// exactly the bytes it holds after the 4-pixel one.
inline bool build_columns(const int16_t *sx, const int16_t *coef, int sw, int dw, std::vector<uint32_t> &tab) {
    tab.clear();
    if (dw < 1 || sw < kWindow || sw > kMaxSrcWidth) return false;       // (16 bytes must fit a source row: the edge wave fetches from last - 12)
    const int nchunks = (dw + kPx - 1) / kPx, dw4 = (dw + 3) / 4 * 4;
    std::vector<uint32_t> t((size_t)nchunks * kPx);
    for (int c = 0; c < nchunks; ++c) {
        const int sx0 = sx[c * kPx];
        if (sx0 < 0 || sx0 > sw - 1) return false;
        for (int j = 0; j < kPx; ++j) {
            const int d = c * kPx + j, nibble = j < 4 ? (sx0 >> (4 * j)) & 15 : 0;
            if (d >= dw4) { t[d] = entry(0, 0, 0, nibble); continue; }
            const int e = d < dw ? d : dw - 1, k = sx[e] - sx0 - (j < 4 ? 0 : 4);
            if (k < 0 || k > kMaxK || coef[2 * e] < 0 || coef[2 * e] > 2048 || coef[2 * e + 1] < 0 || coef[2 * e + 1] > 2048) return false;
            t[d] = entry(coef[2 * e], coef[2 * e + 1], k, nibble);
        }
    }
    tab.swap(t);
    return true;
}

// ---- rows: the shared-row test of k_resize on one group ---------------------------------------------------------------------------------------
// yt: the row table [rows padded to whole groups][4] = sy0, sy1 (clamped), b0, b1.  The group's rows that exist read source rows s0 + d and s0 + d + 1
// (clamped at sh - 1) with d = r or r + 1.
inline bool group_shared(const int16_t *yt, int dy0, int dh, int sh) {
    const int s0 = yt[4 * dy0];
    for (int r = 0; r < kRows; ++r) {
        if (dy0 + r >= dh) continue;
        const int y0 = yt[4 * (dy0 + r)], y1 = yt[4 * (dy0 + r) + 1];
        if ((unsigned)(y0 - s0 - r) > 1u || y1 != (y0 + 1 < sh - 1 ? y0 + 1 : sh - 1)) return false;
    }
    return true;
}
inline bool rows_shared(const int16_t *yt, int dh, int sh) {
    for (int dy0 = 0; dy0 < dh; dy0 += kRows) if (!group_shared(yt, dy0, dh, sh)) return false;
    return true;
}

// ---- a lane's window --------------------------------------------------------------------------------------------------------------------------
// last = the row's last dword offset, (sw - 1) & ~3.  No byte at or beyond last + 4 is read: a lane whose 16 bytes would pass it (an EDGE lane;
// the whole wave then takes the edge form) fetches from last - 12 and moves whole dwords down by shift = 0 / 4 / 8 / 12 bytes, which gives
// d_k = row[min(base + 4 k, last)], the true bytes wherever a tap with a non-zero weight looks.
struct Fetch { int32_t from, shift; };
RPLAN_HD bool lane_is_edge(int base, int last) { return base + (kWindow - 4) > last; }
RPLAN_HD Fetch fetch(int base, int last, bool edge) {
    const int from = edge ? (base < last - (kWindow - 4) ? base : last - (kWindow - 4)) : base;
    return Fetch{from, base - from};
}
struct Window { uint32_t d0, d1, d2, d3; };      // (named dwords: selecting among the elements of an array by `shift` would put the array in memory)
RPLAN_HD Window shift_down(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, int shift) {      // (values, not a reference: selects between loads become an indexed load)
    return Window{shift == 0 ? d0 : shift == 4 ? d1 : shift == 8 ? d2 : d3, shift == 0 ? d1 : shift == 4 ? d2 : d3, shift == 0 ? d2 : d3, d3};
}
// v_alignbyte_b32: bytes s & 3 .. (s & 3) + 3 of {hi, lo}
RPLAN_HD uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, s);
#else
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (s & 3u)));
#endif
}
struct Funnels { uint32_t lo, mid, hi; };       // source bytes sx0 .. + 3, + 4 .. + 7, + 8 .. + 11
RPLAN_HD Funnels funnels(const Window &w, uint32_t sx0) { return Funnels{alignbyte(w.d1, w.d0, sx0), alignbyte(w.d2, w.d1, sx0), alignbyte(w.d3, w.d2, sx0)}; }
// column j's tap bytes as a v_dot2_u32_u16 operand: row[sx] in the low half, row[sx + 1] in the high half
RPLAN_HD uint32_t tap_pair(const Funnels &f, int j, uint32_t sel) { return j < 4 ? resize_vpass::perm_b32(f.mid, f.lo, sel) : resize_vpass::perm_b32(f.hi, f.mid, sel); }

// ---- the grid: which workgroup takes which tile of which frame ------------------------------------------------------------------------------
// A workgroup is four waves = four row groups of the same 64 chunks (a TILE: tx of gx across, ty of gy down).  Two mappings:
//   kMapPlain    grid (gx, gy, nf): block (tx, ty, frame).  Consecutive workgroups are dealt round robin to the device's eight XCDs, each with an L2
//                of its own, so the 128-byte lines on a tile's left and right border and the source row two tiles share are fetched by two L2s.
//   kMapByFrame  grid (8, gx * gy, ceil(nf / 8)): block x is the XCD label (the linear workgroup index modulo 8), and the workgroups of label x
//                take the frames 8 z + x, each walking its frame's tiles in order: a frame goes through ONE L2.  Blocks of frames >= nf leave at once.
// The automatic choice is by frame from kByFrameMinFrames frames on (below that a frame's tiles would crowd onto a few XCDs while the others idle).
// Nothing depends on where a block really runs: a dispatcher that deals otherwise only loses the reuse.
constexpr int kXcds = 8;
constexpr int kMapAuto = 0, kMapPlain = 1, kMapByFrame = 2;
constexpr int kByFrameMinFrames = 32;
constexpr uint32_t kGridYLimit = 65535;

struct Launch { int32_t nchunks, nf, by_frame; uint32_t gx, gy, inv_gx, grid_x, grid_y, grid_z; };
struct Tile { int32_t tx, ty, frame; };

constexpr int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// map: kMapAuto, kMapPlain or kMapByFrame (which falls back to plain where gx * gy is beyond the grid's y limit)
inline Launch launch(int dw, int dh, int nf, int map) {
    Launch L{};
    L.nchunks = (dw + kPx - 1) / kPx; L.nf = nf;
    L.gx = (uint32_t)ceil_div(L.nchunks, 64); L.gy = (uint32_t)ceil_div(dh, 4 * kRows);
    L.inv_gx = 0xFFFFFFFFu / L.gx;
    L.by_frame = (map == kMapByFrame || (map == kMapAuto && nf >= kByFrameMinFrames)) && (uint64_t)L.gx * L.gy <= kGridYLimit;
    if (L.by_frame) { L.grid_x = kXcds; L.grid_y = L.gx * L.gy; L.grid_z = (uint32_t)ceil_div(nf, kXcds); }
    else { L.grid_x = L.gx; L.grid_y = L.gy; L.grid_z = (uint32_t)nf; }
    return L;
}
// The launch-size gate (like kFastPruneMinBlocks): a launch that does not fill the device once -- 256 CUs x 5 workgroups of the kernel's 83 VGPRs --
// is bound by latency, not by bytes, and the 4-pixel kernel's more and shorter waves finish it sooner (one 720p frame: the seven launches take
// 26.8 us with 4 pixels per lane, 29.5 with 8; 256 frames: 283 against 265).  Such launches stay on the 4-pixel kernel unless px = 8 is forced.
constexpr int64_t kMinBlocks = 256 * 5;
inline bool fills_device(const Launch &L) { return (int64_t)L.gx * L.gy * L.nf >= kMinBlocks; }

// Block index -> (tile, frame); the block works iff frame < nf.  By frame, q = mulhi(t, inv) is floor(t / gx) or one less for every t below 2^31
// (describe_strips.h has the argument), so one correction makes the division exact.
RPLAN_HD Tile decode(const Launch &L, uint32_t bx, uint32_t by, uint32_t bz) {
    if (!L.by_frame) return Tile{(int32_t)bx, (int32_t)by, (int32_t)bz};
    uint32_t q = (uint32_t)(((uint64_t)by * L.inv_gx) >> 32), r = by - q * L.gx;
    if (r >= L.gx) { ++q; r -= L.gx; }
    return Tile{(int32_t)r, (int32_t)q, (int32_t)(bz * kXcds + bx)};
}

}   // namespace resize_plan
