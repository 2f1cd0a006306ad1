// CPU check of k_describe's lane maps (slam-module_amd/csrc/describe_lanes.h), for all 64 lanes:
//   window fetch   the packed (row, byte) table and the "three pieces on = 16 rows down" rule cover each of the 45 x 12 window dwords exactly
//                  once and every piece lands on the LDS dword it is (lane + 64 t = 12 row + byte / 4); the 36 spare lanes of the ninth piece read
//                  inside the window and land behind it, inside the wave's slab
//   orientation    the four pieces of a lane read exactly window rows 7 .. 37, dwords 2 .. 9, each once, and become each of the 31 x 8 + 8
//                  patch dwords once (the last 8, the zero row, without a source)
//   moments        the masked dwords with lane_moments' dword arithmetic give, summed over the wave, the m10 = sum u I and m01 = sum v I of
//                  orb_extractor's loop (v = -15 .. 15, |u| <= u_max[|v|]) on random, all-255 and one-hot windows; the weights are checked one
//                  pixel at a time, so every patch byte is counted once with its own (u, v)
//   blur taps      the selected table index is the entry the lane used to read and then select, and the zero slot is all zero in both tables
// Prints "lanes ok" and exits 0, or the first violation and exits 1.
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "describe_lanes.h"

namespace dl = describe_lanes;

// u_max of a radius-15 patch (orb_extractor.cpp:174-186)
static const int kUmax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return false; } while (0)

static bool check_window() {
    std::vector<int> hit(dl::kWinRows * dl::kWinDwords, 0);
    int idle = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const uint32_t pack = dl::win_pack(lane);
        for (int t = 0; t < dl::kWinPieces; ++t) {
            const int row = dl::win_src_row(pack, lane, t), byte = dl::win_src_byte(pack, lane, t), slot = dl::win_slot(lane, t);
            if (!dl::win_active(lane, t)) {                 // a spare lane of the last piece: reads inside the window, lands behind it and inside the slab
                if (row < 0 || row >= dl::kWinRows || byte != 0) FAIL("window: spare lane %d of piece %d reads row %d byte %d", lane, t, row, byte);
                if (slot < dl::kWinRows * dl::kWinDwords || slot >= 48 * dl::kWinDwords || slot >= dl::kSlabDwords) FAIL("window: spare lane %d of piece %d lands on dword %d", lane, t, slot);
                ++idle;
                continue;
            }
            if (row != dl::win_row(pack, t) || byte != dl::win_byte(pack, t)) FAIL("window: lane %d piece %d: source (%d, %d)", lane, t, row, byte);
            if (row < 0 || row >= dl::kWinRows || byte < 0 || byte > 44 || byte % 4) FAIL("window: lane %d piece %d reads row %d byte %d", lane, t, row, byte);
            if (slot != row * dl::kWinDwords + byte / 4) FAIL("window: lane %d piece %d (row %d, byte %d) lands on dword %d", lane, t, row, byte, slot);
            ++hit[slot];
        }
    }
    for (size_t i = 0; i < hit.size(); ++i)
        if (hit[i] != 1) FAIL("window: dword %d fetched %d times", (int)i, hit[i]);
    if (idle != 64 * dl::kWinPieces - dl::kWinRows * dl::kWinDwords) FAIL("window: %d idle pieces", idle);
    return true;
}

static bool check_orientation() {
    std::vector<int> src_hit(dl::kWinRows * dl::kWinDwords, 0), dst_hit(dl::kPatchRows * dl::kPatchDwords, 0);
    for (int lane = 0; lane < 64; ++lane)
        for (int t = 0; t < 4; ++t) {
            const int dst = dl::ori_dst(lane, t);
            if (dst < 0 || dst >= (int)dst_hit.size()) FAIL("orientation: lane %d piece %d writes dword %d", lane, t, dst);
            ++dst_hit[dst];
            if (!dl::ori_active(lane, t)) {
                if (dst < 31 * 8) FAIL("orientation: lane %d piece %d has no source but is patch dword %d", lane, t, dst);
                if (dl::disc_mask(lane, t, kUmax) != 0u) FAIL("orientation: the zero row is not masked (lane %d)", lane);
                continue;
            }
            const int src = dl::ori_src(lane, t), row = src / dl::kWinDwords, dw = src % dl::kWinDwords;
            if (row < 7 || row > 37 || dw < 2 || dw > 9) FAIL("orientation: lane %d piece %d reads window row %d dword %d", lane, t, row, dw);
            if (row - dl::kOriRow0 != (dst >> 3) || dw - dl::kOriDword0 != (dst & 7)) FAIL("orientation: lane %d piece %d: window (%d, %d) -> patch dword %d", lane, t, row, dw, dst);
            ++src_hit[src];
        }
    for (int r = 0; r < dl::kWinRows; ++r)
        for (int c = 0; c < dl::kWinDwords; ++c) {
            const int want = (r >= 7 && r <= 37 && c >= 2 && c <= 9) ? 1 : 0;
            if (src_hit[r * dl::kWinDwords + c] != want) FAIL("orientation: window row %d dword %d read %d times", r, c, src_hit[r * dl::kWinDwords + c]);
        }
    for (size_t i = 0; i < dst_hit.size(); ++i)
        if (dst_hit[i] != 1) FAIL("orientation: patch dword %d written %d times", (int)i, dst_hit[i]);
    return true;
}

// the wave's moments of a 45 x 48-byte window, as the kernel forms them
static void wave_moments(const std::vector<uint8_t> &win, long &m10, long &m01) {
    auto dword = [&](int i) { uint32_t v; std::memcpy(&v, win.data() + 4 * i, 4); return v; };      // (little-endian, as on the device)
    m10 = m01 = 0;
    for (int lane = 0; lane < 64; ++lane) {
        uint32_t d[4];
        for (int t = 0; t < 4; ++t) d[t] = (dl::ori_active(lane, t) ? dword(dl::ori_src(lane, t)) : 0u) & dl::disc_mask(lane, t, kUmax);
        int a, b;
        dl::lane_moments(d, dl::moment_col_weights(lane), dl::moment_row_bias(lane), a, b);
        m10 += a; m01 += b;
    }
}

// orb_extractor.cpp:245-275 on the same window: the keypoint is at row 22, byte 23
static void ref_moments(const std::vector<uint8_t> &win, long &m10, long &m01) {
    m10 = m01 = 0;
    for (int v = -dl::kHalfPatch; v <= dl::kHalfPatch; ++v)
        for (int u = -kUmax[std::abs(v)]; u <= kUmax[std::abs(v)]; ++u) {
            const int I = win[(22 + v) * 48 + 23 + u];
            m10 += u * I; m01 += v * I;
        }
}

static bool same_moments(const std::vector<uint8_t> &win, const char *what, int k) {
    long a, b, c, d;
    wave_moments(win, a, b);
    ref_moments(win, c, d);
    if (a != c || b != d) FAIL("moments: %s %d: (%ld, %ld), the reference has (%ld, %ld)", what, k, a, b, c, d);
    return true;
}

static bool check_moments() {
    std::vector<uint8_t> win(dl::kWinRows * 48);
    for (int k = 0; k < dl::kWinRows * 48; ++k) {                        // one pixel at a time: in the disc it counts once with its (u, v), outside not at all
        std::fill(win.begin(), win.end(), 0);
        win[k] = 255;
        if (!same_moments(win, "one-hot byte", k)) return false;
    }
    std::fill(win.begin(), win.end(), 255);
    if (!same_moments(win, "all-255", 0)) return false;
    uint32_t s = 12345u;
    for (int rep = 0; rep < 200; ++rep) {
        for (auto &b : win) { s = s * 1664525u + 1013904223u; b = (uint8_t)(s >> 24); }
        if (!same_moments(win, "random window", rep)) return false;
    }
    return true;
}

static bool check_taps() {
    uint32_t tab[64 * 4];
    dl::tap_table(tab);
    for (int table = 0; table < 2; ++table)
        for (int j = 0; j < 4; ++j)
            if (tab[(32 * table + dl::kTapZeroSlot) * 4 + j] != 0u) FAIL("taps: the zero slot of table %d holds a tap", table);
    for (int lane = 0; lane < 64; ++lane)
        for (int t = 0; t < 3; ++t) {
            const int n = lane & 15, q = lane >> 4, dt = q - t;
            const bool on = (dt == 0 || dt == 1) && (t < 2 || n <= 6);
            const int want = on ? (dt & 1) * 16 + n : dl::kTapZeroSlot, got = dl::tap_slot(lane, t);
            if (got != want || got < 0 || got >= 32) FAIL("taps: lane %d tile %d selects entry %d, not %d", lane, t, got, want);
        }
    return true;
}

int main() {
    if (!check_window() || !check_orientation() || !check_moments() || !check_taps()) return 1;
    std::printf("lanes ok\n");
    return 0;
}
