// CPU check of the block layout helper of the map-side entry points (slam-module_amd/csrc/ms_layout.h):
//   contract       every offset is a multiple of 256 and offsets never decrease; take(0) advances nothing, so an empty array shares its
//                  offset with the next one; a copied layout goes on from the same offset and neither copy moves the other; ms_at and
//                  MsArray::at return base + offset; fill / put write exactly the bytes of the elements they are given, at the array's
//                  offset, and nothing on either side (guard bytes); get reads the same elements back
//   old chains     ms_triangulate's and ms_project_gate's upload / host / device blocks, with the arithmetic those entry points used to
//                  spell out by hand as the expected values: every offset and every total is the same, for three shapes each, one of them
//                  with an empty array (no observations / no entries)
// Prints "layout ok" and exits 0, or the first violation and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/mi355slam.h"
#include "ms_layout.h"

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return false; } while (0)
#define SAME(got, want) do { if ((size_t)(got) != (size_t)(want)) FAIL("%s: %s = %zu, the chain gives %zu", what, #got, (size_t)(got), (size_t)(want)); } while (0)

static bool check_contract() {
    MsLayout L;
    size_t last = 0;
    for (size_t bytes : {1u, 255u, 256u, 257u, 0u, 0u, 4096u, 3u, 0u, 100000u}) {
        const size_t before = L.end, at = L.take(bytes);
        if (at != before) FAIL("take(%zu) returned %zu, the block ended at %zu", bytes, at, before);
        if (at % 256 || L.end % 256) FAIL("take(%zu): offset %zu / end %zu is no multiple of 256", bytes, at, L.end);
        if (at < last) FAIL("take(%zu): offset %zu after %zu", bytes, at, last);
        if (bytes == 0 && L.end != before) FAIL("take(0) advanced the block by %zu", L.end - before);
        if (bytes > 0 && (L.end < at + bytes || L.end - at - bytes >= 256)) FAIL("take(%zu) advanced the block by %zu", bytes, L.end - at);
        last = at;
    }
    const auto empty = L.array<double>(0);
    const auto next = L.array<int32_t>(5);
    if (empty.off != next.off || empty.bytes() != 0) FAIL("an empty array at %zu does not share its offset with the next one at %zu", empty.off, next.off);

    MsLayout a = L, b = L;                                   // two continuations of one block
    const size_t oa = a.take(300), ob = b.take(7000);
    if (oa != L.end || ob != L.end) FAIL("copies continue at %zu and %zu, the original ended at %zu", oa, ob, L.end);
    if (a.end != L.end + 512 || b.end != L.end + 7168) FAIL("copies ended at %zu and %zu", a.end, b.end);
    if (L.end != oa) FAIL("a copy moved the original to %zu", L.end);

    std::vector<uint8_t> block(4096, 0xa5);
    if (reinterpret_cast<uint8_t *>(ms_at<double>(block.data(), 768)) != block.data() + 768) FAIL("ms_at is not base + offset");
    MsLayout M;
    M.take(100);
    const auto arr = M.array<uint16_t>(37);                  // 74 bytes at offset 256
    if (arr.off != 256 || arr.count != 37 || arr.bytes() != 74) FAIL("array<uint16_t>(37): offset %zu, %zu elements, %zu bytes", arr.off, arr.count, arr.bytes());
    if (reinterpret_cast<uint8_t *>(arr.at(block.data())) != block.data() + 256) FAIL("MsArray::at is not base + offset");
    uint16_t src[37], back[37];
    for (int i = 0; i < 37; ++i) src[i] = (uint16_t)(0x0101 * (i + 1));      // no byte of it is 0xa5
    arr.fill(block.data(), src);
    for (size_t i = 0; i < block.size(); ++i) {
        const bool inside = i >= 256 && i < 256 + 74;
        if (!inside && block[i] != 0xa5) FAIL("fill wrote byte %zu, outside [256, 330)", i);
    }
    if (std::memcmp(block.data() + 256, src, 74) != 0) FAIL("fill did not copy the elements");
    arr.get(block.data(), 0, back, 37);
    if (std::memcmp(back, src, 74) != 0) FAIL("get did not return what fill wrote");

    std::fill(block.begin(), block.end(), (uint8_t)0xa5);
    arr.put(block.data(), 5, src, 3);                        // elements 5 .. 7: bytes 266 .. 271
    for (size_t i = 0; i < block.size(); ++i) {
        const bool inside = i >= 266 && i < 272;
        if (!inside && block[i] != 0xa5) FAIL("put wrote byte %zu, outside [266, 272)", i);
    }
    if (std::memcmp(block.data() + 266, src, 6) != 0) FAIL("put did not copy the elements");
    arr.get(block.data(), 5, back, 3);
    if (std::memcmp(back, src, 6) != 0) FAIL("get did not return what put wrote");
    arr.put(block.data(), 0, nullptr, 0);                    // nothing to copy: the pointer is not touched
    empty.fill(block.data(), nullptr);
    return true;
}

// ms_triangulate: upload block: cameras | focal lengths | sigmas | rows | was | obs_start | obs_kf | obs_octave | obs_x | obs_y | obs_depth; then
// (host only) the results; device-only block: rays | results
static bool check_triangulate(size_t nr, size_t no, size_t nk, size_t nl) {
    char what[96];
    std::snprintf(what, sizeof(what), "triangulate %zu rows, %zu observations, %zu keyframes, %zu levels", nr, no, nk, nl);
    const size_t a4 = 256;
    const size_t o_cam = 0, o_focal = o_cam + ms_align_up(sizeof(ms_pinhole) * nk, a4), o_sigma = o_focal + ms_align_up(4 * nk, a4),
                 o_rows = o_sigma + ms_align_up(4 * nl, a4), o_was = o_rows + ms_align_up(4 * nr, a4), o_start = o_was + ms_align_up(nr, a4),
                 o_kf = o_start + ms_align_up(4 * (nr + 1), a4), o_oct = o_kf + ms_align_up(4 * no, a4), o_x = o_oct + ms_align_up(4 * no, a4),
                 o_y = o_x + ms_align_up(4 * no, a4), o_depth = o_y + ms_align_up(4 * no, a4), up_bytes = o_depth + ms_align_up(4 * no, a4),
                 o_down = up_bytes, host_bytes = o_down + ms_align_up(8 * nr, a4);
    const size_t o_ray = up_bytes, o_out = o_ray + ms_align_up(24 * no, a4), dev_bytes = o_out + ms_align_up(8 * nr, a4);

    MsLayout up;
    const auto l_cam = up.array<ms_pinhole>(nk);
    const auto l_focal = up.array<int32_t>(nk);
    const auto l_sigma = up.array<float>(nl);
    const auto l_rows = up.array<int32_t>(nr);
    const auto l_was = up.array<uint8_t>(nr);
    const auto l_start = up.array<int32_t>(nr + 1);
    const auto l_kf = up.array<int32_t>(no), l_oct = up.array<int32_t>(no);
    const auto l_x = up.array<float>(no), l_y = up.array<float>(no), l_depth = up.array<float>(no);
    MsLayout host = up, dev = up;
    const auto l_down = host.array<int32_t>(2 * nr);
    const auto l_ray = dev.array<double>(3 * no);
    const auto l_out = dev.array<int32_t>(2 * nr);
    SAME(l_cam.off, o_cam); SAME(l_focal.off, o_focal); SAME(l_sigma.off, o_sigma); SAME(l_rows.off, o_rows); SAME(l_was.off, o_was);
    SAME(l_start.off, o_start); SAME(l_kf.off, o_kf); SAME(l_oct.off, o_oct); SAME(l_x.off, o_x); SAME(l_y.off, o_y); SAME(l_depth.off, o_depth);
    SAME(up.end, up_bytes); SAME(l_down.off, o_down); SAME(host.end, host_bytes);
    SAME(l_ray.off, o_ray); SAME(l_out.off, o_out); SAME(dev.end, dev_bytes);
    SAME(l_cam.bytes(), sizeof(ms_pinhole) * nk); SAME(l_was.bytes(), nr); SAME(l_start.bytes(), 4 * (nr + 1)); SAME(l_depth.bytes(), 4 * no);
    SAME(l_ray.bytes(), 24 * no); SAME(l_out.bytes(), 8 * nr);
    if (no == 0 && !(l_kf.off == l_oct.off && l_oct.off == l_depth.off && l_depth.off == up.end && l_ray.off == l_out.off))
        FAIL("%s: the empty observation arrays do not share one offset", what);
    return true;
}

// the view record of project_gate.hip as far as its size goes (the kernels' GvDev)
struct GateView {
    double R[9], t[3], c[3];
    double fx, fy, cx, cy, w, h;
    float threshold, cos_limit;
    int32_t mode, first, count;
    int32_t blk0, nblk;
    int32_t pad;
};
struct Int2 { int32_t x, y; };

// ms_project_gate: upload block: views | block table | mp_index | scale factors | (host only) the views ordered by `first` | n_kept;
// device-only block: n_kept | rank | block counts | block offsets | stand-ins for per-entry outputs
static bool check_gate(size_t n_views, size_t nb, size_t n_entries, size_t n_levels) {
    char what[96];
    std::snprintf(what, sizeof(what), "project gate %zu views, %zu blocks, %zu entries, %zu levels", n_views, nb, n_entries, n_levels);
    const size_t o_view = 0, o_blk = ms_align_up(sizeof(GateView) * n_views, 256), o_idx = o_blk + ms_align_up(8 * nb, 256),
                 o_sf = o_idx + ms_align_up(4 * n_entries, 256), up_bytes = o_sf + ms_align_up(4 * n_levels, 256),
                 o_order = up_bytes, o_down = o_order + ms_align_up(4 * n_views, 256), host_bytes = o_down + ms_align_up(4 * n_views, 256);
    const size_t ne4 = ms_align_up(4 * n_entries, 256);
    const size_t o_nk = up_bytes, o_rank = o_nk + ms_align_up(4 * n_views, 256), o_bc = o_rank + ne4, o_bo = o_bc + ms_align_up(4 * nb, 256),
                 o_x = o_bo + ms_align_up(4 * nb, 256), o_y = o_x + ne4, o_r = o_y + ne4, o_l = o_r + ne4, dev_bytes = o_l + ne4;

    const size_t nv = n_views, ne = n_entries;
    MsLayout up;
    const auto l_view = up.array<GateView>(nv);
    const auto l_blk = up.array<Int2>(nb);
    const auto l_idx = up.array<int32_t>(ne);
    const auto l_sf = up.array<float>(n_levels);
    MsLayout host = up, dev = up;
    const auto l_order = host.array<int32_t>(nv), l_down = host.array<int32_t>(nv);
    const auto l_nk = dev.array<int32_t>(nv), l_rank = dev.array<int32_t>(ne), l_bc = dev.array<int32_t>(nb), l_bo = dev.array<int32_t>(nb);
    const auto l_x = dev.array<float>(ne), l_y = dev.array<float>(ne), l_r = dev.array<float>(ne);
    const auto l_l = dev.array<int32_t>(ne);
    SAME(l_view.off, o_view); SAME(l_blk.off, o_blk); SAME(l_idx.off, o_idx); SAME(l_sf.off, o_sf); SAME(up.end, up_bytes);
    SAME(l_order.off, o_order); SAME(l_down.off, o_down); SAME(host.end, host_bytes);
    SAME(l_nk.off, o_nk); SAME(l_rank.off, o_rank); SAME(l_bc.off, o_bc); SAME(l_bo.off, o_bo);
    SAME(l_x.off, o_x); SAME(l_y.off, o_y); SAME(l_r.off, o_r); SAME(l_l.off, o_l); SAME(dev.end, dev_bytes);
    SAME(l_nk.bytes(), 4 * n_views); SAME(l_blk.bytes(), 8 * nb); SAME(l_idx.bytes(), 4 * n_entries);
    if (ne == 0 && !(l_idx.off == l_sf.off && l_rank.off == l_bc.off && l_x.off == l_l.off && l_l.off == dev.end))
        FAIL("%s: the empty per-entry arrays do not share their offsets with what follows", what);
    return true;
}

int main() {
    static_assert(sizeof(GateView) == 200 && sizeof(Int2) == 8, "stand-ins for project_gate.hip's GvDev and HIP's int2");
    if (!check_contract()) return 1;
    // rows, observations, keyframes, levels: one row without observations; a few rows; sizes past one 256-byte unit in every array
    if (!check_triangulate(1, 0, 3, 8) || !check_triangulate(5, 37, 70, 8) || !check_triangulate(300, 4321, 70, 11)) return 1;
    // views, blocks, entries, levels: views without entries (and so without blocks); one block; several blocks and odd sizes
    if (!check_gate(2, 0, 0, 8) || !check_gate(1, 1, 200, 8) || !check_gate(7, 17, 3011, 12)) return 1;
    std::printf("layout ok\n");
    return 0;
}
