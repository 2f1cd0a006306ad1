// The tile cover of k_fast (orb.hip): which workgroups a pyramid level of w x h pixels is cut into.  Plain C++, no HIP: the
// library builds its tile table from it, and tests/fast_tile_cover_check.cpp checks it on the CPU.
//
// A workgroup is 8 waves of 64 dword-lanes.  Its 512 lanes can be laid out as S sub-rows of 64 / S lanes per wave, S = 1, 2 or 4:
//     S = 1   256 x  32 score positions   248 x  30 outputs
//     S = 2   128 x  64                   120 x  62
//     S = 4    64 x 128                    56 x 126
// (a 1 px NMS halo and the rounding to dwords cost 8 columns and 2 rows whatever the layout).  The wide tile has the most outputs and
// the cheapest row loads, so a level is cut into full columns of it; what is left of the width goes to the layouts that need the
// fewest workgroups for it -- a wave pays its pre-test pass and a workgroup its skeleton whatever number of their lanes lie inside
// the image, so a narrow remainder is cheaper in a few tall tiles than in many wide ones.
//
// FAST needs a 3 px ring inside the image: only positions x <= w - 4, y <= h - 4 can be corners, and tile rows / columns that hold
// none of them are not emitted.
#pragma once
#include <cstdint>
#include <vector>

namespace fast_tiles {

struct Tile { int32_t S, X0, Y0; };              // layout and the first output column / row

constexpr int out_w(int S) { return 256 / S - 8; }
constexpr int out_h(int S) { return 32 * S - 2; }
constexpr int rows_of(int h, int S) { return (h - 3 + out_h(S) - 1) / out_h(S); }   // tile rows that hold a position y <= h - 4

// The fewest workgroups that cover a strip of `r` needed columns (0 < r < 248) of a level of height h, as a list of layouts left to right.
// A piece costs the tile rows of its layout; among equal counts the cover with the fewest, widest pieces wins (S = 1 has the plain
// row loads).  The widths are multiples of 8, so every piece starts on a dword.
inline int cover_strip(int r, int h, std::vector<int> &pieces) {
    int best = -1;
    std::vector<int> best_pieces;
    for (int S = 1; S <= 4; S *= 2) {
        std::vector<int> rest;
        const int n = rows_of(h, S) + (r > out_w(S) ? cover_strip(r - out_w(S), h, rest) : 0);
        if (best < 0 || n < best || (n == best && rest.size() + 1 < best_pieces.size())) {
            best = n;
            best_pieces.assign(1, S);
            best_pieces.insert(best_pieces.end(), rest.begin(), rest.end());
        }
    }
    pieces = best_pieces;
    return best;
}

// Appends the tiles of a level, row-major inside each column strip.
inline void cover(int w, int h, std::vector<Tile> &out) {
    if (w < 4 || h < 4) return;
    const int full = (w - 3) / out_w(1), r = (w - 3) % out_w(1);
    std::vector<int> pieces(full, 1), rest;
    if (r > 0) { cover_strip(r, h, rest); pieces.insert(pieces.end(), rest.begin(), rest.end()); }
    int X0 = 0;
    for (int S : pieces) {
        for (int k = 0; k < rows_of(h, S); ++k) out.push_back(Tile{S, X0, k * out_h(S)});
        X0 += out_w(S);
    }
}

}   // namespace fast_tiles
