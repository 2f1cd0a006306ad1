// orb.hip -- image pyramid + ORB extraction for gfx950 (MI355X), batched over frames.
//
// Replaces, behind the C ABI of include/mi355slam.h:
//   ImagePyramid::update            image_pyramid.cpp:68-86     -> k_resize (chained), k_blur
//   FeatureDetector::detect         feature_detector.cpp:68-134 -> k_fast, k_select
//   OrbExtractor::detectAndExtract  orb_extractor.cpp:73-164    -> k_tracks, k_describe
//
// Data layout in HBM (one extractor, batch of B frames):
//   level 0      : the caller's device image used in place (or uploaded once into the slab)
//   slab[f]      : levels 1..n-1 and ALL blurred levels of frame f, each plane h x pitch bytes,
//                  pitch = w rounded up to 64 B so every row starts 64-B aligned
//   cand[f][l]   : FAST corner keys of level l (post 3x3 NMS), unordered; capacity w*h/4 (the
//                  strict-maximum NMS cannot keep more than one pixel per 2x2 block)
//   det[f][l]    : the selected corners of level l in key order (score desc, y*w+x asc)
//   out[f]       : final keypoints, structure of arrays, tracker points first then level-major
//
// All pixel arithmetic is integer; the float32 steps of orientation/steering use explicit
// round-to-nearest intrinsics (no FMA contraction) so results are bit-identical to the reference's
// x86-64 SSE2 scalar build (CMakeLists.txt:4-5: -O2, no -march).
#include "ms_internal.h"
#include "fast_tiles.h"
#include "describe_order.h"
#include "describe_strips.h"
#include "describe_lanes.h"
#include "describe_steer.h"
#include "describe_brief_index.h"
#include "resize_vpass.h"
#include "resize_plan.h"
#include "orb_geom.h"
#include <cfloat>
#include <cmath>
#include <cstring>

namespace {

using describe_lanes::kHalfPatch;                    // 15, ORB_FAST_PATCH_HALF_SIZE

// (LevelGeom, PyrGeom, TileMap, TileLevel, TileLevels and the constants kPatchRadius, kMaxQuota, kResizeRows, kBlurSeg, kBlurRows: orb_geom.h)
__device__ __forceinline__ int tile_level(const TileMap &tm, int levels, int t) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < MS_MAX_LEVELS; ++k) l += t >= tm.base[k] ? 1 : 0;     // base[k >= levels] = tile total > t: a compare and an add-with-carry per level
    return l;
}

struct FrameSrc {          // where pyramid level 0 lives for this call
    const uint8_t *lvl0;
    uint64_t lvl0_frame_stride;
    int32_t lvl0_pitch;
    uint8_t *slab;
};

// ------------------------------------------------------------------------------------------------
// copy a non-aligned caller image into the slab's level-0 plane (only when in-place use is impossible)
__global__ __launch_bounds__(256) void k_copy_level0(const uint8_t *src, uint64_t frame_stride, uint64_t row_stride,
                                                     uint8_t *slab, uint64_t slab_stride, uint64_t off, int w, int h, int pitch) {
    const int f = blockIdx.z, y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (x < w && y < h) slab[(uint64_t)f * slab_stride + off + (uint64_t)y * pitch + x] = src[(uint64_t)f * frame_stride + (uint64_t)y * row_stride + x];
}

// ------------------------------------------------------------------------------------------------
// P1: cv::resize INTER_LINEAR, 8U (image_pyramid.cpp:79).  Level l from level l-1 of the same frame.
// 4 destination pixels per lane, one dword store.  Per source row a lane fetches three aligned dwords
// (12 bytes cover the <= 8-byte tap window of its 4 pixels for scale factors up to 2) and funnel-shifts
// them into a 64-bit window; the per-column (offset, a0, a1) and per-row (row0, row1, b0, b1) tables are
// packed so a lane needs two 16-byte table loads.  What bounds it, as measured: a level's launch moves the same bytes per
// second whether its planes fit in the last-level cache (45 MB in 13.9 us at the smallest level) or not (400 MB in 110 us at the largest), a
// constant cost per pixel at every footprint -- yet taking a fifth of the vector instructions out (127.2 M -> 100.0 M per 256-frame step: scalar
// row addresses, resize_row; three instructions per pixel in the vertical pass, resize_vpass.h) while the scalar count rose from 81.8 M to 101.9 M
// bought 3.6 % (0.2935 -> 0.2830 ms for the seven launches).  The time followed the SUM of vector and scalar instructions (-3.4 %), not the vector
// count: neither "HBM-bound by design" nor "bound by vector issue" describes it.  The step's 1.0 .. 1.5 GB (counter as read .. corrected) pass at
// 3.6 .. 5.4 TB/s.  Since then: the levels whose tables allow it (every level of a 1.1 or 1.2 pyramid) run k_resize8 below, and this kernel keeps the
// rest (other ratios, WIDE) and px = 4 of ms_orb_set_resize_plan.  Halving the waves there moved the time by under 5 % while the L2s' misses fell from
// 1.39 x to 1.0 x the source bytes: this kernel's short row segments (2.4 lines of 128 bytes, 3.4 touched, the neighbours on other XCDs) are part of its cost.
// unaligned dword / qword accesses (global memory takes them)
struct __attribute__((packed, aligned(1))) U32u { uint32_t v; };
struct __attribute__((packed, aligned(1))) U64u { uint32_t lo, hi; };
typedef unsigned short us2_t __attribute__((ext_vector_type(2)));
typedef short s2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// Everything k_resize needs about its two levels, by value in the kernel arguments: the launch is per level, and reading the
// geometry table instead put nine dependent scalar round trips in front of every wave's first pixel load.
struct ResizeArgs {
    const uint8_t *src; uint64_t src_frame_stride; int32_t src_pitch, sw, sh;  // level l-1
    uint8_t *dst; uint64_t dst_frame_stride; int32_t dst_pitch, dw, dh;        // level l
};

struct ResizeTab {
    const int16_t *xtab;   // [dw][4] : sx, a0, a1, 0
    const int16_t *ytab;   // [dh][4] : sy0, sy1 (clamped rows), b0, b1
};

__device__ __forceinline__ int resize_px(uint64_t w0, uint64_t w1, int k, int a0, int a1, int b0, int b1) {
    const int r0 = (int)((w0 >> (8 * k)) & 255) * a0 + (int)((w0 >> (8 * k + 8)) & 255) * a1;
    const int r1 = (int)((w1 >> (8 * k)) & 255) * a0 + (int)((w1 >> (8 * k + 8)) & 255) * a1;
    const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
    return min(max(v, 0), 255);
}

struct Window3 { uint32_t d0, d1, d2; };
typedef uint32_t u3_t __attribute__((ext_vector_type(3)));
typedef u3_t u3a_t __attribute__((aligned(4)));       // a 12-byte load from a dword-aligned address
// `row` is wave-uniform; the three lane offsets are >= 0 and below the pitch (0 <= base, last_dword <= sw - 1), so they are added as unsigned 32-bit numbers
__device__ __forceinline__ Window3 window_load(const uint8_t *row, int base, int last_dword) {
    typedef const __attribute__((address_space(1))) uint32_t gdword_t;        // (global_load: a generic pointer would become a flat load)
    return {*(gdword_t *)(row + (uint32_t)min(base, last_dword)), *(gdword_t *)(row + (uint32_t)min(base + 4, last_dword)), *(gdword_t *)(row + (uint32_t)min(base + 8, last_dword))};
}
// Start of row `row` of a plane: row and pitch are wave-uniform and >= 0, so the product and the sum are scalar arithmetic, and a load or store of the row is
// this scalar base plus the lane's unsigned 32-bit byte offset (global_load / global_store v_offset, s[base:base+1]) -- no 64-bit multiply-add per lane.
// The empty statement holds the sum in scalar registers: left alone the compiler adds the lane offset to the plane first and the row's product to that,
// one v_mad_u64_u32 per row.
template <class T> __device__ __forceinline__ T *resize_row(T *plane, int row, int pitch) {
    T *p = plane + (uint64_t)(uint32_t)row * (uint32_t)pitch;
    asm("" : "+s"(p));
    return p;
}

// Shared-row path of k_resize.  At a level ratio near 1.2 the tap rows of a group's five destination rows are the NROWS = 6 or 7 consecutive
// source rows s0 .. s0 + NROWS - 1 (clamped at sh - 1 like the table's entries): row r reads rows s0 + d_r and s0 + d_r + 1 with d_r = r or r + 1.
// Each of them is loaded once and run through the horizontal pass once (F[i][c] = the r >> 4 term of column c), where the general path loads and
// filters ten; the destination rows pick their two F rows by the scalar d_r.  Loads, edge-wave handling, taps and the vertical combine are the
// general path's, so the pixels are the same bit for bit.
template <int NROWS>
__device__ __forceinline__ void resize_shared_rows(const uint8_t *S, int spitch, int s0, int sh, int sx0, int base, int last, bool edge, uint4 taps, uint4 sels,
                                                   const short4 (&yt)[kResizeRows], uint8_t *dst, int dy0, int dx0, int dh, int dpitch) {
    const uint32_t A[4] = {taps.x, taps.y, taps.z, taps.w}, sel[4] = {sels.x, sels.y, sels.z, sels.w};      // the caller's per-column operands (taps times 16), by value
    Window3 W[NROWS];
    if (!edge || last >= 8) {
        const int from0 = edge ? min(base, last - 8) : base, shift = base - from0;       // as in the general path
        uint32_t from = (uint32_t)from0;               // 0 <= from <= last - 8 < pitch: an unsigned 32-bit lane offset beside the row's scalar base
        asm volatile("" : "+v"(from));                 // (an offset the compiler cannot see through: the 12-byte branch stays apart from the three-dword one)
#pragma unroll
        for (int i = 0; i < NROWS; ++i) {
            const u3_t a = *(const __attribute__((address_space(1))) u3a_t *)(resize_row(S, min(s0 + i, sh - 1), spitch) + from);
            W[i] = {a.x, a.y, a.z};
        }
        if (edge) {
#pragma unroll
            for (int i = 0; i < NROWS; ++i) W[i] = {shift == 0 ? W[i].d0 : shift == 4 ? W[i].d1 : W[i].d2, shift == 0 ? W[i].d1 : W[i].d2, W[i].d2};
        }
    } else {
#pragma unroll
        for (int i = 0; i < NROWS; ++i) W[i] = window_load(resize_row(S, min(s0 + i, sh - 1), spitch), base, last);
    }
    uint32_t F[NROWS][4];
#pragma unroll
    for (int i = 0; i < NROWS; ++i) {
        const uint32_t lo = __builtin_amdgcn_alignbyte(W[i].d1, W[i].d0, (uint32_t)sx0), hi = __builtin_amdgcn_alignbyte(W[i].d2, W[i].d1, (uint32_t)sx0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            F[i][c] = resize_vpass::f8(__builtin_amdgcn_udot2(__builtin_bit_cast(us2_t, __builtin_amdgcn_perm(hi, lo, sel[c])), __builtin_bit_cast(us2_t, A[c]), 0u, false));
            asm volatile("" : "+v"(F[i][c]));          // the mask happens here, once: left alone the compiler repeats it in every row body that reads the value
        }
    }
    // the two choices of a row are two bodies behind a scalar branch: the empty asm statements differ, which keeps the compiler from merging the
    // bodies into one with eight per-lane selects in front (as many vector instructions as the shared rows save)
    auto emit = [&](int r, bool upper, const uint32_t (&f0)[4], const uint32_t (&f1)[4]) {
        const uint32_t b0 = resize_vpass::row_tap((uint32_t)yt[r].z), b1 = resize_vpass::row_tap((uint32_t)yt[r].w);      // scalar
        uint32_t v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v[c] = resize_vpass::vsum(b0, f0[c], b1, f1[c]);
            asm("" : "+v"(v[c]));                      // one v_add3_u32: left alone the + 2 of the odd columns moves behind their shift into the pair (two more instructions)
        }
        uint32_t packed = resize_vpass::pack4(v[0], v[1], v[2], v[3]);
        if (upper) asm volatile("; rows d + 1, d + 2" : "+v"(packed)); else asm volatile("; rows d, d + 1" : "+v"(packed));
        *(__attribute__((address_space(1))) uint32_t *)(resize_row(dst, dy0 + r, dpitch) + (uint32_t)dx0) = packed;       // 0 <= dx0 < pitch
    };
#pragma unroll
    for (int r = 0; r < kResizeRows; ++r) {
        if (dy0 + r >= dh) continue;                                 // rows of the padded last group (wave-uniform, like every branch here)
        if (r + 2 >= NROWS || yt[r].x - s0 == r) emit(r, false, F[r], F[r + 1]);      // NROWS = 6: the caller has seen d_4 = 4
        else emit(r, true, F[r + 1], F[min(r + 2, NROWS - 1)]);
    }
}

template <bool WIDE>   // WIDE: tap window of 4 pixels may exceed 8 bytes (scale factor > 2) -> per-tap byte loads
__global__ __launch_bounds__(256) void k_resize(ResizeArgs R, ResizeTab T) {
    const struct { int w, h, pitch; } D = {R.dw, R.dh, R.dst_pitch};
    const int sw = R.sw;
    const int f = blockIdx.z;
    const int dy0 = (blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * kResizeRows;   // wave-uniform (SGPR): row addresses stay scalar
    const int dx0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    if (dy0 >= D.h || dx0 >= D.w) return;
    const int spitch = R.src_pitch;
    const uint8_t *S = R.src + (uint64_t)f * R.src_frame_stride;
    uint8_t *dst = R.dst + (uint64_t)f * R.dst_frame_stride;
    // both tables are padded to whole groups (last entry repeated), so a lane's four columns are two 16-byte loads
    const uint4 xa = reinterpret_cast<const uint4 *>(T.xtab)[dx0 >> 1], xb = reinterpret_cast<const uint4 *>(T.xtab)[(dx0 >> 1) + 1];
    const short4 xt[4] = {__builtin_bit_cast(short4, make_uint2(xa.x, xa.y)), __builtin_bit_cast(short4, make_uint2(xa.z, xa.w)),
                          __builtin_bit_cast(short4, make_uint2(xb.x, xb.y)), __builtin_bit_cast(short4, make_uint2(xb.z, xb.w))};
    short4 yt[kResizeRows];
#pragma unroll
    for (int r = 0; r < kResizeRows; ++r) yt[r] = reinterpret_cast<const short4 *>(T.ytab)[dy0 + r];
    if (!WIDE) {
        // the table entries straight from the loaded dwords, (sx | a0 << 16) and (a1 | 0 << 16) per column: read through xt[] they leave the array
        // in memory (the compiler joins the two 16-bit reads of a0, a1 into one dword read at offset 2 of an entry, and with the two row paths
        // below it then places the array in LDS)
        const uint32_t xlo[4] = {xa.x, xa.z, xb.x, xb.z}, xhi[4] = {xa.y, xa.w, xb.y, xb.w};
        const int sx0 = (int16_t)xlo[0], last = (sw - 1) & ~3, base = sx0 & ~3;
        // per column: the two taps as one v_dot2 operand (a0, a1), and a v_perm selector that lifts source bytes k, k+1 of the
        // row's 8-byte window into 16-bit lanes (k = sx - sx0 <= 6)
        uint32_t A[4], sel[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            A[i] = resize_vpass::preshift_taps(__builtin_amdgcn_alignbit(xhi[i], xlo[i], 16));      // times 16: the horizontal pass delivers 16 r (resize_vpass.h)
            sel[i] = 0x0C010C00u + (uint32_t)((int16_t)xlo[i] - sx0) * 0x00010001u;
        }
        // The three dwords of a window are ONE 12-byte load wherever no lane of the wave touches the row's last dwords (a 12-byte load there
        // would run past the row, and past the caller's buffer on the last row of level 0): a third of the vector-memory instructions and of the
        // address arithmetic in front of them (measured when the three dword loads became one: -36 % for half the loads).
        const bool edge = __ballot(base + 8 > last) != 0;        // wave-uniform
        // Scalar test on the group's five table entries: do its rows share six or seven consecutive source rows?  (Rows past the level's
        // last one are padding and do not count.)  Other ratios, and any group that fails the test, take the general path below.
        const int s0 = yt[0].x, sh = R.sh;
        int shared = 1;
#pragma unroll
        for (int r = 0; r < kResizeRows; ++r)
            shared &= (int)(dy0 + r >= D.h) | ((int)((unsigned)(yt[r].x - s0 - r) <= 1u) & (int)(yt[r].y == min(yt[r].x + 1, sh - 1)));
        if (shared) {
            const uint4 taps = make_uint4(A[0], A[1], A[2], A[3]), sels = make_uint4(sel[0], sel[1], sel[2], sel[3]);
            if (dy0 + 4 < D.h && yt[4].x - s0 == 5) resize_shared_rows<7>(S, spitch, s0, sh, sx0, base, last, edge, taps, sels, yt, dst, dy0, dx0, D.h, D.pitch);
            else resize_shared_rows<6>(S, spitch, s0, sh, sx0, base, last, edge, taps, sels, yt, dst, dy0, dx0, D.h, D.pitch);
            return;
        }
        Window3 W0[kResizeRows], W1[kResizeRows];
        if (!edge || last >= 8) {
            // edge wave: the 12 bytes are fetched from min(base, last - 8) and moved down by whole dwords afterwards, which reproduces the
            // clamped dwords exactly (d_k = row[min(base + 4k, last)])
            const int from0 = edge ? min(base, last - 8) : base, shift = base - from0;       // shift = 0, 4 or 8 bytes
            uint32_t from = (uint32_t)from0;              // 0 <= from <= last - 8 < pitch: an unsigned 32-bit lane offset beside each row's scalar base
            asm volatile("" : "+v"(from));                // keeps the compiler from folding this branch into the clamped one below (equal values, three loads each)
#pragma unroll
            for (int r = 0; r < kResizeRows; ++r) {
                const uint8_t *p0 = resize_row(S, yt[r].x, spitch) + from, *p1 = resize_row(S, yt[r].y, spitch) + from;
                const u3_t a = *(const __attribute__((address_space(1))) u3a_t *)(p0), b = *(const __attribute__((address_space(1))) u3a_t *)(p1);   // global_load_dwordx3 (a generic pointer would become a flat load)
                W0[r] = {a.x, a.y, a.z};
                W1[r] = {b.x, b.y, b.z};
            }
            if (edge) {
#pragma unroll
                for (int r = 0; r < kResizeRows; ++r) {
                    W0[r] = {shift == 0 ? W0[r].d0 : shift == 4 ? W0[r].d1 : W0[r].d2, shift == 0 ? W0[r].d1 : W0[r].d2, W0[r].d2};
                    W1[r] = {shift == 0 ? W1[r].d0 : shift == 4 ? W1[r].d1 : W1[r].d2, shift == 0 ? W1[r].d1 : W1[r].d2, W1[r].d2};
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < kResizeRows; ++r) {
                W0[r] = window_load(resize_row(S, yt[r].x, spitch), base, last);
                W1[r] = window_load(resize_row(S, yt[r].y, spitch), base, last);
            }
        }
#pragma unroll
        for (int r = 0; r < kResizeRows; ++r) {
            // window = source bytes sx0 .. sx0+7 of each tap row (byte funnel of the three aligned dwords)
            const uint32_t lo0 = __builtin_amdgcn_alignbyte(W0[r].d1, W0[r].d0, (uint32_t)sx0), hi0 = __builtin_amdgcn_alignbyte(W0[r].d2, W0[r].d1, (uint32_t)sx0);
            const uint32_t lo1 = __builtin_amdgcn_alignbyte(W1[r].d1, W1[r].d0, (uint32_t)sx0), hi1 = __builtin_amdgcn_alignbyte(W1[r].d2, W1[r].d1, (uint32_t)sx0);
            const uint32_t b0 = resize_vpass::row_tap((uint32_t)yt[r].z), b1 = resize_vpass::row_tap((uint32_t)yt[r].w);      // scalar
            uint32_t v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t r0 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2_t, __builtin_amdgcn_perm(hi0, lo0, sel[i])), __builtin_bit_cast(us2_t, A[i]), 0u, false);
                const uint32_t r1 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2_t, __builtin_amdgcn_perm(hi1, lo1, sel[i])), __builtin_bit_cast(us2_t, A[i]), 0u, false);
                v[i] = resize_vpass::vsum(b0, resize_vpass::f8(r0), b1, resize_vpass::f8(r1));      // v >> 2 <= 255 by construction (taps sum to 2048 +- 1)
                asm("" : "+v"(v[i]));                  // one v_add3_u32, as in the shared-row path
            }
            const uint32_t packed = resize_vpass::pack4(v[0], v[1], v[2], v[3]);
            if (dy0 + r < D.h) *(__attribute__((address_space(1))) uint32_t *)(resize_row(dst, dy0 + r, D.pitch) + (uint32_t)dx0) = packed;       // 0 <= dx0 < pitch
        }
    } else {
#pragma unroll
        for (int r = 0; r < kResizeRows; ++r) {
            const uint8_t *S0 = S + (uint64_t)yt[r].x * spitch, *S1 = S + (uint64_t)yt[r].y * spitch;
            uint32_t packed = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int sx = xt[i].x, sx1 = min(sx + 1, sw - 1);
                const uint64_t w0 = (uint64_t)S0[sx] | ((uint64_t)S0[sx1] << 8), w1 = (uint64_t)S1[sx] | ((uint64_t)S1[sx1] << 8);
                packed |= (uint32_t)resize_px(w0, w1, 0, xt[i].y, xt[i].z, yt[r].z, yt[r].w) << (8 * i);
            }
            if (dy0 + r < D.h) *reinterpret_cast<uint32_t *>(dst + (uint64_t)(dy0 + r) * D.pitch + dx0) = packed;
        }
    }
}

// k_resize8: the shared-row form of k_resize<false> with 8 destination pixels per lane (resize_plan.h), for the levels whose tables pass the
// plan's eligibility test (every chunk inside its 16-byte window, every row group on 6 or 7 consecutive source rows).  Per source row a lane
// loads 16 bytes (global_load_dwordx4) and stores 8 per destination row; the horizontal pass is one v_perm + v_dot2 + mask per pixel from
// three byte funnels per row, the vertical pass, the rounding and the packing are resize_vpass.h's: the pixels are k_resize's bit for bit.
// A wave's row segment is twice as long (about 614 source bytes at ratio 1.2), so fewer of the 128-byte lines it touches are shared with the
// neighbouring tile, and from resize_plan::kByFrameMinFrames frames on a frame's tiles all run on one XCD, whose L2 then serves those shared
// lines (the tile borders, the source row two row groups share) instead of every L2 fetching its own copy.  Halving the waves (and with
// them the scalar and vector-memory instructions) is NOT what the time follows: see DESIGN section 10.
struct Resize8Tab {
    const uint32_t *xtab;  // [chunks][8] : resize_plan::entry
    const int16_t *ytab;   // as ResizeTab's
};
typedef u32x4_t u4a_t __attribute__((aligned(4)));       // a 16-byte load from a dword-aligned address
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

template <int NROWS>
__device__ __forceinline__ void resize8_shared_rows(const uint8_t *S, int spitch, int s0, int sh, uint32_t sx0, uint32_t from, int shift, bool edge,
                                                    const uint32_t (&A)[resize_plan::kPx], const uint32_t (&sel)[resize_plan::kPx],
                                                    const short4 (&yt)[kResizeRows], uint8_t *dst, int dy0, uint32_t doff, int dh, int dpitch) {
    resize_plan::Window W[NROWS];
#pragma unroll
    for (int i = 0; i < NROWS; ++i) {
        const u32x4_t a = *(const __attribute__((address_space(1))) u4a_t *)(resize_row(S, min(s0 + i, sh - 1), spitch) + from);
        W[i] = {a.x, a.y, a.z, a.w};
    }
    if (edge) {                                        // a branch of its own (the empty statement cannot be hoisted): as selects the shift costs every wave six instructions per row
#pragma unroll
        for (int i = 0; i < NROWS; ++i) {
            uint32_t d0 = W[i].d0, d1 = W[i].d1, d2 = W[i].d2, d3 = W[i].d3;
            asm volatile("" : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3));
            W[i] = resize_plan::shift_down(d0, d1, d2, d3, shift);
        }
    }
    uint32_t F[NROWS][resize_plan::kPx];
#pragma unroll
    for (int i = 0; i < NROWS; ++i) {
        const resize_plan::Funnels fn = resize_plan::funnels(W[i], sx0);
#pragma unroll
        for (int c = 0; c < resize_plan::kPx; ++c) {
            F[i][c] = resize_vpass::f8(__builtin_amdgcn_udot2(__builtin_bit_cast(us2_t, resize_plan::tap_pair(fn, c, sel[c])), __builtin_bit_cast(us2_t, A[c]), 0u, false));
            asm volatile("" : "+v"(F[i][c]));          // the mask happens here, once (as in resize_shared_rows)
        }
    }
    // two bodies behind a scalar branch, kept apart as in resize_shared_rows
    auto emit = [&](int r, bool upper, const uint32_t (&f0)[resize_plan::kPx], const uint32_t (&f1)[resize_plan::kPx]) {
        const uint32_t b0 = resize_vpass::row_tap((uint32_t)yt[r].z), b1 = resize_vpass::row_tap((uint32_t)yt[r].w);      // scalar
        uint32_t v[resize_plan::kPx];
#pragma unroll
        for (int c = 0; c < resize_plan::kPx; ++c) {
            v[c] = resize_vpass::vsum(b0, f0[c], b1, f1[c]);
            asm("" : "+v"(v[c]));                      // one v_add3_u32
        }
        u32x2_t packed = {resize_vpass::pack4(v[0], v[1], v[2], v[3]), resize_vpass::pack4(v[4], v[5], v[6], v[7])};
        if (upper) asm volatile("; rows d + 1, d + 2" : "+v"(packed)); else asm volatile("; rows d, d + 1" : "+v"(packed));
        *(__attribute__((address_space(1))) u32x2_t *)(resize_row(dst, dy0 + r, dpitch) + doff) = packed;       // 8-byte aligned: rows start 64-byte aligned
    };
#pragma unroll
    for (int r = 0; r < kResizeRows; ++r) {
        if (dy0 + r >= dh) continue;                                 // rows of the padded last group (wave-uniform, like every branch here)
        if (r + 2 >= NROWS || yt[r].x - s0 == r) emit(r, false, F[r], F[r + 1]);      // NROWS = 6: the caller has seen d_4 = 4
        else emit(r, true, F[r + 1], F[min(r + 2, NROWS - 1)]);
    }
}

__global__ __launch_bounds__(256) void k_resize8(ResizeArgs R, Resize8Tab T, resize_plan::Launch P) {
    const resize_plan::Tile tl = resize_plan::decode(P, blockIdx.x, blockIdx.y, blockIdx.z);                 // wave-uniform (SGPRs)
    const int dy0 = (tl.ty * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * kResizeRows;             // wave-uniform: row addresses stay scalar
    const int chunk = tl.tx * 64 + (int)(threadIdx.x & 63);
    if (tl.frame >= P.nf || dy0 >= R.dh || chunk >= P.nchunks) return;       // from here on a ballot counts working lanes only
    const uint8_t *S = R.src + (uint64_t)tl.frame * R.src_frame_stride;
    uint8_t *dst = R.dst + (uint64_t)tl.frame * R.dst_frame_stride;
    const uint32_t doff = (uint32_t)chunk * resize_plan::kPx;              // 8 chunk + 7 < pitch
    const uint4 xa = reinterpret_cast<const uint4 *>(T.xtab)[2 * chunk], xb = reinterpret_cast<const uint4 *>(T.xtab)[2 * chunk + 1];
    const uint32_t e[resize_plan::kPx] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
    uint32_t A[resize_plan::kPx], sel[resize_plan::kPx];
#pragma unroll
    for (int c = 0; c < resize_plan::kPx; ++c) { A[c] = resize_plan::entry_taps(e[c]); sel[c] = resize_plan::entry_sel(e[c]); }
    const uint32_t sx0 = resize_plan::chunk_sx0(e[0], e[1], e[2], e[3]);
    short4 yt[kResizeRows];
#pragma unroll
    for (int r = 0; r < kResizeRows; ++r) yt[r] = reinterpret_cast<const short4 *>(T.ytab)[dy0 + r];
    const int last = (R.sw - 1) & ~3, base = (int)(sx0 & ~3u);
    const bool edge = __ballot(resize_plan::lane_is_edge(base, last)) != 0;        // wave-uniform
    const resize_plan::Fetch ft = resize_plan::fetch(base, last, edge);             // 0 <= from <= last - 12 on an edge wave, from = base <= last - 12 otherwise
    uint32_t from = (uint32_t)ft.from;               // < pitch: an unsigned 32-bit lane offset beside each row's scalar base
    asm volatile("" : "+v"(from));
    const int s0 = yt[0].x, sh = R.sh;
    if (dy0 + 4 < R.dh && yt[4].x - s0 == 5) resize8_shared_rows<7>(S, R.src_pitch, s0, sh, sx0, from, ft.shift, edge, A, sel, yt, dst, dy0, doff, R.dh, R.dst_pitch);
    else resize8_shared_rows<6>(S, R.src_pitch, s0, sh, sx0, from, ft.shift, edge, A, sel, yt, dst, dy0, doff, R.dh, R.dst_pitch);
}

// ------------------------------------------------------------------------------------------------
// P2: cv::GaussianBlur 7x7 sigma 2, BORDER_REFLECT_101, 8U fixed point (image_pyramid.cpp:84).
// One launch covers every level of every frame (tile table in PyrGeom).  No LDS: a lane owns one dword
// (4 pixels) of a row; a wave owns a 256-pixel row segment and walks 8 output rows.
//   vertical pass   on the raw bytes, two pixels per instruction: even/odd bytes of the dword are two
//                   16-bit lanes (sums stay < 2^16 because the 8.8 taps add up to 256) -> v_pk_mad_u16
//   horizontal pass on the 16-bit column sums of the lane and its two neighbours (DPP wave shifts),
//                   v_dot2_u32_u16 with the rounding constant as the initial accumulator
// Lanes 0 and 63 only provide halo (248 outputs per 256 loaded pixels); REFLECT_101 is applied when the
// bytes are loaded, which commutes with the vertical pass.

__device__ __forceinline__ int reflect101(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1);
}

__device__ __forceinline__ uint32_t vsum7(const uint32_t *v) {   // 18,34,48,56,48,34,18 on two packed 16-bit lanes
    const us2_t k0 = {18, 18}, k1 = {34, 34}, k2 = {48, 48}, k3 = {56, 56};
    const us2_t a = __builtin_bit_cast(us2_t, v[0]) + __builtin_bit_cast(us2_t, v[6]);
    const us2_t b = __builtin_bit_cast(us2_t, v[1]) + __builtin_bit_cast(us2_t, v[5]);
    const us2_t c = __builtin_bit_cast(us2_t, v[2]) + __builtin_bit_cast(us2_t, v[4]);
    const us2_t d = __builtin_bit_cast(us2_t, v[3]);
    return __builtin_bit_cast(uint32_t, (us2_t)(a * k0 + b * k1 + c * k2 + d * k3));
}

__device__ __forceinline__ uint32_t dot2(uint32_t a, unsigned lo, unsigned hi, uint32_t acc) {
    const us2_t k = {(unsigned short)lo, (unsigned short)hi};
    return __builtin_amdgcn_udot2(__builtin_bit_cast(us2_t, a), k, acc, false);
}

// lane i <- lane i-1 / lane i+1 of the 64-wide wave in one VALU op (gfx9 DPP wave shifts); the end lane's value is unspecified
__device__ __forceinline__ uint32_t wave_from_prev(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /*wave_shr:1*/, 0xf, 0xf, false); }
__device__ __forceinline__ uint32_t wave_from_next(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /*wave_shl:1*/, 0xf, 0xf, false); }
// the same where lanes 0 / 63 may receive anything (bound_ctrl: no register to initialise in front of the DPP move)
__device__ __forceinline__ uint32_t wave_from_prev_dc(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /*wave_shr:1*/, 0xf, 0xf, true); }
__device__ __forceinline__ uint32_t wave_from_next_dc(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /*wave_shl:1*/, 0xf, 0xf, true); }

// inclusive prefix sum over the 64 lanes: four row_shr steps inside each row of 16, then row_bcast 15 / 31 across rows
__device__ __forceinline__ int wave_scan_add(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111 /*row_shr:1*/, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112 /*row_shr:2*/, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114 /*row_shr:4*/, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118 /*row_shr:8*/, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142 /*row_bcast:15*/, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143 /*row_bcast:31*/, 0xc, 0xf, false);
    return v;
}

__global__ __launch_bounds__(256) void k_blur(FrameSrc src, TileLevels TL, TileMap tm) {
    int t = blockIdx.x;
    const int l = tile_level(tm, TL.levels, t);
    t -= tm.base[l];
    const TileLevel G = TL.L[l];                       // one batch of loads; everything below is arithmetic on it
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform (SGPR): the 14 row addresses are scalar work
    const int trow = G.btiles_x == 1 ? t : (int)__umulhi((uint32_t)t, G.btiles_inv);     // t / btiles_x without the division sequence (2^32 / 1 does not fit)
    const int x = (t - trow * G.btiles_x) * kBlurSeg - 4 + lane * 4;
    const int y0 = trow * (4 * kBlurRows) + wave * kBlurRows;
    const int f = blockIdx.y, w = G.w, h = G.h;
    if (y0 >= h) return;
    const int pitch = l == 0 ? src.lvl0_pitch : G.pitch;
    const uint8_t *img = l == 0 ? src.lvl0 + (uint64_t)f * src.lvl0_frame_stride : src.slab + (uint64_t)f * TL.slab_stride + G.img_off;
    uint32_t e[kBlurRows + 6], o[kBlurRows + 6];
    // the column test is the same for every row of a lane: ONE wave-uniform branch picks the plain-dword path for whole waves
    // (per-load branches cost scalar instructions, and the scalar unit is shared by the CU's four SIMDs)
    if (__ballot(!(x >= 0 && x + 3 < w)) == 0) {
        if (y0 >= 3 && y0 + kBlurRows + 2 < h) {           // no row is reflected: one 64-bit base, the pitch added per row (scalar work is shared by the CU)
            const uint8_t *rp = img + (int64_t)(y0 - 3) * pitch;
#pragma unroll
            for (int r = 0; r < kBlurRows + 6; ++r) {
                const uint32_t d = *reinterpret_cast<const uint32_t *>(rp + x);
                rp += pitch;
                e[r] = d & 0x00FF00FFu;
                o[r] = (d >> 8) & 0x00FF00FFu;
            }
        } else {
#pragma unroll
            for (int r = 0; r < kBlurRows + 6; ++r) {
                const uint32_t d = *reinterpret_cast<const uint32_t *>(img + (uint64_t)reflect101(y0 - 3 + r, h) * pitch + x);
                e[r] = d & 0x00FF00FFu;
                o[r] = (d >> 8) & 0x00FF00FFu;
            }
        }
    } else {
        // A wave on the left or right border (a third of all waves): BORDER_REFLECT_101 without per-byte loads.  Every reflected or
        // straddling pixel of the row lies in its first or last 8 bytes, so the wave fetches those two dwords (one address for all
        // lanes) and a border lane picks its 4 bytes out of them with ONE v_perm whose selector depends only on the lane, not on the row.
        const int xa = min(max(x, 0), w - 4);
        const bool is_l = x < 0, is_r = x > w - 4;
        uint32_t sel_r = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = x + i;
            sel_r |= (uint32_t)((p < w ? p - (w - 8) : (w + 6) - p) & 7) << (8 * i);       // byte of the window [w-8, w-1] that holds pixel reflect(p)
        }
        const bool wave_l = __ballot(is_l) != 0, wave_r = __ballot(is_r) != 0;
#pragma unroll
        for (int r = 0; r < kBlurRows + 6; ++r) {
            const uint8_t *row = img + (uint64_t)reflect101(y0 - 3 + r, h) * pitch;
            uint32_t d = reinterpret_cast<const U32u *>(row + xa)->v;
            if (wave_l) {                                        // pixels -4..-1 = pixels 4, 3, 2, 1
                const uint32_t f0 = reinterpret_cast<const U32u *>(row)->v, f1 = reinterpret_cast<const U32u *>(row + 4)->v;
                d = is_l ? __builtin_amdgcn_perm(f1, f0, 0x01020304u) : d;
            }
            if (wave_r) {
                const uint32_t e0 = reinterpret_cast<const U32u *>(row + (w - 8))->v, e1 = reinterpret_cast<const U32u *>(row + (w - 4))->v;
                d = is_r ? __builtin_amdgcn_perm(e1, e0, sel_r) : d;
            }
            e[r] = d & 0x00FF00FFu;
            o[r] = (d >> 8) & 0x00FF00FFu;
        }
    }
    uint8_t *dst = src.slab + (uint64_t)f * TL.slab_stride + G.blur_off;
#pragma unroll
    for (int j = 0; j < kBlurRows; ++j) {
        const uint32_t Ce = vsum7(e + j), Co = vsum7(o + j);            // columns (x, x+2) and (x+1, x+3)
        // neighbour lanes by DPP wave shifts (VALU, no LDS round trip); lanes 0 and 63 receive a don't-care and store nothing
        const uint32_t Le = wave_from_prev(Ce), Lo = wave_from_prev(Co);
        const uint32_t Re = wave_from_next(Ce), Ro = wave_from_next(Co);
        uint32_t o0 = dot2(Lo, 18, 48, 32768u); o0 = dot2(Le, 0, 34, o0); o0 = dot2(Ce, 56, 34, o0); o0 = dot2(Co, 48, 18, o0);
        uint32_t o1 = dot2(Le, 0, 18, 32768u); o1 = dot2(Lo, 0, 34, o1); o1 = dot2(Ce, 48, 48, o1); o1 = dot2(Co, 56, 34, o1); o1 = dot2(Re, 18, 0, o1);
        uint32_t o2 = dot2(Lo, 0, 18, 32768u); o2 = dot2(Ce, 34, 56, o2); o2 = dot2(Co, 48, 48, o2); o2 = dot2(Re, 34, 0, o2); o2 = dot2(Ro, 18, 0, o2);
        uint32_t o3 = dot2(Ce, 18, 48, 32768u); o3 = dot2(Co, 34, 56, o3); o3 = dot2(Re, 48, 18, o3); o3 = dot2(Ro, 34, 0, o3);
        const int y = y0 + j;
        if (y < h && lane >= 1 && lane <= 62 && x < w)
            *reinterpret_cast<uint32_t *>(dst + (uint64_t)y * G.pitch + x) = (o0 >> 16) | ((o1 >> 16) << 8) | ((o2 >> 16) << 16) | ((o3 >> 16) << 24);
    }
}

// ------------------------------------------------------------------------------------------------
// D1: FAST-9/16 corners + score + 3x3 strict NMS (this build's detector behind
// feature_detector.cpp:89-98).  One launch covers every level of every frame.
// Tile = 248 x 30 outputs; 256 x 32 score positions (1 px NMS halo, rounded to dwords), 4 position rows per wave, 8 waves:
// 34 KB of LDS, so 4 workgroups (32 waves) share a CU -- the kernel is latency-bound (dependent loads,
// five barriers, one returning atomic per tile), not ALU-bound, and needs the occupancy.
// A wave runs the whole of phase A1 and a workgroup its skeleton whatever number of their lanes lie inside the image, so the narrow
// column that is left of a level's width beside the full 248 px columns is cut into TALL tiles of the same area instead: the 64 lanes
// of a wave as 2 sub-rows of 128 px (120 x 62 outputs) or 4 sub-rows of 64 px (56 x 126 outputs), and tile rows without a valid
// position are not launched (fast_tiles.h: 401 instead of 452 workgroups for a 720p pyramid).  The layout is a template parameter
// of the tile body, chosen by one wave-uniform branch on the tile-table entry; the LDS arrays are the same bytes in another pitch.
//   phase A1  compass pre-test on EVERY position, in registers, two pixels per instruction: a lane owns
//             one dword (4 pixels) of a row, the even/odd bytes are two 16-bit lanes; the sign bits of
//             (centre+t - ring) and (ring - (centre-t)) are formed for the ring pixels N, S, E, W.
//             An arc of 9 contiguous ring pixels always covers N or S and E or W (see compass_pass), so a
//             pixel without a brighter pixel in each opposite pair AND without a darker one in each cannot
//             be a corner (exact reject).  Survivors are compacted into an LDS list.
//   phase A2  dense over the survivors: the FAST score itself (max over the 16 arcs of 9 of min(c-r) / min(r-c)) on packed
//             16-bit lanes (two ring pixels per v_pk_min_i16), ring bytes from the tile's pixels in LDS, only on the side whose
//             pre-test the survivor passed; a pixel is a corner iff score > threshold, so no separate mask test is needed;
//             scores go to the LDS score tile
//   phase C   3x3 strict-maximum NMS, dense over the corner list, against the LDS score tile; survivors leave as 32-bit keys
//             ((255-score)<<24 | y*w+x) with ONE global atomic per tile
constexpr int kFastWaves = 8, kFastThreads = 64 * kFastWaves;     // waves per tile: 4 position rows each
constexpr int kFastSeg = 248, kFastRows = 4 * kFastWaves - 2, kFastPosRows = kFastRows + 2, kFastRowsPerWave = 4;
constexpr int kFastPositions = kFastPosRows * (kFastSeg + 2);   // scored positions of a tile: columns 3..252 of its position rows

__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, (us2_t)(__builtin_bit_cast(us2_t, a) - __builtin_bit_cast(us2_t, b)));
}

__device__ __forceinline__ int mbcnt64(unsigned long long m) {      // number of set bits of m below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Compass pre-test on packed 16-bit lanes (pixels 0,2 of a lane's dword in "even" registers, pixels 1,3 in "odd" ones).
// Returns bit 15 of each 16-bit lane set where the pixel survives (the lower bits are not meaningful).
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(s2_t, a), __builtin_bit_cast(s2_t, b))); }
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s2_t, a), __builtin_bit_cast(s2_t, b))); }
__device__ __forceinline__ uint32_t compass_pass(uint32_t n, uint32_t s_, uint32_t e, uint32_t w, uint32_t c, uint32_t T2) {
    // Round 2: a tighter exact reject for two operations less.  The complement of an arc of 9 is an arc of 7, which cannot hold two ring
    // pixels that are 8 apart: every arc of 9 contains N or S, and E or W.  So a brighter corner needs max(N, S) > c + t AND max(E, W) > c + t
    // (a darker one min(N, S) < c - t AND min(E, W) < c - t) -- one pixel from EACH opposite pair, not any two of the four.
    // Both sides in one sign: t - max(min(max(N, S), max(E, W)) - c, c - max(min(N, S), min(E, W))) < 0.
    const uint32_t a = pk_max(n, s_), b = pk_min(n, s_), cx = pk_max(e, w), d = pk_min(e, w);
    return pk_sub(T2, pk_max(pk_sub(pk_min(a, cx), c), pk_sub(c, pk_max(b, d))));
}

// One side of the FAST score: max over the 16 arcs of 9 of min(v), on packed 16-bit lanes P[k] = (v[k], v[k+8]).  A 9-arc starting
// at k < 8 is the suffix v[k..7] of the first half plus the prefix v[8..8+k] of the second, the one starting at k+8 the mirror
// image, so running prefix / suffix minima of P (7 packed ops each) and one combine per k with the halves swapped (free operand
// select) give all 16 arc minima, and their maximum, in 29 ops.
// With v = d = centre - ring this is the "ring darker" score; with v = ~d = -d - 1 (ring - centre - 1) it is the "ring brighter"
// score minus one, because ~ reverses the order: max over arcs of min(~d) = ~(min over arcs of max(d)).
__device__ __forceinline__ int arc_score(const s2_t P[8]) {
    s2_t pmn[8], smn[8];
    pmn[0] = P[0];
    smn[7] = P[7];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        pmn[k] = __builtin_elementwise_min(pmn[k - 1], P[k]);
        smn[7 - k] = __builtin_elementwise_min(smn[8 - k], P[7 - k]);
    }
    s2_t best = __builtin_elementwise_min(smn[0], pmn[0].yx);
#pragma unroll
    for (int k = 1; k < 8; ++k) best = __builtin_elementwise_max(best, __builtin_elementwise_min(smn[k], pmn[k].yx));   // arcs starting at k (.x) and k+8 (.y)
    return max((int)best.x, (int)best.y);
}

// v_pk_mad_u16: s * r + k per 16-bit lane (modulo 2^16, so it serves signed lanes as well)
__device__ __forceinline__ s2_t pk_mad(uint32_t s, uint32_t r, uint32_t k) {
    return __builtin_bit_cast(s2_t, (us2_t)(__builtin_bit_cast(us2_t, s) * __builtin_bit_cast(us2_t, r) + __builtin_bit_cast(us2_t, k)));
}

// One step of a lane's list append: one SDWA compare copies the top bit of byte B of `m` (the survivor bit of pixel B) into VCC, lanes
// whose bit is set write a 16-bit entry at LDS byte address `at` and advance it -- STORE is ds_write_b16 for the low half of `entry`,
// ds_write_b16_d16_hi for its high half, so one register carries the entries of two pixels.  Exec is narrowed to the writers for the
// two instructions in between and restored, so unset pixels cost no select and no store.
#define FAST_LIST_APPEND(m, at, entry, B, STORE)                                                                      \
    do {                                                                                                              \
        unsigned long long saved_;                                                                                    \
        asm volatile("v_cmp_gt_i32_sdwa vcc, 0, sext(%[mm]) src0_sel:DWORD src1_sel:BYTE_" #B "\n\t"                 \
                     "s_and_saveexec_b64 %[sv], vcc\n\t"                                                              \
                     STORE " %[a], %[e]\n\t"                                                                         \
                     "v_add_u32 %[a], 2, %[a]\n\t"                                                                    \
                     "s_mov_b64 exec, %[sv]"                                                                          \
                     : [a] "+v"(at), [sv] "=&s"(saved_)                                                               \
                     : [mm] "v"(m), [e] "v"(entry)                                                                    \
                     : "vcc", "memory");                                                                              \
    } while (0)

// One tile in the lane layout S (fast_tiles.h): a wave's 64 dword-lanes are S sub-rows of LW = 64 / S lanes, group g = S wave + lane / LW owns
// position rows 4g .. 4g+3 of the tile and a lane the dword column cl = lane mod LW.  S = 1 is the wide tile with its scalar row addresses; for
// S = 2 and 4 (the narrow remainder columns of a level) the row index is per lane and every wave takes the clamped border loads.
template <int S, bool PRUNE>
__device__ __forceinline__ void fast_tile(const FrameSrc &src, uint32_t *__restrict__ cand, int32_t *__restrict__ cand_count, uint32_t *score_hist, const TileLevels &TL,
                                          const TileLevel &G, const int l, const int X0, const int Y0,
                                          uint8_t *s_sc, uint16_t *s_pre, uint8_t *s_pix, int *s_np, int *s_m, int *s_base, int *s_thr) {
    constexpr int LW = 64 / S, TW = 256 / S;                   // lanes and bytes of a tile row
    constexpr int kOutRows = kFastPosRows * S - 2;             // 30, 62 or 126 output rows
    uint32_t *s_out = reinterpret_cast<uint32_t *>(s_pix);              // (rows + 6) * LW keys >= (TW - 8) / 2 * (rows / 2) possible NMS survivors
    const int f = PRUNE ? blockIdx.x : blockIdx.y, w = G.w, h = G.h;
    const int pitch = l == 0 ? src.lvl0_pitch : G.pitch;
    const uint8_t *img = l == 0 ? src.lvl0 + (uint64_t)f * src.lvl0_frame_stride : src.slab + (uint64_t)f * TL.slab_stride + G.img_off;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform, in an SGPR: row addresses stay scalar
    const int cl = S == 1 ? lane : (lane & (LW - 1));          // the lane's dword column
    const int grp = S == 1 ? wave : S * wave + lane / LW;      // its group of 4 position rows (wave-uniform for S = 1)
    // The level's score histogram (see k_fast) is requested by wave 0 in front of its rows (the last wave has the six extra rows to fetch): one 16-byte
    // load per lane, 4 bins each, past the CU's L1 (sc1), so what other tiles have added during this launch is seen.
    uint32_t *hbin = PRUNE ? score_hist + ((size_t)(f * TL.levels + l) << 8) : nullptr;
    u32x4_t hq = {0u, 0u, 0u, 0u};
    if (PRUNE && wave == 0) hq = __builtin_amdgcn_raw_buffer_load_b128(__builtin_amdgcn_make_buffer_rsrc(hbin, 0, 1024, 0x00020000), 16 * lane, 0, 16 /* sc1 */);
    // The wave's 10 image rows are requested FIRST, so their latency runs under the LDS clear and the barrier.
    const int x = X0 - 4 + 4 * cl;
    uint32_t rows[kFastRowsPerWave + 6];
    const int yw = Y0 - 1 + grp * kFastRowsPerWave;
    if (S == 1 && __ballot(!(x >= 0 && x + 3 < w)) == 0 && yw >= 3 && yw + kFastRowsPerWave + 2 < h) {     // whole wave inside the image: plain dword loads, one uniform branch
        const uint8_t *rp = img + (int64_t)(yw - 3) * pitch;
#pragma unroll
        for (int r = 0; r < kFastRowsPerWave + 6; ++r) { rows[r] = *reinterpret_cast<const uint32_t *>(rp + x); rp += pitch; }
    } else {
        // a wave on the image border: still ONE dword load per row and lane (a third of all waves are such waves; per-byte loads with
        // their branches made them cost three times an interior wave).  The address is clamped into the row, a lane that straddles the
        // right edge shifts its pixels down, pixels outside the image are zero.
        const int xa = min(max(x, 0), w - 4);
        const uint32_t sh = (uint32_t)(8 * (x - xa)) & 31u, keep = (x >= 0 && x < w) ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (int r = 0; r < kFastRowsPerWave + 6; ++r)
            rows[r] = (reinterpret_cast<const U32u *>(img + (uint64_t)min(max(yw - 3 + r, 0), h - 1) * pitch + xa)->v >> sh) & keep;
    }
    if (tid == 0) { *s_np = 0; *s_m = 0; }
    for (int i = tid; i < kFastPosRows * 256 / 4; i += kFastThreads) reinterpret_cast<uint32_t *>(s_sc)[i] = 0;
    // the rows go to LDS as well: group g owns tile rows 4g .. 4g+3 (image rows Y0-4+4g ..), the last group also the six below
#pragma unroll
    for (int r = 0; r < kFastRowsPerWave + 6; ++r)
        if (r < kFastRowsPerWave || grp == kFastWaves * S - 1) reinterpret_cast<uint32_t *>(s_pix)[(grp * kFastRowsPerWave + r) * LW + cl] = rows[r];
    // The tile's threshold: sigma = the largest s >= threshold with at least sel_k known candidates of score > s, else the configured threshold.
    // n(s) = sum of the bins above s falls with s, so the lanes whose FIRST bin still has n >= sel_k are a prefix of the wave and the last of them
    // holds sigma among its four bins.
    if (PRUNE && wave == 0) {
        const int K = G.sel_k;
        const int incl = wave_scan_add((int)(hq.x + hq.y + hq.z + hq.w));
        const int n3 = __builtin_amdgcn_readlane(incl, 63) - incl, n2 = n3 + (int)hq.w, n1 = n2 + (int)hq.z, n0 = n1 + (int)hq.y;     // n(4 lane + i)
        const unsigned long long reach = __ballot(n0 >= K);
        const int top = reach ? 63 - __clzll((long long)reach) : 0;
        const int sigma = 4 * lane + (n3 >= K ? 3 : n2 >= K ? 2 : n1 >= K ? 1 : 0);
        if (lane == top) *s_thr = (reach && K > 0) ? max(TL.fast_threshold, sigma) : TL.fast_threshold;
    }
    __syncthreads();
    const int thr = PRUNE ? __builtin_amdgcn_readfirstlane(*s_thr) : TL.fast_threshold;
    // ---- phase A1: position rows pr = 4 grp .. 4 grp + 3  <->  image rows Y0-1+pr; columns X0-4+4*cl .. +3
    {
        const uint32_t T2 = (uint32_t)thr * 0x00010001u;
        // which of the lane's 4 pixels are valid positions (the same for every row): bit 8i + 7 for pixel i.  Column c = 4 cl + i in
        // [3, TW - 4] and image column x + i in [3, w - 4] (x = X0 - 4 + 4 cl) is one run lo <= i <= hi whose ends are a scalar minus 4 cl
        const int lo = min(max(max(3, 7 - X0) - 4 * cl, 0), 4), hi = min(max(min(TW - 4, w - X0) - 4 * cl, -1), 3);
        const uint32_t vmask = (uint32_t)(0x80808080ull << (8 * lo)) & (uint32_t)(0x80808080ull >> (8 * (3 - hi)));
        // every loaded row split ONCE into its even / odd bytes as 16-bit lanes: a row serves as S, centre and N of three position rows
        uint32_t re[kFastRowsPerWave + 6], ro[kFastRowsPerWave + 6];
#pragma unroll
        for (int j = 0; j < kFastRowsPerWave + 6; ++j) { re[j] = rows[j] & 0x00FF00FFu; ro[j] = __builtin_amdgcn_perm(0u, rows[j], 0x0C030C01u); }
        uint32_t fr[kFastRowsPerWave];                   // survivors of row r: the top bit of byte i <-> pixel i
        uint32_t cnt4 = 0;                               // their number, row r in byte r (the rows r of a wave have at most 250, 2 x 122 or 4 x 58 positions, so sums over lanes stay in the byte)
#pragma unroll
        for (int r = 0; r < kFastRowsPerWave; ++r) {
            const int y = yw + r;
            fr[r] = 0;
            if (S == 1 && (y < 3 || y >= h - 3)) continue;               // wave-uniform
            const uint32_t ce = re[r + 3], co = ro[r + 3];
            // the neighbour lanes' halves by DPP wave shifts (one VALU op each); the first / last lane of a sub-row gets a don't-care (lanes 0 / 63, or
            // a lane of the neighbouring sub-row): their edge pixels are masked by vmask, and columns 3 and TW - 4 take both E and W from their own lane or an inner one
            const uint32_t cep = wave_from_prev_dc(ce), cen = wave_from_next_dc(ce), cop = wave_from_prev_dc(co), con = wave_from_next_dc(co);
            // even pixels x, x+2: (+3,0) = x+3, x+5 = odd byte 3 of this lane, odd byte 1 of the next; (-3,0) = x-3, x-1 = the previous lane's odd bytes
            const uint32_t pe = compass_pass(re[r + 6], re[r], __builtin_amdgcn_alignbit(con, co, 16), cop, ce, T2);
            // odd pixels x+1, x+3: (+3,0) = x+4, x+6 = the next lane's even bytes; (-3,0) = x-2, x = even byte 2 of the previous lane, even byte 0 of this one
            const uint32_t po = compass_pass(ro[r + 6], ro[r], cen, __builtin_amdgcn_alignbit(ce, cep, 16), co, T2);
            fr[r] = __builtin_amdgcn_perm(po, pe, 0x07030501u) & vmask;  // the sign bytes of the four pixels side by side (pixel i in byte i)
            if (S != 1) fr[r] = (y < 3 || y >= h - 3) ? 0u : fr[r];      // the row is per lane here: masked, not branched
            cnt4 += (uint32_t)__popc(fr[r]) << (8 * r);
        }
        // ONE list append per wave, in the order row by row, lane by lane (neighbouring list slots = neighbouring pixels of a row, which
        // keeps the ring reads of phase A2 off each other's LDS banks): a single DPP scan of the packed per-row counts gives every lane
        // its offset inside each row, the row totals come out of lane 63, one lane adds their sum to the tile's counter.
        const uint32_t incl = (uint32_t)wave_scan_add((int)cnt4);
        const uint32_t tot4 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63), excl = incl - cnt4;
        int base = 0;
        if (lane == 0) base = atomicAdd(s_np, (int)((tot4 & 255u) + ((tot4 >> 8) & 255u) + ((tot4 >> 16) & 255u) + (tot4 >> 24)));
        base = __builtin_amdgcn_readfirstlane(base);
        const uint32_t ebase = ((uint32_t)((grp * kFastRowsPerWave) << 8) | (uint32_t)(4 * cl)) * 0x00010001u;   // in both 16-bit halves (pr < 128: 15 bits)
        const uint32_t pre_addr = (uint32_t)(uintptr_t)s_pre;
#pragma unroll
        for (int r = 0; r < kFastRowsPerWave; ++r) {
            uint32_t at = pre_addr + 2u * ((uint32_t)base + ((excl >> (8 * r)) & 255u));      // byte address of the lane's first slot of this row
            base += (int)((tot4 >> (8 * r)) & 255u);
            const uint32_t e32 = ebase + ((uint32_t)((r << 8) + 3) | ((uint32_t)((r << 8) + 2) << 16));   // the entries of pixels 3 | 2
            const uint32_t e10 = ebase + ((uint32_t)((r << 8) + 1) | ((uint32_t)(r << 8) << 16));         // and of pixels 1 | 0
            FAST_LIST_APPEND(fr[r], at, e32, 3, "ds_write_b16");
            FAST_LIST_APPEND(fr[r], at, e32, 2, "ds_write_b16_d16_hi");
            FAST_LIST_APPEND(fr[r], at, e10, 1, "ds_write_b16");
            FAST_LIST_APPEND(fr[r], at, e10, 0, "ds_write_b16_d16_hi");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __syncthreads();
    // ---- phase A2 + B: the survivors are SCORED directly (corner <=> score > threshold), on packed 16-bit lanes:
    //      P[k] = (d[k], d[k+8]) with d = centre - ring pixel (or ~d for the other side), one arc ladder (arc_score) per side.
    //      The ring comes from the tile's pixels in LDS (17 byte reads with immediate offsets from one base): as 7 wide global loads per
    //      survivor the texture addresser had ~30 cache lines to look up per instruction.  A wave appends its corners IN PLACE, into the
    //      slots of the survivor list it has already consumed (slots 64w + kFastThreads i + j belong to wave w), so no second list is needed.
    const int np = *s_np;
    int ncw = 0;                                                         // corners of this wave so far (wave-uniform)
    for (int i = tid; i < np; i += kFastThreads) {
        const int e = s_pre[i], pr = e >> 8, c = e & 255;
        const uint8_t *q = s_pix + pr * TW + (c - 3);                    // top-left of the 7x7 box: tile row pr + 3 is the centre's
        uint32_t R[9];
        {
            const int rdx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
            const int rdy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
            R[8] = q[3 * TW + 3];
#pragma unroll
            for (int k = 0; k < 8; ++k) {                                // ring pixels k and k+8 as the two 16-bit lanes (the second byte read lands in the high half)
                us2_t v;
                v.x = q[(3 + rdy[k]) * TW + 3 + rdx[k]];
                v.y = q[(3 + rdy[k + 8]) * TW + 3 + rdx[k + 8]];
                R[k] = __builtin_bit_cast(uint32_t, v);
            }
        }
        // A corner is a corner on ONE side only: with t >= 1, an arc of 9 whose pixels are all darker than c - t overlaps every other
        // arc of 9 (9 + 9 > 16), so the "ring brighter" score is negative there, and vice versa.  And a side scores above t only where
        // its compass pre-test holds (phase A1's test, redone here on the pairs (0,+-3) = R[0] and (+-3,0) = R[4]).  So a survivor scores
        // the side it passed with ONE arc ladder; the few that passed both (0.24 % of the survivors on the benchmark's frames) and are not corners
        // on the darker-ring side score the other side as well, in a pass the wave takes only when one of its lanes needs it.
        const uint32_t cc = R[8] * 0x00010001u;
        const s2_t dv = __builtin_bit_cast(s2_t, pk_sub(cc, R[0])), dh = __builtin_bit_cast(s2_t, pk_sub(cc, R[4]));     // d = c - r, pairs (N, S) and (E, W)
        const s2_t up = __builtin_elementwise_min(__builtin_elementwise_max(dv, dv.yx), __builtin_elementwise_max(dh, dh.yx));
        const s2_t dn = __builtin_elementwise_max(__builtin_elementwise_min(dv, dv.yx), __builtin_elementwise_min(dh, dh.yx));
        const bool ring_dark = up.x > thr, ring_bright = dn.x < -thr;
        // ring darker: P = d = c - r = (-1) r + c;  ring brighter: P = ~d = r - c - 1 = r + ~c, whose ladder is the score minus one
        const uint32_t m = ring_dark ? 0u : 0xFFFFFFFFu;
        const uint32_t sgn = ring_dark ? 0xFFFFFFFFu : 0x00010001u;
        s2_t P[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) P[k] = pk_mad(sgn, R[k], cc ^ m);
        int best = arc_score(P) - (int)m;
        const bool again = ring_dark && ring_bright && best <= thr;
        if (__ballot(again) != 0) {                                     // wave-uniform
            const uint32_t cc1 = cc + 0x00010001u;
#pragma unroll
            for (int k = 0; k < 8; ++k) P[k] = __builtin_bit_cast(s2_t, pk_sub(R[k], cc1));
            const int b2 = arc_score(P) + 1;
            if (again) best = max(best, b2);
        }
        const bool corner = best > thr;
        const unsigned long long cm = __ballot(corner);
        if (corner) {
            const int slot = ncw + mbcnt64(cm);
            s_sc[pr * TW + c] = (uint8_t)best;
            s_pre[64 * wave + kFastThreads * (slot >> 6) + (slot & 63)] = (uint16_t)e;
        }
        ncw += (int)__popcll(cm);
    }
    ncw = __builtin_amdgcn_readfirstlane(ncw);          // lanes that left the loop early missed the last updates; lane 0 stays to the end
    __syncthreads();
    // ---- phase C: 3x3 strict-maximum NMS, dense over the corner list (only outputs: px X0..X0+TW-9 = columns 4..TW-5,
    //      rows Y0..Y0+kOutRows-1 = position rows 1..kOutRows; the halo corners only serve as neighbours)
    for (int i = lane; i < ncw; i += 64) {                               // every wave walks its own corner sublist
        const int e = s_pre[64 * wave + kFastThreads * (i >> 6) + (i & 63)], pr = e >> 8, c = e & 255;
        const int px = X0 - 4 + c, y = Y0 - 1 + pr;
        if (pr < 1 || pr > kOutRows || c < 4 || c > TW - 5 || px >= w || y >= h) continue;
        const uint8_t *sp = s_sc + pr * TW + c;
        const int sc = sp[0];
        const bool keep = sc > sp[-TW - 1] && sc > sp[-TW] && sc > sp[-TW + 1] && sc > sp[-1] &&
                          sc > sp[1] && sc > sp[TW - 1] && sc > sp[TW] && sc > sp[TW + 1];
        if (keep) {
            s_out[atomicAdd(s_m, 1)] = ((uint32_t)(255 - sc) << 24) | (uint32_t)(y * w + px);
            if (PRUNE) (void)__hip_atomic_fetch_add(hbin + sc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // result unused: no return value to wait for
        }
    }
    __syncthreads();
    const int m = *s_m;
    if (m == 0) return;
    if (tid == 0) *s_base = atomicAdd(&cand_count[f * TL.levels + l], m);
    __syncthreads();
    for (int i = tid; i < m; i += kFastThreads) {
        const int pos = *s_base + i;
        if (pos < G.cand_cap) cand[(uint64_t)f * TL.cand_stride + G.cand_off + pos] = s_out[i];
    }
}

//
// The threshold a tile works with is raised by what the launch has already found.  k_select looks at the sel_k strongest
// candidates of a (frame, level) only, and keys order by score first: once sel_k candidates of score > sigma are known, no candidate of score
// <= sigma can be selected, so a tile may run ALL of FAST with max(threshold, sigma).  Every candidate above it is still found, and its NMS
// outcome is the same (only a strictly greater neighbour suppresses it, and that one is above the raised threshold too); ties at the cut are
// safe because the count is of STRICTLY greater scores.  The known candidates are a histogram of 256 score bins per (frame, level): phase C adds
// every candidate it appends (the tile's own outputs inside the image, never the halo), k_select zeroes the bins when it consumes the level,
// nothing is carried from one call to the next.  Bins only grow during a launch, so a stale or torn read is a lower bound of every bin and gives
// a sigma that is merely smaller: still exact.  The grid runs the frame as its FASTEST dimension: a frame's tiles then start one after another
// (about resident workgroups / frames at a time), and later tiles see what earlier ones found.
// PRUNE = false is the kernel without any of this, in the tile-fastest launch shape: a launch whose workgroups (nearly) all start together has nothing to
// learn from -- a single frame, a few frames -- and must not pay for the bin load, the scan, the atomics and k_select's zeroing (frame by frame, eight
// sequences side by side, they cost 12 % of the frame rate).  The host's rule (orb_enqueue_kernels): prune when the launch has more than kFastPruneMinBlocks
// workgroups.
template <bool PRUNE>
__global__ __launch_bounds__(kFastThreads) void k_fast(FrameSrc src, uint32_t *__restrict__ cand, int32_t *__restrict__ cand_count, uint32_t *score_hist,
                                              const uint2 *__restrict__ tile_tab, TileLevels TL) {
    __shared__ __attribute__((aligned(16))) uint8_t s_sc[kFastPosRows * 256];        // score tile, [32 S][256 / S] (the outermost two columns are never touched)
    __shared__ __attribute__((aligned(16))) uint16_t s_pre[kFastPositions + 8];     // compass survivors (+ dump slot); each wave's corners overwrite its own consumed slots
    __shared__ __attribute__((aligned(16))) uint8_t s_pix[(kFastPosRows + 6) * 256]; // the tile's pixels, [32 S + 6][256 / S] (image rows Y0-4 ..) for the ring reads; NMS keys afterwards
    __shared__ int s_np, s_m, s_base, s_thr;
    // The scalar unit is shared by the CU's four SIMDs and every wave of a tile repeats the tile's scalar work, so that work is kept
    // short: the tile's level, layout and first output column / row come from a host-built table (one scalar load instead of a 15-step
    // search and a division), and the ten row addresses of an interior wave are one 64-bit base plus the pitch (2 scalar adds per row
    // instead of two clamps, a 64-bit multiply and an add).
    const uint2 te = tile_tab[PRUNE ? blockIdx.y : blockIdx.x];             // level | S << 4,  X0 | Y0 << 16
    const int l = (int)(te.x & 15u), X0 = (int)(te.y & 0xFFFFu), Y0 = (int)(te.y >> 16);
    const TileLevel G = TL.L[l];                       // one batch of loads; everything below is arithmetic on it
    const uint32_t S = te.x >> 4;
    if (S == 1u) fast_tile<1, PRUNE>(src, cand, cand_count, score_hist, TL, G, l, X0, Y0, s_sc, s_pre, s_pix, &s_np, &s_m, &s_base, &s_thr);         // one wave-uniform branch
    else if (S == 2u) fast_tile<2, PRUNE>(src, cand, cand_count, score_hist, TL, G, l, X0, Y0, s_sc, s_pre, s_pix, &s_np, &s_m, &s_base, &s_thr);
    else fast_tile<4, PRUNE>(src, cand, cand_count, score_hist, TL, G, l, X0, Y0, s_sc, s_pre, s_pix, &s_np, &s_m, &s_base, &s_thr);
}

// ------------------------------------------------------------------------------------------------
// D1 selection: per (frame, level) keep the `quota` smallest keys (= strongest corners, ties by raster
// index), sort them, then apply the 19 px border filter of feature_detector.cpp:106-123 and the camera
// validity mask (dropInvalidKeypoints, orb_extractor.cpp:221-237) with an ORDERED compaction.
// Radix select (4 x 8 bits, LDS histogram) -> LDS bitonic sort of <= 4096 keys.  Deterministic:
// the unordered candidate list only feeds order-insensitive steps.
// With a minimum distance (gfttMinDistance scaled per level, feature_detector.cpp:79-82) the best
// min(4*quota, 4096) corners are sorted and the sequential "keep a corner unless a kept one is closer than
// min_dist" walk is solved as a parallel fixed point: corners are hashed into an LDS grid (cell >= min_dist), a
// corner is rejected as soon as an earlier kept neighbour exists and kept once all its earlier neighbours are
// decided -- the unique fixed point is exactly the greedy result; the first `quota` kept corners are output.
constexpr int kGridCells = 8192;

// NTH: threads per block.  256 for a batch (thousands of blocks); 1024 when only a few frames are in flight -- a level's candidates are then walked by ONE block
// five times (four radix passes and the gather), and a single 720p frame's level 0 has tens of thousands of them: 54 us of a frame's 143 us with 256 threads.
template <bool SPACED, int NTH>   // SPACED: some level has a minimum keypoint distance (uses 66 KB more LDS for the grid)
__global__ __launch_bounds__(NTH) void k_select(const PyrGeom *g, const uint32_t *__restrict__ cand, int32_t *__restrict__ cand_count,
                                                const uint8_t *__restrict__ valid_mask,
                                                int16_t *__restrict__ det_x, int16_t *__restrict__ det_y, uint8_t *__restrict__ det_score,
                                                int32_t *__restrict__ det_count, uint32_t *__restrict__ score_hist, int32_t *__restrict__ last_count) {
    __shared__ uint32_t s_key[kMaxQuota];
    __shared__ int s_hist[256];
    __shared__ int s_cnt, s_digit, s_k, s_run, s_kept, s_open;
    __shared__ int s_w1[4], s_w2[4];
    __shared__ uint8_t s_state[SPACED ? kMaxQuota : 1];          // 0 undecided, 1 kept, 2 rejected
    const int l = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const LevelGeom &G = g->L[l];
    const uint32_t *keys = cand + (uint64_t)f * g->cand_stride + G.cand_off;
    const int n_found = cand_count[f * g->levels + l];
    const int n = min(n_found, G.cand_cap), n4 = n >> 2;
    const uint4 *keys4 = reinterpret_cast<const uint4 *>(keys);          // (every level's list starts 16-byte aligned: cand_cap is a multiple of 4)
    const int quota = G.quota, min_dist = G.min_dist;
    const bool spaced = SPACED && min_dist >= 2;
    const int want = spaced ? min(4 * quota, kMaxQuota) : quota;      // how many of the strongest corners are sorted
    uint32_t kth = 0xFFFFFFFFu;
    if (n > want && want > 0) {
        uint32_t prefix = 0, mask = 0;
        if (tid == 0) s_k = want;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            // one block walks a level's list, and a block's memory parallelism is what its waves keep in flight: 16-byte loads, two per thread (a
            // dword per lane and trip moved ~20 GB/s: 14 us per pass over a 720p frame's level 0)
            for (int i = tid; i < n4; i += 2 * NTH) {
                const uint4 q0 = keys4[i], q1 = i + NTH < n4 ? keys4[i + NTH] : uint4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
                const uint32_t kk[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                const int lim = i + NTH < n4 ? 8 : 4;
#pragma unroll
                for (int u = 0; u < 8; ++u) if (u < lim && (kk[u] & mask) == prefix) atomicAdd(&s_hist[(kk[u] >> shift) & 255], 1);
            }
            for (int i = 4 * n4 + tid; i < n; i += NTH) { const uint32_t k = keys[i]; if ((k & mask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255], 1); }
            __syncthreads();
            // the digit of the k-th smallest key: the first bin whose running count reaches k.  (One thread walking the 256 bins was ~10 us per pass --
            // a chain of dependent LDS reads -- and four passes of it were most of a single frame's 44 us in this kernel.)
            {
                const int kk = s_k;
                int h = tid < 256 ? s_hist[tid] : 0, c = h;                  // inclusive running count over the bins: wave scan, then the waves' totals
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(c, off, 64); if ((tid & 63) >= off) c += v; }
                if ((tid & 63) == 63 && tid < 256) s_w1[tid >> 6] = c;
                __syncthreads();
                if (tid < 256) {
                    for (int w = 0; w < (tid >> 6); ++w) c += s_w1[w];
                    const bool last = tid == 255;                            // (k never exceeds the total: the last bin takes what is left, like the walk did)
                    if ((c >= kk || last) && c - h < kk) { s_digit = tid; s_k = kk - (c - h); }
                }
            }
            __syncthreads();
            prefix |= (uint32_t)s_digit << shift;
            mask |= 255u << shift;
            __syncthreads();
        }
        kth = prefix;
    }
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    if (want > 0)
    {
        for (int i = tid; i < n4; i += 2 * NTH) {
            const uint4 q0 = keys4[i], q1 = i + NTH < n4 ? keys4[i + NTH] : uint4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            const uint32_t kk[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
            const int lim = i + NTH < n4 ? 8 : 4;
#pragma unroll
            for (int u = 0; u < 8; ++u) if (u < lim && kk[u] <= kth) { const int p = atomicAdd(&s_cnt, 1); if (p < kMaxQuota) s_key[p] = kk[u]; }
        }
        for (int i = 4 * n4 + tid; i < n; i += NTH) { const uint32_t k = keys[i]; if (k <= kth) { const int p = atomicAdd(&s_cnt, 1); if (p < kMaxQuota) s_key[p] = k; } }
    }
    __syncthreads();
    const int m = min(s_cnt, kMaxQuota);
    int np2 = 1;
    while (np2 < m) np2 <<= 1;
    for (int i = m + tid; i < np2; i += NTH) s_key[i] = 0xFFFFFFFFu;
    __syncthreads();
    // bitonic sort.  A compare-exchange distance below 64 keeps both partners inside one wave's 64 consecutive elements (of every NTH-strided round), so
    // those steps only need the wave's own LDS order; the block meets after the steps at distance >= 64 and before the next stage starts with one
    // (45 steps for 512 keys, 6 block barriers instead of 45: a single frame's level is ONE block, and its barriers were most of its time)
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += NTH) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const uint32_t a = s_key[i], b = s_key[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { s_key[i] = b; s_key[ixj] = a; }
                }
            }
            if (j >= 64 || (j == 1 && k >= 64)) __syncthreads();
            else { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
        }
    __syncthreads();
    // minimum-distance walk as a fixed point
    if constexpr (SPACED) if (spaced) {
        __shared__ int16_t s_x[kMaxQuota], s_y[kMaxQuota], s_next[kMaxQuota];
        __shared__ int s_head[kGridCells];
        int cell = min_dist;
        while (((G.w + cell - 1) / cell) * ((G.h + cell - 1) / cell) > kGridCells) ++cell;
        const int gw = (G.w + cell - 1) / cell, gh = (G.h + cell - 1) / cell;
        for (int i = tid; i < gw * gh; i += NTH) s_head[i] = -1;
        __syncthreads();
        for (int i = tid; i < m; i += NTH) {
            const int idx = (int)(s_key[i] & 0xFFFFFFu), y = idx / G.w, x = idx - y * G.w;
            s_x[i] = (int16_t)x; s_y[i] = (int16_t)y; s_state[i] = 0;
        }
        __syncthreads();
        for (int i = tid; i < m; i += NTH)                      // cell lists (their internal order does not matter)
            s_next[i] = (int16_t)atomicExch(&s_head[(s_y[i] / cell) * gw + s_x[i] / cell], i);
        __syncthreads();
        const int d2 = min_dist * min_dist;
        for (int round = 0; round < kMaxQuota; ++round) {
            if (tid == 0) s_open = 0;
            __syncthreads();
            for (int i = tid; i < m; i += NTH) {
                if (s_state[i]) continue;
                const int x = s_x[i], y = s_y[i], cx = x / cell, cy = y / cell;
                bool rejected = false, waiting = false;
                for (int yy = max(cy - 1, 0); yy <= min(cy + 1, gh - 1) && !rejected; ++yy)
                    for (int xx = max(cx - 1, 0); xx <= min(cx + 1, gw - 1) && !rejected; ++xx)
                        for (int j = s_head[yy * gw + xx]; j >= 0; j = s_next[j]) {
                            if (j >= i) continue;                       // only corners earlier in key order matter
                            const int dx = x - s_x[j], dy = y - s_y[j];
                            if (dx * dx + dy * dy >= d2) continue;
                            const int st = s_state[j];
                            if (st == 1) { rejected = true; break; }
                            if (st == 0) waiting = true;
                        }
                if (rejected) s_state[i] = 2;
                else if (!waiting) s_state[i] = 1;
                else s_open = 1;
            }
            __syncthreads();
            const int open = s_open;
            __syncthreads();
            if (!open) break;
        }
    }
    // ordered compaction: first `quota` kept corners, then the border / validity filter
    if (tid == 0) { s_run = 0; s_kept = 0; }
    __syncthreads();
    const int W0 = g->width, H0 = g->height;
    // (the two prefix sums per chunk are over 0 / 1 flags: a ballot and two popcounts per wave, one barrier each for the waves' totals)
    const int wv = tid >> 6, ln = tid & 63;
    for (int base = 0; base < m; base += 256) {                  // chunks of 256 (threads beyond 256 only keep the barriers company)
        const int i = base + tid;
        int x = 0, y = 0, sc = 0, keep = 0;
        if (i < m && tid < 256) {
            const uint32_t k = s_key[i];
            const int idx = (int)(k & 0xFFFFFFu);
            y = idx / G.w; x = idx - y * G.w; sc = 255 - (int)(k >> 24);
            keep = spaced ? (s_state[i] == 1) : 1;
        }
        const unsigned long long bk = __ballot(keep != 0);
        if (ln == 0 && wv < 4) s_w1[wv] = __popcll(bk);
        __syncthreads();
        int incl = __popcll(bk & ((2ull << ln) - 1ull)), kept_chunk = 0;
        for (int w = 0; w < 4; ++w) { if (w < wv) incl += s_w1[w]; kept_chunk += s_w1[w]; }
        const int kept_before = s_kept, run = s_run;
        int ok = tid < 256 && keep && (kept_before + incl - 1 < quota);        // maxTracks = quota_l
        if (ok) {
            ok = x >= kPatchRadius && y >= kPatchRadius && x < G.w - kPatchRadius && y < G.h - kPatchRadius;
            if (ok && valid_mask) {
                const int mx = __float2int_rn(__fmul_rn((float)x, G.scale)), my = __float2int_rn(__fmul_rn((float)y, G.scale));
                ok = mx >= 0 && my >= 0 && mx < W0 && my < H0 && valid_mask[(uint64_t)my * W0 + mx] != 0;
            }
        }
        const unsigned long long bo = __ballot(ok != 0);
        if (ln == 0 && wv < 4) s_w2[wv] = __popcll(bo);
        __syncthreads();
        int incl2 = __popcll(bo & ((2ull << ln) - 1ull)), out_chunk = 0;
        for (int w = 0; w < 4; ++w) { if (w < wv) incl2 += s_w2[w]; out_chunk += s_w2[w]; }
        if (ok) {
            const uint64_t slot = (uint64_t)f * g->det_stride + G.det_base + run + incl2 - 1;
            det_x[slot] = (int16_t)x; det_y[slot] = (int16_t)y; det_score[slot] = (uint8_t)sc;
        }
        __syncthreads();                                         // everyone has read s_run / s_kept / the waves' totals
        if (tid == 0) { s_run = run + out_chunk; s_kept = kept_before + kept_chunk; }
        __syncthreads();
    }
    if (tid == 0) { det_count[f * g->levels + l] = s_run; last_count[f * g->levels + l] = n_found; cand_count[f * g->levels + l] = 0; }      // the list is consumed: k_fast of the next extract appends from zero (no memset launch per call)
    if (score_hist && n_found > 0 && tid < 256) score_hist[((size_t)(f * g->levels + l) << 8) + tid] = 0;       // and so are the level's score bins (k_fast's raised threshold; null when the launch did not prune): nothing is carried into the next call
}

// ------------------------------------------------------------------------------------------------
// Tracker features (orb_extractor.cpp:89-124): level lk_level, x = cvRound(pt.x/scale), margin 19,
// camera validity at (pt.x, pt.y); survivors keep their input order.  One wave per frame.
__global__ __launch_bounds__(64) void k_tracks(const PyrGeom *g, const float *__restrict__ track_xy, const int32_t *__restrict__ track_id,
                                               const int32_t *__restrict__ n_tracks, const uint8_t *__restrict__ valid_mask,
                                               int16_t *__restrict__ trk_x, int16_t *__restrict__ trk_y, float *__restrict__ trk_px,
                                               float *__restrict__ trk_py, int32_t *__restrict__ trk_id, int32_t *__restrict__ trk_count) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n = n_tracks ? min(n_tracks[f], g->max_tracks) : 0;
    const LevelGeom &G = g->L[g->lk_level];
    int run = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool ok = false; int x = 0, y = 0; float px = 0.f, py = 0.f;
        if (i < n) {
            px = track_xy[((uint64_t)f * g->max_tracks + i) * 2];
            py = track_xy[((uint64_t)f * g->max_tracks + i) * 2 + 1];
            x = __float2int_rn(__fdiv_rn(px, G.scale));
            y = __float2int_rn(__fdiv_rn(py, G.scale));
            ok = x >= kPatchRadius && y >= kPatchRadius && x < G.w - kPatchRadius && y < G.h - kPatchRadius;
            if (ok && valid_mask) {
                const int mx = __float2int_rn(px), my = __float2int_rn(py);
                ok = mx >= 0 && my >= 0 && mx < g->width && my < g->height && valid_mask[(uint64_t)my * g->width + mx] != 0;
            }
        }
        const unsigned long long bal = __ballot(ok);
        if (ok) {
            const uint64_t slot = (uint64_t)f * g->max_tracks + run + __popcll(bal & ((1ull << lane) - 1ull));
            trk_x[slot] = (int16_t)x; trk_y[slot] = (int16_t)y; trk_px[slot] = px; trk_py[slot] = py;
            trk_id[slot] = track_id ? track_id[(uint64_t)f * g->max_tracks + i] : i;
        }
        run += __popcll(bal);
    }
    if (lane == 0) trk_count[f] = run;
}

// ------------------------------------------------------------------------------------------------
// O1 + O2: one wavefront per keypoint.
//   ic_angle (orb_extractor.cpp:245-275): integer moments over the radius-15 disc of the UNBLURRED
//   level, 961 candidate offsets strided over the 64 lanes, DPP/shuffle reduction, cv::fastAtan2.
//   descriptor (orb_extractor.cpp:284-352): lane j evaluates BRIEF tests j, j+64, j+128, j+192 on the
//   BLURRED level; four 64-bit ballots are the 256 descriptor bits (test t -> word t/32, bit t%32).

// moments -> angle -> (cos, sin): describe_steer.h (plain C++, checked on the CPU by tests/describe_steer_check.cpp)

__device__ __forceinline__ int wave_sum(int v) {      // DPP inclusive scan, total broadcast from lane 63
    return __builtin_amdgcn_readlane(wave_scan_add(v), 63);
}

// Visit position -> detection, two dwords per position (x | y << 16, level | output slot << 8: coordinates up to the 32767 ms_orb_create admits), and the frame's keypoint total: k_describe's waves found their keypoint through a chain
// of dependent loads (the counts of all levels -> a 16-step search for the level -> the level's base in the geometry table -> the coordinates), ~150 scalar
// instructions and three round trips in front of the window fetch of EVERY wave.  One block per (level, frame) writes the level's run of the table once.
// SPATIAL: the level's run is visited in the order of describe_order::key instead of k_select's score order (the outputs stay in their slots).
template <bool SPATIAL>            // (a kernel of its own: the plain table needs no LDS)
__global__ __launch_bounds__(256) void k_slots(const int16_t *__restrict__ det_x, const int16_t *__restrict__ det_y, const int32_t *__restrict__ det_count,
                                               const int32_t *__restrict__ trk_count, uint2 *__restrict__ slot_tab, int32_t *__restrict__ out_count,
                                               TileLevels TL, int det_stride, int capacity) {
    __shared__ uint32_t s_key[SPATIAL ? kMaxQuota : 1];                              // a detection's key below the band (describe_order::in_band_key), grouped by band
    __shared__ uint16_t s_y[SPATIAL ? kMaxQuota : 1];
    __shared__ int s_start[SPATIAL ? describe_order::kMaxBands : 1], s_cur[SPATIAL ? describe_order::kMaxBands : 1], s_w[4];
    const int l = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    int base = trk_count[f];
    for (int k = 0; k < l; ++k) base += det_count[f * TL.levels + k];
    const int cnt = det_count[f * TL.levels + l];
    const int n = max(min(min(cnt, capacity - base), kMaxQuota), 0);       // the level's detections that have an output slot
    const uint64_t s0 = (uint64_t)f * det_stride + TL.L[l].det_base;
    uint2 *const tab = slot_tab + (uint64_t)f * capacity + base;
    // (the output slot of detection i of the level is base + i whatever position visits it)
    if constexpr (!SPATIAL) {
        for (int i = tid; i < n; i += 256) tab[i] = uint2{(uint32_t)(uint16_t)det_x[s0 + i] | ((uint32_t)(uint16_t)det_y[s0 + i] << 16), describe_order::pack(l, base + i)};
    } else {
        // Visit position of a detection = how many of the level's keys (describe_order.h: row band, x along the band, index) are smaller than its own.  The
        // band is the key's top, so that is the count of the bands above plus the count of smaller keys INSIDE its band: a histogram of the bands, its running
        // sum, the keys grouped by band (in whatever order the appends land: the keys are distinct, a rank does not depend on it), and one walk over the own
        // band's keys per detection -- n * n / bands compares for a level spread over its bands where a sort network's log^2 n steps each wait for LDS
        // (a bitonic sort of 64-bit keys here: 0.040 ms per 256 x 720p launch against 0.005 ms for the plain table; this: 0.013 ms).  A level whose detections all lie
        // in ONE band pays n * n (estimated, not measured: 4096 of them ~0.5 ms in its block; a quota of 600 ~4 us).
        for (int b = tid; b < describe_order::kMaxBands; b += 256) s_cur[b] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += 256) atomicAdd(&s_cur[min(describe_order::band_of(det_y[s0 + i] & 0x7FFF), (uint32_t)describe_order::kMaxBands - 1)], 1);
        __syncthreads();
        {   // exclusive running sum over the bands: four bands per thread, wave scan, the waves' totals
            int c[4], sum = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { c[k] = s_cur[4 * tid + k]; sum += c[k]; }
            const int incl = wave_scan_add(sum);
            if ((tid & 63) == 63) s_w[tid >> 6] = incl;
            __syncthreads();
            int at = incl - sum;
            for (int w = 0; w < (tid >> 6); ++w) at += s_w[w];
#pragma unroll
            for (int k = 0; k < 4; ++k) { s_start[4 * tid + k] = at; s_cur[4 * tid + k] = at; at += c[k]; }
        }
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
            const int x = det_x[s0 + i] & 0x7FFF, y = det_y[s0 + i] & 0x7FFF;           // (coordinates are 0 .. 32767)
            const uint32_t band = describe_order::band_of(y);
            const int p = atomicAdd(&s_cur[band], 1);                                   // < n: the bands' counts sum to n
            s_key[p] = describe_order::in_band_key(x, band, i); s_y[p] = (uint16_t)y;
        }
        __syncthreads();                                                                // s_cur[band] is now the band's end
        for (int p = tid; p < n; p += 256) {
            const uint32_t mine = s_key[p], y = s_y[p], band = describe_order::band_of((int)y);
            const int lo = s_start[band], hi = s_cur[band];
            int pos = lo;
            for (int q = lo; q < hi; ++q) pos += s_key[q] < mine;
            const int i = (int)(mine & ((1u << describe_order::kIndexBits) - 1));
            const uint32_t along = mine >> describe_order::kIndexBits, x = (band & 1u) ? (uint32_t)((1 << describe_order::kCoordBits) - 1) - along : along;
            tab[pos] = uint2{x | (y << 16), describe_order::pack(l, base + i)};
        }
    }
    if (l == TL.levels - 1 && tid == 0) out_count[f] = min(base + cnt, capacity);
}

// Keypoints per wave.  A wave of k_describe walks a STRIP of keypoints one after another (describe_strips.h: 8 in the long region of a large launch, then 4, 2 and 1;
// 1 throughout for a launch without more than two device-fulls of blocks), in the same registers and the same LDS slab, and pays once per strip what a wave of one
// keypoint paid per keypoint: the tables to LDS, the lane tables, the frame's counts, the block barrier, and the chain of dependent scalar loads slot entry ->
// level -> geometry -> frame pointers (13 s_waitcnt lgkmcnt(0), 5 vmcnt and the barrier in the 197 instructions in front of the first window load; now 31
// instructions and no wait between a keypoint's record and its window loads).  Measured on 256 x 720p (profiles/r08_a_ab_describe_strips.txt), ms per launch:
//     one keypoint per wave (the parent)         0.4376 .. 0.4437
//     long strips of 2 / 4 / 8                   0.436  / 0.4168 .. 0.4188 / 0.4394 .. 0.4416
// Longer is not better: the slots in flight at one time span r times as many frames, whose pyramids share the caches (FETCH_SIZE + 17 % at r = 4, + 24 % at
// r = 8), and that eats what the setup saves -- while the blocks of a frame are dealt to all eight L2s.  With each XCD's blocks on a contiguous run of the
// plan (describe_strips::remap; profiles/r09_a_ab_describe_order.txt) FETCH_SIZE falls to 31 % at strips of 4 and to 57 % at 8, and 8 is the fastest:
//     remap, long strips of 2 / 4 / 8            0.4320 .. 0.4329 / 0.4105 .. 0.4127 / 0.4009 .. 0.4039      (same session: without remap, 4: 0.4191 .. 0.4215)
// With the next keypoint's window fetched under the BRIEF tests of the current one (64 VGPRs, no scratch, the
// same LDS) the kernel took 0.4185 .. 0.4196 ms against 0.4168 .. 0.4188 without: not kept.
// What round 1 measured on ITS kernel (separate blurred patch, a level search per wave, 7 waves per SIMD, the blur on the vector pipe) does not carry over:
// "four one after another with the next one's patches prefetched" was 0.63 of 0.60 ms there, and of the same list the per-slot table (0.583 -> 0.542 ms)
// and the eighth wave per SIMD (0.542 -> 0.511 ms) paid once the kernel had changed.  Still on record from that round: two keypoints SIDE BY SIDE in a wave
// cost registers (100 VGPRs, 30 KB LDS, slower: DESIGN section 10); 16-byte row pieces and one scattered store for all outputs did nothing.

// A keypoint of a wave's strip as the loop wants it: everything a lane resolved in front of the loop (k_describe), read back as scalars
struct DescKp { int x, y, oct, tid_out, pitch, w, h, slot; float ox, oy; bool inner; uint64_t off; };
// The per-wave tables live in the dwords of the wave's slab that neither the window (0 .. 575, with the parked ninth piece) nor pass 1 of the
// blur (row 47's fourth 16-byte unit ends at dword 579) touches: the geometry of the 16 levels, 6 dwords each, and the strip's keypoints, 12 each
constexpr int kDescGeoDword = 584, kDescGeoStride = 6, kDescRecDword = kDescGeoDword + kDescGeoStride * MS_MAX_LEVELS, kDescRecStride = 12;
static_assert(kDescRecDword % 4 == 0 && kDescRecDword + kDescRecStride * describe_strips::kMaxStrip <= describe_lanes::kSlabDwords, "per-wave tables fit behind the window");
struct DescRec { uint4 a, b, c; };                           // a record as the lanes read it (all the same one: the address is wave-uniform)
__device__ __forceinline__ DescRec desc_read(const uint32_t *rec) {
    return DescRec{*reinterpret_cast<const uint4 *>(rec), *reinterpret_cast<const uint4 *>(rec + 4), *reinterpret_cast<const uint4 *>(rec + 8)};
}
__device__ __forceinline__ DescKp desc_scalars(const DescRec &r) {
    const uint4 a = r.a, b = r.b, c = r.c;
    auto s = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    DescKp K;
    K.x = (int)s(a.x); K.y = (int)s(a.y); K.oct = (int)(s(a.z) & 0xFFu); K.inner = (s(a.z) >> 8) != 0; K.tid_out = (int)s(a.w);
    K.ox = __uint_as_float(s(b.x)); K.oy = __uint_as_float(s(b.y)); K.pitch = (int)s(b.z); K.w = (int)s(b.w);
    K.h = (int)s(c.x); K.off = (uint64_t)s(c.y) | ((uint64_t)s(c.z) << 32); K.slot = (int)s(c.w);
    return K;
}
typedef int v4i_t __attribute__((ext_vector_type(4)));
// amdgpu_waves_per_eu(8, 8): the register allocation aims at 8 waves per SIMD (the kernel is bound by how many keypoints are in flight)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_describe(FrameSrc src, TileLevels TL, describe_strips::Plan plan, const uint4 *__restrict__ moment_tab, const float4 *__restrict__ pattern_f,
                                                  const uint2 *__restrict__ slot_tab, int capacity, int max_tracks, int lk_level, int xcd_runs,
                                                  const int16_t *__restrict__ trk_x, const int16_t *__restrict__ trk_y, const float *__restrict__ trk_px,
                                                  const float *__restrict__ trk_py, const int32_t *__restrict__ trk_id, const int32_t *__restrict__ trk_count,
                                                  float *__restrict__ out_x, float *__restrict__ out_y, float *__restrict__ out_angle,
                                                  int32_t *__restrict__ out_octave, uint32_t *__restrict__ out_desc, int32_t *__restrict__ out_track,
                                                  const int32_t *__restrict__ out_count) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // block -> (frame, first slot of the block's strips, strip length): scalar arithmetic on the plan's region records (describe_strips.h), no load.
    // xcd_runs: the blocks that the dispatcher deals to one XCD take a contiguous run of the plan's blocks, whole frames through one L2 (remap)
    const describe_strips::Strip strip = describe_strips::decode(plan, xcd_runs ? describe_strips::remap(plan, blockIdx.x) : blockIdx.x);
    const int f = strip.frame, R = min(strip.r, describe_strips::kMaxStrip);
    const int slot0 = strip.slot0 + wv;                      // the wave's first slot; its k-th keypoint is slot0 + 4 k.  Wave-uniform: everything derived from it is scalar
    // A keypoint is a chain of dependent memory round trips (its slot -> coordinates -> patch -> angle -> BRIEF samples) and the
    // everything that does not depend on the keypoint is requested up front -- the lane's patch-offset table and the counts of
    // ALL levels in one batch (not one load per loop trip).
    // What does not depend on the keypoint and is needed late -- the blur's tap operands (right before the blur) and the 256 BRIEF point pairs (after the
    // orientation) -- was fetched from global memory where it was needed, behind the LDS fences no load may cross: two exposed round trips in the middle of every
    // wave's chain, and this kernel is bound by the LENGTH of that chain (ablation: prologue + window fetch alone 0.35 of 0.60 ms, no prologue chain -0.07 ms,
    // a quarter fewer vector instructions 0.00 ms).  They are block-wide tables in LDS now, loaded first thing, under the count loads.
    __shared__ uint4 s_tab[32 + 256];                        // [0..31] horizontal taps (dt, n), [32..287] the point pairs [q][lane]
    // (every load of the prologue is issued before the first of them is waited for: the stores to LDS stand together in front of the barrier.  All four waves
    // fetch the tap table and half of wave 0 stores it -- behind a test of the thread index the load was waited for before the next one was issued)
    const uint4 tap_v = moment_tab[64 + (lane & 31)], pair_v = reinterpret_cast<const uint4 *>(pattern_f)[threadIdx.x];
    const uint4 dm = moment_tab[lane];                       // disc mask of the lane's four patch dwords
    const uint32_t dmask[4] = {dm.x, dm.y, dm.z, dm.w};
    const uint32_t wpack_w = reinterpret_cast<const uint32_t *>(moment_tab + 96)[lane];    // (row, byte) of the lane's first three window pieces (describe_lanes::win_pack)
    const uint2 vert_w = reinterpret_cast<const uint2 *>(moment_tab + 112)[lane];          // the lane's two dwords of pass 2's A operand, the vertical taps (describe_lanes::vert_operand)
    __shared__ __attribute__((aligned(16))) uint32_t s_patch[4][describe_lanes::kSlabDwords];   // a wave's slab: see below
    uint32_t *const win = &s_patch[wv][0], *const geo = win + kDescGeoDword, *const rec = win + kDescRecDword;
    // Everything a strip's keypoints need from memory is requested here, together, from addresses that depend on the block index and the kernel
    // arguments alone (one round trip in front of the barrier, none per keypoint): the frame's totals; the strip's table entries (k_slots), lane j
    // the entry of the wave's j-th keypoint (the lanes behind the strip read its last entry once more), with the tracker's fields wherever the slot CAN
    // be a tracker point (slot < max_tracks: whether it is one, slot < trk_count[f], is known only when the loads are back); and the geometry of all
    // levels, lane l that of level l, into the wave's table (a lane-indexed read of the kernel arguments).  Level 0 is entered as the other levels are:
    // its pitch, and its plane as an offset from the frame's part of the slab (a 64-bit difference; the sum below wraps back to the caller's pointer).
    const int total = out_count[f], nt = trk_count[f];
    const uint8_t *const slab_f = src.slab + (uint64_t)f * TL.slab_stride;
    const int myslot = slot0 + 4 * min(lane, R - 1);
    const uint2 ent = slot_tab[(uint64_t)f * capacity + min(myslot, capacity - 1)];
    int tx = 0, ty = 0, tid = -1;
    float tpx = 0.f, tpy = 0.f;
    if (myslot < max_tracks) {
        const uint64_t s2 = (uint64_t)f * max_tracks + myslot;
        tx = trk_x[s2]; ty = trk_y[s2]; tpx = trk_px[s2]; tpy = trk_py[s2]; tid = trk_id[s2];
    }
    const TileLevel &GL = TL.L[lane & (MS_MAX_LEVELS - 1)];
    const int g_pitch = GL.pitch, g_w = GL.w, g_h = GL.h;
    const float g_scale = GL.scale;
    const uint64_t g_off = GL.img_off;
    if (threadIdx.x < 32) s_tab[threadIdx.x] = tap_v;
    s_tab[32 + threadIdx.x] = pair_v;
    if (lane < MS_MAX_LEVELS) {
        const uint64_t off = lane == 0 ? (uint64_t)(uintptr_t)src.lvl0 + (uint64_t)f * src.lvl0_frame_stride - (uint64_t)(uintptr_t)slab_f : g_off;
        uint32_t *g = geo + kDescGeoStride * lane;
        g[0] = (uint32_t)(lane == 0 ? src.lvl0_pitch : g_pitch); g[1] = (uint32_t)g_w; g[2] = (uint32_t)g_h; g[3] = __float_as_uint(g_scale);
        g[4] = (uint32_t)off; g[5] = (uint32_t)(off >> 32);
    }
    __syncthreads();                                         // the tables are in LDS (every wave of the block is still here); the ONLY block barrier: the waves finish independently
    const int trips = describe_strips::trips(strip.slot0, wv, R, total);
    if (trips <= 0) return;                                  // a strip wholly at or beyond the frame's total
    // lane j resolves the strip's j-th keypoint -- coordinates, level, geometry, whether its window lies inside the level and where the window starts --
    // and leaves it in the wave's table: the loop reads one record per keypoint back as scalars, and a keypoint's level selects its geometry without
    // a memory load that depends on the level
    if (lane < R) {
        const bool trk = myslot < nt;
        const int level = trk ? lk_level : min(describe_order::level_of(ent.y), MS_MAX_LEVELS - 1);      // (an entry beyond the total is stale, not wild; its record is not read)
        const uint32_t *g = geo + kDescGeoStride * level;
        const int pitch = (int)g[0], w = (int)g[1], h = (int)g[2];
        const float scale = __uint_as_float(g[3]);
        const int x = trk ? tx : (int)(ent.x & 0xFFFFu), y = trk ? ty : (int)(ent.x >> 16);
        const float ox = trk ? tpx : __fmul_rn((float)x, scale), oy = trk ? tpy : __fmul_rn((float)y, scale);     // orb_extractor.cpp:156
        const bool inner = x >= 23 && x + 24 < w && y >= 22 && y + 22 < h;          // the whole window lies inside the level
        // the plane's offset in the frame's slab; for an inner keypoint the window's corner at once
        const uint64_t off = ((uint64_t)g[4] | ((uint64_t)g[5] << 32)) + (inner ? (uint64_t)((int64_t)(y - 22) * pitch + (x - 23)) : 0ull);
        uint32_t *r = rec + kDescRecStride * lane;
        *reinterpret_cast<uint4 *>(r) = uint4{(uint32_t)x, (uint32_t)y, (uint32_t)level | (inner ? 256u : 0u), (uint32_t)(trk ? tid : -1)};
        *reinterpret_cast<uint4 *>(r + 4) = uint4{__float_as_uint(ox), __float_as_uint(oy), (uint32_t)pitch, (uint32_t)w};
        *reinterpret_cast<uint4 *>(r + 8) = uint4{(uint32_t)h, (uint32_t)off, (uint32_t)(off >> 32), (uint32_t)(trk ? myslot : describe_order::slot_of(ent.y))};   // the output slot: a detection's is its table entry's (k_slots)
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    DescKp K = desc_scalars(desc_read(rec));
    // ONE window of the (unblurred) level is copied into the wave's LDS slab with coalesced row loads: 45 rows x 48 B around the keypoint
    // (x-23 .. x+24, y-22 .. y+22; 9 wave-wide dword loads).  It holds the 31 x 31 orientation patch (each lane takes four of its dwords, with everything
    // outside the radius-15 disc zeroed, into registers for the moments) AND everything the 39 x 39 BLURRED patch of the BRIEF tests depends on (19 + 3 pixels each way),
    // so the blur (image_pyramid.cpp:84: 7 x 7, sigma 2, REFLECT_101) is computed here, for the patch only, with k_blur's own arithmetic --
    // vertical pass on packed 16-bit lanes, horizontal pass with v_dot2 and one rounding -- and the blurred pyramid is no longer
    // written and read back for every frame (2 P bytes and a 0.49 ms kernel per 256-frame step; round 1 fetched 31 x 32 B of the level plus
    // 39 x 40 B of its blurred twin = 70 row pieces per keypoint, now 45).  k_blur still exists: ImagePyramid::getBlurredLevel runs it on demand.
    // The slab (s_patch, above): the window (a whole number of 16-byte units: its rows are read as ds_read_b128); the blurred patch takes its place.  The 32 x 8
    // dwords behind it held a masked copy of the orientation patch until the moments were taken from registers: pass 1 of the blur still reads window "rows" 45 .. 47
    // there (zero weights), the wave's tables lie behind those, and the slab keeps its size and bank layout.
    // The strip walk: the wave's keypoints one after another in the same registers and the same slab.  Wave-level fences only -- nothing in the loop waits for
    // another wave, and its bound (trips) depends on the kernel arguments and the frame's total alone.
    typedef __attribute__((address_space(3))) uint8_t lds_u8_t;
    const uint32_t pbase = (uint32_t)(uintptr_t)(const lds_u8_t *)win + describe_brief_index::kIndexBias;   // the blurred patch's LDS address and the index's constant in one (wave-uniform)
    const int lane_w = lane;
    // (every load of the prologue is waited for HERE, vmcnt(0): left to the loop's first use of the lane tables, the wait stands at the head of the loop and
    // there also waits for the stores of the previous keypoint)
    __builtin_amdgcn_s_waitcnt(0x0F70);
#pragma unroll 1
    for (int k = 0; k < trips; ++k) {
        // What depends on the lane alone is formed anew for every keypoint, as a wave of one keypoint formed it once: carried around the loop in registers
        // (the compiler's choice when it sees that it does not change) it costs the kernel its eighth wave per SIMD.  The empty statements hide that from it.
        int lane_k = lane_w;
        uint32_t wpack = wpack_w, vd0 = vert_w.x, vd1 = vert_w.y;
        asm volatile("" : "+v"(lane_k), "+v"(wpack), "+v"(vd0), "+v"(vd1));
        const int lane = lane_k;
        const int pitch = K.pitch, w = K.w, h = K.h, kx = K.x, ky = K.y;
        uint32_t *pb = win;                                  // (pass 1 of the blur has read the whole window into registers before pass 2 writes the first blurred dword)
        // the next keypoint's record is requested here and read back behind the window's fence, which waits for LDS anyway: from the second keypoint of a
        // strip on, no wait on scalar or vector memory stands between a keypoint's record and its window loads (the last trip reads its own record once more)
        const DescRec next = desc_read(rec + kDescRecStride * min(k + 1, trips - 1));
        if (K.inner) {                                       // wave-uniform: the whole window lies inside the level
            // piece t = 3 a + b is window dword lane + 64 t: the dword column of piece b, 16 a rows further down (describe_lanes.h).  Three lane offsets from
            // the packed table (all >= 0: the uniform part of each address is the minimum of what the piece reads, §11 of DESIGN.md), three uniform row bases.
            // The last piece exists for lanes 0 .. 27 only; the others fetch the first dword of its row base once more and park it behind the window (dwords
            // 540 .. 575 of the slab, which nothing reads as data), so that all nine loads are in flight together: behind a lane test the ninth load was
            // issued only after the first eight had returned -- one more round trip in every keypoint's chain.
            const uint8_t *corner = slab_f + K.off;   // (the record of an inner keypoint holds its window's corner)
            uint32_t off[3];
#pragma unroll
            for (int b = 0; b < 3; ++b) off[b] = __umul24((wpack >> (10 * b)) & 15u, (uint32_t)pitch) + ((wpack >> (10 * b + 4)) & 63u);
#pragma unroll
            for (int t = 0; t < describe_lanes::kWinPieces; ++t) {
                const uint8_t *rows = corner + (uint32_t)(16 * (t / 3)) * (uint32_t)pitch;
                win[lane + 64 * t] = reinterpret_cast<const U32u *>(rows + (describe_lanes::win_active(lane, t) ? off[t % 3] : 0u))->v;
            }
        } else {                                                          // a keypoint within 24 pixels of the border (a few per cent): BORDER_REFLECT_101 byte by byte
            const uint8_t *img = slab_f + K.off;
#pragma unroll 1
            for (int t = 0; t < 9; ++t) {
                const int i = lane + 64 * t, r = i / 12, c = i - 12 * r;
                if (i >= 45 * 12) break;
                const uint8_t *row = img + (int64_t)reflect101(ky - 22 + r, h) * pitch;
                uint32_t v = 0;
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) v |= (uint32_t)row[reflect101(kx - 23 + 4 * c + bb, w)] << (8 * bb);
                win[i] = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const DescKp Kn = desc_scalars(next);
        int m10, m01;
        {   // orientation patch: rows y-15 .. y+15 = window rows 7 .., columns x-15 .. = window dword 2 ..; everything outside the radius-15 disc zeroed (the mask of
            // the 32nd row is zero).  Patch dword lane + 64 t is 8 window rows below dword lane + 64 (t - 1): one lane base, four reads at constant offsets.
            // O1: moments m10 = sum u I, m01 = sum v I over the disc (orb_extractor.cpp:245-275; integer sums, any order) on the lane's own four masked dwords,
            // straight from the registers (describe_lanes::lane_moments: v_sad_u8 / v_dot4_u32_u8); the wave sums run under the blur's matrix products.
            const uint32_t *ob = win + describe_lanes::ori_base(lane);
            uint32_t d[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) d[t] = (describe_lanes::ori_active(lane, t) ? ob[8 * describe_lanes::kWinDwords * t] : 0u) & dmask[t];
            int p10, p01;
            describe_lanes::lane_moments(d, describe_lanes::moment_col_weights(lane), describe_lanes::moment_row_bias(lane), p10, p01);
            m10 = wave_sum(p10); m01 = wave_sum(p01);
        }
        {   // blurred patch rows y-19 .. y+19 (output row ro <- window rows ro .. ro+6), columns x-19 .. x+19 = window bytes 4 .. 42, ON THE MATRIX CORES (round 3):
            // a separable 7-tap filter is two products with banded constant matrices, out = V (P Hh), and every quantity of k_blur's fixed-point arithmetic is an
            // integer that i8 operands with i32 accumulators carry exactly.
            //   pass 1   T' = (P - 128) Hh: A = window rows as they lie in LDS (lane (i, kg): row 16 m + i, bytes 16 kg .. + 15, one ds_read_b128, xor 0x80 = -128
            //            as signed bytes; the bytes past column 47 and the rows past 44 meet zero weights), B = the taps by column (host table).  T' = T - 32768 fits 16 bits
            //   between  T' leaves the accumulators as its high and low bytes (4 v_perm per tile for both planes); the C layout holds 4 consecutive ROWS of a column per
            //            lane -- and so does a B operand, up to the order of its K index.  No lane exchanges anything: the lane's three dwords of a byte plane ARE
            //            its B operand of pass 2, {d[0], d[1], d[2], 0}, with K byte 16 q + 4 m + r standing for T' row 16 m + 4 q + r (describe_lanes.h)
            //   pass 2   out = V T' as 256 x (high bytes) + (low bytes - 128): A = the vertical taps in the same K order, two dwords per lane from the host's table at
            //            dword positions yt and yt + 1; two chained products per 16 x 16 tile (the first starts from 33024 = (rounding + the offsets' share) / 256,
            //            is shifted up by 8 and becomes the second's C), byte 2 of each sum is the blurred pixel; the C layout holds 4 consecutive pixels of a
            //            COLUMN per lane = one dword of the patch, which is stored column-major (39 columns of 40 bytes; the BRIEF index swaps its arguments)
            // 27 v_mfma_i32_16x16x64_i8 + ~155 vector instructions per keypoint (~195 with the transposes of the A form), where the packed-16-bit form (k_blur's, 60 lanes x 8 rows) took ~350: the kernel sits at
            // the VALU issue limit and the matrix pipe was idle.
            const int n = lane & 15, q = lane >> 4;
            // B operands of pass 1, tile t: lane (n, kg) holds rows 16 kg .. + 15 of column 16 t + n -- non-zero only for kg - t = 0 or 1, and for columns <= 38
            // -- entry lane - 16 t of the table, or the table's all-zero entry: the lane selects the index, not the four dwords (describe_lanes::tap_slot)
            auto taps = [&](int t) { return __builtin_bit_cast(v4i_t, s_tab[describe_lanes::tap_slot(lane, t)]); };
            v4i_t Aw[3];                                     // the window rows as pass 1's A operands (read BEFORE the first blurred dword takes the window's place)
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                uint4 a4 = *reinterpret_cast<const uint4 *>(win + (16 * m + n) * 12 + 4 * q);
                a4.x ^= 0x80808080u; a4.y ^= 0x80808080u; a4.z ^= 0x80808080u; a4.w ^= 0x80808080u;
                Aw[m] = __builtin_bit_cast(v4i_t, a4);
            }
            const int d0 = (int)vd0, d1 = (int)vd1;
            const v4i_t Va[3] = {{d0, d1, 0, 0}, {0, d0, d1, 0}, {0, 0, d0, d1}};     // the vertical taps of row tiles 0 .. 2 (in the last, d1 meets B's zero dword)
            // one column tile at a time (pass 1 -> bytes -> pass 2 -> store): the three tiles' intermediates side by side cost the kernel its eighth wave per SIMD
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const v4i_t Hb = taps(t), zero = {0, 0, 0, 0};
                uint32_t hd[3], ld[3];
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const v4i_t T = __builtin_amdgcn_mfma_i32_16x16x64_i8(Aw[m], Hb, zero, 0, 0, 0);
                    const uint32_t x01 = __builtin_amdgcn_perm((uint32_t)T[1], (uint32_t)T[0], 0x04000501u);      // [r0.b1, r1.b1, r0.b0, r1.b0]
                    const uint32_t x23 = __builtin_amdgcn_perm((uint32_t)T[3], (uint32_t)T[2], 0x04000501u);
                    hd[m] = __builtin_amdgcn_perm(x23, x01, 0x05040100u);
                    ld[m] = __builtin_amdgcn_perm(x23, x01, 0x07060302u) ^ 0x80808080u;
                }
                const v4i_t B2h = {(int)hd[0], (int)hd[1], (int)hd[2], 0}, B2l = {(int)ld[0], (int)ld[1], (int)ld[2], 0};   // K bytes 12 .. 15 of a group = T' rows 48 .. 63: zero data
#pragma unroll
                for (int yt = 0; yt < 3; ++yt) {
                    // (33024 + the high sums) << 8 with the start value behind the product, in the shift's own instruction (v_lshl_add_u32): the first product
                    // starts from the inline zero, and no four registers hold the constant
                    v4i_t acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(Va[yt], B2h, zero, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] = (int)(((uint32_t)acc[r] << 8) + (33024u << 8));
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(Va[yt], B2l, acc, 0, 0, 0);
                    if (describe_lanes::blur_store_valid(lane, t, yt))      // lane (n, q): rows 16 yt + 4 q .. + 3 of patch column 16 t + n (byte 2 of each sum; the sums stay below 2^24)
                        pb[describe_lanes::blur_store_dword(lane, t, yt)] = __builtin_amdgcn_perm((uint32_t)acc[1], (uint32_t)acc[0], 0x0C0C0602u) | __builtin_amdgcn_perm((uint32_t)acc[3], (uint32_t)acc[2], 0x06020C0Cu);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const float angle_deg = describe_steer::fast_atan2((float)m01, (float)m10);
        const float angle = describe_steer::deg_to_rad(angle_deg);
        // sin(v) is cos(pi / 2 - v): lane 1 evaluates the shifted argument while lane 0 evaluates v, one cos_approx for both; every lane reads the two
        // results back as scalars
        const float cs = describe_steer::cos_approx(lane == 1 ? describe_steer::sin_argument(angle) : angle);
        const float ca = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cs), 0));
        const float sa = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cs), 1));
        // the column is x cos - y sin = x cos + y (-sin), the same float bit for bit (a product's sign is exact): with the sign turned once per keypoint, row and
        // column of a point are the same two multiplies and one add, and the compiler packs each step of the pair into one v_pk_*_f32.  The empty statement
        // keeps it from folding the negation back into a subtraction.
        float nsa = -sa;
        asm volatile("" : "+s"(nsa));
        // O2: steered BRIEF on the blurred patch
        unsigned long long bits[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 pt = __builtin_bit_cast(float4, s_tab[32 + q * 64 + lane]);             // the test's two points, already float
            const float x1 = pt.x, y1 = pt.y, x2 = pt.z, y2 = pt.w;
            // rows and columns + 19 lie in 0 .. 38 (the pattern stays inside the 39 x 39 patch under every rotation).  The products and the add / sub are the
            // reference's, one rounding each; rounding to the integer is one more float add, and the conversion, both + 19 and the patch's LDS address are one
            // constant behind one 24-bit multiply-add (describe_brief_index.h: 6 instructions per point where v_rndne + v_cvt per coordinate made it 11)
            const uint32_t r1 = describe_brief_index::round_bits(__fadd_rn(__fmul_rn(x1, sa), __fmul_rn(y1, ca)));
            const uint32_t c1 = describe_brief_index::round_bits(__fadd_rn(__fmul_rn(x1, ca), __fmul_rn(y1, nsa)));
            const uint32_t r2 = describe_brief_index::round_bits(__fadd_rn(__fmul_rn(x2, sa), __fmul_rn(y2, ca)));
            const uint32_t c2 = describe_brief_index::round_bits(__fadd_rn(__fmul_rn(x2, ca), __fmul_rn(y2, nsa)));
            const uint32_t i1 = describe_brief_index::index_from_bits(c1, r1, pbase), i2 = describe_brief_index::index_from_bits(c2, r2, pbase);     // (column, row): the patch is column-major
            bits[q] = __ballot(*(const lds_u8_t *)(uintptr_t)i1 < *(const lds_u8_t *)(uintptr_t)i2);
        }
        const uint64_t o = (uint64_t)f * capacity + K.slot;        // (slot0 + 4 k is the VISIT position)
        if (lane < 8) out_desc[o * 8 + lane] = (uint32_t)(bits[lane >> 1] >> ((lane & 1) * 32));
        if (lane == 0) { out_x[o] = K.ox; out_y[o] = K.oy; out_angle[o] = angle_deg; out_octave[o] = K.oct; out_track[o] = K.tid_out; }
        // the last BRIEF read of the patch has been consumed (the ballots): the next keypoint's window may take the slab
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        K = Kn;
    }
}

}  // namespace

// =================================================================================================
// host side of the extractor
// =================================================================================================
struct ms_orb {
    ms_ctx *ctx = nullptr;
    ms_orb_config cfg{};
    PyrGeom geom{};
    TileMap blur_tiles{};
    TileLevels tile_levels{};          // per-level geometry of the tiled kernels, passed by value
    // the device block and the pointers into it, one d_<name> per array of orb_geom.h's lists (a per-level one is null where the level has no such table)
    uint8_t *d_block = nullptr;
#define ORB_X_MEMBER(T, name, n) T *d_##name = nullptr;
#define ORB_XL_MEMBER(T, name, n) T *d_##name[MS_MAX_LEVELS] = {nullptr};
    ORB_BLOCK_CONSTANTS(ORB_X_MEMBER, ORB_XL_MEMBER)
    ORB_BLOCK_WORK(ORB_X_MEMBER)
#undef ORB_X_MEMBER
#undef ORB_XL_MEMBER
    size_t cand_count_bytes = 0, score_hist_bytes = 0;
    uint8_t *d_mask = nullptr;         // ms_orb_set_valid_mask: an allocation of its own, it comes and goes
    bool wide[MS_MAX_LEVELS] = {false};
    int resize_px = 0, resize_map = 0;                // ms_orb_set_resize_plan: 0 = automatic
    int describe_order = describe_order::kDefaultMode;   // bit 0: XCD-contiguous blocks (describe_strips::remap), bit 1: spatial visit order (k_slots) (ms_orb_set_describe_order)
    int describe_strip = 0;                   // k_describe: 0 = the automatic launch plan (describe_strips.h), 1 .. 8 = every wave walks that many keypoints (ms_orb_set_describe_strip)
    // optional per-stage HIP events (ms_orb_set_profiling)
    bool profiling = false;
    bool blur_valid = false;           // the blurred planes of the slab hold the last batch (k_blur runs on demand only)
    // a ring of kProfRing event sets: a profiled call records into the next one, so the stage times of the last kProfRing calls can be read
    // after a run of calls -- without a host wait between them (ms_orb_stage_ms_back)
    static constexpr int kProfRing = 128;
    hipEvent_t evr[kProfRing][MS_ORB_STAGES + 1] = {{nullptr}};
    hipEvent_t *ev = evr[0];           // the set of the current / last profiled call
    long long prof_calls = 0;
    // host frames come in as up to kChunks pieces on a stream of their own: piece k+1 is copied while the kernels of piece k run
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copied[4] = {nullptr}, ev_free[4] = {nullptr}, ev_end = nullptr;
    int chunked_frames = 0;            // n_frames of the last chunked call (its ev_free[] mark the pieces of exactly that split); 0 = none
    bool end_recorded = false;
    // level 0's k_fast beside the resize chain (orb_enqueue_kernels): on a side stream between a fork and a join event of the context stream
    int ftiles_level0 = 0;             // the first entries of d_ftile_tab are level 0's
    int fast_overlap = 0;              // ms_orb_set_fast_overlap: 0 = automatic, 1 = never, 2 = always
    int fast_launches = 0, fast_pruning = 0;   // k_fast launches of the last call, and how many of them were k_fast<true> (ms_orb_last_fast_launches)
    hipStream_t side_stream = nullptr; // exists where max_batch can reach the automatic rule, or once mode 2 was asked for: the copy stream where the
    bool side_owned = false;           // extractor has one (idle in the calls that split automatically), else a stream of its own
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // state of the last call
    FrameSrc last_src{};
    int last_frames = 0;
    bool lvl0_in_slab = false;
    uint64_t lvl0_off = 0;
    int lvl0_pitch = 0;
};

#define MS_TRY(x) do { int rc__ = (x); if (rc__ != MS_OK) return rc__; } while (0)

// KeyPoint::serialize (key_point.hpp:22-25): ar(pt.x, pt.y, angle, octave, octave, bearing, descriptor) -- 19 dwords per keypoint
// (x, y, angle f32; octave i32 twice; bearing 3 x f64; descriptor 8 x u32).  Thread = one dword of one record: coalesced stores.
__global__ __launch_bounds__(256) void k_pack_keypoints(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ angle,
                                                       const int32_t *__restrict__ octave, const uint32_t *__restrict__ desc, const double *__restrict__ bearing,
                                                       uint64_t base, int n, uint32_t *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 19) return;
    const int k = i / 19, w = i - 19 * k;
    const uint64_t s = base + (uint64_t)k;
    uint32_t v;
    if (w == 0) v = __float_as_uint(x[s]);
    else if (w == 1) v = __float_as_uint(y[s]);
    else if (w == 2) v = __float_as_uint(angle[s]);
    else if (w < 5) v = (uint32_t)octave[s];
    else if (w < 11) v = bearing ? reinterpret_cast<const uint32_t *>(bearing)[6 * (uint64_t)k + (w - 5)] : 0u;
    else v = desc[s * 8 + (w - 11)];
    out[i] = v;
}

// lays the device block out, allocates it, points the handle's d_<name> into it, uploads the constants in one copy and zeroes the rest
static int orb_take_block(ms_orb *o, const OrbGeom &R, const OrbTables &C) {
    ms_ctx *c = o->ctx;
    const OrbBlock K = orb_block_layout(o->cfg, R, C);
    MS_HIP(c, hipMalloc(reinterpret_cast<void **>(&o->d_block), K.end));
#define ORB_X_BIND(T, name, n) o->d_##name = K.name.at(o->d_block);
#define ORB_XL_BIND(T, name, n) for (int l = 0; l < MS_MAX_LEVELS; ++l) o->d_##name[l] = K.name[l].count ? K.name[l].at(o->d_block) : nullptr;
    ORB_BLOCK_CONSTANTS(ORB_X_BIND, ORB_XL_BIND)
    ORB_BLOCK_WORK(ORB_X_BIND)
#undef ORB_X_BIND
#undef ORB_XL_BIND
    o->cand_count_bytes = K.cand_count.bytes(); o->score_hist_bytes = K.score_hist.bytes();
    std::vector<uint8_t> stage;
    orb_stage_constants(K, R, C, stage);
    MS_HIP(c, hipMemcpyAsync(o->d_block, stage.data(), K.const_end, hipMemcpyHostToDevice, c->stream));
    MS_HIP(c, hipMemsetAsync(o->d_block + K.const_end, 0, K.end - K.const_end, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));          // `stage` goes out of scope
    return MS_OK;
}

// the side stream of level 0's k_fast with its fork and join events
static int orb_create_side_stream(ms_orb *o) {
    ms_ctx *c = o->ctx;
    if (o->side_stream) return MS_OK;
    if (!o->ev_fork) MS_HIP(c, hipEventCreateWithFlags(&o->ev_fork, hipEventDisableTiming));
    if (!o->ev_join) MS_HIP(c, hipEventCreateWithFlags(&o->ev_join, hipEventDisableTiming));
    // The copy stream does the job where there is one: automatic mode never splits the pieces of a batch of host frames, so that stream is idle in every
    // call that does.  A stream more per extractor is not free: with one merely EXISTING beside the copy stream (the step itself did not split) the
    // bench's PCIe-inclusive step, which keeps four streams busy, went from 4.4 to 5.5 ms with four hardware queues and to 5.1 with eight
    // (DESIGN section 10); with the copy stream in its place it stays where it was.
    // Default priority: at the lowest one (hipDeviceGetStreamPriorityRange) detection fills in behind the resize blocks and overlaps less -- measured,
    // +1.8 % on the 256-frame step against +2.2 %.
    if (o->copy_stream) { o->side_stream = o->copy_stream; return MS_OK; }
    MS_HIP(c, hipStreamCreateWithFlags(&o->side_stream, hipStreamNonBlocking));      // last: the stream exists only with both its events
    o->side_owned = true;
    return MS_OK;
}

// the copy stream and its events (batches of host frames only; a one-frame extractor never uses them), and the side stream where a call can be
// large enough for the split k_fast
static int orb_create_streams(ms_orb *o) {
    ms_ctx *c = o->ctx;
    MS_HIP(c, hipEventCreateWithFlags(&o->ev_end, hipEventDisableTiming));
    if (o->cfg.max_batch >= 32) {
        MS_HIP(c, hipStreamCreateWithFlags(&o->copy_stream, hipStreamNonBlocking));
        for (int i = 0; i < 4; ++i) {
            MS_HIP(c, hipEventCreateWithFlags(&o->ev_copied[i], hipEventDisableTiming));
            MS_HIP(c, hipEventCreateWithFlags(&o->ev_free[i], hipEventDisableTiming));
        }
    }
    if (orb_fast_split_auto(o->cfg.max_batch, o->ftiles_level0, o->geom.ftiles_total)) MS_TRY(orb_create_side_stream(o));
    return MS_OK;
}

extern "C" {

int ms_orb_create(ms_ctx *ctx, const ms_orb_config *cfg, ms_orb **out) {
    if (!ctx || !cfg || !out) return MS_ERR_INVALID;
    *out = nullptr;
    // on the host, nothing allocated: the geometry (which is also the check of the configuration) and the constant tables
    OrbGeom R;
    char why[256];
    const int bad = orb_geometry(*cfg, R, why, sizeof(why));
    if (bad != MS_OK) return ms_fail(ctx, bad, "ms_orb_create: %s", why);
    OrbTables C;
    orb_tables(R.geom, C);
    MS_HIP(ctx, hipSetDevice(ctx->device));
    ms_orb *o = new ms_orb();
    o->ctx = ctx;
    o->cfg = *cfg;
    o->geom = R.geom; o->tile_levels = R.tile_levels; o->blur_tiles = R.blur_tiles;
    o->lvl0_off = R.lvl0_off; o->lvl0_pitch = R.lvl0_pitch; o->ftiles_level0 = R.ftiles_level0;
    for (int l = 1; l < cfg->levels; ++l) o->wide[l] = C.level[l].wide;
    // from here on one way out: ms_orb_destroy takes whatever exists
    if (orb_take_block(o, R, C) != MS_OK) { ms_orb_destroy(o); return ms_fail(ctx, MS_ERR_HIP, "ms_orb_create: device allocation failed"); }
    if (orb_create_streams(o) != MS_OK) { ms_orb_destroy(o); return ms_fail(ctx, MS_ERR_HIP, "ms_orb_create: stream / event creation failed"); }
    *out = o;
    return MS_OK;
}

void ms_orb_destroy(ms_orb *o) {
    if (!o) return;
    (void)hipSetDevice(o->ctx->device);
    (void)hipStreamSynchronize(o->ctx->stream);
    if (o->d_block) (void)hipFree(o->d_block);
    if (o->d_mask) (void)hipFree(o->d_mask);
    for (auto &set : o->evr) for (int i = 0; i <= MS_ORB_STAGES; ++i) if (set[i]) (void)hipEventDestroy(set[i]);
    if (o->copy_stream) { (void)hipStreamSynchronize(o->copy_stream); (void)hipStreamDestroy(o->copy_stream); }
    for (int i = 0; i < 4; ++i) { if (o->ev_copied[i]) (void)hipEventDestroy(o->ev_copied[i]); if (o->ev_free[i]) (void)hipEventDestroy(o->ev_free[i]); }
    if (o->ev_end) (void)hipEventDestroy(o->ev_end);
    if (o->side_owned) { (void)hipStreamSynchronize(o->side_stream); (void)hipStreamDestroy(o->side_stream); }
    if (o->ev_fork) (void)hipEventDestroy(o->ev_fork);
    if (o->ev_join) (void)hipEventDestroy(o->ev_join);
    delete o;
}

int ms_orb_capacity(const ms_orb *o) { return o ? o->geom.capacity : MS_ERR_INVALID; }

int ms_orb_set_describe_strip(ms_orb *o, int r) {
    if (!o || r < 0 || r > describe_strips::kMaxStrip) return MS_ERR_INVALID;
    o->describe_strip = r;
    return MS_OK;
}

int ms_orb_set_resize_plan(ms_orb *o, int px, int map) {
    if (!o || (px != 0 && px != 4 && px != 8) || map < resize_plan::kMapAuto || map > resize_plan::kMapByFrame) return MS_ERR_INVALID;
    o->resize_px = px; o->resize_map = map;
    return MS_OK;
}

int ms_orb_set_describe_order(ms_orb *o, int mode) {
    if (!o || mode < 0 || (mode & ~describe_order::kModeMask)) return MS_ERR_INVALID;
    o->describe_order = mode;
    return MS_OK;
}

int ms_orb_set_fast_overlap(ms_orb *o, int mode) {
    if (!o || mode < 0 || mode > 2) return MS_ERR_INVALID;
    if (mode == 2 && o->geom.levels > 1) {          // a small extractor has no side stream yet
        MS_HIP(o->ctx, hipSetDevice(o->ctx->device));
        MS_TRY(orb_create_side_stream(o));
    }
    o->fast_overlap = mode;
    return MS_OK;
}

int ms_orb_set_profiling(ms_orb *o, int enable) {
    if (!o) return MS_ERR_INVALID;
    ms_ctx *c = o->ctx;
    if (enable && !o->evr[0][0])
        for (auto &set : o->evr) for (int i = 0; i <= MS_ORB_STAGES; ++i) MS_HIP(c, hipEventCreate(&set[i]));
    o->profiling = enable != 0;
    return MS_OK;
}

int ms_orb_stage_ms_back(ms_orb *o, int calls_back, float *ms) {
    if (!o || !ms || calls_back < 0 || calls_back >= ms_orb::kProfRing) return MS_ERR_INVALID;
    ms_ctx *c = o->ctx;
    if (!o->evr[0][0] || calls_back >= o->prof_calls) return ms_fail(c, MS_ERR_INVALID, "ms_orb_stage_ms_back: no profiled call %d calls back", calls_back);
    hipEvent_t *set = o->evr[(o->prof_calls - 1 - calls_back) % ms_orb::kProfRing];
    MS_HIP(c, hipEventSynchronize(set[MS_ORB_STAGES]));
    for (int i = 0; i < MS_ORB_STAGES; ++i) MS_HIP(c, hipEventElapsedTime(&ms[i], set[i], set[i + 1]));
    return MS_OK;
}

int ms_orb_stage_ms(ms_orb *o, float *ms) {
    if (!o || !ms) return MS_ERR_INVALID;
    ms_ctx *c = o->ctx;
    if (!o->profiling || o->last_frames == 0) return ms_fail(c, MS_ERR_INVALID, "ms_orb_stage_ms: profiling is off or nothing ran");
    MS_HIP(c, hipEventSynchronize(o->ev[MS_ORB_STAGES]));
    for (int i = 0; i < MS_ORB_STAGES; ++i) MS_HIP(c, hipEventElapsedTime(&ms[i], o->ev[i], o->ev[i + 1]));
    return MS_OK;
}

int ms_orb_set_valid_mask(ms_orb *o, const uint8_t *mask) {
    if (!o) return MS_ERR_INVALID;
    ms_ctx *c = o->ctx;
    MS_HIP(c, hipStreamSynchronize(c->stream));
    if (!mask) { if (o->d_mask) { MS_HIP(c, hipFree(o->d_mask)); o->d_mask = nullptr; } return MS_OK; }
    const size_t n = (size_t)o->cfg.width * o->cfg.height;
    if (!o->d_mask) MS_HIP(c, hipMalloc(reinterpret_cast<void **>(&o->d_mask), n));
    MS_HIP(c, hipMemcpy(o->d_mask, mask, n, hipMemcpyHostToDevice));
    return MS_OK;
}

static int orb_extract_enqueue(ms_orb *o, const uint8_t *images, int on_device, int n_frames, size_t frame_stride, size_t row_stride,
                               const float *track_xy, const int32_t *track_id, const int32_t *n_tracks, bool &counters_dirty);

int ms_orb_extract(ms_orb *o, const uint8_t *images, int on_device, int n_frames, size_t frame_stride, size_t row_stride,
                   const float *track_xy, const int32_t *track_id, const int32_t *n_tracks) {
    if (!o || !images) return MS_ERR_INVALID;
    bool counters_dirty = false;
    const int rc = orb_extract_enqueue(o, images, on_device, n_frames, frame_stride, row_stride, track_xy, track_id, n_tracks, counters_dirty);
    // k_fast fills the candidate counters and k_select puts them back to zero; a call that fails in between must not leave them to the next one
    if (rc != MS_OK && counters_dirty) {
        if (o->side_stream) {           // a part-launch of k_fast may still be appending on the side stream
            (void)hipEventRecord(o->ev_join, o->side_stream);
            (void)hipStreamWaitEvent(o->ctx->stream, o->ev_join, 0);
        }
        (void)hipMemsetAsync(o->d_cand_count, 0, o->cand_count_bytes, o->ctx->stream);
        (void)hipMemsetAsync(o->d_score_hist, 0, o->score_hist_bytes, o->ctx->stream);
    }
    return rc;
}

// the kernels of one extract over frames [f0, f0 + nf) of the batch: every per-frame array is linear in the frame index, so a piece of the batch
// is the same launches on offset pointers (in_pieces: this is such a piece, its frames copied from the host on the copy stream)
static int orb_enqueue_kernels(ms_orb *o, FrameSrc src, int f0, int nf, bool have_tracks, bool have_ids, bool in_pieces, bool &counters_dirty) {
    ms_ctx *c = o->ctx;
    const PyrGeom &G = o->geom;
    hipStream_t st = c->stream;
    const size_t F = (size_t)f0, T = (size_t)o->cfg.max_tracks, L = (size_t)G.levels;
    src.lvl0 += F * src.lvl0_frame_stride; src.slab += F * G.slab_stride;
    uint32_t *cand = o->d_cand + F * G.cand_stride;
    int32_t *cand_count = o->d_cand_count + F * L, *det_count = o->d_det_count + F * L, *trk_count = o->d_trk_count + F, *last_count = o->d_last_count + F * L;
    // k_fast learns a raised threshold from its own launch only where a frame's tiles run at different times: with more workgroups than twice what the
    // device holds at once (4 per CU on 256 CUs).  Below that (nearly) all tiles start before any has finished; they run the plain kernel, tile-fastest.
    const bool prune = (long long)nf * G.ftiles_total > kFastPruneMinBlocks;
    uint32_t *score_hist = prune ? o->d_score_hist + F * L * 256 : nullptr;
    // Level 0 is the caller's image and needs no resized level, and k_fast is bound by vector issue where the resize chain waits on memory: a call
    // large enough runs level 0's tiles (the first ftiles_level0 entries of the tile table) on the side stream beside the resizes, the other levels'
    // behind them on the context stream, and joins the two in front of k_select.  Both parts are the same instantiation on the same lists, counters
    // and bins: the lists are unordered and the raised threshold is exact whatever a tile has seen (k_fast).  A piece of a batch of host frames
    // (in_pieces) keeps the single launch unless the split is forced: its kernels already run beside the next piece's copy, the step is bound by the
    // copies, and the side stream is the copy stream, which has the next piece's frames to carry.
    const int tiles0 = o->ftiles_level0, tiles1 = G.ftiles_total - tiles0;
    const bool split = o->side_stream && tiles1 > 0 && o->fast_overlap != 1 &&
                       (o->fast_overlap == 2 || (!in_pieces && orb_fast_split_auto(nf, tiles0, G.ftiles_total)));
    auto launch_fast = [&](hipStream_t s, int tile0, int tiles) {
        ++o->fast_launches; o->fast_pruning += prune;
        if (prune) hipLaunchKernelGGL(k_fast<true>, dim3(nf, tiles), dim3(kFastThreads), 0, s, src, cand, cand_count, score_hist, o->d_ftile_tab + tile0, o->tile_levels);     // frame fastest: see k_fast
        else hipLaunchKernelGGL(k_fast<false>, dim3(tiles, nf), dim3(kFastThreads), 0, s, src, cand, cand_count, score_hist, o->d_ftile_tab + tile0, o->tile_levels);
    };
    int16_t *det_x = o->d_det_x + F * G.det_stride, *det_y = o->d_det_y + F * G.det_stride;
    uint8_t *det_score = o->d_det_score + F * G.det_stride;
    int stage = 0;
    if (o->profiling) { o->ev = o->evr[o->prof_calls % ms_orb::kProfRing]; ++o->prof_calls; }
#define MS_STAGE_MARK() do { if (o->profiling) MS_HIP(c, hipEventRecord(o->ev[stage++], st)); } while (0)
    MS_STAGE_MARK();
    if (split) {
        // the fork lies behind all that must precede the call on the context stream: the previous call's kernels (its k_select and k_describe read
        // what this launch writes), k_copy_level0, a piece's wait for its copy.  The stage marks stay on the context stream: with the split the
        // `resize` interval holds level 0's detection and `fast` the other levels plus the join.
        MS_HIP(c, hipEventRecord(o->ev_fork, st));
        MS_HIP(c, hipStreamWaitEvent(o->side_stream, o->ev_fork, 0));
        counters_dirty = true;
        launch_fast(o->side_stream, 0, tiles0);
        MS_KERNEL_CHECK(c, "k_fast");
        MS_HIP(c, hipEventRecord(o->ev_join, o->side_stream));
    }
    MsRange pyramid_range("pyramid");
    for (int l = 1; l < G.levels; ++l) {
        dim3 grid(ms_div_up(G.L[l].w, 256), ms_div_up(G.L[l].h, 4 * kResizeRows), nf);
        const ResizeTab RT{o->d_xtab[l], o->d_ytab[l]};
        ResizeArgs RA{};
        if (l == 1) { RA.src = src.lvl0; RA.src_frame_stride = src.lvl0_frame_stride; RA.src_pitch = src.lvl0_pitch; }
        else { RA.src = src.slab + G.L[l - 1].img_off; RA.src_frame_stride = G.slab_stride; RA.src_pitch = G.L[l - 1].pitch; }
        RA.sw = G.L[l - 1].w; RA.sh = G.L[l - 1].h;
        RA.dst = src.slab + G.L[l].img_off; RA.dst_frame_stride = G.slab_stride; RA.dst_pitch = G.L[l].pitch; RA.dw = G.L[l].w; RA.dh = G.L[l].h;
        // the 8-pixel kernel on the levels whose tables allow it, for launches that fill the device (a frame or a few: the 4-pixel kernel, resize_plan.h)
        const resize_plan::Launch P = resize_plan::launch(RA.dw, RA.dh, nf, o->resize_map);
        if (o->d_xtab8[l] && (o->resize_px == 8 || (o->resize_px == 0 && resize_plan::fills_device(P))))
            hipLaunchKernelGGL(k_resize8, dim3(P.grid_x, P.grid_y, P.grid_z), dim3(256), 0, st, RA, Resize8Tab{o->d_xtab8[l], o->d_ytab[l]}, P);
        else if (o->wide[l]) hipLaunchKernelGGL(k_resize<true>, grid, dim3(256), 0, st, RA, RT);
        else hipLaunchKernelGGL(k_resize<false>, grid, dim3(256), 0, st, RA, RT);
        MS_KERNEL_CHECK(c, "k_resize");
    }
    pyramid_range.end();
    MS_STAGE_MARK();
    // The blurred pyramid (image_pyramid.cpp:82-85) is not materialised per frame any more: its only consumer on the path, the BRIEF tests,
    // blurs its own 39 x 39 patches inside k_describe.  ImagePyramid::getBlurredLevel (ms_orb_download_level) runs k_blur on demand.
    o->blur_valid = false;
    MS_STAGE_MARK();
    MsRange detect_range("detect");
    counters_dirty = true;
    if (split) launch_fast(st, tiles0, tiles1); else launch_fast(st, 0, G.ftiles_total);
    MS_KERNEL_CHECK(c, "k_fast");
    if (split) MS_HIP(c, hipStreamWaitEvent(st, o->ev_join, 0));      // k_select consumes both parts' lists
    MS_STAGE_MARK();
    const bool few = nf * G.levels <= 64;                           // a frame or a handful: one block per level is the whole launch -- give it 1024 threads
    if (o->cfg.min_distance > 0.f) {
        if (few) hipLaunchKernelGGL((k_select<true, 1024>), dim3(G.levels, nf), dim3(1024), 0, st, o->d_geom, cand, cand_count, o->d_mask, det_x, det_y, det_score, det_count, score_hist, last_count);
        else hipLaunchKernelGGL((k_select<true, 256>), dim3(G.levels, nf), dim3(256), 0, st, o->d_geom, cand, cand_count, o->d_mask, det_x, det_y, det_score, det_count, score_hist, last_count);
    } else {
        if (few) hipLaunchKernelGGL((k_select<false, 1024>), dim3(G.levels, nf), dim3(1024), 0, st, o->d_geom, cand, cand_count, o->d_mask, det_x, det_y, det_score, det_count, score_hist, last_count);
        else hipLaunchKernelGGL((k_select<false, 256>), dim3(G.levels, nf), dim3(256), 0, st, o->d_geom, cand, cand_count, o->d_mask, det_x, det_y, det_score, det_count, score_hist, last_count);
    }
    MS_KERNEL_CHECK(c, "k_select");
    counters_dirty = false;
    MS_STAGE_MARK();
    if (o->cfg.max_tracks > 0) {                                    // (an extractor built without tracker features: d_trk_count stays at its initial zero)
        hipLaunchKernelGGL(k_tracks, dim3(nf), dim3(64), 0, st, o->d_geom, have_tracks ? o->d_track_xy + F * T * 2 : nullptr,
                           (have_tracks && have_ids) ? o->d_track_id + F * T : nullptr, have_tracks ? o->d_n_tracks + F : nullptr, o->d_mask,
                           o->d_trk_x + F * T, o->d_trk_y + F * T, o->d_trk_px + F * T, o->d_trk_py + F * T, o->d_trk_id + F * T, trk_count);
        MS_KERNEL_CHECK(c, "k_tracks");
    }
    MS_STAGE_MARK();
    detect_range.end();
    MsRange describe_range("describe");
    const size_t C = (size_t)G.capacity;
    if (o->describe_order & describe_order::kSpatial)
        hipLaunchKernelGGL(k_slots<true>, dim3(G.levels, nf), dim3(256), 0, st, det_x, det_y, det_count, trk_count, o->d_slot_tab + F * C, o->d_count + F, o->tile_levels, G.det_stride, G.capacity);
    else
        hipLaunchKernelGGL(k_slots<false>, dim3(G.levels, nf), dim3(256), 0, st, det_x, det_y, det_count, trk_count, o->d_slot_tab + F * C, o->d_count + F, o->tile_levels, G.det_stride, G.capacity);
    MS_KERNEL_CHECK(c, "k_slots");
    // which block describes which slots: long strips first, a tail of one-keypoint blocks twice what the device holds at once (8 blocks per CU); a launch
    // without more blocks than that tail -- a single frame, the frame-by-frame legs -- is one keypoint per wave throughout
    describe_strips::Plan plan;
    if (!describe_strips::build(nf, G.capacity, 8ll * std::max(c->n_cu, 1), o->describe_strip, plan)) return ms_fail(c, MS_ERR_CAPACITY, "k_describe: %d frames of %d slots exceed the grid", nf, G.capacity);
    hipLaunchKernelGGL(k_describe, dim3(plan.blocks), dim3(256), 0, st, src, o->tile_levels, plan, o->d_moment_tab, o->d_pattern_f,
                       o->d_slot_tab + F * C, G.capacity, G.max_tracks, G.lk_level, o->describe_order & describe_order::kRemap, o->d_trk_x + F * T, o->d_trk_y + F * T, o->d_trk_px + F * T, o->d_trk_py + F * T, o->d_trk_id + F * T, trk_count, o->d_x + F * C, o->d_y + F * C,
                       o->d_angle + F * C, o->d_octave + F * C, o->d_desc + F * C * 8, o->d_track + F * C, o->d_count + F);
    MS_KERNEL_CHECK(c, "k_describe");
    MS_STAGE_MARK();
#undef MS_STAGE_MARK
    return MS_OK;
}

static int orb_extract_enqueue(ms_orb *o, const uint8_t *images, int on_device, int n_frames, size_t frame_stride, size_t row_stride,
                               const float *track_xy, const int32_t *track_id, const int32_t *n_tracks, bool &counters_dirty) {
    ms_ctx *c = o->ctx;
    const PyrGeom &G = o->geom;
    if (n_frames < 1 || n_frames > o->cfg.max_batch) return ms_fail(c, MS_ERR_CAPACITY, "ms_orb_extract: n_frames %d outside [1,%d]", n_frames, o->cfg.max_batch);
    if (row_stride < (size_t)G.width || frame_stride < row_stride * (size_t)(G.height - 1) + G.width)
        return ms_fail(c, MS_ERR_INVALID, "ms_orb_extract: strides smaller than the frame");
    MS_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    o->fast_launches = o->fast_pruning = 0;
    MS_TRY(ms_ctx_order_after_downloads(c));               // asynchronous downloads of the previous outputs (ms_dev_download_async) finish before they are overwritten
    FrameSrc src{};
    src.slab = o->d_slab;
    const bool have_tracks = track_xy && n_tracks && o->cfg.max_tracks > 0;
    if (have_tracks) {
        const size_t T = o->cfg.max_tracks;
        MS_HIP(c, hipMemcpyAsync(o->d_track_xy, track_xy, (size_t)n_frames * T * 2 * sizeof(float), hipMemcpyHostToDevice, st));
        MS_HIP(c, hipMemcpyAsync(o->d_n_tracks, n_tracks, (size_t)n_frames * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (track_id) MS_HIP(c, hipMemcpyAsync(o->d_track_id, track_id, (size_t)n_frames * T * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    // (d_cand_count is zero here: allocated zeroed, and k_select puts every counter it has consumed back to zero)
    const bool aligned = on_device && (reinterpret_cast<uintptr_t>(images) % 16 == 0) && (row_stride % 16 == 0) && (frame_stride % 16 == 0);
    if (aligned) {   // use the caller's frames in place as pyramid level 0 (image_pyramid.cpp:75 without the copy)
        src.lvl0 = images; src.lvl0_frame_stride = frame_stride; src.lvl0_pitch = (int)row_stride;
        o->lvl0_in_slab = false;
        MS_TRY(orb_enqueue_kernels(o, src, 0, n_frames, have_tracks, track_id != nullptr, false, counters_dirty));
    } else {
        uint8_t *dst = o->d_slab + o->lvl0_off;
        src.lvl0 = dst; src.lvl0_frame_stride = G.slab_stride; src.lvl0_pitch = o->lvl0_pitch;
        o->lvl0_in_slab = true;
        // frames whose rows are as far apart on the host as in the slab move as whole frames: one linear copy each, or ONE 2-D copy for a run of frames
        // ("rows" = whole frames, host pitch = frame_stride, slab pitch = slab_stride) -- 256 x 21 us of per-frame copies were 5.4 ms of a 9.7 ms step
        const bool whole = row_stride == (size_t)o->lvl0_pitch;
        const size_t frame_bytes = row_stride * (size_t)(G.height - 1) + G.width;
        auto copy_frames = [&](int f0, int nf, hipStream_t cs) -> int {
            if (whole && nf > 1) {
                MS_HIP(c, hipMemcpy2DAsync(dst + (size_t)f0 * G.slab_stride, G.slab_stride, images + (size_t)f0 * frame_stride, frame_stride, frame_bytes, nf, hipMemcpyHostToDevice, cs));
            } else {
                for (int f = f0; f < f0 + nf; ++f) {
                    if (whole) MS_HIP(c, hipMemcpyAsync(dst + (size_t)f * G.slab_stride, images + (size_t)f * frame_stride, frame_bytes, hipMemcpyHostToDevice, cs));
                    else MS_HIP(c, hipMemcpy2DAsync(dst + (size_t)f * G.slab_stride, o->lvl0_pitch, images + (size_t)f * frame_stride, row_stride, G.width, G.height, hipMemcpyHostToDevice, cs));
                }
            }
            return MS_OK;
        };
        const int kChunks = 4;
        const bool chunked = !on_device && !o->profiling && n_frames >= 8 * kChunks && o->copy_stream != nullptr;
        if (on_device) {
            dim3 grid(ms_div_up(G.width, 256), G.height, n_frames);
            hipLaunchKernelGGL(k_copy_level0, grid, dim3(256), 0, st, images, (uint64_t)frame_stride, (uint64_t)row_stride, o->d_slab,
                               G.slab_stride, o->lvl0_off, G.width, G.height, o->lvl0_pitch);
            MS_KERNEL_CHECK(c, "k_copy_level0");
            MS_TRY(orb_enqueue_kernels(o, src, 0, n_frames, have_tracks, track_id != nullptr, false, counters_dirty));
        } else if (!chunked) {
            MS_TRY(copy_frames(0, n_frames, st));
            MS_TRY(orb_enqueue_kernels(o, src, 0, n_frames, have_tracks, track_id != nullptr, false, counters_dirty));
        } else {
            // Piece k's kernels run under piece k+1's copy (the copy engine and the CUs work side by side; the design rule: copies on a stream of their own).
            // A piece of the slab may be overwritten once the PREVIOUS call's kernels on it are done: its ev_free when that call was split the same way,
            // else the end of that call.  With pinned host memory the call returns after enqueueing; pageable memory is staged by the runtime (correct, no overlap).
            const int per = ms_div_up(n_frames, kChunks);
            const bool same_split = o->chunked_frames == n_frames;      // (0 unless the LAST call was split: any other call resets it)
            if (!same_split && o->end_recorded) MS_HIP(c, hipStreamWaitEvent(o->copy_stream, o->ev_end, 0));
            for (int k = 0; k < kChunks; ++k) {
                const int f0 = k * per, nf = std::min(per, n_frames - f0);
                if (nf <= 0) break;
                if (same_split) MS_HIP(c, hipStreamWaitEvent(o->copy_stream, o->ev_free[k], 0));
                MS_TRY(copy_frames(f0, nf, o->copy_stream));
                MS_HIP(c, hipEventRecord(o->ev_copied[k], o->copy_stream));
                MS_HIP(c, hipStreamWaitEvent(st, o->ev_copied[k], 0));
                MS_TRY(orb_enqueue_kernels(o, src, f0, nf, have_tracks, track_id != nullptr, true, counters_dirty));
                MS_HIP(c, hipEventRecord(o->ev_free[k], st));
            }
            o->chunked_frames = n_frames;
        }
        if (!chunked) o->chunked_frames = 0;
    }
    if (aligned) o->chunked_frames = 0;
    if (o->ev_end) { MS_HIP(c, hipEventRecord(o->ev_end, st)); o->end_recorded = true; }
    o->last_src = src;
    o->last_frames = n_frames;
    return MS_OK;
}

int ms_keypoints_pack(ms_ctx *c, const ms_keypoints *view, int frame, int n, const double *bearing, uint8_t *records_host) {
    if (!c || !view || !view->x || !view->y || !view->angle || !view->octave || !view->desc || frame < 0 || n < 0 || n > view->capacity || (n && !records_host))
        return MS_ERR_INVALID;
    if (n == 0) return MS_OK;
    MS_HIP(c, hipSetDevice(c->device));
    void *scratch = nullptr;
    MS_TRY(ms_scratch(c, (size_t)n * MS_KEYPOINT_RECORD_BYTES, &scratch));
    hipLaunchKernelGGL(k_pack_keypoints, dim3(ms_div_up(n * 19, 256)), dim3(256), 0, c->stream, view->x, view->y, view->angle, view->octave, view->desc, bearing,
                       (uint64_t)frame * (uint64_t)view->capacity, n, static_cast<uint32_t *>(scratch));
    MS_KERNEL_CHECK(c, "k_pack_keypoints");
    MS_HIP(c, hipMemcpyAsync(records_host, scratch, (size_t)n * MS_KEYPOINT_RECORD_BYTES, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    return MS_OK;
}

int ms_keypoints_unpack(const uint8_t *records, int n, float *x, float *y, float *angle, int32_t *octave, double *bearing, uint32_t *desc) {
    if (n < 0 || (n && !records)) return MS_ERR_INVALID;
    for (int k = 0; k < n; ++k) {
        const uint8_t *r = records + (size_t)k * MS_KEYPOINT_RECORD_BYTES;
        int32_t o1, o2;
        std::memcpy(&o1, r + 12, 4); std::memcpy(&o2, r + 16, 4);
        if (o1 != o2) return MS_ERR_INVALID;                    // KeyPoint::serialize writes `octave` twice; a record where they differ is corrupt
        if (x) std::memcpy(x + k, r, 4);
        if (y) std::memcpy(y + k, r + 4, 4);
        if (angle) std::memcpy(angle + k, r + 8, 4);
        if (octave) octave[k] = o1;
        if (bearing) std::memcpy(bearing + 3 * (size_t)k, r + 20, 24);
        if (desc) std::memcpy(desc + 8 * (size_t)k, r + 44, 32);
    }
    return MS_OK;
}

int ms_orb_device_view(ms_orb *o, ms_keypoints *v) {
    if (!o || !v) return MS_ERR_INVALID;
    v->capacity = o->geom.capacity; v->count = o->d_count; v->x = o->d_x; v->y = o->d_y; v->angle = o->d_angle;
    v->octave = o->d_octave; v->desc = o->d_desc; v->track_id = o->d_track;
    return MS_OK;
}

int ms_orb_download(ms_orb *o, int frame, float *x, float *y, float *angle, int32_t *octave, uint32_t *desc, int32_t *track_id, int32_t *n) {
    if (!o || !n) return MS_ERR_INVALID;
    ms_ctx *c = o->ctx;
    if (frame < 0 || frame >= o->last_frames) return ms_fail(c, MS_ERR_INVALID, "ms_orb_download: frame %d not in last batch", frame);
    MS_HIP(c, hipStreamSynchronize(c->stream));
    int32_t cnt = 0;
    MS_HIP(c, hipMemcpy(&cnt, o->d_count + frame, sizeof(int32_t), hipMemcpyDeviceToHost));
    const size_t cap = o->geom.capacity, b = (size_t)frame * cap, k = (size_t)cnt;
    if (x) MS_HIP(c, hipMemcpy(x, o->d_x + b, k * 4, hipMemcpyDeviceToHost));
    if (y) MS_HIP(c, hipMemcpy(y, o->d_y + b, k * 4, hipMemcpyDeviceToHost));
    if (angle) MS_HIP(c, hipMemcpy(angle, o->d_angle + b, k * 4, hipMemcpyDeviceToHost));
    if (octave) MS_HIP(c, hipMemcpy(octave, o->d_octave + b, k * 4, hipMemcpyDeviceToHost));
    if (desc) MS_HIP(c, hipMemcpy(desc, o->d_desc + b * 8, k * 32, hipMemcpyDeviceToHost));
    if (track_id) MS_HIP(c, hipMemcpy(track_id, o->d_track + b, k * 4, hipMemcpyDeviceToHost));
    *n = cnt;
    return MS_OK;
}

int ms_orb_last_candidate_counts(ms_orb *o, int32_t *out) {
    if (!o || !out) return MS_ERR_INVALID;
    ms_ctx *c = o->ctx;
    if (o->last_frames < 1) return ms_fail(c, MS_ERR_INVALID, "ms_orb_last_candidate_counts: nothing ran");
    MS_HIP(c, hipStreamSynchronize(c->stream));
    MS_HIP(c, hipMemcpy(out, o->d_last_count, sizeof(int32_t) * (size_t)o->last_frames * o->geom.levels, hipMemcpyDeviceToHost));
    return MS_OK;
}

int ms_orb_last_fast_launches(const ms_orb *o, int32_t *launches, int32_t *pruning) {
    if (!o || !launches || !pruning) return MS_ERR_INVALID;
    *launches = o->fast_launches; *pruning = o->fast_pruning;
    return MS_OK;
}

int ms_orb_level_size(const ms_orb *o, int level, int32_t *w, int32_t *h) {
    if (!o || level < 0 || level >= o->geom.levels || !w || !h) return MS_ERR_INVALID;
    *w = o->geom.L[level].w; *h = o->geom.L[level].h;
    return MS_OK;
}

int ms_orb_download_level(ms_orb *o, int frame, int level, int blurred, uint8_t *dst) {
    if (!o || !dst) return MS_ERR_INVALID;
    ms_ctx *c = o->ctx;
    if (frame < 0 || frame >= o->last_frames || level < 0 || level >= o->geom.levels) return ms_fail(c, MS_ERR_INVALID, "ms_orb_download_level: bad frame/level");
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const LevelGeom &L = o->geom.L[level];
    const uint8_t *p; size_t pitch;
    if (blurred) {
        if (!o->blur_valid) {                                  // the blurred levels of the last batch, computed when somebody asks for them
            hipLaunchKernelGGL(k_blur, dim3(o->geom.btiles_total, o->last_frames), dim3(256), 0, c->stream, o->last_src, o->tile_levels, o->blur_tiles);
            MS_KERNEL_CHECK(c, "k_blur");
            MS_HIP(c, hipStreamSynchronize(c->stream));
            o->blur_valid = true;
        }
        p = o->d_slab + (size_t)frame * o->geom.slab_stride + L.blur_off; pitch = L.pitch;
    }
    else if (level == 0) { p = o->last_src.lvl0 + (size_t)frame * o->last_src.lvl0_frame_stride; pitch = o->last_src.lvl0_pitch; }
    else { p = o->d_slab + (size_t)frame * o->geom.slab_stride + L.img_off; pitch = L.pitch; }
    MS_HIP(c, hipMemcpy2D(dst, L.w, p, pitch, L.w, L.h, hipMemcpyDeviceToHost));
    return MS_OK;
}

int ms_orb_download_detections(ms_orb *o, int frame, int level, int32_t *x, int32_t *y, int32_t *score, int32_t *n) {
    if (!o || !n) return MS_ERR_INVALID;
    ms_ctx *c = o->ctx;
    if (frame < 0 || frame >= o->last_frames || level < 0 || level >= o->geom.levels) return ms_fail(c, MS_ERR_INVALID, "ms_orb_download_detections: bad frame/level");
    MS_HIP(c, hipStreamSynchronize(c->stream));
    int32_t cnt = 0;
    MS_HIP(c, hipMemcpy(&cnt, o->d_det_count + frame * o->geom.levels + level, 4, hipMemcpyDeviceToHost));
    const size_t b = (size_t)frame * o->geom.det_stride + o->geom.L[level].det_base;
    std::vector<int16_t> hx(cnt), hy(cnt); std::vector<uint8_t> hs(cnt);
    if (cnt) {
        MS_HIP(c, hipMemcpy(hx.data(), o->d_det_x + b, cnt * 2, hipMemcpyDeviceToHost));
        MS_HIP(c, hipMemcpy(hy.data(), o->d_det_y + b, cnt * 2, hipMemcpyDeviceToHost));
        MS_HIP(c, hipMemcpy(hs.data(), o->d_det_score + b, cnt, hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < cnt; ++i) { if (x) x[i] = hx[i]; if (y) y[i] = hy[i]; if (score) score[i] = hs[i]; }
    *n = cnt;
    return MS_OK;
}

}  // extern "C"
