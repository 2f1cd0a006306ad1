// ms_scan.h -- the stream-compaction skeleton of the map kernels: a lane's rank among the kept lanes of its workgroup, the
// exclusive sum of one int per lane over the workgroup, and the one-workgroup exclusive scan of per-block totals.  Device code only; it is
// included by the .hip files that pack something (project_gate, covis, map_cull, obs_lists, map_refresh, match_tracked, map_fuse, create_points, ba_window, search_bind, loop_chain, pose_tables, frame_finish, keyframe_admit, bow_vector, map_extract, frame_admit, map_publish).
//
// BLOCK is the workgroup size, a multiple of 64; s_wave is BLOCK / 64 ints of LDS that the caller declares.  Everything is int32 and
// bounded by the entry points' capacity checks.  Integer addition is exact and associative, so the order in which a scan adds its terms
// changes no bit of the result: any correct scan gives the same offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int32_t kNone = 0x7fffffff;                        // "no position / no owner" in the map kernels' mark arrays

// the lanes of a ballot mask before this one
__device__ __forceinline__ int lanes_before(unsigned long long mask) { return __popcll(mask & ((1ull << (threadIdx.x & 63)) - 1ull)); }

// The sum of wave_total (read from each wave's last lane) over the waves before this lane's; the sum over all waves through `total`, the
// same in every lane.  ONE __syncthreads(): every thread of the workgroup must call it, and s_wave must not be written again
// (a second call with the same s_wave included) before another barrier.
template <int BLOCK>
__device__ __forceinline__ int waves_before(int wave_total, int32_t *s_wave, int &total) {
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) s_wave[wave] = wave_total;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) {
        const int c = s_wave[w];
        if (w < wave) before += c;
        total += c;
    }
    return before;
}

// The number of threads with `kept` before this one in thread order; the workgroup's count through `total`.  Barrier contract of
// waves_before: call it before any early return.
template <int BLOCK>
__device__ __forceinline__ int block_rank(bool kept, int32_t *s_wave, int &total) {
    const unsigned long long mask = __ballot(kept);
    return waves_before<BLOCK>(__popcll(mask), s_wave, total) + lanes_before(mask);
}

// The sum of v over the threads before this one in thread order; the workgroup's sum through `total`.  Barrier contract of waves_before.
template <int BLOCK>
__device__ __forceinline__ int block_exclusive(int v, int32_t *s_wave, int &total) {
    const int lane = threadIdx.x & 63;
    int inc = v;                                             // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    return waves_before<BLOCK>(inc, s_wave, total) + inc - v;
}

// Called by ONE whole workgroup: off[0 .. n) = the exclusive scan of cnt[0 .. n), BLOCK elements per trip with a running carry; returns the
// grand total in every thread.  cnt == off is allowed: a thread reads its element before it writes it, and no other thread touches it.
// Every trip ends with a barrier (s_wave is written again in the next trip, or by the caller's next scan).
template <int BLOCK>
__device__ inline int block_offsets(const int32_t *cnt, int32_t *off, int n, int32_t *s_wave) {
    int carry = 0;
    for (int i0 = 0; i0 < n; i0 += BLOCK) {
        const int i = i0 + (int)threadIdx.x;
        int total;
        const int before = block_exclusive<BLOCK>(i < n ? cnt[i] : 0, s_wave, total);
        if (i < n) off[i] = carry + before;
        carry += total;
        __syncthreads();
    }
    return carry;
}
