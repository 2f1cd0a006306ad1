// map_publish.hip -- the map as the mapper hands it to someone outside: the last two steps of addKeyframeCommonInner on the device map tables.
//   publishMapForViewer         mapper_helpers.cpp:814-879 (called at :1117, :1129)   the viewer's map points and the keyframes' poseWC
//   updatePointCloudRecording   :881-909 (called at :1125)                            the point-cloud record as a stream of changes
//
// ms_map_publish, FIVE launches whatever the sizes:
//   k_publish_clear     zeroes the two mark bitmaps (one bit per row: localMap, nowVisible); lane i < n_list writes pose_wc[i], the rigid inverse of
//                       kf_pose[kf_list[i]], into the head block
//   k_publish_mark      one lane per entry of local_rows and per entry of the current slot's row: a VALID entry ORs its row's bit into a bitmap word --
//                       the call's only atomics, and an OR gives the same word in any order
//   k_publish_count     one lane per row: whether the row is published and which event it gives; per workgroup the two stream counts and the six class
//                       counts of the head
//   k_publish_offsets   ONE workgroup: block_offsets over each stream's counts, the class sums, the head
//   k_publish_pack      as k_publish_count; returns at once when a stream exceeds its capacity (every verdict before any write).  The k-th row of a
//                       stream writes element k of its arrays in the block that goes down, laid out for exactly n_pub and n_ev elements; an event's row
//                       writes rec_pos / rec_state
// A row's lane reads mp_pos[r] as its whole 24-byte row and a wave reads 64 adjacent rows.  Every position is an integer prefix count, a row is
// read and written by its own lane only, and nothing depends on the capacities: the same tables give the same bytes on every call.  A row r is used
// only after (uint32)r < n_mp held.
#include "ms_internal.h"
#include "ms_scan.h"
#include <algorithm>
#include <cstring>

namespace {

constexpr int kBlock = 256;
// the head is `counts` in the header's order: n_pub, n_ev | NEW, MOVED, REMOVED | localMap, nowVisible | skipped as NOT_TRIANGULATED
constexpr int kHeadPub = 0, kHeadEv = 1, kHeadInts = 8;
constexpr uint8_t kNew = 1, kMoved = 2, kGone = 3;           // ev_kind; rec_state: 0 never recorded, 1 recorded, 2 removed

// The block that goes down second, for n published rows and m events: every array at its exact length, the byte arrays last so that every
// other element is 4-byte aligned.  The device lays it out from the head, the host from the head's copy.
struct Packed {
    size_t pub_row, pub_pos, pub_norm, pub_color, ev_row, ev_pos, ev_norm, pub_status, pub_bits, ev_kind, end;
    __host__ __device__ Packed(size_t n, size_t m) {
        pub_row = 0; pub_pos = 4 * n; pub_norm = 16 * n; pub_color = 28 * n;
        ev_row = 40 * n; ev_pos = ev_row + 4 * m; ev_norm = ev_row + 16 * m;
        pub_status = ev_row + 28 * m; pub_bits = pub_status + n; ev_kind = pub_bits + n; end = ev_kind + m;
    }
};

struct PublishArgs {
    const double *mp_pos;
    const float *mp_norm;
    const uint8_t *mp_flags, *mp_live, *mp_color;
    const int32_t *n_obs;
    const int32_t *kf_mp;
    const double *kf_pose;
    const int32_t *local_rows;
    float *rec_pos;
    uint8_t *rec_state;
    const int32_t *kf_list;              // workspace [n_list]
    uint32_t *local_bits, *vis_bits;     // workspace [n_words] each
    int32_t *blk_count, *blk_off;        // workspace [kHeadInts * n_blk]: count q of workgroup b at q * n_blk + b
    int32_t *head;                       // [kHeadInts], the start of the block that goes down first
    float *pose_wc;                      // [16 * n_list] behind it
    uint8_t *packed;                     // the block that goes down second
    int32_t n_mp, stride, n_local, n_list, n_words, n_blk, current_slot, min_record_obs, cap_pub, cap_ev;
    bool view, record;
};

__global__ __launch_bounds__(kBlock) void k_publish_clear(const PublishArgs A) {
    const int i = blockIdx.x * kBlock + (int)threadIdx.x;
    if (i < A.n_words) { A.local_bits[i] = 0u; A.vis_bits[i] = 0u; }
    if (i >= A.n_list) return;
    const double *P = A.kf_pose + 12 * (size_t)A.kf_list[i];           // rows 0-2 of poseCW: R | t
    float *out = A.pose_wc + 16 * (size_t)i;
    for (int j = 0; j < 3; ++j) {                                        // row j of poseWC: column j of R | -R^T t (cameraCenterOf's expression; the unit has no contraction)
        out[4 * j + 0] = (float)P[j]; out[4 * j + 1] = (float)P[4 + j]; out[4 * j + 2] = (float)P[8 + j];
        out[4 * j + 3] = (float)(-((P[j] * P[3] + P[4 + j] * P[7]) + P[8 + j] * P[11]));
    }
    out[12] = 0.f; out[13] = 0.f; out[14] = 0.f; out[15] = 1.f;
}

__global__ __launch_bounds__(kBlock) void k_publish_mark(const PublishArgs A) {
    const int i = blockIdx.x * kBlock + (int)threadIdx.x;
    if (i < A.n_local) {
        const uint32_t r = (uint32_t)A.local_rows[i];
        if (r < (uint32_t)A.n_mp) atomicOr(A.local_bits + (r >> 5), 1u << (r & 31));
    } else if (A.current_slot >= 0 && i - A.n_local < A.stride) {
        const uint32_t r = (uint32_t)A.kf_mp[(size_t)A.current_slot * A.stride + (i - A.n_local)];
        if (r < (uint32_t)A.n_mp) atomicOr(A.vis_bits + (r >> 5), 1u << (r & 31));
    }
}

// What the lane's row gives: whether it is published, with its bits and whether it was skipped as NOT_TRIANGULATED; its event (0: none) and the
// position as the record holds it.
struct Row {
    int r;
    bool pub, skipped;
    uint8_t bits, kind;
    float p[3];
};
__device__ inline Row publish_row(const PublishArgs &A) {
    Row w{};
    w.r = blockIdx.x * kBlock + (int)threadIdx.x;
    if (w.r >= A.n_mp) return w;
    const size_t r = (size_t)w.r;
    const bool present = A.mp_live[r] != 0;
    if (A.view && present) {                                 // :830
        w.pub = (A.mp_flags[r] & 3) != 0;
        w.skipped = !w.pub;
        if (w.pub) w.bits = (uint8_t)((A.local_bits[r >> 5] >> (r & 31) & 1u) | (A.vis_bits[r >> 5] >> (r & 31) & 1u) << 1);
    }
    if (!A.record) return w;
    const uint8_t state = A.rec_state[r];
    if (!present) {                                          // :902-907
        if (state == 1) w.kind = kGone;
        return w;
    }
    if (A.n_obs[r] < A.min_record_obs) return w;             // :889
    const double x = A.mp_pos[3 * r], y = A.mp_pos[3 * r + 1], z = A.mp_pos[3 * r + 2];
    w.p[0] = (float)x; w.p[1] = (float)y; w.p[2] = (float)z; // cast<float>(): round to nearest even
    if (state != 1) w.kind = kNew;                           // :892; a removed row that is present again is a new map point
    else if (A.rec_pos[3 * r] != w.p[0] || A.rec_pos[3 * r + 1] != w.p[1] || A.rec_pos[3 * r + 2] != w.p[2]) w.kind = kMoved;      // :895, Eigen's !=
    return w;
}

__global__ __launch_bounds__(kBlock) void k_publish_count(const PublishArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const Row w = publish_row(A);
    // three sums of three 10-bit fields each: no field exceeds the workgroup's 256 lanes
    const int share[3] = {(int)w.pub | (int)(w.kind != 0) << 10 | (int)w.skipped << 20,
                          (int)(w.kind == kNew) | (int)(w.kind == kMoved) << 10 | (int)(w.kind == kGone) << 20,
                          (int)(w.pub && (w.bits & 1)) | (int)(w.pub && (w.bits & 2)) << 10};
    int sum[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        block_exclusive<kBlock>(share[q], s_wave, sum[q]);
        __syncthreads();                                     // s_wave is written again by the next sum
    }
    if (threadIdx.x == 0) {
        const int v[kHeadInts] = {sum[0] & 1023, sum[0] >> 10 & 1023, sum[1] & 1023, sum[1] >> 10 & 1023, sum[1] >> 20 & 1023, sum[2] & 1023, sum[2] >> 10 & 1023, sum[0] >> 20 & 1023};
        for (int q = 0; q < kHeadInts; ++q) A.blk_count[(size_t)q * A.n_blk + blockIdx.x] = v[q];
    }
}

__global__ __launch_bounds__(kBlock) void k_publish_offsets(const PublishArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    for (int q = 0; q < kHeadInts; ++q) {                    // the two streams' offsets are used; a class only needs its total
        const int total = block_offsets<kBlock>(A.blk_count + (size_t)q * A.n_blk, A.blk_off + (size_t)q * A.n_blk, A.n_blk, s_wave);
        if (threadIdx.x == 0) A.head[q] = total;
    }
}

__global__ __launch_bounds__(kBlock) void k_publish_pack(const PublishArgs A) {
    __shared__ int32_t s_wave[kBlock / 64];
    const int n_pub = A.head[kHeadPub], n_ev = A.head[kHeadEv];
    if (n_pub > A.cap_pub || n_ev > A.cap_ev) return;        // the same answer in every lane of the grid: nothing is written
    const Row w = publish_row(A);
    int total;
    const int kp = A.blk_off[blockIdx.x] + block_rank<kBlock>(w.pub, s_wave, total);
    __syncthreads();                                         // s_wave is written again by the second rank
    const int ke = A.blk_off[(size_t)A.n_blk + blockIdx.x] + block_rank<kBlock>(w.kind != 0, s_wave, total);
    const Packed L((size_t)n_pub, (size_t)n_ev);
    const size_t r = (size_t)w.r;
    if (w.pub) {                                             // kp < n_pub <= cap_pub
        const size_t k = (size_t)kp;
        reinterpret_cast<int32_t *>(A.packed + L.pub_row)[k] = w.r;
        float *pos = reinterpret_cast<float *>(A.packed + L.pub_pos) + 3 * k, *norm = reinterpret_cast<float *>(A.packed + L.pub_norm) + 3 * k;
        float *color = reinterpret_cast<float *>(A.packed + L.pub_color) + 3 * k;
        for (int a = 0; a < 3; ++a) {
            pos[a] = (float)A.mp_pos[3 * r + a];
            norm[a] = A.mp_norm[3 * r + a];
            color[a] = A.mp_color ? __fdiv_rn((float)A.mp_color[3 * r + a], 255.0f) : 0.f;       // :834
        }
        (A.packed + L.pub_status)[k] = (A.mp_flags[r] & 1) ? 0 : 2;      // int(MapPointStatus): TRIANGULATED 0, UNSURE 2
        (A.packed + L.pub_bits)[k] = w.bits;
    }
    if (w.kind) {                                            // ke < n_ev <= cap_ev
        const size_t k = (size_t)ke;
        const bool gone = w.kind == kGone;
        reinterpret_cast<int32_t *>(A.packed + L.ev_row)[k] = w.r;
        (A.packed + L.ev_kind)[k] = w.kind;
        float *pos = reinterpret_cast<float *>(A.packed + L.ev_pos) + 3 * k, *norm = reinterpret_cast<float *>(A.packed + L.ev_norm) + 3 * k;
        for (int a = 0; a < 3; ++a) {
            pos[a] = gone ? 0.f : w.p[a];                    // :902
            norm[a] = gone ? 0.f : A.mp_norm[3 * r + a];
            if (!gone) A.rec_pos[3 * r + a] = w.p[a];
        }
        A.rec_state[r] = gone ? 2 : 1;
    }
}

}  // namespace

extern "C" int ms_map_publish(ms_ctx *c, const double *mp_pos, const float *mp_norm, const uint8_t *mp_flags, const uint8_t *mp_live, const int32_t *n_obs,
                              const uint8_t *mp_color, int n_mp, const int32_t *kf_mp, int n_kf, int stride, const double *kf_pose, const int32_t *local_rows, int n_local,
                              float *rec_pos, uint8_t *rec_state, const ms_map_publish_args *args, const int32_t *kf_list, int n_list, int32_t *pub_row, float *pub_pos,
                              float *pub_norm, float *pub_color, uint8_t *pub_status, uint8_t *pub_bits, int cap_pub, int32_t *ev_row, uint8_t *ev_kind, float *ev_pos,
                              float *ev_norm, int cap_ev, float *pose_wc, int32_t *counts) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_map_publish_validate(mp_pos, mp_norm, mp_flags, mp_live, n_obs, mp_color, n_mp, kf_mp, n_kf, stride, kf_pose, local_rows, n_local, rec_pos, rec_state, args,
                                      kf_list, n_list, pub_row, pub_pos, pub_norm, pub_color, pub_status, pub_bits, cap_pub, ev_row, ev_kind, ev_pos, ev_norm, cap_ev, pose_wc,
                                      counts, c->err, sizeof(c->err))))
        return rc;
    for (int q = 0; q < kHeadInts; ++q) counts[q] = 0;
    if (n_mp == 0 && n_list == 0) return MS_OK;
    MsRange range("mapPublish");
    const bool view = (args->what & MS_PUBLISH_VIEW) != 0, record = (args->what & MS_PUBLISH_RECORD) != 0;
    const size_t nm = (size_t)n_mp, nl = (size_t)n_list, n_words = (nm + 31) / 32;
    const int n_blk = std::max(ms_div_up(n_mp, kBlock), 1);
    // no stream holds more elements than the map has rows or the caller's arrays hold: the bound of the block that goes down second
    const size_t bound_pub = view ? std::min((size_t)cap_pub, nm) : 0, bound_ev = record ? std::min((size_t)cap_ev, nm) : 0;
    // upload block: the listed slots
    MsLayout up;
    const auto l_list = up.array<int32_t>(nl);
    MsLayout dev = up;
    // device-only block: the two bitmaps | counts per workgroup | their offsets; then the two blocks that go down: head | pose_wc, and the packed streams
    const auto l_local = dev.array<uint32_t>(n_words), l_vis = dev.array<uint32_t>(n_words);
    const auto l_bc = dev.array<int32_t>((size_t)kHeadInts * n_blk), l_bo = dev.array<int32_t>((size_t)kHeadInts * n_blk);
    MsLayout first;
    const auto l_head = first.array<int32_t>(kHeadInts);
    const auto l_pose = first.array<float>(16 * nl);
    const size_t first_at = dev.take(first.end), packed_at = dev.take(Packed(bound_pub, bound_ev).end);
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_MAP_PUBLISH];
    if ((rc = ms_grow(c, W.host, W.host_bytes, up.end, true))) return rc;
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, dev.end, false))) return rc;
    // the pinned block holds both downloads side by side and is sized by the bounds, not by the answer: it does not grow when the answer does
    const size_t second_at = first.end;
    if ((rc = ms_pinned(c, second_at + Packed(bound_pub, bound_ev).end))) return rc;
    void *hs = W.host, *ds = W.dev, *d1 = ms_at<uint8_t>(W.dev, first_at);
    PublishArgs A{};
    A.mp_pos = mp_pos; A.mp_norm = mp_norm; A.mp_flags = mp_flags; A.mp_live = mp_live; A.mp_color = mp_color; A.n_obs = n_obs; A.kf_mp = kf_mp; A.kf_pose = kf_pose;
    A.local_rows = local_rows; A.rec_pos = rec_pos; A.rec_state = rec_state;
    A.kf_list = l_list.at(ds); A.local_bits = l_local.at(ds); A.vis_bits = l_vis.at(ds); A.blk_count = l_bc.at(ds); A.blk_off = l_bo.at(ds);
    A.head = l_head.at(d1); A.pose_wc = l_pose.at(d1); A.packed = ms_at<uint8_t>(W.dev, packed_at);
    A.n_mp = n_mp; A.stride = stride; A.n_local = n_local; A.n_list = n_list; A.n_words = (int32_t)n_words; A.n_blk = n_blk;
    A.current_slot = args->current_slot; A.min_record_obs = args->min_record_obs; A.cap_pub = cap_pub; A.cap_ev = cap_ev;
    A.view = view; A.record = record;
    if (n_list > 0) {
        l_list.fill(hs, kf_list);
        MS_HIP(c, hipMemcpyAsync(ds, hs, up.end, hipMemcpyHostToDevice, c->stream));
    }
    const dim3 block(kBlock);
    const size_t n_marks = (size_t)n_local + (args->current_slot >= 0 ? (size_t)stride : 0);
    const dim3 by_word((unsigned)std::max<size_t>((std::max(n_words, nl) + kBlock - 1) / kBlock, 1)), by_mark((unsigned)std::max<size_t>((n_marks + kBlock - 1) / kBlock, 1));
    const dim3 by_row((unsigned)n_blk);
    hipLaunchKernelGGL(k_publish_clear, by_word, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_publish_clear");
    hipLaunchKernelGGL(k_publish_mark, by_mark, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_publish_mark");
    hipLaunchKernelGGL(k_publish_count, by_row, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_publish_count");
    hipLaunchKernelGGL(k_publish_offsets, dim3(1), block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_publish_offsets");
    hipLaunchKernelGGL(k_publish_pack, by_row, block, 0, c->stream, A);
    MS_KERNEL_CHECK(c, "k_publish_pack");
    // the first download: the head and pose_wc.  The second is sized by the head, which the caps cannot do: they are the size of the map and the answer
    // usually is not
    MS_HIP(c, hipMemcpyAsync(c->pinned, d1, first.end, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    void *ps = c->pinned;
    const int32_t *head = l_head.at(ps);
    for (int q = 0; q < kHeadInts; ++q) counts[q] = head[q];
    const int n_pub = head[kHeadPub], n_ev = head[kHeadEv];
    if (n_pub > cap_pub || n_ev > cap_ev)
        return ms_fail(c, MS_ERR_CAPACITY, "map publish: %d published rows and %d events; the output arrays hold %d and %d (nothing is written)", n_pub, n_ev, cap_pub, cap_ev);
    l_pose.get(ps, 0, pose_wc, 16 * nl);
    if (n_pub == 0 && n_ev == 0) return MS_OK;
    const Packed L((size_t)n_pub, (size_t)n_ev);
    uint8_t *p2 = ms_at<uint8_t>(c->pinned, second_at);
    MS_HIP(c, hipMemcpyAsync(p2, A.packed, L.end, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const size_t n = (size_t)n_pub, m = (size_t)n_ev;
    if (n) {
        std::memcpy(pub_row, p2 + L.pub_row, 4 * n); std::memcpy(pub_pos, p2 + L.pub_pos, 12 * n); std::memcpy(pub_norm, p2 + L.pub_norm, 12 * n);
        std::memcpy(pub_color, p2 + L.pub_color, 12 * n); std::memcpy(pub_status, p2 + L.pub_status, n); std::memcpy(pub_bits, p2 + L.pub_bits, n);
    }
    if (m) {
        std::memcpy(ev_row, p2 + L.ev_row, 4 * m); std::memcpy(ev_kind, p2 + L.ev_kind, m); std::memcpy(ev_pos, p2 + L.ev_pos, 12 * m);
        std::memcpy(ev_norm, p2 + L.ev_norm, 12 * m);
    }
    return MS_OK;
}
