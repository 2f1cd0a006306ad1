// bow_vector.hip -- the keyframe's BowVector on the device: DBoW2's BowVector::addWeight sums and normalize(L1), the last
// arithmetic of addKeyframeCommonInner (mapper_helpers.cpp:1099, bow_index.cpp:44-48) that went through the host.  tests/bow_vector_ref.py
// restates the rule and is the specification: the keypoints with weight > 0, ordered by (word, index); one entry per distinct word whose
// value adds that word's weights one by one in ascending index; the norm adds fabs(value) one by one in ascending word order; iff the
// norm is > 0 every value is divided by it.
//
// ms_bow_vector and ms_bow_db_add_words (bowdb.hip), ONE launch whatever n is:
//   k_bow_vector   ONE workgroup of 1024 threads, n <= 8192.  The 64-bit keys word << 13 | index of the kept keypoints (the others are a
//                  sentinel above every key) are sorted in LDS (bitonic, as k_bowdb_rank sorts its records); each sorted position fetches
//                  its weight into a second LDS array; a segment head is a position whose word differs from the one before it, heads are
//                  packed through the shared block rank with the count carried across the eight trips, and a head's lane walks its own
//                  segment in order.  The values replace the sorted weights behind a barrier.  ONE lane adds the norm (below); every lane
//                  divides its entries; then the verdict, and only with a clean verdict and room the words and values are written
// The norm is one dependent chain whatever adds it.  One lane reading LDS was kept: the loads do not depend on the sum and are issued
// ahead of it, so the chain is the dependent v_add_f64 alone; the lane-order form of k_bowdb_score puts two v_readlane per term into
// the same chain without shortening it, and needs the other 63 lanes for nothing.
// Integer arithmetic decides every position, the only atomic is an integer add of the verdict counter, and no sum is a tree: the same
// inputs give the same bytes on every call.
#include "ms_internal.h"
#include "ms_scan.h"
#include <cmath>

namespace {

constexpr int kThreads = 1024;
constexpr int kMaxKp = MS_COVIS_MAX_STRIDE;                  // 8192 keys (64 KB) and 8192 weights (64 KB) of the CU's 160 KB of LDS
constexpr int kTrips = kMaxKp / kThreads;
constexpr int kIndexBits = 13;
constexpr unsigned long long kNoKey = ~0ull;                 // a keypoint that is not kept; a real key has 45 bits
static_assert(kMaxKp == 1 << kIndexBits, "the key holds the index in its low 13 bits");

__global__ __launch_bounds__(kThreads) void k_bow_vector(const int32_t *__restrict__ word, const double *__restrict__ weight, int n, int vocab_words, int cap,
                                                         int32_t *out_words, double *out_values, unsigned long long *seg, int32_t *__restrict__ head) {
    __shared__ unsigned long long s_key[kMaxKp];             // sorted keys; then the entries' words << 13
    __shared__ double s_val[kMaxKp];                         // weights in sorted order; then the entries' values
    __shared__ int32_t s_wave[kThreads / 64];
    __shared__ int32_t s_bad;
    __shared__ double s_norm;
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_bad = 0;
    int P = 2;                                               // the sorted range: a power of two, n <= P <= 8192
    while (P < n) P <<= 1;
    int bad = 0;                                             // kept keypoints with a word outside the vocabulary; later, non-finite values
    for (int i = tid; i < P; i += kThreads) {
        unsigned long long key = kNoKey;
        if (i < n && weight[i] > 0.0) {                      // DBoW2's rule as written: a NaN, a zero, a negative weight are skipped, their word is not read
            const uint32_t w = (uint32_t)word[i];
            key = ((unsigned long long)w << kIndexBits) | (unsigned)i;
            bad += w >= (uint32_t)vocab_words;
        }
        s_key[i] = key;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += kThreads) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const unsigned long long a = s_key[i], b = s_key[j];
                if (((i & size) == 0) ? b < a : a < b) { s_key[i] = b; s_key[j] = a; }
            }
            __syncthreads();
        }
    for (int p = tid; p < P; p += kThreads) {
        const unsigned long long key = s_key[p];
        s_val[p] = key != kNoKey ? weight[key & (kMaxKp - 1)] : 0.0;      // the index of a kept keypoint: < n
    }
    __syncthreads();
    // ---- heads and their sums: eight trips whatever n is (block_rank holds a barrier).  Trip t's entries land at e <= p < 1024 (t + 1); the
    // trips after it read positions from 1024 (t + 1) - 1 on, and of that one the word alone, which an entry written there keeps
    int n_words = 0;
#pragma unroll 1
    for (int t = 0; t < kTrips; ++t) {
        const int p = t * kThreads + tid;
        unsigned long long key = kNoKey;
        bool first = false;
        if (p < P) {
            key = s_key[p];
            first = key != kNoKey && (p == 0 || (s_key[p - 1] >> kIndexBits) != (key >> kIndexBits));
        }
        int total;
        const int e = n_words + block_rank<kThreads>(first, s_wave, total);
        double v = 0.0;
        if (first) {
            const unsigned long long w = key >> kIndexBits;
            int k = p;
            do { v += s_val[k]; ++k; } while (k < P && (s_key[k] >> kIndexBits) == w);      // ascending index; the sentinel ends the last segment
        }
        n_words += total;
        __syncthreads();                                     // every walk of this trip has read
        if (first) { s_val[e] = v; s_key[e] = key & ~(unsigned long long)(kMaxKp - 1); }
        __syncthreads();                                     // s_wave is written again by the next trip
    }
    if (tid == 0) {                                          // BowVector::normalize(L1): one chain in ascending word order
        double norm = 0.0;
        for (int e = 0; e < n_words; ++e) norm += fabs(s_val[e]);
        s_norm = norm;
    }
    __syncthreads();
    const double norm = s_norm;
    for (int e = tid; e < n_words; e += kThreads) {
        double v = s_val[e];
        if (norm > 0.0) { v = v / norm; s_val[e] = v; }
        bad += !isfinite(v);
    }
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    if ((tid & 63) == 0 && bad) atomicAdd(&s_bad, bad);
    __syncthreads();
    const int n_bad = s_bad;
    if (tid == 0) { head[0] = n_words; head[1] = n_bad; }
    if (n_bad > 0 || n_words > cap) return;                  // the verdict, the same in every lane: nothing is written
    if (seg) {                                               // the pool's layout (bowdb.hip): ceil(len / 2) cells of words, then len cells of values
        out_words = reinterpret_cast<int32_t *>(seg);
        out_values = reinterpret_cast<double *>(seg + ((n_words + 1) >> 1));
        if (tid == 0 && (n_words & 1)) out_words[n_words] = 0;
    }
    for (int e = tid; e < n_words; e += kThreads) { out_words[e] = (int32_t)(uint32_t)(s_key[e] >> kIndexBits); out_values[e] = s_val[e]; }
}

}  // namespace

int ms_bow_vector_enqueue(ms_ctx *c, const int32_t *word, const double *weight, int n, int vocab_words, int cap, int32_t *words, double *values,
                          unsigned long long *seg, int32_t *head) {
    hipLaunchKernelGGL(k_bow_vector, dim3(1), dim3(kThreads), 0, c->stream, word, weight, n, vocab_words, cap, words, values, seg, head);
    MS_KERNEL_CHECK(c, "k_bow_vector");
    return MS_OK;
}

extern "C" int ms_bow_vector(ms_ctx *c, const int32_t *word, const double *weight, int n, int vocab_words, int cap, int32_t *words, double *values,
                             int32_t *counts) {
    if (!c) return MS_ERR_INVALID;
    int rc;
    if ((rc = ms_bow_vector_validate(word, weight, n, vocab_words, cap, words, values, counts, c->err, sizeof(c->err)))) return rc;
    counts[0] = counts[1] = 0;
    MsRange range("bowVector");
    MS_HIP(c, hipSetDevice(c->device));
    MsWorkspace &W = c->ws[MS_WS_BOW_VECTOR];
    if ((rc = ms_grow(c, W.dev, W.dev_bytes, 16, false))) return rc;
    if ((rc = ms_pinned(c, 16))) return rc;
    int32_t *head = static_cast<int32_t *>(W.dev);
    if ((rc = ms_bow_vector_enqueue(c, word, weight, n, vocab_words, cap, words, values, nullptr, head))) return rc;
    MS_HIP(c, hipMemcpyAsync(c->pinned, head, 8, hipMemcpyDeviceToHost, c->stream));
    MS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *h = static_cast<const int32_t *>(c->pinned);
    counts[0] = h[0]; counts[1] = h[1];
    if (h[1] > 0)
        return ms_fail(c, MS_ERR_INVALID, "bow vector: %d kept keypoints have a word outside [0, %d) or a value that is not finite (nothing is written)", h[1], vocab_words);
    if (h[0] > cap) return ms_fail(c, MS_ERR_CAPACITY, "bow vector: %d words, the outputs hold %d (nothing is written)", h[0], cap);
    return MS_OK;
}
