// bowdb.hip -- N3b: the keyframe database behind BowIndex::add / remove / getBowSimilar (bow_index.cpp:44-57, :95-176).
//
// The reference files every keyframe under each of its words in an inverted index (std::vector<std::list<MapKf>>, one list per
// vocabulary word), counts shared words into a std::map, scores the entries above the count threshold with DBoW2's L1Scoring,
// sorts and cuts.  Adds and queries alternate one for one (one of each per keyframe), so here there is no inverted index: each
// entry's BowVector lies in a device word pool and a query scans the live entries.
//
//   k_bowdb_count  grid (entry block, query): the query's sorted words in LDS, every entry word looked up by a fixed-step binary
//                  search, a wave per entry sums its hits; one integer atomicMax per workgroup gives maxInCommon
//   k_bowdb_score  same grid: minInCommon from the float formula of :143-144; a surviving entry's L1 score is summed in double over
//                  the common words in ascending word order -- lanes compute the terms of 64 consecutive entry words, the wave adds
//                  them one by one in lane order, so the sum is DBoW2's sequence of additions; survivors are appended to the query's
//                  candidate list with an integer atomicMax on the best score's ordered key
//   k_bowdb_rank   grid (candidate chunk of 4096, query): the cut (:169-173) applied to each candidate, the kept ones sorted in LDS
//                  (bitonic, 1024 threads) by (score desc, map asc, kf asc); with one chunk this writes the result directly
//   k_bowdb_merge  only when a query has more than 4096 candidates: every kept element's rank is its position in its sorted chunk plus
//                  the number of elements before it in each other chunk (binary search); ranks are unique because ids are
//
//   k_bow_vector   (bow_vector.hip) for ms_bow_db_add_words: the BowVector of a descent that lies on the device, assembled and packed
//                  straight into the segment reserved at the pool top; the host commits the entry after the 8-byte head has come down
//
// Counting and scoring stay two passes: minInCommon depends on the maximum over all entries, so a fused pass would score every
// entry that shares a single word.  Every step is integer or an ordered double sum, so results do not depend on scheduling.
#include "ms_internal.h"
#include <cmath>
#include <cstring>

namespace {

constexpr int kQueryLds = 8192;          // query words held in LDS (32 KiB); longer queries are searched in global memory
constexpr int kEntriesPerBlock = 16;     // count / score: 4 waves, 4 entries each
constexpr int kSortCap = 4096;           // rank: candidates sorted by one workgroup in LDS (64 KiB)
constexpr long long kGroupBudget = 1ll << 22;   // query x slot cells of scratch per launch group (20 B each)

struct DbEntry {                         // device entry table row; the host keeps the master copy
    long long off;                       // pool cell (8 B) of the segment: ceil(len/2) cells of words, then len cells of values
    int32_t len, map_id, kf_id, live;
};
struct DbQuery {                         // one query of a launch: its sorted words / values and the id it excludes
    const int32_t *words;
    const double *values;
    int32_t n, ex_on, ex_map, ex_kf;
};
struct DbMove { long long src, dst; int32_t cells, slot; };

__host__ __device__ inline long long seg_cells(int len) { return (long long)((len + 1) >> 1) + len; }

// the total order of the result: score descending (-0 == +0 through the canonical key), then (map_id, kf_id) ascending
// record = {key, map_id, kf_id, score bits}; key = the score's order-preserving unsigned image, >= 1 for every real record
__device__ __forceinline__ uint32_t score_key(float s) {
    const uint32_t b = __float_as_uint(s == 0.0f ? 0.0f : s);
    const uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return k ? k : 1u;
}
__device__ __forceinline__ float key_score(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ bool before(const int4 &a, const int4 &b) {
    const uint32_t ka = (uint32_t)a.x, kb = (uint32_t)b.x;
    return ka != kb ? ka > kb : (a.y != b.y ? a.y < b.y : a.z < b.z);
}

// lower bound with a fixed number of steps (p2 = the smallest power of two > n), so the unrolled searches of a lane run side by side
__device__ __forceinline__ int lbound(const int32_t *w, int n, int p2, int32_t x) {
    int pos = 0;
    for (int step = p2 >> 1; step > 0; step >>= 1)
        if (pos + step <= n && w[pos + step - 1] < x) pos += step;
    return pos;
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ const int32_t *stage_query(const DbQuery &Q, int32_t *lds) {
    if (Q.n > kQueryLds) return Q.words;
    for (int i = threadIdx.x; i < Q.n; i += blockDim.x) lds[i] = Q.words[i];
    __syncthreads();
    return lds;
}

__device__ __forceinline__ bool excluded(const DbQuery &Q, const DbEntry &e) { return Q.ex_on && e.map_id == Q.ex_map && e.kf_id == Q.ex_kf; }

// state per query of a group: [0] maxInCommon, [1] best score key, [2] candidates, [3] unused
__global__ __launch_bounds__(256) void k_bowdb_count(const DbEntry *__restrict__ ents, int n_slots, const unsigned long long *__restrict__ pool,
                                                     const DbQuery *__restrict__ qs, int32_t *__restrict__ common, int32_t *__restrict__ state) {
    __shared__ int32_t lw[kQueryLds];
    __shared__ int32_t wmax[4];
    const int qi = blockIdx.y;
    const DbQuery Q = qs[qi];
    const int32_t *qw = stage_query(Q, lw);
    int p2 = 1;
    while (p2 <= Q.n) p2 <<= 1;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    int best = 0;
    const int s_end = min(n_slots, (int)(blockIdx.x + 1) * kEntriesPerBlock);
    for (int slot = blockIdx.x * kEntriesPerBlock + wave; slot < s_end; slot += 4) {
        const DbEntry e = ents[slot];
        int c = 0;
        if (e.live && !excluded(Q, e) && Q.n > 0) {
            const int32_t *ew = reinterpret_cast<const int32_t *>(pool + e.off);
            for (int k0 = 0; k0 < e.len; k0 += 256) {         // four independent searches per lane in flight
                int32_t x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int k = k0 + 64 * u + lane; x[u] = k < e.len ? ew[k] : -1; }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int p = lbound(qw, Q.n, p2, x[u]);
                    c += (p < Q.n && qw[p] == x[u]) ? 1 : 0;
                }
            }
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        }
        if (lane == 0) common[(size_t)qi * n_slots + slot] = c;
        best = max(best, c);
    }
    if (lane == 0) wmax[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
        if (m > 0) atomicMax(&state[4 * qi], m);
    }
}

__global__ __launch_bounds__(256) void k_bowdb_score(const DbEntry *__restrict__ ents, int n_slots, const unsigned long long *__restrict__ pool,
                                                     const DbQuery *__restrict__ qs, const int32_t *__restrict__ common, int32_t *__restrict__ state,
                                                     float min_in_common_ratio, int4 *__restrict__ cand) {
    __shared__ int32_t lw[kQueryLds];
    const int qi = blockIdx.y;
    const int max_in_common = state[4 * qi];
    if (max_in_common == 0) return;                                               // :132-134: nothing shares a word
    const DbQuery Q = qs[qi];
    const int32_t *qw = stage_query(Q, lw);
    int p2 = 1;
    while (p2 <= Q.n) p2 <<= 1;
    const unsigned min_in_common = (unsigned)(min_in_common_ratio * (float)max_in_common);     // :143-144, float32 multiply, truncation
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int s_end = min(n_slots, (int)(blockIdx.x + 1) * kEntriesPerBlock);
    for (int slot = blockIdx.x * kEntriesPerBlock + wave; slot < s_end; slot += 4) {
        const unsigned c = (unsigned)common[(size_t)qi * n_slots + slot];
        if (!(c > min_in_common)) continue;                                       // :148 (uniform over the wave)
        const DbEntry e = ents[slot];
        const int32_t *ew = reinterpret_cast<const int32_t *>(pool + e.off);
        const double *ev = reinterpret_cast<const double *>(pool + e.off + ((e.len + 1) >> 1));
        double s = 0.0;
        for (int k0 = 0; k0 < e.len; k0 += 64) {
            const int k = k0 + lane;
            double t = 0.0;
            bool hit = false;
            if (k < e.len) {
                const int32_t x = ew[k];
                const int p = lbound(qw, Q.n, p2, x);
                if (p < Q.n && qw[p] == x) {
                    const double vi = Q.values[p], wi = ev[k];
                    t = fabs(vi - wi) - fabs(vi) - fabs(wi);                      // L1Scoring::score, one common word
                    hit = true;
                }
            }
            // the terms in ascending word order: lane order within the 64 words, chunks in order
            for (unsigned long long m = __ballot(hit); m; m &= m - 1) s += readlane_f64(t, __builtin_ctzll(m));
        }
        const float score = (float)(-s / 2.0);
        if (lane == 0) {
            const uint32_t key = score_key(score);
            const int pos = atomicAdd(&state[4 * qi + 2], 1);
            cand[(size_t)qi * n_slots + pos] = make_int4((int)key, e.map_id, e.kf_id, (int)__float_as_uint(score));
            atomicMax(reinterpret_cast<unsigned *>(&state[4 * qi + 1]), key);
        }
    }
}

// out: per query (global index q0 + qi) max_out records of {key, map, kf, score bits}; n_total[q0 + qi]
__global__ __launch_bounds__(1024) void k_bowdb_rank(int4 *__restrict__ cand, int n_slots, const int32_t *__restrict__ state, float score_ratio,
                                                     int32_t *__restrict__ chunk_kept, int n_chunks, int4 *__restrict__ out, int max_out,
                                                     int32_t *__restrict__ n_total, int q0) {
    __shared__ int4 rec[kSortCap];
    __shared__ int n_kept;
    const int qi = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const int cnt = state[4 * qi + 2], base = b * kSortCap;
    if (base >= cnt && b > 0) { if (tid == 0) chunk_kept[qi * n_chunks + b] = 0; return; }
    const float min_score = key_score((uint32_t)state[4 * qi + 1]) * score_ratio;        // :170 (float; unused when cnt == 0)
    if (tid == 0) n_kept = 0;
    __syncthreads();
    int4 *cq = cand + (size_t)qi * n_slots;
    const int m = min(kSortCap, cnt - base);
    for (int i = tid; i < m; i += 1024) {
        const int4 r = cq[base + i];
        if (!(__uint_as_float((uint32_t)r.w) < min_score)) rec[atomicAdd(&n_kept, 1)] = r;        // :171: cut at the first score < minScore
    }
    __syncthreads();
    const int k = n_kept;
    int P = 2;
    while (P < k) P <<= 1;
    for (int i = k + tid; i < P; i += 1024) rec[i] = make_int4(0, 0x7FFFFFFF, 0x7FFFFFFF, 0);      // key 0: after every real record
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += 1024) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const int4 a = rec[i], c = rec[j];
                const bool up = (i & size) == 0;
                if (up ? before(c, a) : before(a, c)) { rec[i] = c; rec[j] = a; }
            }
            __syncthreads();
        }
    if (cnt <= kSortCap) {                                                        // one chunk: this is the result
        int4 *o = out + (size_t)(q0 + qi) * max_out;
        for (int i = tid; i < min(k, max_out); i += 1024) o[i] = rec[i];
        if (tid == 0) n_total[q0 + qi] = k;
    } else {
        for (int i = tid; i < k; i += 1024) cq[base + i] = rec[i];
        if (tid == 0) chunk_kept[qi * n_chunks + b] = k;
    }
}

__global__ __launch_bounds__(256) void k_bowdb_merge(const int4 *__restrict__ cand, int n_slots, const int32_t *__restrict__ state,
                                                     const int32_t *__restrict__ chunk_kept, int n_chunks, int4 *__restrict__ out, int max_out,
                                                     int32_t *__restrict__ n_total, int q0) {
    const int qi = blockIdx.y;
    const int cnt = state[4 * qi + 2];
    if (cnt <= kSortCap) return;                                                  // k_bowdb_rank wrote it
    const int used = (cnt + kSortCap - 1) / kSortCap;
    const int32_t *kept = chunk_kept + qi * n_chunks;
    const int e = blockIdx.x * 256 + threadIdx.x, b = e / kSortCap, i = e % kSortCap;
    const int4 *cq = cand + (size_t)qi * n_slots;
    if (e == 0) {
        int total = 0;
        for (int c = 0; c < used; ++c) total += kept[c];
        n_total[q0 + qi] = total;
    }
    if (b >= used || i >= kept[b]) return;
    const int4 x = cq[b * kSortCap + i];
    int rank = i;
    for (int c = 0; c < used; ++c) {
        if (c == b) continue;
        const int4 *s = cq + c * kSortCap;
        int lo = 0, len = kept[c];                                                // elements of chunk c that come before x
        while (len > 0) {
            const int h = len >> 1;
            if (before(s[lo + h], x)) { lo += h + 1; len -= h + 1; } else len = h;
        }
        rank += lo;
    }
    if (rank < max_out) out[(size_t)(q0 + qi) * max_out + rank] = x;
}

__global__ __launch_bounds__(256) void k_bowdb_compact(const DbMove *__restrict__ moves, const unsigned long long *__restrict__ src,
                                                       unsigned long long *__restrict__ dst, DbEntry *__restrict__ ents) {
    const DbMove mv = moves[blockIdx.x];
    for (int i = threadIdx.x; i < mv.cells; i += 256) dst[mv.dst + i] = src[mv.src + i];
    if (threadIdx.x == 0) ents[mv.slot].off = mv.dst;
}

inline uint64_t id_key(int32_t map_id, int32_t kf_id) { return ((uint64_t)(uint32_t)map_id << 32) | (uint32_t)kf_id; }
inline uint64_t id_hash(uint64_t k) {                                             // splitmix64 finaliser
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull; k ^= k >> 27; k *= 0x94d049bb133111ebull; return k ^ (k >> 31);
}

}  // namespace

struct ms_bow_db {
    ms_ctx *ctx = nullptr;
    int n_words = 0;
    // entries: host master table, free slots, (map, kf) -> slot by open addressing (linear probing, backward-shift deletion); all grow-only
    std::vector<DbEntry> ent;
    std::vector<int32_t> free_slots;
    int n_slots = 0, n_free = 0, n_live = 0;
    std::vector<uint64_t> hkey;
    std::vector<int32_t> hslot;                  // -1 = empty
    // device: entry table, word pool (two blocks: compaction copies the live segments from one to the other)
    DbEntry *d_ent = nullptr;
    int ent_cap = 0;
    unsigned long long *d_pool[2] = {nullptr, nullptr};
    long long pool_cap = 0, pool_top = 0, live_cells = 0;
    // device scratch of the queries (grow-only)
    struct Buf { void *p = nullptr; size_t bytes = 0; };
    Buf d_qdesc, d_qvec, d_state, d_common, d_cand, d_chunk, d_result, d_moves;
    Buf d_head;                                  // {n_words, n_bad} of ms_bow_db_add_words
    // page-locked staging: uploads are appended, the arena is reused after the stream has been synchronised; downloads land in `out`
    uint8_t *stage = nullptr;
    size_t stage_cap = 0, stage_pos = 0;
    uint8_t *outp = nullptr;
    size_t out_cap = 0;
    std::vector<DbQuery> qdesc;
    std::vector<DbMove> moves;
};

namespace {

int sync_stream(ms_bow_db *db) {
    MS_HIP(db->ctx, hipStreamSynchronize(db->ctx->stream));
    db->stage_pos = 0;
    return MS_OK;
}

int grow_dev(ms_bow_db *db, ms_bow_db::Buf &b, size_t bytes) {
    if (bytes <= b.bytes) return MS_OK;
    if (b.p) { int rc = sync_stream(db); if (rc) return rc; MS_HIP(db->ctx, hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
    const size_t want = ms_align_up(bytes + bytes / 2, 4096);
    MS_HIP(db->ctx, hipMalloc(&b.p, want));
    b.bytes = want;
    ++g_ms_host_allocs;
    return MS_OK;
}

int grow_pinned(ms_bow_db *db, uint8_t *&p, size_t &cap, size_t bytes) {
    if (bytes <= cap) return MS_OK;
    if (p) { int rc = sync_stream(db); if (rc) return rc; MS_HIP(db->ctx, hipHostFree(p)); p = nullptr; cap = 0; }
    const size_t want = ms_align_up(bytes + bytes / 2, 4096);
    MS_HIP(db->ctx, hipHostMalloc(reinterpret_cast<void **>(&p), want, hipHostMallocDefault));
    cap = want;
    ++g_ms_host_allocs;
    return MS_OK;
}

// `bytes` of the page-locked arena for an upload enqueued next; the arena restarts after a synchronisation (no copy from it is then pending)
int stage_take(ms_bow_db *db, size_t bytes, uint8_t **out) {
    bytes = ms_align_up(bytes, 16);
    if (db->stage_pos + bytes > db->stage_cap) {
        int rc = sync_stream(db);
        if (rc) return rc;
        if ((rc = grow_pinned(db, db->stage, db->stage_cap, std::max(bytes, (size_t)1 << 20)))) return rc;
    }
    *out = db->stage + db->stage_pos;
    db->stage_pos += bytes;
    return MS_OK;
}

int upload(ms_bow_db *db, void *dst, const void *src, size_t bytes) {
    uint8_t *s = nullptr;
    int rc = stage_take(db, bytes, &s);
    if (rc) return rc;
    std::memcpy(s, src, bytes);
    MS_HIP(db->ctx, hipMemcpyAsync(dst, s, bytes, hipMemcpyHostToDevice, db->ctx->stream));
    return MS_OK;
}

int find_slot(const ms_bow_db *db, uint64_t key) {
    if (db->hkey.empty()) return -1;
    const size_t mask = db->hkey.size() - 1;
    for (size_t h = id_hash(key) & mask;; h = (h + 1) & mask) {
        if (db->hslot[h] < 0) return -1;
        if (db->hkey[h] == key) return db->hslot[h];
    }
}

void hash_insert(ms_bow_db *db, uint64_t key, int32_t slot) {
    const size_t mask = db->hkey.size() - 1;
    size_t h = id_hash(key) & mask;
    while (db->hslot[h] >= 0) h = (h + 1) & mask;
    db->hkey[h] = key; db->hslot[h] = slot;
}

void hash_erase(ms_bow_db *db, uint64_t key) {
    const size_t mask = db->hkey.size() - 1;
    size_t h = id_hash(key) & mask;
    while (db->hkey[h] != key || db->hslot[h] < 0) h = (h + 1) & mask;
    db->hslot[h] = -1;
    for (size_t j = (h + 1) & mask; db->hslot[j] >= 0; j = (j + 1) & mask) {    // backward shift: keep every probe chain unbroken
        const size_t home = id_hash(db->hkey[j]) & mask;
        if (((j - home) & mask) >= ((j - h) & mask)) { db->hkey[h] = db->hkey[j]; db->hslot[h] = db->hslot[j]; db->hslot[j] = -1; h = j; }
    }
}

// table capacity for `entries` slots: host arrays, hash (load <= 1/2) and the device table
int reserve_entries(ms_bow_db *db, int entries) {
    if (entries <= db->ent_cap) return MS_OK;
    const int cap = std::max(entries, db->ent_cap + db->ent_cap / 2 + 16);
    db->ent.resize((size_t)cap); db->free_slots.resize((size_t)cap);
    g_ms_host_allocs += 2;
    size_t hcap = 16;
    while (hcap < 2 * (size_t)cap) hcap <<= 1;
    if (hcap != db->hkey.size()) {
        std::vector<uint64_t> ok(std::move(db->hkey));
        std::vector<int32_t> os(std::move(db->hslot));
        db->hkey.assign(hcap, 0); db->hslot.assign(hcap, -1);
        g_ms_host_allocs += 2;
        for (size_t i = 0; i < os.size(); ++i) if (os[i] >= 0) hash_insert(db, ok[i], os[i]);
    }
    DbEntry *nd = nullptr;
    MS_HIP(db->ctx, hipMalloc(&nd, sizeof(DbEntry) * (size_t)cap));
    ++g_ms_host_allocs;
    if (db->d_ent) {
        MS_HIP(db->ctx, hipMemcpyAsync(nd, db->d_ent, sizeof(DbEntry) * (size_t)db->n_slots, hipMemcpyDeviceToDevice, db->ctx->stream));
        int rc = sync_stream(db);
        if (rc) { (void)hipFree(nd); return rc; }
        MS_HIP(db->ctx, hipFree(db->d_ent));
    }
    db->d_ent = nd;
    db->ent_cap = cap;
    return MS_OK;
}

// room for a segment of `cells` at the pool top: compact the live segments into the other block, and grow both blocks if that is not enough
int reserve_pool(ms_bow_db *db, long long cells) {
    if (db->pool_top + cells <= db->pool_cap) return MS_OK;
    const long long need = db->live_cells + cells;
    ms_ctx *c = db->ctx;
    unsigned long long *src = db->d_pool[0], *dst = db->d_pool[1], *spare = nullptr;
    long long new_cap = db->pool_cap;
    if (need > db->pool_cap * 3 / 4) {                                            // grow: a new pair, the live data moves into the first
        new_cap = std::max(2 * db->pool_cap, 2 * need);
        unsigned long long *a = nullptr, *b = nullptr;
        MS_HIP(c, hipMalloc(&a, 8 * (size_t)new_cap));
        hipError_t e = hipMalloc(&b, 8 * (size_t)new_cap);
        if (e != hipSuccess) { (void)hipFree(a); return ms_fail(c, MS_ERR_HIP, "bow db: pool growth failed: %s", hipGetErrorString(e)); }
        g_ms_host_allocs += 2;
        dst = a; spare = b;
    }
    db->moves.clear();
    long long top = 0;
    for (int s = 0; s < db->n_slots; ++s) {
        DbEntry &en = db->ent[(size_t)s];
        if (!en.live) continue;
        const long long n = seg_cells(en.len);
        if (n > 0) db->moves.push_back(DbMove{en.off, top, (int32_t)n, s});
        en.off = top;
        top += n;
    }
    if (!db->moves.empty()) {
        const size_t bytes = sizeof(DbMove) * db->moves.size();
        int rc = grow_dev(db, db->d_moves, bytes);
        if (!rc) rc = upload(db, db->d_moves.p, db->moves.data(), bytes);
        if (rc) return rc;
        hipLaunchKernelGGL(k_bowdb_compact, dim3((unsigned)db->moves.size()), dim3(256), 0, c->stream, static_cast<const DbMove *>(db->d_moves.p), src, dst, db->d_ent);
        MS_KERNEL_CHECK(c, "k_bowdb_compact");
    }
    if (spare) {
        int rc = sync_stream(db);
        if (rc) return rc;
        MS_HIP(c, hipFree(db->d_pool[0]));
        MS_HIP(c, hipFree(db->d_pool[1]));
        db->d_pool[0] = dst; db->d_pool[1] = spare;
        db->pool_cap = new_cap;
    } else {
        db->d_pool[1] = src; db->d_pool[0] = dst;
    }
    db->pool_top = top;
    return MS_OK;
}

int check_vector(ms_ctx *c, const char *what, int n, int n_words, const int32_t *words, const double *values) {
    if (n < 0 || (n > 0 && (!words || !values))) return ms_fail(c, MS_ERR_INVALID, "%s: n = %d with missing arrays", what, n);
    for (int i = 0; i < n; ++i) {
        if (words[i] < 0 || words[i] >= n_words) return ms_fail(c, MS_ERR_INVALID, "%s: word %d at %d is outside [0, %d)", what, words[i], i, n_words);
        if (i > 0 && words[i] <= words[i - 1]) return ms_fail(c, MS_ERR_INVALID, "%s: words are not strictly ascending at %d", what, i);
        if (!std::isfinite(values[i])) return ms_fail(c, MS_ERR_INVALID, "%s: value at %d is not finite", what, i);
    }
    return MS_OK;
}

// runs q queries (descriptors in db->qdesc) and downloads max_out records each plus the counts into db->outp; synchronises
int run_queries(ms_bow_db *db, int q, float min_in_common_ratio, float score_ratio, int max_out) {
    ms_ctx *c = db->ctx;
    const int ns = db->n_slots;
    const int n_chunks = ms_div_up(ns, kSortCap);
    const int g = (int)std::max(1ll, std::min((long long)q, kGroupBudget / std::max(ns, 1)));
    const size_t res_head = ms_align_up(4 * (size_t)q, 16), res_bytes = res_head + 16 * (size_t)q * max_out;
    int rc;
    if ((rc = grow_dev(db, db->d_qdesc, sizeof(DbQuery) * (size_t)q)) || (rc = grow_dev(db, db->d_state, 16 * (size_t)g)) ||
        (rc = grow_dev(db, db->d_common, 4 * (size_t)g * ns)) || (rc = grow_dev(db, db->d_cand, 16 * (size_t)g * ns)) ||
        (rc = grow_dev(db, db->d_chunk, 4 * (size_t)g * n_chunks)) || (rc = grow_dev(db, db->d_result, res_bytes)) ||
        (rc = grow_pinned(db, db->outp, db->out_cap, res_bytes)))
        return rc;
    if ((rc = upload(db, db->d_qdesc.p, db->qdesc.data(), sizeof(DbQuery) * (size_t)q))) return rc;
    int32_t *ntot = static_cast<int32_t *>(db->d_result.p);
    int4 *out = reinterpret_cast<int4 *>(static_cast<uint8_t *>(db->d_result.p) + res_head);
    const DbQuery *qd = static_cast<const DbQuery *>(db->d_qdesc.p);
    int32_t *state = static_cast<int32_t *>(db->d_state.p);
    for (int q0 = 0; q0 < q; q0 += g) {
        const int gq = std::min(g, q - q0);
        MS_HIP(c, hipMemsetAsync(state, 0, 16 * (size_t)gq, c->stream));
        const dim3 scan(ms_div_up(ns, kEntriesPerBlock), gq);
        hipLaunchKernelGGL(k_bowdb_count, scan, dim3(256), 0, c->stream, db->d_ent, ns, db->d_pool[0], qd + q0, static_cast<int32_t *>(db->d_common.p), state);
        MS_KERNEL_CHECK(c, "k_bowdb_count");
        hipLaunchKernelGGL(k_bowdb_score, scan, dim3(256), 0, c->stream, db->d_ent, ns, db->d_pool[0], qd + q0, static_cast<const int32_t *>(db->d_common.p),
                           state, min_in_common_ratio, static_cast<int4 *>(db->d_cand.p));
        MS_KERNEL_CHECK(c, "k_bowdb_score");
        hipLaunchKernelGGL(k_bowdb_rank, dim3(n_chunks, gq), dim3(1024), 0, c->stream, static_cast<int4 *>(db->d_cand.p), ns, state, score_ratio,
                           static_cast<int32_t *>(db->d_chunk.p), n_chunks, out, max_out, ntot, q0);
        MS_KERNEL_CHECK(c, "k_bowdb_rank");
        if (n_chunks > 1) {
            hipLaunchKernelGGL(k_bowdb_merge, dim3(ms_div_up(n_chunks * kSortCap, 256), gq), dim3(256), 0, c->stream, static_cast<const int4 *>(db->d_cand.p), ns,
                               state, static_cast<const int32_t *>(db->d_chunk.p), n_chunks, out, max_out, ntot, q0);
            MS_KERNEL_CHECK(c, "k_bowdb_merge");
        }
    }
    MS_HIP(c, hipMemcpyAsync(db->outp, db->d_result.p, res_bytes, hipMemcpyDeviceToHost, c->stream));
    return sync_stream(db);
}

// query i's first min(n_total, max_out) records from db->outp (dense, stride mo) into the caller's arrays at `at`
int copy_out(const ms_bow_db *db, int q, int i, int mo, int max_out, int at, int32_t *out_map, int32_t *out_kf, float *out_score, int *n_total) {
    const int32_t *ntot = reinterpret_cast<const int32_t *>(db->outp);
    const int4 *rec = reinterpret_cast<const int4 *>(db->outp + ms_align_up(4 * (size_t)q, 16)) + (size_t)i * mo;
    const int k = std::min(ntot[i], max_out);
    for (int j = 0; j < k; ++j) {
        if (out_map) out_map[at + j] = rec[j].y;
        if (out_kf) out_kf[at + j] = rec[j].z;
        if (out_score) { const uint32_t b = (uint32_t)rec[j].w; std::memcpy(&out_score[at + j], &b, 4); }
    }
    n_total[i] = ntot[i];
    return k;
}

}  // namespace

extern "C" {

int ms_bow_db_create(ms_ctx *c, int n_words, int initial_entries, long long initial_words, ms_bow_db **out) {
    if (!c || !out || n_words < 1 || initial_entries < 0 || initial_words < 0) return ms_fail(c, MS_ERR_INVALID, "bow db: bad create arguments");
    *out = nullptr;
    MS_HIP(c, hipSetDevice(c->device));
    ms_bow_db *db = new ms_bow_db();
    ++g_ms_host_allocs;
    db->ctx = c; db->n_words = n_words;
    int rc = reserve_entries(db, std::max(initial_entries, 16));
    if (!rc) {
        db->pool_cap = std::max(4096ll, 2 * (initial_words + initial_words / 2 + initial_entries));
        hipError_t e = hipMalloc(&db->d_pool[0], 8 * (size_t)db->pool_cap);
        if (e == hipSuccess) e = hipMalloc(&db->d_pool[1], 8 * (size_t)db->pool_cap);
        g_ms_host_allocs += 2;
        if (e != hipSuccess) rc = ms_fail(c, MS_ERR_HIP, "bow db: pool allocation failed: %s", hipGetErrorString(e));
    }
    if (!rc) rc = grow_pinned(db, db->stage, db->stage_cap, (size_t)1 << 20);
    db->qdesc.reserve(1); db->moves.reserve(64);
    g_ms_host_allocs += 2;
    if (rc) { ms_bow_db_destroy(db); return rc; }
    *out = db;
    return MS_OK;
}

void ms_bow_db_destroy(ms_bow_db *db) {
    if (!db) return;
    (void)hipStreamSynchronize(db->ctx->stream);
    for (void *p : {(void *)db->d_ent, (void *)db->d_pool[0], (void *)db->d_pool[1], db->d_qdesc.p, db->d_qvec.p, db->d_state.p, db->d_common.p,
                    db->d_cand.p, db->d_chunk.p, db->d_result.p, db->d_moves.p, db->d_head.p})
        if (p) (void)hipFree(p);
    if (db->stage) (void)hipHostFree(db->stage);
    if (db->outp) (void)hipHostFree(db->outp);
    delete db;
}

int ms_bow_db_add(ms_bow_db *db, int32_t map_id, int32_t kf_id, int n, const int32_t *words, const double *values) {
    if (!db) return MS_ERR_INVALID;
    ms_ctx *c = db->ctx;
    int rc = check_vector(c, "bow db add", n, db->n_words, words, values);
    if (rc) return rc;
    const uint64_t key = id_key(map_id, kf_id);
    if (find_slot(db, key) >= 0) return ms_fail(c, MS_ERR_INVALID, "bow db add: (%d, %d) is already in the database", map_id, kf_id);
    MS_HIP(c, hipSetDevice(c->device));
    if (db->n_free == 0 && (rc = reserve_entries(db, db->n_slots + 1))) return rc;
    const long long cells = seg_cells(n);
    if ((rc = reserve_pool(db, cells))) return rc;
    const int slot = db->n_free > 0 ? db->free_slots[(size_t)--db->n_free] : db->n_slots++;
    DbEntry &e = db->ent[(size_t)slot];
    e = DbEntry{db->pool_top, n, map_id, kf_id, 1};
    if (n > 0) {
        uint8_t *st = nullptr;
        if ((rc = stage_take(db, 8 * (size_t)cells, &st))) return rc;
        std::memset(st, 0, 8 * (size_t)((n + 1) >> 1));
        std::memcpy(st, words, 4 * (size_t)n);
        std::memcpy(st + 8 * (size_t)((n + 1) >> 1), values, 8 * (size_t)n);
        MS_HIP(c, hipMemcpyAsync(db->d_pool[0] + e.off, st, 8 * (size_t)cells, hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = upload(db, db->d_ent + slot, &e, sizeof(DbEntry)))) return rc;
    db->pool_top += cells;
    db->live_cells += cells;
    ++db->n_live;
    hash_insert(db, key, slot);
    return MS_OK;
}

// BowIndex::add for a keyframe whose descent lies on the device: the segment is reserved for the bound of n words, k_bow_vector
// assembles the vector straight into it, and the host commits the entry only after the head {n_words, n_bad} has come down.
int ms_bow_db_add_words(ms_bow_db *db, int32_t map_id, int32_t kf_id, const int32_t *word_dev, const double *weight_dev, int n, int32_t *n_words) {
    if (!db) return MS_ERR_INVALID;
    ms_ctx *c = db->ctx;
    if (n_words) *n_words = 0;
    if (n < 0 || (n > 0 && (!word_dev || !weight_dev))) return ms_fail(c, MS_ERR_INVALID, "bow db add words: n = %d with missing arrays", n);
    if (n > MS_COVIS_MAX_STRIDE) return ms_fail(c, MS_ERR_CAPACITY, "bow db add words: %d keypoints, cap %d", n, MS_COVIS_MAX_STRIDE);
    if (reinterpret_cast<uintptr_t>(weight_dev) & 7u) return ms_fail(c, MS_ERR_INVALID, "bow db add words: weight must be 8-byte aligned");
    const uint64_t key = id_key(map_id, kf_id);
    if (find_slot(db, key) >= 0) return ms_fail(c, MS_ERR_INVALID, "bow db add words: (%d, %d) is already in the database", map_id, kf_id);
    MsRange range("bowIndexAddWords");
    MS_HIP(c, hipSetDevice(c->device));
    int rc;
    if (db->n_free == 0 && (rc = reserve_entries(db, db->n_slots + 1))) return rc;
    if ((rc = reserve_pool(db, seg_cells(n)))) return rc;                         // the bound: at most n words
    if ((rc = grow_dev(db, db->d_head, 16)) || (rc = grow_pinned(db, db->outp, db->out_cap, 16))) return rc;
    int32_t *head = static_cast<int32_t *>(db->d_head.p);
    if ((rc = ms_bow_vector_enqueue(c, word_dev, weight_dev, n, db->n_words, n, nullptr, nullptr, db->d_pool[0] + db->pool_top, head))) return rc;
    MS_HIP(c, hipMemcpyAsync(db->outp, head, 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = sync_stream(db))) return rc;
    const int32_t len = reinterpret_cast<const int32_t *>(db->outp)[0], n_bad = reinterpret_cast<const int32_t *>(db->outp)[1];
    if (n_bad > 0)
        return ms_fail(c, MS_ERR_INVALID, "bow db add words: %d kept keypoints have a word outside [0, %d) or a value that is not finite (the database is unchanged)", n_bad,
                       db->n_words);
    if (len < 0 || len > n) return ms_fail(c, MS_ERR_HIP, "bow db add words: the device counted %d words of %d keypoints", len, n);
    // ---- the commit: nothing above changed what a query sees
    const int slot = db->n_free > 0 ? db->free_slots[(size_t)db->n_free - 1] : db->n_slots;
    const DbEntry e{db->pool_top, len, map_id, kf_id, 1};
    if ((rc = upload(db, db->d_ent + slot, &e, sizeof(DbEntry)))) return rc;
    if (db->n_free > 0) --db->n_free; else ++db->n_slots;
    db->ent[(size_t)slot] = e;
    const long long cells = seg_cells(len);                                       // the unused tail of the bound is not consumed
    db->pool_top += cells;
    db->live_cells += cells;
    ++db->n_live;
    hash_insert(db, key, slot);
    if (n_words) *n_words = len;
    return MS_OK;
}

// A live entry's vector, downloaded: what keyframe.shared->bowVec held.
int ms_bow_db_entry(ms_bow_db *db, int32_t map_id, int32_t kf_id, int cap, int32_t *words_host, double *values_host, int *n) {
    if (!db) return MS_ERR_INVALID;
    ms_ctx *c = db->ctx;
    if (!n || cap < 0 || (cap > 0 && (!words_host || !values_host))) return ms_fail(c, MS_ERR_INVALID, "bow db entry: cap = %d with missing arrays", cap);
    *n = 0;
    const int slot = find_slot(db, id_key(map_id, kf_id));
    if (slot < 0) return ms_fail(c, MS_ERR_INVALID, "bow db entry: (%d, %d) is not in the database", map_id, kf_id);
    const DbEntry &e = db->ent[(size_t)slot];
    *n = e.len;
    if (e.len > cap) return ms_fail(c, MS_ERR_CAPACITY, "bow db entry: (%d, %d) has %d words, the arrays hold %d", map_id, kf_id, e.len, cap);
    if (e.len == 0) return MS_OK;
    MS_HIP(c, hipSetDevice(c->device));
    const size_t bytes = 8 * (size_t)seg_cells(e.len);
    int rc;
    if ((rc = grow_pinned(db, db->outp, db->out_cap, bytes))) return rc;
    MS_HIP(c, hipMemcpyAsync(db->outp, db->d_pool[0] + e.off, bytes, hipMemcpyDeviceToHost, c->stream));
    if ((rc = sync_stream(db))) return rc;
    std::memcpy(words_host, db->outp, 4 * (size_t)e.len);
    std::memcpy(values_host, db->outp + 8 * (size_t)((e.len + 1) >> 1), 8 * (size_t)e.len);
    return MS_OK;
}

int ms_bow_db_remove(ms_bow_db *db, int32_t map_id, int32_t kf_id) {
    if (!db) return MS_ERR_INVALID;
    const uint64_t key = id_key(map_id, kf_id);
    const int slot = find_slot(db, key);
    if (slot < 0) return MS_OK;                                                   // bow_index.cpp:50-57 finds nothing to erase
    DbEntry &e = db->ent[(size_t)slot];
    e.live = 0;
    const int32_t zero = 0;
    int rc = upload(db, &db->d_ent[slot].live, &zero, 4);
    if (rc) { e.live = 1; return rc; }
    db->live_cells -= seg_cells(e.len);
    --db->n_live;
    db->free_slots[(size_t)db->n_free++] = slot;
    hash_erase(db, key);
    return MS_OK;
}

int ms_bow_db_size(const ms_bow_db *db) { return db ? db->n_live : MS_ERR_INVALID; }

int ms_bow_db_query(ms_bow_db *db, int n, const int32_t *words, const double *values, int32_t ex_map, int32_t ex_kf,
                    float min_in_common_ratio, float score_ratio,
                    int max_out, int32_t *out_map, int32_t *out_kf, float *out_score, int *n_total) {
    if (!db || !n_total || max_out < 0 || (max_out > 0 && (!out_map || !out_kf || !out_score))) return MS_ERR_INVALID;
    ms_ctx *c = db->ctx;
    MsRange range("getBowSimilar");
    int rc = check_vector(c, "bow db query", n, db->n_words, words, values);
    if (rc) return rc;
    *n_total = 0;
    if (n == 0 || db->n_live == 0) return MS_OK;
    MS_HIP(c, hipSetDevice(c->device));
    const long long cells = seg_cells(n);
    if ((rc = grow_dev(db, db->d_qvec, 8 * (size_t)cells))) return rc;
    uint8_t *st = nullptr;
    if ((rc = stage_take(db, 8 * (size_t)cells, &st))) return rc;
    std::memset(st, 0, 8 * (size_t)((n + 1) >> 1));
    std::memcpy(st, words, 4 * (size_t)n);
    std::memcpy(st + 8 * (size_t)((n + 1) >> 1), values, 8 * (size_t)n);
    MS_HIP(c, hipMemcpyAsync(db->d_qvec.p, st, 8 * (size_t)cells, hipMemcpyHostToDevice, c->stream));
    const unsigned long long *qv = static_cast<const unsigned long long *>(db->d_qvec.p);
    db->qdesc.resize(1);                                                          // capacity reserved at create
    db->qdesc[0] = DbQuery{reinterpret_cast<const int32_t *>(qv), reinterpret_cast<const double *>(qv + ((n + 1) >> 1)), n, ex_kf != -1, ex_map, ex_kf};
    const int mo = std::max(1, std::min(max_out, db->n_slots));
    if ((rc = run_queries(db, 1, min_in_common_ratio, score_ratio, mo))) return rc;
    copy_out(db, 1, 0, mo, max_out, 0, out_map, out_kf, out_score, n_total);
    return MS_OK;
}

int ms_bow_db_query_ids(ms_bow_db *db, int q, const int32_t *map_ids, const int32_t *kf_ids,
                        float min_in_common_ratio, float score_ratio, int max_out_per_query,
                        int32_t *out_map, int32_t *out_kf, float *out_score, int *n_total) {
    if (!db || q < 0 || (q > 0 && (!map_ids || !kf_ids || !n_total)) || max_out_per_query < 0 ||
        (max_out_per_query > 0 && q > 0 && (!out_map || !out_kf || !out_score)))
        return MS_ERR_INVALID;
    ms_ctx *c = db->ctx;
    MsRange range("getBowSimilar");
    if (q == 0) return MS_OK;
    if (db->qdesc.capacity() < (size_t)q) ++g_ms_host_allocs;
    db->qdesc.resize((size_t)q);
    for (int i = 0; i < q; ++i) {
        const int slot = find_slot(db, id_key(map_ids[i], kf_ids[i]));
        if (slot < 0) return ms_fail(c, MS_ERR_INVALID, "bow db query_ids: (%d, %d) is not in the database", map_ids[i], kf_ids[i]);
        const DbEntry &e = db->ent[(size_t)slot];
        const unsigned long long *p = db->d_pool[0] + e.off;
        db->qdesc[(size_t)i] = DbQuery{reinterpret_cast<const int32_t *>(p), reinterpret_cast<const double *>(p + ((e.len + 1) >> 1)), e.len, 1, e.map_id, e.kf_id};
    }
    MS_HIP(c, hipSetDevice(c->device));
    const int mo = std::max(1, std::min(max_out_per_query, db->n_slots));
    int rc = run_queries(db, q, min_in_common_ratio, score_ratio, mo);
    if (rc) return rc;
    for (int i = 0, at = 0; i < q; ++i) at += copy_out(db, q, i, mo, max_out_per_query, at, out_map, out_kf, out_score, n_total);
    return MS_OK;
}

}  // extern "C"
