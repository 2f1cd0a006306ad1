#pragma once
// ba_handle.h -- host side: struct ms_ba, the team launches of this process, host scratch of ms_ba_create.  Used by ba_prep.h and the entry points.
// Included by ba.hip only, like ba_prep.h: both use the types and kernels of its anonymous namespace.

struct ms_ba {
    ms_ctx *ctx = nullptr;
    int n = 0;
    std::vector<BaProb> host;          // device pointers inside
    std::vector<ms_ba_problem> dims;   // sizes only
    BaProb *d_probs = nullptr;
    // k_ba_lm's fused trial schedule: the same descriptors with Hpp / bp / Hll / bl pointing at a second set of arrays (behind d_probs on the device); alt_ptrs[i].Hpp == nullptr:
    // problem i has no second set and the whole handle runs the plain schedule
    struct AltPtrs { double *Hpp, *bp, *Hll, *bl; };
    std::vector<AltPtrs> alt_ptrs;
    std::vector<BaProb> host_alt;
    BaProb *d_probs_alt = nullptr;
    bool alt_ok = false;
    char *d_arena = nullptr;
    size_t arena_bytes = 0;
    int team = 0;                      // workgroups per problem of the next launch (ms_ba_set_team; 0 = automatic)
    int factor_team = 0;               // of these, workgroups in the distributed Cholesky of a large system (ms_ba_set_factor_team; 0 = automatic)
    std::vector<double> chol_tiles;    // per problem: row tiles a Cholesky panel touches on average
    int cus = 0;
    bool pose_only = false;            // every problem has ONE free pose and only fixed points: k_ba_pose_only instead of k_ba_lm (poseBundleAdjust)
    bool one_pose = false;             // every problem has ONE free pose and at least one free point: k_ba_one_pose (stage 1 of localBundleAdjust)
    int one_pose_lg = 0;               // log2 of the lanes per point of the last k_ba_one_pose launch
    bool last_one_pose = false;        // the last launch was k_ba_one_pose (its fallback after a barrier gave up is the same kernel with one workgroup)
    int launched_team = 1;             // team size of the last launch
    bool team_checked = true;          // the last team launch has been looked at (every problem's gave-up marker) and, if need be, repeated
    int debug_fail_barriers = 0;       // test hook: team barriers give up at once (ms_ba_debug_fail_team_barriers)
    int team_fallbacks = 0;            // launches repeated with one workgroup per problem after a team barrier gave up
    int solves = 0;                    // launches so far (ms_ba_copy_state refuses a source that has never been solved)
    // a single small problem (poseBundleAdjust): its results are packed and copied into h_result right behind the solver launch, so that ms_ba_download only
    // waits for ev_done and reads them -- no pack launch and device-to-host round trip after the wait (0.03 ms of a 0.08 ms solve)
    void *h_result = nullptr;          // page-locked, stays with the handle OBJECT (pooled per context)
    size_t h_result_bytes = 0, pack_doubles = 0;
    double *d_pack = nullptr;          // in the arena; nullptr: no eager results for this handle
    int32_t *h_verdict = nullptr;      // page-locked word, stays with the handle object: "a team barrier gave up somewhere in the last launch", collected behind every team launch
    bool verdict_eager = false;        // h_verdict belongs to the last launch
    bool eager = false;                // h_result holds the last launch's results
    bool self_packed = false;          // the last launch was k_ba_pose_only with BaProb::pack set: d_pack is already what k_ba_pack_result would write
    bool work_dirty = false;           // a pose-only handle whose work areas [work_lo[p], work_hi[p]) were never cleared: the general kernel needs them zero (ms_ba_solve)
    std::vector<size_t> work_lo, work_hi;
    bool quiet = false;                // everything this handle put on the stream is known to have finished (ev_done was seen, nothing enqueued since): ms_ba_destroy need not wait
    hipEvent_t ev_done = nullptr;      // the end of this handle's last launch (what reads its results waits for it ON THE HOST, politely: ba_wait_event)
    bool pending = false;
};

// Team launches of this process, per device: what is (or may still be) running, so that the workgroups of all concurrent team launches
// together never exceed the CUs (see ms_ba_solve)
struct TeamLaunch { hipEvent_t ev; hipStream_t stream; int wgs; bool live; };
static std::mutex g_team_mu;
static std::vector<TeamLaunch> g_team_live[64];
static int g_team_query_errors = 0;        // hipEventQuery answers other than success / not-ready seen by the admission list (guarded by g_team_mu)
#define MS_TRY_BA(x) do { int rc__ = (x); if (rc__ != MS_OK) return rc__; } while (0)

constexpr size_t kBaEagerMax = (size_t)64 << 10;        // results of a single problem up to this size are packed and copied behind every launch (ms_ba struct: h_result).
                                                        // (Tried at 512 KB, i.e. for a whole C4 window too: -0.025 ms for the window alone, but the front end of the same
                                                        //  sequence, running beside it, fell from 2.7-3.0 k to 2.0-2.2 k frames/s; kept for small problems)
constexpr size_t kBaStageMax = (size_t)4 << 20;        // creates whose inputs fit are uploaded from the context's page-locked staging block without a wait
// SE3 edges that touch pose `pi` (k_ba_pose_only / k_ba_one_pose keep their constants in PO_MAXE LDS slots; edges between fixed poses need none)
static int ba_edges_at_free_pose(const ms_ba_problem &Q, int pi) {
    int t = 0;
    for (int k = 0; k < Q.n_pose_edge; ++k) t += Q.edge_i[k] == pi || Q.edge_j[k] == pi;
    return t;
}
// the descriptors of the second linearisation set: host_alt[i] = host[i] with the four output arrays exchanged (rebuilt whenever host[] is about to be uploaded: the
// two must agree in everything else -- team sizes included)
static void ba_make_alt(ms_ba *B) {
    B->host_alt.assign(B->host.begin(), B->host.end());
    B->alt_ok = !B->host.empty() && B->alt_ptrs.size() == B->host.size();
    for (size_t i = 0; i < B->host_alt.size() && B->alt_ok; ++i) {
        const ms_ba::AltPtrs &a = B->alt_ptrs[i];
        if (!a.Hpp) { B->alt_ok = false; break; }
        BaProb &q = B->host_alt[i];
        q.Hpp = a.Hpp; q.bp = a.bp; q.Hll = a.Hll; q.bl = a.bl;
    }
}
// (both descriptor sets, in stream order)
static hipError_t ba_upload_descriptors(ms_ba *B, hipStream_t st) {
    ba_make_alt(B);
    hipError_t e = hipMemcpyAsync(B->d_probs, B->host.data(), sizeof(BaProb) * B->n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(B->d_probs_alt, B->host_alt.data(), sizeof(BaProb) * B->n, hipMemcpyHostToDevice, st);
    return e;
}
// The end of a handle's last launch, as an event the handle owns: whatever reads the launch's results waits for it ON THE HOST, politely (ba_wait_event), before it
// enqueues anything -- not with hipStreamSynchronize, and not with a wait packet behind the launch (round 4, tools/hog_probe.py: a stream with packets queued behind
// a 2 ms kernel slowed the front end of ANOTHER sequence 10 ... 90 x, one that holds one launch at a time 3 ... 15 x).
static int ba_launch_done(ms_ctx *c, ms_ba *B) {
    B->quiet = false;
    if (!B->ev_done) { MS_HIP(c, hipEventCreateWithFlags(&B->ev_done, hipEventDisableTiming)); ++g_ba_host_allocs; }
    MS_HIP(c, hipEventRecord(B->ev_done, c->stream));
    B->pending = true;
    return MS_OK;
}
static void ba_delete_object(ms_ba *B) {
    if (B->ev_done) (void)hipEventDestroy(B->ev_done);
    if (B->h_result) (void)hipHostFree(B->h_result);
    if (B->h_verdict) (void)hipHostFree(B->h_verdict);
    delete B;
}
// A host wait for a solver launch (milliseconds) that leaves the processor to the other sequences' threads: hipStreamSynchronize / hipEventSynchronize spin, and
// seven threads spinning in them made the thread that drives another sequence's front end 3 ... 15 x slower (tools/hog_probe.py: x 3.3 beside two streams whose
// threads wait in hipStreamSynchronize, x 1.09 beside the same streams with the threads asleep) -- on this runtime a waiting thread is not free for the others.
// Two phases: for the first ~120 us the event is polled with a yield in between (poseBundleAdjust's launch is 0.08 ms: a frame must not pay a timer's granularity
// for it), after that the thread sleeps 20 us at a time, with its timer slack set to 1 us once (the default 50 us slack turned every 25 us sleep into ~75 us:
// 0.18 ms in ms_ba_download for a 0.08 ms kernel, tools/pose_path_probe.py).
static int ba_wait_event(ms_ctx *c, hipEvent_t ev) {
    thread_local bool slack_set = false;
    constexpr auto kSpin = std::chrono::microseconds(120), kSleep = std::chrono::microseconds(20);
    static const bool fine_slack = !std::getenv("MS_WAIT_COARSE");
    const auto t0 = std::chrono::steady_clock::now();
    for (bool spinning = true;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return MS_OK;
        if (q != hipErrorNotReady) { (void)hipGetLastError(); return ms_fail(c, MS_ERR_HIP, "waiting for a solver launch failed: %s", hipGetErrorString(q)); }
        if (spinning) {
            std::this_thread::yield();
            spinning = std::chrono::steady_clock::now() - t0 < kSpin;
        } else {
            if (!slack_set && fine_slack) { (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL); slack_set = true; }      // (nanoseconds; the calling thread only)
            std::this_thread::sleep_for(kSleep);
        }
    }
}
static int ba_wait_pending(ms_ba *B) {
    if (!B->pending) return MS_OK;
    MS_TRY_BA(ba_wait_event(B->ctx, B->ev_done));
    B->pending = false;
    B->quiet = true;
    return MS_OK;
}

// ---------------------------------------------------------------- host scratch of ms_ba_create: no allocation per window after warm-up
// Everything ms_ba_create builds on the host (index structures, batch lists, the streams: ~40 arrays per problem) lives in a per-thread bump arena that keeps its
// memory from call to call: a sliding-window BA per keyframe allocates nothing once the first windows have sized it.  (A batch that does not fit overflows into
// plain blocks, freed at the next call.)  g_ba_host_allocs counts every allocation this file makes on the host or the device -- arena growth, overflow blocks,
// handle objects, device blocks, events -- so a test can hold "none after warm-up" against it (ms_debug_host_allocs; tests/host_shim_smoke.cpp).
struct BaArena {
    static constexpr size_t kKeepMax = (size_t)64 << 20;            // what a thread keeps between calls: enough for a handful of windows per call, not for a 256-window batch
    char *base = nullptr;
    size_t cap = 0, used = 0, total = 0;
    std::vector<void *> overflow;
    void begin() {                                                  // start of a create: nothing of the previous call is alive any more
        const size_t want = std::min(kKeepMax, total + total / 4);
        if (want > cap) { std::free(base); cap = ms_align_up(want, (size_t)1 << 20); base = static_cast<char *>(std::malloc(cap)); ++g_ba_host_allocs; }
        used = 0; total = 0;
    }
    void end() {                                                    // end of a create: what did not fit goes back at once (the arena itself stays)
        for (void *p : overflow) std::free(p);
        overflow.clear();
    }
    void *take(size_t bytes, size_t align) {
        const size_t at = ms_align_up(used, align);
        total = ms_align_up(total, align) + bytes;
        if (base && at + bytes <= cap) { used = at + bytes; return base + at; }
        void *p = std::malloc(bytes ? bytes : 1);
        ++g_ba_host_allocs;
        overflow.push_back(p);
        return p;
    }
    ~BaArena() { end(); std::free(base); }
};
static thread_local BaArena tl_ba_arena;
template <class T>
struct BaAlloc {
    typedef T value_type;
    BaAlloc() = default;
    template <class U> BaAlloc(const BaAlloc<U> &) {}
    T *allocate(size_t n) { return static_cast<T *>(tl_ba_arena.take(n * sizeof(T), alignof(T) < 16 ? 16 : alignof(T))); }
    void deallocate(T *, size_t) {}
    template <class U> bool operator==(const BaAlloc<U> &) const { return true; }
    template <class U> bool operator!=(const BaAlloc<U> &) const { return false; }
};
template <class T> using bvec = std::vector<T, BaAlloc<T>>;
