"""The BowVector on the device against tests/bow_vector_ref.py, its specification: ms_bow_vector's words, value bits and
counts at the sizes where a path changes, with canaries behind both outputs and the same bytes on a second call; every refusal with the
outputs untouched; ms_bow_db_add_words against the host path (the restatement plus ms_bow_db_add into a twin database), entry by entry and
query by query, through compaction and growth of a small pool; and the chain extractor -> ms_keyframe_admit -> ms_keyframe_admit_words ->
add_words against the admission's downloaded descent."""
import ctypes as C
import functools

import numpy as np
import pytest

import bow_synth
import bow_vector_ref as R
import keyframe_admit_ref as KR
import mi355slam

pytestmark = pytest.mark.gpu
CAN, PAD = 0x5A, 16
VOCAB = 100_000
CUR = 0x7FFFFFFF                                             # any map id
INVALID, CAPACITY = mi355slam.MS_ERR_INVALID, mi355slam.MS_ERR_CAPACITY


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def reference(key):
    """The restatement, computed once per input (the inputs are built from their key alone)."""
    word, weight, vocab = make_input(key)
    return R.bow_vector(word, weight, vocab)


def make_input(key):
    kind = key[0]
    if kind == "size":
        _, n, layout = key
        rng = np.random.default_rng(1000 + n)
        if layout == "distinct":
            word = rng.permutation(VOCAB)[:n].astype(np.int32)
        elif layout == "one word":
            word = np.full(n, 4242, np.int32)
        else:                                                # about three keypoints per word, scattered
            pool = rng.choice(VOCAB, max(1, n // 3), replace=False)
            word = pool[rng.integers(0, len(pool), n)].astype(np.int32)
        weight = np.exp2(rng.uniform(-12.0, 4.0, n))         # sums that depend on their order
        if n > 4:
            weight[rng.random(n) < 0.05] = 0.0               # stop words
        return word, weight, VOCAB
    if kind == "placement":
        # equal words adjacent in i, maximally apart, and straddling the multiples of 64, 256 and 1024; the words 0 and VOCAB - 1
        n = 2100
        rng = np.random.default_rng(7)
        word = (1000 + rng.permutation(50_000)[:n]).astype(np.int32)      # distinct fillers
        for w, places in ((0, (0, n - 1)), (VOCAB - 1, (10, 11, 12)), (7, (63, 64)), (8, (255, 256)), (9, (1023, 1024)), (10, (2047, 2048, 64 * 3 - 1, 64 * 3)),
                          (11, (1, 1025, 2049)), (60_000, (500, 501)), (1, (2, 2098)), (VOCAB - 2, (1500, 3))):
            word[list(places)] = w
        return word, np.exp2(rng.uniform(-20.0, 6.0, n)), VOCAB
    if kind == "order":
        return R.order_sensitive()
    if kind == "case":
        word, weight = R.cases(VOCAB)[key[1]]
        return word, weight, VOCAB
    raise KeyError(key)


def run(ctx, word, weight, vocab, cap=None, n=None):
    """One ms_bow_vector call on fresh buffers filled with a canary.  Returns (rc, n_words, n_bad, words bytes, values bytes), the output buffers in
    full, canaries behind them included."""
    n = len(word) if n is None else n
    cap = max(n, 1) if cap is None else cap
    dw = ctx.upload(np.ascontiguousarray(word, np.int32) if len(word) else np.zeros(1, np.int32))
    dwt = ctx.upload(np.ascontiguousarray(weight, np.float64) if len(weight) else np.zeros(1, np.float64))
    ow, ov = ctx.upload(np.full(4 * cap + PAD, CAN, np.uint8)), ctx.upload(np.full(8 * cap + PAD, CAN, np.uint8))
    rc, n_words, n_bad = mi355slam.bow_vector_device(ctx, dw, dwt, n, vocab, cap, ow, ov)
    out = rc, n_words, n_bad, ow.download(np.uint8, (4 * cap + PAD,)), ov.download(np.uint8, (8 * cap + PAD,))
    for b in (dw, dwt, ow, ov):
        b.free()
    return out


def untouched(raw):
    return (raw == CAN).all()


def check_against_reference(ctx, key, label=None):
    word, weight, vocab = make_input(key)
    words, values, n_words, n_bad = reference(key)
    assert n_bad == 0
    rc, gn, gb, raw_w, raw_v = run(ctx, word, weight, vocab)
    assert (rc, gn, gb) == (0, n_words, 0), (label or key, rc, gn, gb, n_words, mi355slam.lib().ms_last_error(ctx._h))
    assert same_bits(raw_w[:4 * n_words].view(np.int32), words), label or key
    assert same_bits(raw_v[:8 * n_words].view(np.float64), values), label or key
    assert untouched(raw_w[4 * n_words:]) and untouched(raw_v[8 * n_words:]), label or key      # nothing behind the vector, the canaries included
    again = run(ctx, word, weight, vocab)
    assert again[:3] == (rc, gn, gb) and same_bits(again[3], raw_w) and same_bits(again[4], raw_v), label or key
    return n_words


# ---- 1. ms_bow_vector against the restatement
@pytest.mark.parametrize("layout", ["distinct", "one word", "three per word"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 2000, 8192])
def test_sizes_at_which_a_path_changes(ctx, n, layout):
    n_words = check_against_reference(ctx, ("size", n, layout))
    if n >= 63:
        assert n_words == 1 if layout == "one word" else n_words > n // 4


def test_placements_of_equal_words_and_the_first_and_last_word_of_the_vocabulary(ctx):
    key = ("placement",)
    word, weight, vocab = make_input(key)
    words = reference(key)[0]
    assert words[0] == 0 and words[-1] == VOCAB - 1 and len(words) == 2100 - 14 and len(set(word[[63, 64]])) == len(set(word[[1023, 1024]])) == 1
    check_against_reference(ctx, key)


def test_the_order_sensitive_input(ctx):
    """tests/test_bow_vector_ref.py asserts that descending segments, a descending norm and pairwise sums each give other bits for this input."""
    check_against_reference(ctx, ("order",))


@pytest.mark.parametrize("name", list(R.cases(VOCAB)))
def test_the_named_cases_of_the_restatement(ctx, name):
    check_against_reference(ctx, ("case", name))


def test_a_capacity_one_short_and_bad_inputs_are_refused_with_the_outputs_untouched(ctx):
    message = lambda: mi355slam.lib().ms_last_error(ctx._h).decode()
    key = ("size", 257, "three per word")
    word, weight, vocab = make_input(key)
    n_words = reference(key)[2]
    rc, gn, gb, raw_w, raw_v = run(ctx, word, weight, vocab, cap=n_words - 1)
    assert rc == CAPACITY and (gn, gb) == (n_words, 0) and untouched(raw_w) and untouched(raw_v) and "%d words, the outputs hold %d" % (n_words, n_words - 1) in message()
    rc, gn, gb, raw_w, raw_v = run(ctx, word, weight, vocab, cap=n_words)       # exactly enough
    assert rc == 0 and gn == n_words and same_bits(raw_v[:8 * n_words].view(np.float64), reference(key)[1]) and untouched(raw_v[8 * n_words:])
    kept = np.flatnonzero(weight > 0)
    for bad_word in (VOCAB, -1, -2**31, 2**31 - 1):
        for at in (kept[0], kept[-1]):
            w = word.copy()
            w[at] = bad_word
            assert R.bow_vector(w, weight, vocab)[3] == 1
            rc, gn, gb, raw_w, raw_v = run(ctx, w, weight, vocab)
            assert rc == INVALID and gb == 1 and untouched(raw_w) and untouched(raw_v) and "1 kept keypoints have a word outside [0, %d)" % VOCAB in message(), (bad_word, at)
            wt = weight.copy()
            wt[at] = 0.0                                     # the same word at weight 0 is never looked at
            want = R.bow_vector(w, wt, vocab)
            rc, gn, gb, raw_w, raw_v = run(ctx, w, wt, vocab)
            assert (rc, gn, gb) == (0, want[2], 0) and same_bits(raw_v[:8 * gn].view(np.float64), want[1]) and same_bits(raw_w[:4 * gn].view(np.int32), want[0])
    wt = weight.copy()
    wt[kept[3]] = np.inf
    assert R.bow_vector(word, wt, vocab)[3] == 1
    rc, gn, gb, raw_w, raw_v = run(ctx, word, wt, vocab)
    assert rc == INVALID and gb == 1 and untouched(raw_w) and untouched(raw_v)
    # the host validation runs in front of the device: nothing is written, the counts included
    counts = np.full(2, -77, np.int32)
    buf = ctx.alloc(64)
    rc = mi355slam.lib().ms_bow_vector(ctx._h, mi355slam._vp(buf), mi355slam._vp(buf), 8193, VOCAB, 4, mi355slam._vp(buf), mi355slam._vp(buf), mi355slam._vp(counts))
    assert rc == CAPACITY and (counts == -77).all() and "8193 keypoints" in message()
    rc = mi355slam.lib().ms_bow_vector(ctx._h, mi355slam._vp(buf), mi355slam._vp(buf), 4, 0, 4, mi355slam._vp(buf), mi355slam._vp(buf), mi355slam._vp(counts))
    assert rc == INVALID and (counts == -77).all() and "a vocabulary of 0 words" in message()
    buf.free()


def test_the_binding_takes_host_arrays(ctx):
    key = ("size", 257, "three per word")
    word, weight, vocab = make_input(key)
    words, values = mi355slam.bow_vector(ctx, word, weight, len(word), vocab)
    assert same_bits(words, reference(key)[0]) and same_bits(values, reference(key)[1])
    with pytest.raises(mi355slam.MsError):
        mi355slam.bow_vector(ctx, np.array([VOCAB], np.int32), np.array([1.0]), 1, vocab)


# ---- 2. add_words against the host path
def descent(rng, place, n=300, per_place=400):
    """A keyframe's word / weight per keypoint: most words from its place's share of the vocabulary, some from anywhere, stop words at weight 0."""
    own = place * per_place + rng.integers(0, per_place, n)
    word = np.where(rng.random(n) < 0.8, own, rng.integers(0, VOCAB, n)).astype(np.int32)
    weight = np.exp2(rng.uniform(-6.0, 3.0, n))
    weight[rng.random(n) < 0.08] = 0.0
    return word, weight


def query_same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and
            same_bits(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2], np.float32).view(np.uint32)))


class Twins:
    """One database filled through add_words, its twin through the restatement and ms_bow_db_add."""

    def __init__(self, ctx, **kw):
        self.ctx, self.dev, self.host, self.live = ctx, mi355slam.BowDatabase(ctx, VOCAB, **kw), mi355slam.BowDatabase(ctx, VOCAB, **kw), {}

    def add(self, kf, word, weight):
        words, values, n_words, n_bad = R.bow_vector(word, weight, VOCAB)
        assert n_bad == 0
        assert self.dev.add_words(CUR, kf, word, weight) == n_words
        self.host.add(CUR, kf, words, values)
        self.live[kf] = (words, values)

    def remove(self, kf):
        self.dev.remove(CUR, kf); self.host.remove(CUR, kf)
        del self.live[kf]

    def check_entries(self, kfs=None):
        assert self.dev.size == self.host.size == len(self.live)
        for kf in (self.live if kfs is None else kfs):
            for db in (self.dev, self.host):
                w, v = db.entry(CUR, kf)
                assert same_bits(w, self.live[kf][0]) and same_bits(v, self.live[kf][1]), kf

    def check_queries(self, ids, vectors, grid):
        for mr, sr in grid:
            a, b = self.dev.query_ids(ids, mr, sr), self.host.query_ids(ids, mr, sr)
            assert all(query_same(x, y) for x, y in zip(a, b)), (mr, sr)
            for w, v in vectors:
                assert query_same(self.dev.query(w, v, None, mr, sr), self.host.query(w, v, None, mr, sr)), (mr, sr)

    def close(self):
        self.dev.close(); self.host.close()


GRID = [(mr, sr) for mr in (0.0, 0.5, 0.8, 1.0) for sr in (0.0, 0.75, 1.0)]      # the ratio grid of test_gpu_bow_db.py


def test_a_hundred_entries_equal_the_host_path_entry_by_entry_and_query_by_query(ctx):
    rng = np.random.default_rng(31)
    t = Twins(ctx, capacity=32)
    for kf in range(100):
        n = int(rng.integers(150, 400)) if kf % 10 else (0, 1, 2000)[kf // 10 % 3]
        t.add(kf, *descent(rng, kf % 8, n))
    t.check_entries()
    assert len(t.live[0][0]) == 0 and len(t.live[20][0]) > 500      # n_words = 0 is an entry; a long one
    ids = [(CUR, kf) for kf in range(100)]                   # every entry is a query, over the whole grid
    vectors = [R.bow_vector(*descent(rng, p), VOCAB)[:2] for p in (0, 5)]
    t.check_queries(ids, vectors, GRID)
    r = t.dev.query_ids([(CUR, 57)], 0.0, 0.0)[0]
    assert len(r[0]) >= 10 and r[1][0] % 8 == 57 % 8           # its own place ranks first: the scores are real
    t.close()


def test_a_small_pool_goes_through_compaction_and_growth(ctx):
    """A pool of 4096 cells (the smallest) and keyframes of 300 keypoints (a bound of 450 cells, about 330 used).  Phase 1 keeps 4 entries live:
    the top reaches the end every dozen adds while live + bound stays under 3/4 of the pool, so reserve_pool compacts.  Phase 2 removes nothing:
    live + bound passes 3/4 and the pool grows.  An entry whose len or whose share of pool_top the host got wrong is overwritten by a later one or
    cut by a compaction."""
    lib = mi355slam.lib()
    lib.ms_debug_host_allocs.restype = C.c_longlong
    rng = np.random.default_rng(32)
    t = Twins(ctx, capacity=4, words_per_entry=1)
    cells = 0
    for kf in range(40):
        t.add(kf, *descent(rng, kf % 8))
        n = len(t.live[kf][0])
        cells += (n + 1) // 2 + n
        if kf >= 4:
            t.remove(kf - 4)
        if kf % 13 == 12:
            t.check_entries()
    assert cells > 2 * 4096 and sum((len(w) + 1) // 2 + len(w) for w, _ in t.live.values()) + 450 < 3 * 4096 // 4      # filled twice over, never near the growth rule
    t.check_entries()
    t.check_queries([(CUR, kf) for kf in t.live], [], [(0.0, 0.0), (0.8, 0.75)])
    before = lib.ms_debug_host_allocs()
    for kf in range(40, 60):
        t.add(kf, *descent(rng, kf % 8))
    assert sum((len(w) + 1) // 2 + len(w) for w, _ in t.live.values()) > 4096 and lib.ms_debug_host_allocs() > before      # more than the first pool held
    t.check_entries()
    t.check_queries([(CUR, kf) for kf in list(t.live)[::5]], [R.bow_vector(*descent(rng, 3), VOCAB)[:2]], [(0.0, 0.0), (0.5, 0.75)])
    t.close()


def test_a_sliding_window_allocates_nothing_once_warm(ctx):
    lib = mi355slam.lib()
    lib.ms_debug_host_allocs.restype = C.c_longlong
    rng = np.random.default_rng(33)
    on_device = []
    for i in range(8):                                       # the descents lie on the device before the window starts
        word, weight = descent(rng, i)
        on_device.append((ctx.upload(word), ctx.upload(weight), len(word), R.bow_vector(word, weight, VOCAB)))
    db = mi355slam.BowDatabase(ctx, VOCAB, capacity=64, words_per_entry=100)      # 19 328 cells: the window of 40 compacts every 60 adds or so
    counts = []
    for kf in range(200):
        dw, dwt, n, want = on_device[kf % 8]
        rc, n_words = db.add_words_device(CUR, kf, dw, dwt, n)
        assert rc == 0 and n_words == want[2]
        if kf >= 40:
            db.remove(CUR, kf - 40)
        if kf % 25 == 0:
            w, v = db.entry(CUR, kf)
            assert same_bits(w, want[0]) and same_bits(v, want[1])
        counts.append(lib.ms_debug_host_allocs())
    assert counts[-1] == counts[100], (counts[100], counts[-1])
    assert db.size == 40
    for kf in (160, 199):
        w, v = db.entry(CUR, kf)
        assert same_bits(w, on_device[kf % 8][3][0]) and same_bits(v, on_device[kf % 8][3][1])
    db.close()
    for dw, dwt, _, _ in on_device:
        dw.free(); dwt.free()


def test_a_refused_add_leaves_the_database_unchanged_and_the_id_free(ctx):
    rng = np.random.default_rng(34)
    t = Twins(ctx, capacity=8)
    for kf in range(12):
        t.add(kf, *descent(rng, kf % 3))
    ids = [(CUR, kf) for kf in (0, 5, 11)]
    probe = R.bow_vector(*descent(rng, 1), VOCAB)[:2]
    before = [t.dev.query_ids(ids, 0.0, 0.0), t.dev.query(*probe, None, 0.0, 0.0)]
    word, weight = descent(rng, 2)
    bad = word.copy()
    bad[np.flatnonzero(weight > 0)[5]] = VOCAB
    message = lambda: mi355slam.lib().ms_last_error(ctx._h).decode()
    with pytest.raises(mi355slam.MsError):
        t.dev.add_words(CUR, 5, word, weight)                # a duplicate id
    assert "(%d, 5) is already in the database" % CUR in message()
    with pytest.raises(mi355slam.MsError):
        t.dev.add_words(CUR, 77, bad, weight)                # a word outside the vocabulary
    assert "1 kept keypoints have a word outside" in message()
    inf = weight.copy()
    inf[np.flatnonzero(weight > 0)[0]] = np.inf
    with pytest.raises(mi355slam.MsError):
        t.dev.add_words(CUR, 77, word, inf)
    assert t.dev.size == 12
    rc, n, w, v = t.dev.entry_device(CUR, 77, 4)
    assert rc == INVALID and n == 0
    after = [t.dev.query_ids(ids, 0.0, 0.0), t.dev.query(*probe, None, 0.0, 0.0)]
    assert all(query_same(x, y) for x, y in zip(before[0], after[0])) and query_same(before[1], after[1])
    t.check_entries()
    t.add(77, word, weight)                                  # the same id with good input
    t.check_entries([77, 11])
    t.check_queries(ids + [(CUR, 77)], [probe], [(0.0, 0.0), (0.8, 0.75)])
    # entry: a capacity one short reports the length and writes nothing
    n_words = len(t.live[77][0])
    rc, n, w, v = t.dev.entry_device(CUR, 77, n_words - 1)
    assert rc == CAPACITY and n == n_words and (w == -7).all() and (v == -7.0).all()
    t.close()


# ---- 3. the chain
def test_extractor_to_admit_to_add_words_equals_the_downloaded_descent(ctx, oracle):
    lib = mi355slam.lib()
    fresh = mi355slam.Context(0)
    assert mi355slam.keyframe_admit_words_device(fresh) == (INVALID, 0, 0, 0)      # before any admit
    fresh.close()
    imgs = np.stack([oracle.synth_frame(640, 480, 1000, 2 * i, i) for i in range(2)])
    ex = mi355slam.OrbExtractor(ctx, 640, 480, max_kpts=1000, max_batch=2)
    ex.extract(imgs)
    ctx.sync()
    v = bow_synth.make_vocab(22, k=10, depth=3, stop_words=0.1)
    vocab = mi355slam.BowVocabulary(ctx, v["parent"], v["desc"], v["weight"], v["word"], v["depth_levels"])
    n_vocab = int(v["word"].max()) + 1
    view, cap, stride = ex.device_view(), ex.capacity, ex.capacity + 7
    tables = KR.empty_tables(2, stride, 2 * stride, 1)
    tab = {k: ctx.upload(tables[k]) for k in KR.TABLES}
    frames = [mi355slam.AdmitFrame(ctx, cap) for _ in range(2)]
    dev, host = mi355slam.BowDatabase(ctx, n_vocab), mi355slam.BowDatabase(ctx, n_vocab)
    cam = (520.25, 519.5, 318.75, 241.125, 640, 480)
    try:
        for f in range(2):
            args = dict(slot=f, desc_base=f * stride, pose=np.arange(12.0) + f, cam=cam, levels_up=1, vocab=vocab)
            rc, r = mi355slam.keyframe_admit_device(ctx, view, f, tab, 2, stride, 50, 2 * stride, args, frames[f], host=("word", "weight"))
            assert rc == 0 and r["counts"][0] > 500, lib.ms_last_error(ctx._h)
            dw, dwt, n = mi355slam.keyframe_admit_words(ctx)
            assert n == r["counts"][0] and dw and dwt
            word, weight = np.zeros(n, np.int32), np.zeros(n, np.float64)
            ctx.check(lib.ms_dev_download(ctx._h, mi355slam._vp(word), C.c_void_p(dw), C.c_size_t(4 * n)), "ms_dev_download")
            ctx.check(lib.ms_dev_download(ctx._h, mi355slam._vp(weight), C.c_void_p(dwt), C.c_size_t(8 * n)), "ms_dev_download")
            assert same_bits(word, r["word"]) and same_bits(weight, r["weight"]) and (weight == 0).any() and (weight > 0).sum() > 400
            words, values, n_words, n_bad = R.bow_vector(r["word"], r["weight"], n_vocab)
            assert n_bad == 0 and 50 < n_words < n                # words are shared: the sums are real
            assert dev.add_words(CUR, f, dw, dwt, n) == n_words
            host.add(CUR, f, words, values)
            got = dev.entry(CUR, f)
            assert same_bits(got[0], words) and same_bits(got[1], values) and same_bits(host.entry(CUR, f)[1], values)
            kw, kv = KR.bow_vector(r["word"], r["weight"])        # the restatement 9.19 pinned
            assert np.array_equal(kw, words) and same_bits(kv, values)
        for mr, sr in ((0.0, 0.0), (0.8, 0.75)):
            a, b = dev.query_ids([(CUR, 0), (CUR, 1)], mr, sr), host.query_ids([(CUR, 0), (CUR, 1)], mr, sr)
            assert all(query_same(x, y) for x, y in zip(a, b)) and (mr > 0 or list(a[0][1]) == [1])
        # an admit that is refused takes the descent away: by the host validation, and by the device's verdict
        rc, _ = mi355slam.keyframe_admit_device(ctx, view, 0, tab, 2, stride, 50, 2 * stride, dict(slot=2, desc_base=0, pose=np.arange(12.0), cam=cam), frames[0], host=False)
        assert rc == INVALID and mi355slam.keyframe_admit_words_device(ctx) == (INVALID, 0, 0, 0)
        rc, r = mi355slam.keyframe_admit_device(ctx, view, 0, tab, 2, stride, 50, 2 * stride, dict(slot=0, desc_base=0, pose=np.arange(12.0), cam=cam), frames[0], host=False)
        assert rc == 0 and mi355slam.keyframe_admit_words_device(ctx)[0] == 0      # no vocabulary: word = -1, weight = 0
        dw, dwt, n = mi355slam.keyframe_admit_words(ctx)
        assert dev.add_words(CUR, 2, dw, dwt, n) == 0 and len(dev.entry(CUR, 2)[0]) == 0
        rc, _ = mi355slam.keyframe_admit_device(ctx, view, 0, tab, 2, stride, 50, 100, dict(slot=1, desc_base=0, pose=np.arange(12.0), cam=cam), frames[0], host=False)
        assert rc == CAPACITY and mi355slam.keyframe_admit_words_device(ctx) == (INVALID, 0, 0, 0)
        with pytest.raises(mi355slam.MsError):
            mi355slam.keyframe_admit_words(ctx)
    finally:
        dev.close(); host.close(); vocab.close(); ex.close()
        for b in tab.values():
            b.free()
        for fr in frames:
            fr.free()
