"""ms_bow_db (BowIndex::add / remove / getBowSimilar on the device) against the plain restatement in tests/bow_db_ref.py:
the same ids in the same order and the same float32 score bits, for both query forms."""
import ctypes
import subprocess

import numpy as np
import pytest

import bow_db_ref as R
import bow_synth

pytestmark = pytest.mark.gpu
N_WORDS = 1_000_000
CUR = R.CURRENT_MAP_ID


def same(got, want):
    gm, gk, gs = got
    wm, wk, ws = want
    return (np.array_equal(gm, wm) and np.array_equal(gk, wk) and len(gs) == len(ws)
            and np.array_equal(np.asarray(gs, np.float32).view(np.uint32), np.asarray(ws, np.float32).view(np.uint32)))


def build(ctx, entries, **kw):
    import mi355slam
    db = mi355slam.BowDatabase(ctx, N_WORDS, **kw)
    ref = R.RefIndex()
    for mp, kf, w, v in entries:
        db.add(mp, kf, w, v); ref.add(mp, kf, w, v)
    return db, ref


def check_queries(db, ref, queries, ids, mr, sr):
    for w, v, ex in queries:
        got = db.query(w, v, exclude=ex, min_in_common_ratio=mr, score_ratio=sr)
        want = ref.query(w, v, exclude=ex, min_in_common_ratio=mr, score_ratio=sr)
        assert same(got, want), (mr, sr, len(got[0]), len(want[0]))
    if ids:
        got = db.query_ids(ids, min_in_common_ratio=mr, score_ratio=sr)
        for i, (mp, kf) in enumerate(ids):
            assert same(got[i], ref.query_id(mp, kf, min_in_common_ratio=mr, score_ratio=sr)), (mp, kf, mr, sr)


@pytest.mark.parametrize("n", [1, 100, 5000])
def test_databases_of_several_sizes_over_the_ratio_grid(ctx, n):
    s, entries = R.make_db(11 + n, n, n_places=max(2, n // 25))
    db, ref = build(ctx, entries, capacity=max(16, n // 4))
    assert db.size == n
    queries = [s.keyframe() + (None,) for _ in range(2)] + [(entries[-1][2], entries[-1][3], (entries[-1][0], entries[-1][1]))]
    ids = [(e[0], e[1]) for e in entries[:: max(1, n // 4)]][:4]
    for mr in (0.0, 0.5, 0.8, 1.0):
        for sr in (0.0, 0.75, 1.0):
            check_queries(db, ref, queries, ids, mr, sr)
    db.close()


def test_exclusion_is_of_one_id_and_duplicates_tie_in_id_order(ctx):
    s = R.Synth(5, n_places=3)
    w, v = s.keyframe(place=0)
    entries = [(CUR, 5, w, v), (0, 5, w, v), (1, 5, w, v), (CUR, 4, w, v), (0, 2, w, v)]
    entries += [(CUR, 10 + i) + s.keyframe() for i in range(30)]
    db, ref = build(ctx, entries)
    got = db.query(w, v, exclude=(CUR, 5), min_in_common_ratio=0.8, score_ratio=0.75)
    assert same(got, ref.query(w, v, exclude=(CUR, 5), min_in_common_ratio=0.8, score_ratio=0.75))
    ids = list(zip(got[0], got[1]))
    assert (CUR, 5) not in ids and ids[:4] == [(0, 2), (0, 5), (1, 5), (CUR, 4)]
    assert len(set(got[2][:4].view(np.uint32))) == 1
    for mr in (0.0, 0.8):
        check_queries(db, ref, [], [(0, 5), (CUR, 5), (1, 5)], mr, 0.75)


def test_no_common_words_empty_database_and_empty_vectors(ctx):
    import mi355slam
    db = mi355slam.BowDatabase(ctx, N_WORDS, capacity=4)
    m, k, sc = db.query([1, 2, 3], [0.2, 0.3, 0.5])
    assert len(m) == len(k) == len(sc) == 0 and db.size == 0
    db.add(0, 0, [], [])
    db.add(0, 1, [10, 20, 30], [0.25, 0.25, 0.5])
    db.add(0, 2, [], [])
    assert db.size == 3
    assert len(db.query([1, 2, 3], [0.2, 0.3, 0.5], min_in_common_ratio=0.0, score_ratio=0.0)[0]) == 0    # nothing shared
    assert len(db.query([], [], min_in_common_ratio=0.0, score_ratio=0.0)[0]) == 0
    r = db.query_ids([(0, 0), (0, 1), (0, 2)], min_in_common_ratio=0.0, score_ratio=0.0)
    assert [len(x[0]) for x in r] == [0, 0, 0]
    m, k, sc = db.query([20, 40], [0.5, 0.5], min_in_common_ratio=0.0, score_ratio=0.0)
    assert list(k) == [1] and sc[0] == np.float32(0.25)
    db.close()


def test_more_survivors_than_one_sort_holds(ctx):
    """20 000 near-identical entries: every one survives, so the ranking takes the multi-chunk path; values from a small set make ties."""
    rng = np.random.default_rng(4)
    base = np.sort(rng.choice(N_WORDS, 12, replace=False)).astype(np.int32)
    entries = []
    for i in range(20000):
        w = base[rng.random(12) < 0.9] if i % 3 else base
        v = R.normalize_l1(rng.integers(1, 4, len(w)).astype(np.float64))
        entries.append((CUR if i % 2 else 0, i // 2, w, v))
    db, ref = build(ctx, entries, capacity=1024, words_per_entry=12)
    qv = R.normalize_l1(np.arange(1, 13, dtype=np.float64))
    for mr, sr in [(0.0, 0.0), (0.5, 0.5), (0.0, 0.9)]:
        got = db.query(base, qv, exclude=(CUR, 7), min_in_common_ratio=mr, score_ratio=sr)
        want = ref.query(base, qv, exclude=(CUR, 7), min_in_common_ratio=mr, score_ratio=sr)
        assert same(got, want) and (len(want[0]) > 4096 or sr == 0.9)
    got = db.query_ids([(0, 0), (CUR, 3)], min_in_common_ratio=0.0, score_ratio=0.0)
    assert same(got[0], ref.query_id(0, 0, min_in_common_ratio=0.0, score_ratio=0.0)) and len(got[0][0]) == 19999
    assert same(got[1], ref.query_id(CUR, 3, min_in_common_ratio=0.0, score_ratio=0.0))
    db.close()


def test_mapper_order_over_500_keyframes_with_growth_and_reuse(ctx):
    """the atlas first, then per keyframe: query (loop_closer.cpp:132), add (mapper_helpers.cpp:1099) and a cull (:387);
    a database created far too small grows, removed slots and segments are reused"""
    import mi355slam
    s = R.Synth(21, n_places=25)
    db = mi355slam.BowDatabase(ctx, N_WORDS, capacity=8, words_per_entry=16)
    ref = R.RefIndex()
    for kf in range(40):
        w, v = s.keyframe()
        db.add(0, kf, w, v); ref.add(0, kf, w, v)
    live = []
    rng = np.random.default_rng(3)
    for kf in range(500):
        w, v = s.keyframe()
        mr, sr = (0.8, 0.75) if kf % 2 else (0.5, 0.0)
        assert same(db.query(w, v, exclude=(CUR, kf), min_in_common_ratio=mr, score_ratio=sr),
                    ref.query(w, v, exclude=(CUR, kf), min_in_common_ratio=mr, score_ratio=sr)), kf
        db.add(CUR, kf, w, v); ref.add(CUR, kf, w, v); live.append(kf)
        if len(live) > 60 and rng.random() < 0.7:
            old = live.pop(int(rng.integers(0, len(live) - 10)))
            db.remove(CUR, old); ref.remove(CUR, old)
        if kf % 50 == 49:
            ids = [(CUR, x) for x in live[-3:]] + [(0, 1)]
            got = db.query_ids(ids, min_in_common_ratio=mr, score_ratio=sr)
            for i, (mp, k) in enumerate(ids):
                assert same(got[i], ref.query_id(mp, k, min_in_common_ratio=mr, score_ratio=sr))
        assert db.size == len(ref)
    db.close()


def test_errors_leave_the_database_unchanged(ctx):
    import mi355slam
    s, entries = R.make_db(8, 30, n_places=3)
    db, ref = build(ctx, entries, capacity=16)
    w, v = s.keyframe()
    bad = [([5, 3, 9], [0.3, 0.3, 0.4]), ([3, 3, 9], [0.3, 0.3, 0.4]), ([3, 9, N_WORDS], [0.3, 0.3, 0.4]), ([-1, 3, 9], [0.3, 0.3, 0.4]),
           ([3, 5, 9], [0.3, np.nan, 0.4]), ([3, 5, 9], [0.3, np.inf, 0.4])]
    for bw, bv in bad:
        with pytest.raises(mi355slam.MsError):
            db.add(CUR, 999, bw, bv)
        with pytest.raises(mi355slam.MsError):
            db.query(bw, bv)
    with pytest.raises(mi355slam.MsError):
        db.add(entries[3][0], entries[3][1], w, v)                   # already live
    with pytest.raises(mi355slam.MsError):
        db.query_ids([(entries[0][0], entries[0][1]), (77, 77)])      # not in the database
    db.remove(77, 77)                                                 # absent: ignored
    assert db.size == 30
    check_queries(db, ref, [(w, v, None)], [(entries[3][0], entries[3][1])], 0.5, 0.5)
    db.close()


def test_sliding_window_allocates_nothing_once_warm(ctx):
    import mi355slam
    L = mi355slam.lib()
    L.ms_debug_host_allocs.restype = ctypes.c_longlong
    s = R.Synth(33, n_places=15)
    db = mi355slam.BowDatabase(ctx, N_WORDS, capacity=64)
    ref = R.RefIndex()
    counts = []
    for kf in range(300):
        w, v = s.keyframe()
        db.add(CUR, kf, w, v); ref.add(CUR, kf, w, v)
        if kf >= 40:
            db.remove(CUR, kf - 40); ref.remove(CUR, kf - 40)
        got = db.query(w, v, exclude=(CUR, kf), min_in_common_ratio=0.8, score_ratio=0.75)
        if kf % 25 == 0:
            assert same(got, ref.query(w, v, exclude=(CUR, kf), min_in_common_ratio=0.8, score_ratio=0.75))
        counts.append(L.ms_debug_host_allocs())
    assert counts[-1] == counts[100], (counts[100], counts[-1])
    db.close()


def test_end_to_end_revisits_rank_first(oracle, ctx):
    """frames -> OrbExtractor -> BowVocabulary.transform -> the BowVector the mirror assembles -> add; a shifted revisit of a scene
    finds that scene's keyframe first"""
    import mi355slam
    scenes = [oracle.synth_frame(640, 480, 2000 + i) for i in range(5)]
    revisit = oracle.synth_frame(640, 480, 2003, 6, 4)
    ex = mi355slam.OrbExtractor(ctx, 640, 480, max_batch=1)
    descs = []
    for img in scenes + [revisit]:
        ex.extract(img)
        descs.append(ex.download(0)["desc"])
    v = bow_synth.make_vocab(9, k=10, depth=4)
    rng = np.random.default_rng(2)
    pool = np.concatenate(descs[:5])
    v["desc"][1:] = pool[rng.integers(0, len(pool), len(v["desc"]) - 1)] ^ bow_synth.flip_bits(rng, np.zeros((len(v["desc"]) - 1, 8), np.uint32), 0.05)
    voc = mi355slam.BowVocabulary(ctx, v["parent"], v["desc"], v["weight"], v["word"], v["depth_levels"])
    n_words = int(v["word"].max()) + 1
    vecs = []
    for d in descs:
        wd, wt, nd = voc.transform(d, 4)
        ow, ov = oracle.bow_assemble(wd, wt, nd)[:2]
        vecs.append((ow, ov))
    db = mi355slam.BowDatabase(ctx, n_words)
    ref = R.RefIndex()
    for i in range(5):
        db.add(CUR, i, *vecs[i]); ref.add(CUR, i, *vecs[i])
    for mr, sr in [(0.8, 0.75), (0.0, 0.0)]:
        got = db.query(*vecs[5], exclude=(CUR, 5), min_in_common_ratio=mr, score_ratio=sr)
        assert same(got, ref.query(*vecs[5], exclude=(CUR, 5), min_in_common_ratio=mr, score_ratio=sr))
        assert got[1][0] == 3
    db.add(CUR, 5, *vecs[5]); ref.add(CUR, 5, *vecs[5])
    r = db.query_ids([(CUR, 5), (CUR, 3)], min_in_common_ratio=0.0, score_ratio=0.0)
    assert r[0][1][0] == 3 and r[1][1][0] == 5
    assert same(r[0], ref.query_id(CUR, 5, min_in_common_ratio=0.0, score_ratio=0.0))
    db.close(); voc.close()


def test_host_mirror_matches_its_restatement():
    from test_bow_db_abi import build_smoke
    out = subprocess.check_output([build_smoke()], text=True, timeout=300)
    assert "bow db ok" in out, out
