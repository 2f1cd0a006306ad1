"""The plain-Python restatement of getBowSimilar (tests/bow_db_ref.py) against cases computed by hand."""
import numpy as np

import bow_db_ref as R


def test_three_word_l1_score_is_exact():
    # every common word contributes |v - w| - |v| - |w| = -2 min(v, w) for positive values: -(0.5 + 0.5 + 0.5) / -2 = 0.75
    q = ([1, 2, 3], [0.5, 0.25, 0.25])
    e = ([1, 2, 3], [0.25, 0.25, 0.5])
    assert R.l1_score(*q, *e) == np.float32(0.75)
    # 1 - ||q - e||_1 / 2 with ||q - e||_1 = 0.5
    idx = R.RefIndex()
    idx.add(0, 7, *e)
    m, k, s = idx.query(*q, min_in_common_ratio=0.0, score_ratio=0.0)
    assert list(m) == [0] and list(k) == [7] and s.view(np.uint32)[0] == np.float32(0.75).view(np.uint32)


def _shared(n, tail):
    """a vector sharing the query's words 0 .. n-1 plus words of its own"""
    w = list(range(n)) + [100 + tail * 10 + i for i in range(3)]
    return w, [1.0 / len(w)] * len(w)


def test_min_in_common_truncates_and_equal_count_is_excluded():
    q = (list(range(10)), [0.1] * 10)
    idx = R.RefIndex()
    for kf, n in enumerate([7, 4, 3]):
        idx.add(R.CURRENT_MAP_ID, kf, *_shared(n, kf))
    # maxInCommon 7: 0.5f * 7 = 3.5 -> 3; counts 7 and 4 exceed it, 3 equals it and is dropped
    m, k, _ = idx.query(*q, min_in_common_ratio=0.5, score_ratio=0.0)
    assert sorted(k) == [0, 1]
    # 0.8f * 7 = 5.6 -> 5: only the 7
    _, k, _ = idx.query(*q, min_in_common_ratio=0.8, score_ratio=0.0)
    assert list(k) == [0]
    # an exact product: maxInCommon 8, 0.5f * 8 = 4 -> an entry sharing 4 words is dropped, 5 kept
    idx2 = R.RefIndex()
    for kf, n in enumerate([8, 5, 4]):
        idx2.add(0, kf, *_shared(n, kf))
    _, k, _ = idx2.query(*q, min_in_common_ratio=0.5, score_ratio=0.0)
    assert sorted(k) == [0, 1]
    # the query's own id is not counted: maxInCommon is now 5, 0.5f * 5 = 2.5 -> 2, so 5 and 4 both pass (scores 0.5 and 0.4)
    _, k, _ = idx2.query(*q, exclude=(0, 0), min_in_common_ratio=0.5, score_ratio=0.0)
    assert list(k) == [1, 2]
    _, k, _ = idx2.query(*q, exclude=(0, 0), min_in_common_ratio=0.5, score_ratio=0.9)
    assert list(k) == [1]


def test_score_equal_to_min_score_is_kept():
    q = ([1, 2, 3], [0.5, 0.25, 0.25])
    idx = R.RefIndex()
    idx.add(0, 1, [1, 2, 3], [0.25, 0.25, 0.5])       # 0.75 (best)
    idx.add(0, 2, [1, 2, 5], [0.125, 0.25, 0.625])    # min(0.5, 0.125) + min(0.25, 0.25) = 0.375 == 0.75 * 0.5: kept
    idx.add(0, 3, [2, 7], [0.25, 0.75])               # 0.25 < 0.375: cut
    m, k, s = idx.query(*q, min_in_common_ratio=0.0, score_ratio=0.5)
    assert list(k) == [1, 2] and list(s) == [np.float32(0.75), np.float32(0.375)]
    _, k, _ = idx.query(*q, min_in_common_ratio=0.0, score_ratio=0.0)
    assert list(k) == [1, 2, 3]


def test_ties_in_score_follow_id_order_and_remove_forgets():
    idx = R.RefIndex()
    w, v = [3, 5, 9], [0.25, 0.25, 0.5]
    for mp, kf in [(R.CURRENT_MAP_ID, 2), (0, 9), (0, 2), (R.CURRENT_MAP_ID, 1)]:
        idx.add(mp, kf, w, v)
    m, k, s = idx.query(w, v, exclude=(R.CURRENT_MAP_ID, 2), min_in_common_ratio=0.0, score_ratio=1.0)
    assert list(zip(m, k)) == [(0, 2), (0, 9), (R.CURRENT_MAP_ID, 1)] and len(set(s)) == 1
    idx.remove(0, 9)
    idx.remove(5, 5)          # absent: nothing happens
    m, k, _ = idx.query(w, v, min_in_common_ratio=0.0, score_ratio=1.0)
    assert list(zip(m, k)) == [(0, 2), (R.CURRENT_MAP_ID, 1), (R.CURRENT_MAP_ID, 2)] and len(idx) == 3


def test_synthetic_revisits_rank_their_place_first():
    s, entries = R.make_db(3, 60, n_places=6)
    idx = R.RefIndex()
    for mp, kf, w, v in entries:
        idx.add(mp, kf, w, v)
    w, v = s.keyframe(place=2)
    m, k, sc = idx.query(w, v, min_in_common_ratio=0.8, score_ratio=0.75)
    assert len(m) >= 1 and np.all(np.diff(sc) <= 0)
    assert all(np.all(np.diff(e[2]) > 0) for e in entries) and abs(sum(entries[0][3]) - 1.0) < 1e-12
