"""tests/map_fuse_ref.py, the specification of ms_map_fuse and ms_map_replace_pairs: its two forms agree, and the base scene
holds every condition the GPU test relies on.  The conditions are asserted on the restatement, so a change of the generator that loses one
fails here and not silently on the device."""
import numpy as np
import pytest

import map_fuse_ref as R

SCENE = R.make_scene()


def both(T, mp_index, views, cand, source_slot):
    a = R.fuse_tables(T, mp_index, views, cand, source_slot)
    b = R.fuse_sequential(T, mp_index, views, cand, source_slot)
    assert R.same(a, b, R.TABLE_KEYS + R.LIST_KEYS) == []
    assert a["views_done"] == b["views_done"]
    return a


@pytest.fixture(scope="module")
def walked():
    S = SCENE
    return {src: both(S["T"], S["mp_index"], S["views"], S["cand"], src) for src in (-1, S["source_slot"])}


def test_scene_shape_and_candidates_round_trip():
    S = SCENE
    assert S["T"]["kf_mp"].shape == (40, 640) and len(S["T"]["mp_live"]) == 3000 and len(S["views"]) == 6
    assert sum((S["T"]["kf_mp"][s] >= 0).sum() == 0 for s in range(40)) == 3
    got = R.candidates(len(S["mp_index"]), S["views"], S["n_kept"], S["kept_entry"], S["top_idx"], S["top_dist"], S["max_dist"])
    assert np.array_equal(got, S["cand"])
    for slot, first, count in S["views"]:                    # a view lists a row once
        assert len(set(S["mp_index"][first:first + count].tolist())) == count
    assert S["source_slot"] not in [v[0] for v in S["views"]]
    listed = S["T"]["kf_mp"][(S["T"]["kf_mp"] >= 0) & (S["T"]["kf_mp"] < 3000)]
    assert S["T"]["mp_live"][listed].all()                   # the pre-pass would turn the scene away otherwise


def test_both_forms_agree_on_the_scene_and_the_scene_holds_its_conditions(walked):
    S, w = SCENE, walked[-1]
    slot, first, count = S["views"][0]
    n_cand = int((S["cand"][first:first + count] >= 0).sum())
    assert n_cand > 2 * R.TRIP and count > 2 * R.TRIP        # more candidates than two trips of the compaction: three trips of entries
    for t0 in range(0, count, R.TRIP):                       # every code in every trip of that view
        codes = set(w["outcome"][first + t0:first + min(t0 + R.TRIP, count)].tolist())
        assert codes == set(range(8)), (t0, codes)
    assert w["outcome"][first + count - 1 - np.argmax(w["outcome"][first:first + count][::-1] >= 4)] >= 4       # an action in the last trip
    assert (first + count - 1 - np.argmax(w["outcome"][first:first + count][::-1] >= 6)) >= first + 2 * R.TRIP  # a replace in the last trip
    note = w["note"]
    for key in ("winner_later_loses", "gained_then_2", "loser_later_1", "unlisted_then_3", "ties", "track_transfer", "track_both", "track_outside"):
        assert note[key] >= 1, key
    assert w["views_done"] == 6 and (w["counts"] > 0).all() and w["counts"].sum() == sum(v[2] for v in S["views"])
    assert len(w["erased_rows"]) == w["counts"][6] + w["counts"][7]
    # kp / other carry what the header says
    assert ((w["kp"] >= 0) == (w["outcome"] >= 4)).all() and ((w["other"] >= 0) == (w["outcome"] >= 5)).all()
    # the invariant the walk preserves
    kf = w["kf_mp"]
    assert w["mp_live"][kf[(kf >= 0) & (kf < 3000)]].all()
    assert np.array_equal(w["n_obs"], R.observation_count(kf, 3000) * (w["mp_live"] != 0))


def test_early_stop_and_walking_on(walked):
    S = SCENE
    stopped, full = walked[S["source_slot"]], walked[-1]
    assert 1 <= stopped["views_done"] < len(S["views"]) and full["views_done"] == len(S["views"])
    done = stopped["views_done"]
    end = S["views"][done - 1][1] + S["views"][done - 1][2]
    assert np.array_equal(stopped["outcome"][:end], full["outcome"][:end])       # the views walked are walked alike
    assert (stopped["outcome"][end:] == 0).all() and (stopped["kp"][end:] == -1).all()
    assert not np.array_equal(stopped["kf_mp"][S["source_slot"]], S["T"]["kf_mp"][S["source_slot"]])
    assert stopped["counts"].sum() == sum(v[2] for v in S["views"][:done])


def test_both_forms_agree_on_200_small_tables():
    rng = np.random.default_rng(11)
    seen = np.zeros(8, np.int64)
    stops = 0
    for _ in range(200):
        n_kf, stride, n_mp = int(rng.integers(1, 9)), int(rng.integers(1, 24)), int(rng.integers(1, 60))
        T = R.make_tables(rng, n_kf, stride, n_mp, int(rng.integers(0, stride + 1)), tracks=bool(rng.integers(0, 2)), dead=0.2)
        n_views = int(rng.integers(0, 5))
        slots = rng.integers(0, n_kf, n_views)
        mp_index, views, cand = R.make_views(rng, T, slots, rng.integers(0, n_mp + 1, n_views), with_cand=0.8)
        free = [s for s in range(n_kf) if s not in slots]
        src = int(rng.choice(free)) if free and rng.random() < 0.5 else -1
        w = both(T, mp_index, views, cand, src)
        seen += w["counts"]
        stops += w["views_done"] < n_views
    assert (seen > 20).all() and stops >= 5


def test_pairs_forms_agree_and_cover_every_outcome():
    rng = np.random.default_rng(3)
    S = SCENE
    pairs = R.make_pairs(rng, S["T"], 60)
    a, b = R.replace_pairs_tables(S["T"], pairs), R.replace_pairs_sequential(S["T"], pairs)
    assert R.same(a, b, R.TABLE_KEYS + ("outcome", "erased_rows", "erased_into")) == []
    assert set(a["outcome"].tolist()) == {0, 1, 2}
    assert set(a["erased_into"].tolist()) & set(a["erased_rows"].tolist())       # a chain: a winner that is replaced later
    for _ in range(50):
        T = R.make_tables(rng, int(rng.integers(1, 9)), int(rng.integers(1, 24)), int(rng.integers(4, 60)), 8, tracks=bool(rng.integers(0, 2)), dead=0.2)
        pairs = R.make_pairs(rng, T, int(rng.integers(0, 12)))
        a, b = R.replace_pairs_tables(T, pairs), R.replace_pairs_sequential(T, pairs)
        assert R.same(a, b, R.TABLE_KEYS + ("outcome", "erased_rows", "erased_into")) == []


def test_geometry_scene_holds_what_the_chain_test_needs():
    S = R.make_geometry_scene()
    w = R.deduplicate_sequential(S)
    assert w["near"] == 0                                    # no entry whose scale level two logf implementations may round apart
    assert w["changes"] >= 1                                 # a later adjacent keyframe meets rows its predecessors' replaces put into the current list
    assert (w["counts"][[0, 2, 3, 4, 5, 6, 7]] > 0).all() and len(w["erased_rows"]) >= 20
    kf = w["kf_mp"]
    assert w["mp_live"][kf[kf >= 0]].all() and np.array_equal(w["n_obs"], R.observation_count(kf, len(w["mp_live"])) * (w["mp_live"] != 0))
    for s in range(kf.shape[0]):                             # a slot lists a row once, before and after
        for table in (S["T"]["kf_mp"], kf):
            v = table[s][table[s] >= 0]
            assert len(set(v.tolist())) == len(v)
