"""tests/search_bind_ref.py, the specification of ms_search_bind: its two forms agree with each other and with
project_gate_ref.search_by_projection, and the scenes of tests/test_gpu_search_bind.py hold the conditions that file relies on.  CPU only."""
import numpy as np
import pytest

import project_gate_ref as G
import search_bind_ref as R


@pytest.mark.parametrize("name", R.GPU_SCENES)
def test_the_two_forms_agree_on_every_gpu_scene(name):
    S = R.gpu_scene(name)
    w = S["want"]
    assert R.agree(S, w, R.sequential(S)) == []
    assert w["n_matched"] == int(w["counts"][3] + w["counts"][4]) and int(w["counts"][:5].sum()) == S["n_kept"]
    assert int((w["outcome"] >= 8).sum() + w["counts"][4]) == int(w["counts"][5]) == w["note"]["rescans"]
    assert not w["skip"][w["lists"]["top_idx"][w["lists"]["top_idx"] >= 0]].any()          # the scoring never lists a keypoint its mask marks
    assert (w["usable"] == 0).sum() == w["n_matched"] and not (w["usable"][w["skip"] > 0] == 0).any()


@pytest.mark.parametrize("seed", (77, 1, 2, 3))
def test_both_forms_equal_search_by_projection_on_the_matcher_scene(seed):
    sc, kf, S = R.matcher_scene(seed)
    w = R.tables(S)
    assert R.agree(S, w, R.sequential(S)) == []
    bound = S["bound"].copy()
    want = G.search_by_projection(kf, bound, sc["table"], sc["views"][0], sc["sf"], sc["scale_factor"])
    assert [(int(e), int(w["match_kp"][e])) for e in S["kept_entry"] if w["match_kp"][e] >= 0] == want and len(want) >= 50
    assert np.array_equal(bound, R.bound_mask(w["kf_mp"], S["slot"], S["n_kp"], S["n_mp"]))
    assert w["note"]["rescans"] == 0                         # why the clustered scenes exist: this one never runs a list out


@pytest.mark.parametrize("name, trips, kp_trips", [("clustered", 3, 3), ("kp1100", 2, 2), ("kp2100", 3, 3), ("small", 1, 1)])
def test_every_outcome_occurs_in_every_trip(name, trips, kp_trips):
    S = R.gpu_scene(name)
    per_trip = R.codes_per_trip(S, S["want"])
    assert len(per_trip) == trips and -(-S["n_kp"] // R.TRIP) == kp_trips
    for codes in per_trip:
        assert codes == set(R.CODES), codes
    assert S["want"]["note"]["conflicts"] > S["n_kept"] // 2 and S["want"]["note"]["rescans"] > S["n_kept"] // 4


def test_sizes_the_issue_names():
    S = R.gpu_scene("clustered")
    assert (S["n_kept"], S["stride"]) == (2720, 2816) and S["n_kp"] < S["stride"]
    assert R.gpu_scene("kp1100")["n_kp"] == 1100 and R.gpu_scene("kp2100")["n_kp"] == 2100 == R.gpu_scene("kp2100")["stride"]


def test_first_trip_of_the_lead_scene_steps_no_query():
    S = R.gpu_scene("lead")
    w, L = S["want"], S["want"]["lists"]
    first = slice(0, R.TRIP)
    assert ((L["top_idx"][first, 0] < 0) | (L["top_dist"][first, 0] > R.THR_HIGH)).all()
    per_trip = R.codes_per_trip(S, w)
    assert per_trip[0] == {0, 1} and per_trip[1] == set(R.CODES) and w["n_matched"] > 100


def test_band_scene_rescans_over_three_passes_with_best_and_second_apart():
    S = R.gpu_scene("band")
    w, sp = S["want"], S["spots"]
    assert np.array_equal(S["fs"].order, np.arange(S["n_kp"]))                   # sorted position = keypoint index
    assert w["outcome"][:5].tolist() == [3, 3, 3, 4, 4] and w["lists"]["n_scored"][3] == S["n_kp"] == 2100
    assert sorted(w["lists"]["top_idx"][3].tolist()) == sorted([sp["A"], sp["B"], sp["C"], sp["D"]])
    taken = np.zeros(S["n_kp"], np.uint8)
    taken[[sp["A"], sp["B"], sp["C"]]] = 1                   # three of the four list entries are taken when the main query is walked
    key, j = R.scored(S, 3, taken)
    assert (j[0], j[1]) == (sp["D"], sp["E"]) and (key[:2] & 0xFFFFF).tolist() == [sp["D"], sp["E"]]
    assert sp["D"] // R.TRIP == 1 and sp["E"] // R.TRIP == 2 and len(R.band(S["fs"], S["q_x"][3], S["q_y"][3], S["q_radius"][3])) == 2100
    e = lambda q: S["kept_entry"][q] - S["first"]
    assert w["match_kp"][e(3)] == sp["D"] and w["match_kp"][e(4)] == sp["E"]


def test_score_lists_is_the_order_of_the_sequential_scan():
    """best2_update over the scan (keyframe_matcher.cpp:368-377) keeps the two smallest by (distance, scan position): the order of the lists."""
    rng = np.random.default_rng(0)
    for _ in range(200):
        d = rng.integers(0, 6, rng.integers(1, 9))
        best, best2, i1, i2 = 256, 256, -1, -1
        for i, x in enumerate(d):
            if x < best:
                best2, i2, best, i1 = best, i1, x, i
            elif x < best2:
                best2, i2 = x, i
        o = np.argsort(d * 1024 + np.arange(len(d)), kind="stable")
        assert i1 == o[0] and (len(d) < 2 or (i2 == o[1] and best2 == d[o[1]]))
