"""tests/loop_chain_ref.py, the specification of the loop closer's pieces on the map tables: its std::map-style restatement and
its tables form agree on every scene, and the scenes hold the conditions the device tests (tests/test_gpu_loop_chain.py) rely on."""
import numpy as np
import pytest

import loop_chain_ref as R


def same(a, b, names):
    for k in names:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.parametrize("name", R.SCENES)
def test_the_map_form_and_the_tables_form_agree(name):
    S = R.gpu_scene(name)
    t, w = S["tables"], S["want"]
    v = R.pairs_tables(S, t)
    assert v["n_pairs"] == w["n_pairs"] > 0
    same(v, w, ("pair_start", "cur_pose", "cand_pose") + R.PAIR_ARRAYS)
    assert np.array_equal(w["kp1"], np.concatenate([np.flatnonzero([r is None for r in why]) for why in w["reasons"]]))       # observations.at(kf.id) is the walked keypoint
    kp1, kp2, start = R.keypoint_lists(S, S["lists"])
    assert start[-1] == len(kp1) > 0
    same(R.sim3_lists_tables(S, t, kp1, kp2, start), S["want_sim3"], R.SIM3_ARRAYS)
    for kf_id, slot in S["slot_of"].items():
        for require in (0, 1):
            a, b = R.usable_mask_map(S, kf_id, require), R.usable_mask_tables(t, slot, t["n_kp"][slot], require)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_masks_tell_present_from_triangulated():
    S = R.gpu_scene("base")
    t = S["tables"]
    u0, rows = R.usable_mask_tables(t, S["cur"], S["n_kp_cur"], 0)
    u1, _ = R.usable_mask_tables(t, S["cur"], S["n_kp_cur"], 1)
    assert 0 < u1.sum() < u0.sum() < S["n_kp_cur"] and np.array_equal(u1, (rows >= 0).astype(np.uint8))
    stale = [kp for slot, kp, _ in S["stale"] if slot == S["cur"]]
    assert stale and not u0[stale].any() and (t["kf_mp"][S["cur"], stale] >= 0).all()            # a dead row is no map point


def test_the_base_scene_holds_what_the_device_tests_rely_on():
    S = R.gpu_scene("base")
    t, w = S["tables"], S["want"]
    assert (S["n_kf"], S["stride"], S["n_mp"], S["n_kp_cur"], S["n_levels"]) == (12, 640, 3000, 600, 8)
    assert sorted(S["n_kp_cand"]) == [0, 1, 256, 257, 600]
    n_trips = -(-S["n_kp_cur"] // R.TRIP)
    assert n_trips == 3
    why = R.drop_reasons(S, t, w)
    for c, n in enumerate(S["n_kp_cand"]):
        if n < 16:
            continue
        for tr in range(n_trips):                            # every drop reason, and a kept pair behind the first trip, in every trip of every large candidate
            trip = why[c][tr * R.TRIP:(tr + 1) * R.TRIP]
            for reason in R.DROPS:
                assert reason in trip, (c, tr, reason)
            assert tr == 0 or None in trip, (c, tr)
    counts = np.diff(w["pair_start"])
    first_trip = [sum(r is None for r in why[c][:R.TRIP]) for c in range(len(counts))]
    assert any(f == 0 and n > 0 for f, n in zip(first_trip, counts))                             # a first trip without a kept pair, pairs behind it
    assert any(counts[c] == 0 and counts[:c].any() and counts[c + 1:].any() for c in range(len(counts)))     # an empty candidate between two others
    assert counts[list(S["n_kp_cand"]).index(1)] == 1 and counts[list(S["n_kp_cand"]).index(0)] == 0
    o1, o2 = t["kp_octave"][S["cur"], w["kp1"]], np.concatenate([t["kp_octave"][s, w["kp2"][a:b]] for s, a, b in zip(S["cand_slot"], w["pair_start"], w["pair_start"][1:])])
    assert (o1 != o2).any() and (w["thr1"] != w["thr2"]).any()                                   # the two keypoints of a pair on different octaves
    dead_cur = [e for e in S["stale"] if e[0] == S["cur"]]
    assert dead_cur and len(S["stale"]) > len(dead_cur)                                          # dead rows on both sides


def test_the_candidate_scene_goes_past_one_trip_of_the_offsets_scan():
    S = R.gpu_scene("cands257")
    counts = np.diff(S["want"]["pair_start"])
    assert len(counts) == R.TRIP + 1 and S["stride"] == 8 and counts[:R.TRIP].sum() > 0 and counts[R.TRIP] > 0     # a carry that the last candidate uses


def test_zero_sizes_of_the_restatement():
    S = dict(R.gpu_scene("small"))
    none = [np.full(S["n_kp_cur"], -1, np.int32) for _ in S["cand_slot"]]
    for w in (R.pairs_map(S, none), R.pairs_tables(S, S["tables"], none)):
        assert w["n_pairs"] == 0 and not w["pair_start"].any() and w["pts1"].shape == (0, 3)


def test_the_arithmetic_is_the_pinned_one():
    P = np.array([[0.1, 0.7, -0.3, 1e-3], [0.9, 1e-9, 0.2, 5.0], [-0.4, 0.3, 0.8, -2.0]])
    p = np.array([3.1, -1.7, 1e5])
    x = R.cam_point(P, p)
    for i in range(3):
        assert x[i] == ((P[i, 0] * p[0] + P[i, 1] * p[1]) + P[i, 2] * p[2]) + P[i, 3]
    assert R.cam_point(np.stack([P, P]), np.stack([p, p])).shape == (2, 3)
    sig = R.level_sigma_sq(8)
    assert sig.dtype == np.float32 and (R.CHI_SQ_2D * sig).dtype == np.float32 and sig[0] == 1 and (np.diff(sig) > 0).all()
