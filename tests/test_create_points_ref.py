"""tests/create_points_ref.py, the specification of the device createNewMapPoints, against itself on the CPU: the sequential
restatement of mapper_helpers.cpp:271-318 and the staged, table-form one agree on every table, mask and list after every adjacent keyframe,
and the fixture reaches every case the GPU tests rely on."""
import numpy as np

import create_points_ref as R
import mi355slam
import triangulate_ref as TR

PACKED = ("matched", "match_kp1", "match_kp2", "rows", "status", "reason", "created_rows", "created_kp1", "created_kp2")


def test_the_fixture_reaches_every_case():
    sc, free_rows, st, results, counts = R.fixture()
    print(counts)
    for k in ("created", "angle", "depth_or_reprojection", "depth_branch", "fails_then_created", "masked_later", "empty_adjacent", "second_trip", "flipped_order"):
        assert counts[k] > 0, k
    assert counts["skipped"] == 1 and [r is None for r in results] == [s == R.CURRENT for s in R.ADJACENT]
    assert sc["n_kp"][R.CURRENT] == 300 > R.TRIP and sc["kf_mp"].shape == (6, 320) and len(sc["mp_live"]) == 1024
    assert sorted(sc["kf_id"].tolist()) != sc["kf_id"].tolist() and any(sc["kf_id"][s] > sc["kf_id"][R.CURRENT] for s in R.ADJACENT)


def test_sequential_and_staged_agree_after_every_adjacent():
    sc, free_rows, st, results, _ = R.fixture()
    st2, staged = R.staged(sc, R.CURRENT, R.ADJACENT, free_rows)
    assert R.same_state(st, st2) and not R.same_state(st, sc)
    for a, b in zip(results, staged):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert a["slot"] == b["slot"] and a["n_matches"] == b["n_matches"]
        for k in PACKED:
            assert np.array_equal(a[k], b[k]), (a["slot"], k)
        assert R.same_state(a["state"], b["state"]) and R.same_masks(a["state"]["masks"], b["state"]["masks"]), a["slot"]
        L = b["lists"]
        assert np.array_equal(L["obs_start"], 2 * np.arange(a["n_matches"] + 1)) and (L["n_obs_row"] == 2).all() and (L["was_triangulated"] == 0).all()
        assert (sc["kf_id"][L["obs_kf"][0::2]] < sc["kf_id"][L["obs_kf"][1::2]]).all()                  # ascending KfId inside every list


def test_midpoint_mode_agrees_too():
    sc, free_rows, _, _, _ = R.fixture()
    a, ra = R.sequential(sc, R.CURRENT, R.ADJACENT[:2], free_rows, TR.MIDPOINT)
    b, rb = R.staged(sc, R.CURRENT, R.ADJACENT[:2], free_rows, TR.MIDPOINT)
    assert R.same_state(a, b) and all(np.array_equal(x["status"], y["status"]) for x, y in zip(ra, rb))


def test_a_failed_row_stays_free_and_its_keypoints_usable():
    sc, free_rows, st, results, _ = R.fixture()
    first = results[0]
    failed = first["status"] == TR.NOT_TRIANGULATED
    rows = first["rows"][failed]
    after = first["state"]
    assert len(rows) and not after["mp_live"][rows].any() and not after["mp_flags"][rows].any()
    assert (after["kf_mp"][R.CURRENT, first["match_kp1"][failed]] == -1).all() and (after["masks"][R.CURRENT][first["match_kp1"][failed]] == 1).all()
    assert set(rows.tolist()) & set(results[1]["rows"].tolist())                                         # handed to the next adjacent


def test_lists_violations_and_capacity_of_the_restatement():
    sc, free_rows, _, results, _ = R.fixture()
    adj, matched = results[0]["slot"], results[0]["matched"]
    n = results[0]["n_matches"]
    assert R.lists_of(sc, R.CURRENT, adj, matched, free_rows[:n - 1])[:2] == (R.CAPACITY, n)
    assert R.lists_of(sc, R.CURRENT, adj, matched, free_rows, cap_rows=n - 1)[:2] == (R.CAPACITY, n)
    j = int(results[0]["match_kp1"][-1])
    for key, change in (("range", lambda m, s: m.__setitem__(j, sc["n_kp"][adj])), ("twice", lambda m, s: m.__setitem__(j, m[results[0]["match_kp1"][0]])),
                        ("bound", lambda m, s: s["kf_mp"].__setitem__((R.CURRENT, j), 5)), ("live", lambda m, s: s["mp_live"].__setitem__(free_rows[1], 1)),
                        ("octave", lambda m, s: s["kp"]["octave"].__setitem__((R.CURRENT, j), 8))):
        m, s = matched.copy(), R.copy_state(sc)
        s["kp"] = {k: v.copy() for k, v in sc["kp"].items()}
        change(m, s)
        rc, _, L, _, _, v = R.lists_of(s, R.CURRENT, adj, m, free_rows)
        assert rc == R.INVALID and L is None and v[key] >= 1, key


def test_unbound_mask_edges():
    kf_mp = np.array([[-1, 10, 9, 0, 11, -2 ** 31, 2 ** 31 - 1]], np.int32)
    assert R.unbound_mask(kf_mp, 10, 0, 7).tolist() == [1, 1, 0, 0, 1, 1, 1]


def test_create_E21_of_the_package_has_the_bits_of_the_oracle():
    sc = R.fixture()[0]
    for adj in (0, 3, 4, 5):
        P1, P2 = sc["poses"][R.CURRENT].reshape(3, 4), sc["poses"][adj].reshape(3, 4)
        got = mi355slam.create_E21(P2[:, :3], P2[:, 3], P1[:, :3], P1[:, 3])
        assert got.tobytes() == np.ascontiguousarray(R.essential(sc, R.CURRENT, adj)).tobytes()
