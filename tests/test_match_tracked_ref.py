"""tests/match_tracked_ref.py against itself: the staged form of the device chain equals the sequential restatement of matchTrackedFeatures,
and the generated scene holds what the GPU tests rely on (conditions on the INPUTS: a seed that breaks one is redrawn, the condition stays)."""
import numpy as np
import pytest

import map_refresh_ref as MR
import match_tracked_ref as R
import triangulate_ref as TR

SCENES = ("desc", "no_desc", "empty_trip")


@pytest.mark.parametrize("name", SCENES)
def test_the_stages_equal_the_sequential_walk(name):
    sc, frame, new_rows, want = R.fixture(name)
    seq = R.sequential(sc, frame, new_rows)
    assert seq["rc"] == 0 and want["rc"] == 0
    assert np.array_equal(seq["outcome"], want["outcome"]) and seq["counts"] == want["counts"]
    for k in ("created_rows", "created_kp", "tracked_rows", "checked_rows"):
        assert np.array_equal(seq[k], want[k]), k
    assert R.same_state(seq["state"], want["state"])
    assert not R.same_state(sc, want["state"])


def test_every_outcome_occurs_five_times_and_the_binding_ones_in_every_trip():
    with_desc, without = R.fixture("desc")[3]["outcome"], R.fixture("no_desc")[3]["outcome"]
    count = np.bincount(with_desc, minlength=7) + np.bincount(without, minlength=7)
    assert (count >= 5).all(), count
    assert np.bincount(with_desc, minlength=7)[R.NO_DESCRIPTORS] == 0 and np.bincount(without, minlength=7)[R.CREATED] == 0
    assert len(with_desc) == R.N_KP > 2 * R.TRIP             # three trips
    for o in (R.CREATED, R.TRACKED, R.CHECKED):
        assert (with_desc[R.TRIP:2 * R.TRIP] == o).any() and (with_desc[2 * R.TRIP:] == o).any(), o
    tracked = (R.fixture("desc")[1]["kp_track"] >= 0).sum()
    assert 0.4 * R.N_KP <= tracked <= 0.6 * R.N_KP


def test_the_first_trip_of_the_empty_trip_frame_binds_nothing():
    o = R.fixture("empty_trip")[3]["outcome"]
    assert (o[:R.TRIP] == R.NO_TRACK).all()
    for k in (R.CREATED, R.TRACKED, R.CHECKED):
        assert (o[R.TRIP:] == k).sum() >= 5


def test_first_last_leaves_unsure_triangulated_and_failed_rows():
    for name in SCENES:
        status = R.fixture(name)[3]["status"]
        assert {TR.NOT_TRIANGULATED, TR.UNSURE, TR.TRIANGULATED} <= set(status.tolist()), name
        st, res = R.fixture(name)[3]["state"], R.fixture(name)[3]
        assert (st["mp_flags"][res["tracked_rows"]] == np.array(TR.FLAG_OF_STATUS, np.uint8)[status]).all()


def test_tracks_are_rejected_by_liveness_alone_and_by_the_track_id_alone():
    sc, frame, _, _ = R.fixture("desc")
    reasons = [R.presence(sc, int(t))[1] for t in frame["kp_track"] if t >= 0]
    assert reasons.count(3) >= 1 and reasons.count(4) >= 1 and reasons.count(2) >= 4 and reasons.count(1) >= 5
    for t in frame["kp_track"]:
        if t >= 0 and R.presence(sc, int(t))[1] == 3:
            assert sc["mp_track"][sc["track_row"][t - sc["track_base"]]] == t        # only mp_live says no
        if t >= 0 and R.presence(sc, int(t))[1] == 4:
            assert sc["mp_live"][sc["track_row"][t - sc["track_base"]]]              # only mp_track says no


@pytest.mark.parametrize("name", SCENES)
def test_the_two_observation_rule_equals_the_general_medoid(name):
    """Every UNSURE row after the walk has at most two descriptors and the general medoid picks the first (also asserted inside finish())."""
    sc, frame, new_rows, want = R.fixture(name)
    st = want["state"]
    unsure = [int(r) for r in want["tracked_rows"] if st["mp_flags"][r] == 2]
    assert len(unsure) >= 5
    some_with_one = False
    for r in unsure:
        d = R.descriptors_of(st, r)
        assert len(R.observations(st, r)[0]) == 2 and len(d) <= 2
        some_with_one |= len(d) == 1
        if len(d):
            assert MR.medoid_of(d) == 0 and np.array_equal(st["table"]["desc"][r], d[0])
    assert some_with_one or name != "no_desc"
    rng = np.random.default_rng(3)                           # and on descriptors at large: two of them, any distance apart, equal ones included
    for _ in range(200):
        a = rng.integers(0, 2 ** 32, (1, 8), dtype=np.uint64).astype(np.uint32)
        b = a ^ (rng.integers(0, 2 ** 32, (1, 8), dtype=np.uint64).astype(np.uint32) & np.uint32(rng.choice([0, 1, 0xffff, 0xffffffff])))
        assert MR.medoid_of(np.concatenate([a, b])) == 0
    ones = np.full((1, 8), 0xffffffff, np.uint32)
    assert MR.medoid_of(np.concatenate([ones, ~ones])) == 0  # 256 bits apart: the medians are still 0


def test_refresh_rows_of_the_two_kinds_of_frame():
    for name in SCENES:
        sc, frame, new_rows, want = R.fixture(name)
        st = want["state"]
        promoted = [int(r) for r in want["tracked_rows"] if st["mp_flags"][r] & 1]
        expect = promoted + (want["checked_rows"].tolist() if want["has_desc"] else [])
        assert want["refresh_rows"].tolist() == expect and len(promoted) >= 5


def test_capacity_and_violations_leave_the_tables_alone():
    sc, frame, new_rows, want = R.fixture("desc")
    n = want["counts"][0]
    short = R.walk(sc, frame, new_rows[:n - 1])
    assert short["rc"] == R.CAPACITY and short["counts"][0] == n and R.same_state(short["state"], sc)
    assert np.array_equal(short["outcome"], want["outcome"])
    exact = R.walk(sc, frame, new_rows[:n])
    assert exact["rc"] == 0 and np.array_equal(exact["created_rows"], new_rows[:n])
    for which in ("bound", "live", "octave"):
        bad = R.copy_state(sc)
        bad["kp"] = {k: v.copy() for k, v in sc["kp"].items()}
        if which == "bound":
            bad["kf_mp"][R.CURRENT, int(want["created_kp"][0])] = 5
        elif which == "live":
            bad["mp_live"][new_rows[1]] = 1
        else:
            bad["kp"]["octave"][R.CURRENT, int(np.flatnonzero(want["outcome"] == R.TRACKED)[0])] = 8
        got = R.walk(bad, frame, new_rows)
        assert got["rc"] == R.INVALID and got["violations"][which] == 1 and R.same_state(got["state"], bad), which
