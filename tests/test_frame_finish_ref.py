"""tests/frame_finish_ref.py, the specification of ms_frame_finish, against a literal walk of setPointCloudOutput
(mapper_helpers.cpp:484-497) and removeKeyframe (:375-408) over per-point dictionaries of observations built from the tables; a list of
removed slots against its slots one at a time; and the conditions each GPU scene is there to hit."""
import numpy as np
import pytest

import mi355slam
import frame_finish_ref as R

NAMES = list(R.SCENES)


@pytest.fixture(autouse=True, scope="module")
def the_call_the_restatement_specifies():
    """A specification of a call the library does not have says nothing about the library; its codes are the library's."""
    assert hasattr(mi355slam.lib(), "ms_frame_finish") and hasattr(mi355slam.KeyframeTable, "frame_finish")
    assert (R.OK, R.CAPACITY) == (0, mi355slam.MS_ERR_CAPACITY)


class Map:
    """mapDB as the reference holds it: keyframes[kfId].mapPoints, and mapPoints[row].observations = the (kfId, keypoint) pairs."""

    def __init__(self, t):
        self.t, self.n_mp = t, len(t["mp_flags"])
        self.live = np.ones(self.n_mp, bool) if t["mp_live"] is None else t["mp_live"].astype(bool)
        self.flags = t["mp_flags"].copy()
        self.keyframes = {int(k): [int(r) for r in t["kf_mp"][s]] for s, k in enumerate(t["kf_id"]) if k >= 0}
        self.slot_of = {int(k): s for s, k in enumerate(t["kf_id"]) if k >= 0}
        self.observations = {}
        for k, mps in self.keyframes.items():
            for j, r in enumerate(mps):
                if 0 <= r < self.n_mp:
                    self.observations.setdefault(r, []).append((k, j))

    def point_cloud(self, kf_id, n_kp):                      # :484-497
        out = []
        for j, r in enumerate(self.keyframes[kf_id][:n_kp]):
            if not 0 <= r < self.n_mp or not self.live[r]:
                continue
            if self.flags[r] & 1:
                out.append((r, j, -1 if self.t["mp_track"] is None else int(self.t["mp_track"][r]), self.t["mp_pos"][r].tobytes()))
        return out

    def remove_keyframe(self, kf_id):                        # :391-408
        erase, erased, touched = [], 0, []
        for r in self.keyframes[kf_id]:
            if not 0 <= r < self.n_mp:
                continue
            erased += 1
            touched.append(r)
            self.observations[r] = [o for o in self.observations.get(r, []) if o[0] != kf_id]         # eraseObservation
            if not self.observations[r] and self.live[r] and r not in erase:
                erase.append(r)
        for r in erase:                                      # removeMapPoint
            self.live[r] = False
            self.flags[r] = 0
        del self.keyframes[kf_id]
        return erase, erased, touched


def walk(sc):
    t = sc["t"]
    m = Map(t)
    cl = m.point_cloud(int(t["kf_id"][sc["cloud_slot"]]), sc["n_kp"]) if sc["cloud_slot"] >= 0 else []
    removed, erased, touched = [], 0, []
    for s in sc["remove"]:
        e, n, rows = m.remove_keyframe(int(t["kf_id"][s]))
        removed += e; erased += n; touched += rows
    return m, cl, removed, erased, touched


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_equals_the_literal_walk(name):
    sc, want = R.cached(name)
    t = sc["t"]
    m, cl, removed, erased, touched = walk(sc)
    assert [(int(r), int(j), int(k), p.tobytes()) for r, j, k, p in zip(want["cloud_row"], want["cloud_kp"], want["cloud_track"], want["cloud_pos"])] == cl
    # a row orphaned by a later slot of the list after an earlier one claimed it: the walk reports it when it empties, the tables in first-claim order
    assert sorted(want["removed_rows"].tolist()) == sorted(removed) and len(set(removed)) == len(removed)
    first = {}
    for r in touched:
        first.setdefault(r, len(first))
    assert want["removed_rows"].tolist() == sorted(removed, key=first.get)
    assert want["counts"].tolist() == [len(cl), len(removed), erased] and want["rc"] == R.OK
    if sc["remove"]:
        assert np.array_equal(want["mp_live"].astype(bool), m.live) and np.array_equal(want["mp_flags"], m.flags)
        for s in sc["remove"]:
            assert (want["kf_mp"][s] == -1).all()
        others = [s for s in range(len(t["kf_id"])) if s not in sc["remove"]]
        assert np.array_equal(want["kf_mp"][others], t["kf_mp"][others])
        rows = sorted(set(touched))
        assert [int(want["n_obs"][r]) for r in rows] == [len(m.observations[r]) for r in rows]
        rest = np.setdiff1d(np.arange(m.n_mp), rows)
        assert np.array_equal(want["n_obs"][rest], t["n_obs"][rest])
    else:
        for k in R.TABLES:
            assert (want[k] is None and t[k] is None) or np.array_equal(want[k], t[k]), k


@pytest.mark.parametrize("name", ["per_frame", "two_removed", "second_offsets_trip"])
def test_a_list_equals_its_slots_one_at_a_time(name):
    sc, want = R.cached(name)
    t, kf_id = dict(sc["t"]), sc["t"]["kf_id"].copy()
    removed, erased = [], 0
    for s in sc["remove"]:
        one = R.finish(dict(t, kf_id=kf_id), [s], -1, 0)
        assert one["rc"] == R.OK and one["counts"][0] == 0
        removed += one["removed_rows"].tolist()
        erased += int(one["counts"][2])
        t.update({k: one[k] for k in R.TABLES})
        kf_id[s] = -1                                        # the caller's part
    assert sorted(removed) == sorted(want["removed_rows"].tolist()) and erased == want["counts"][2]
    for k in ("kf_mp", "mp_flags", "mp_live"):
        assert np.array_equal(t[k], want[k]), k
    live = want["mp_live"].astype(bool)                      # a removed row's count is 0 either way; a row that stays ends at the same count
    assert np.array_equal(t["n_obs"][live], want["n_obs"][live])


def test_capacity_keeps_every_table():
    sc, want = R.cached("per_frame")
    n = len(want["removed_rows"])
    short = R.finish(sc["t"], sc["remove"], sc["cloud_slot"], sc["n_kp"], cap_removed=n - 1)
    assert short["rc"] == R.CAPACITY and short["counts"].tolist() == want["counts"].tolist() and len(short["removed_rows"]) == 0
    for k in R.TABLES:
        assert np.array_equal(short[k], sc["t"][k]), k
    for k in ("cloud_row", "cloud_kp", "cloud_track", "cloud_pos"):
        assert np.array_equal(short[k], want[k]), k
    exact = R.finish(sc["t"], sc["remove"], sc["cloud_slot"], sc["n_kp"], cap_removed=n)
    assert exact["rc"] == R.OK and np.array_equal(exact["removed_rows"], want["removed_rows"])


def test_the_noops():
    sc, _ = R.cached("per_frame")
    t = sc["t"]
    out = R.finish(t, [], -1, 0)
    assert out["counts"].tolist() == [0, 0, 0] and all(np.array_equal(out[k], t[k]) for k in R.TABLES)
    assert R.finish(t, [], 3, 0)["counts"].tolist() == [0, 0, 0]
    empty = dict(t, mp_flags=np.zeros(0, np.uint8), mp_live=np.zeros(0, np.uint8), mp_pos=np.zeros((0, 3)), mp_track=np.zeros(0, np.int32), n_obs=np.zeros(0, np.int32))
    out = R.finish(empty, [3], 3, 60)
    assert out["counts"].tolist() == [0, 0, 0] and (out["kf_mp"][3] == -1).all() and np.array_equal(out["kf_mp"][:3], t["kf_mp"][:3])


@pytest.mark.parametrize("name", NAMES)
def test_each_scene_hits_what_it_is_for(name):
    sc, want = R.cached(name)
    R.scene_conditions(name, sc, want)
