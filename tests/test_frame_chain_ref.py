"""The front end's chain as a chain, on the CPU: tests/frame_chain_ref.py runs its whole schedule -- extract, three
publishes, six frames of admit / bind / refresh / pose / finish, the removal of the oldest keyframe, the second extract -- on ONE state,
the pose step solved by the CPU oracle.  After every step the invariants I1 - I5 hold and n_obs is the transpose of kf_mp where the chain
promises it.  The scene's conditions are asserted here so that tests/test_gpu_frame_chain.py, which runs the same schedule on the device,
cannot pass on a scene that exercises nothing:

  - every frame keeps 270 - 300 features (more than 256: the second trip of every one-workgroup keypoint walk), drops some by `keep` and
    some by the mask, takes depths from the image;
  - outcomes 2, 3, 4, 5 and 6 occur in every frame, and FIRST_LAST makes rows TRIANGULATED.  Outcomes 0 and 1 do NOT occur, and cannot:
    ms_frame_admit refuses an id < 0 and hands every kept feature's id down (keyframe.cpp:129), so no keypoint is without a track, and
    a front-end frame has no descriptors (conversion C4 of frame_chain_ref);
  - the removal of the oldest keyframe orphans at least 10 rows, and a track of one of them is in frame 3 and reads absent there;
  - frames 3 and 4 are admitted into slots that frames 0 and 1 left;
  - NEW, MOVED and REMOVED events all occur in the record;
  - the second extract succeeds with another row count than the first.

Two sensitivity tests break one contract each on the restatement side and see the chain fail within the same frame."""
import numpy as np
import pytest

import frame_chain_ref as C
import frame_finish_ref as FF
import map_publish_ref as MP
import match_tracked_ref as MT
import triangulate_ref as TR


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run_chain(oracle, until=None):
    """The schedule on a fresh state.  Returns the log: per step (step, outputs, stale rows of n_obs, the state's kf_id afterwards)."""
    w = C.world()
    st, run, log = C.initial_state(w, 0x5A), {}, []
    solve = lambda prob, frame, g: oracle.ba_solve(prob, frame["max_iters"], False)["pose"][0]
    for i, step in enumerate(C.schedule()):
        label = "step %d %s" % (i, step)
        before = {k: st[k] for k in ("mp_live", "track_row", "mp_track", "kf_mp", "n_obs")}
        out = C.apply_step(st, w, step, run, solve)
        C.check_invariants(st, label)
        stale = C.check_n_obs(st, step, out, label)
        log.append(dict(step=step, out=out, stale=stale, kf_id=st["kf_id"].copy(), before=before,
                        after={k: st[k] for k in ("mp_live", "track_row", "mp_track", "kf_mp", "mp_flags")}))
        if until is not None and step == until:
            break
    return w, st, run, log


@pytest.fixture(scope="module")
def chain(oracle):
    return run_chain(oracle)


def of(log, name, arg=None):
    return [e for e in log if e["step"][0] == name and (arg is None or e["step"][1] == arg)]


def test_the_frames_are_what_the_schedule_asks_for(chain):
    w, st, run, log = chain
    assert len(w["frames"]) == 6 and w["src"]["track_base"] > 0 and w["src"]["kf_mp"].shape == (10, 320) and (w["src"]["kf_id"] >= 0).sum() == 9
    src = w["src"]
    empty = src["kf_mp"][C.EMPTY_SRC_SLOT]
    assert src["kf_id"][C.EMPTY_SRC_SLOT] < 0 and ((empty >= 0) & (empty < C.N_SRC_MP)).any()             # stale entries in an empty slot
    assert (src["mp_live"] == 0).any() and {0, 2, 3} <= set(src["mp_flags"].tolist())
    tr = src["track_row"]
    named = tr[(tr >= 0) & (tr < C.N_SRC_MP)]
    assert (src["mp_track"][named] != C.TRACK_BASE + np.flatnonzero((tr >= 0) & (tr < C.N_SRC_MP))).any()   # recycled tracks
    assert len(w["active1"]) == 5 and st["kf_mp"].shape == (8, 320)
    assert 0 < w["n_mp_dst"] - of(log, "extract", 1)[0]["out"]["counts"][0] <= 64                          # a little above the active row count
    for f in range(6):
        c = of(log, "admit", f)[0]["out"]["counts"]
        assert 270 <= c[0] <= 300 and c[0] > 256 and c[1] > 0 and c[2] > 0 and c[3] > 0, (f, c)
    assert all((fr["feat"]["depth"] > 0).any() and (fr["feat"]["depth"] < 0).any() for fr in w["frames"])      # the feature's own depth, and the image's


def test_every_outcome_a_tracker_frame_can_have_occurs_in_every_frame(chain):
    w, st, run, log = chain
    promoted = 0
    for f in range(6):
        out = of(log, "bind", f)[0]["out"]
        n = np.bincount(out["outcome"], minlength=7)
        assert all(n[k] > 0 for k in (MT.TRACKED, MT.CHECKED, MT.FRUSTUM, MT.REPROJECTION, MT.NO_DESCRIPTORS)), (f, n)
        assert n[MT.NO_TRACK] == 0 and n[MT.CREATED] == 0, (f, n)                                         # see the module docstring
        promoted += int((out["status"] == TR.TRIANGULATED).sum())
        assert len(of(log, "refresh", f)[0]["out"]["refresh_rows"]) == int((out["status"] == TR.TRIANGULATED).sum())      # no descriptors: the promoted rows only
        p = of(log, "pose", f)[0]["out"]
        assert p["ran"] and p["g"]["n"] >= 10, (f, p["g"]["n"])
    assert promoted > 0


def test_the_removed_keyframe_orphans_rows_and_their_tracks_read_absent(chain):
    w, st, run, log = chain
    removal = of(log, "remove")[0]
    orphans = removal["out"]["removed_rows"]
    assert len(orphans) >= 10 and removal["out"]["counts"][0] == 0
    before, after = removal["before"], removal["after"]
    assert before["mp_live"][orphans].all() and not after["mp_live"][orphans].any() and not after["mp_flags"][orphans].any()
    assert same_bits(before["track_row"], after["track_row"]) and same_bits(before["mp_track"], after["mp_track"])      # no write to the tracks
    kp_track = of(log, "admit", 3)[0]["out"]["kp_track"]
    outcome = of(log, "bind", 3)[0]["out"]["outcome"]
    rows = after["track_row"][kp_track - C.TRACK_BASE]
    hit = np.flatnonzero(np.isin(rows, orphans) & (after["mp_track"][np.clip(rows, 0, st["n_mp"] - 1)] == kp_track))
    assert len(hit) >= 1 and (outcome[hit] == MT.NO_DESCRIPTORS).all()                                     # the row is there, carries the track, and is not live


def test_removed_slots_are_admitted_into_again(chain):
    w, st, run, log = chain
    assert C.FRAME_SLOT[3] == C.FRAME_SLOT[0] and C.FRAME_SLOT[4] == C.FRAME_SLOT[1] and C.FRAME_STAYS == (False, False, True, False, False, True)
    for f in (0, 1, 3, 4):
        fin = of(log, "finish", f)[0]
        slot = C.FRAME_SLOT[f]
        assert fin["out"]["remove"] == [slot] and fin["kf_id"][slot] == -1 and (fin["after"]["kf_mp"][slot] == -1).all()
        assert ((fin["before"]["kf_mp"][slot] >= 0)).sum() > 30                                          # the frame had bound rows
    for f in (2, 5):
        fin = of(log, "finish", f)[0]
        assert fin["out"]["remove"] == [] and fin["kf_id"][C.FRAME_SLOT[f]] == w["frames"][f]["kf_id"]


def test_the_cloud_is_the_point_array_of_the_pose_gather(chain):
    w, st, run, log = chain
    for f in range(6):
        g, cloud = of(log, "pose", f)[0]["out"]["g"], of(log, "finish", f)[0]["out"]
        assert g["n"] == len(cloud["cloud_row"]) > 0
        assert same_bits(cloud["cloud_pos"], g["point"]) and same_bits(cloud["cloud_kp"], g["kept"].astype(np.int32))
        assert same_bits(cloud["cloud_row"], of(log, "finish", f)[0]["before"]["kf_mp"][C.FRAME_SLOT[f], g["kept"]])


def test_every_kind_of_event_occurs_in_the_record(chain):
    w, st, run, log = chain
    counts = np.array([e["out"]["counts"] for e in of(log, "publish")])
    assert len(counts) == 3 and (counts[:, 0] > 0).all()
    assert counts[0, 2] > 0 and counts[0, 3] == 0 and counts[0, 4] == 0                                   # the first call: NEW only
    assert counts[1, 3] > 0                                                                               # FIRST_LAST moved recorded rows
    assert counts[:, 2].sum() > 0 and counts[:, 3].sum() > 0 and counts[:, 4].sum() > 0
    kinds = np.concatenate([e["out"]["ev_kind"] for e in of(log, "publish")])
    assert {MP.NEW, MP.MOVED, MP.REMOVED} <= set(kinds.tolist())


def test_the_second_extract_has_another_row_count(chain):
    w, st, run, log = chain
    a, b = (of(log, "extract", i)[0]["out"]["counts"] for i in (1, 2))
    assert a[0] != b[0] and b[0] <= w["n_mp_dst"] and b[2] > 0 and len(w["active2"]) == len(w["active1"]) + 1
    assert not same_bits(w["src"]["mp_pos"], w["src2"]["mp_pos"])
    second = of(log, "extract", 2)[0]
    assert (second["kf_id"][:6] >= 0).all() and (second["kf_id"][6:] == -1).all()                         # frame 2's slot is gone with the old copy


def test_where_n_obs_is_stale(chain):
    """The table of DESIGN 9.24: n_obs is the transpose after an extract, after ms_observation_count and, for the rows the removed
    slot listed, after a finish (asserted in run_chain by check_n_obs).  The match leaves exactly the rows it bound stale, by one; a
    finish that removes the frame repairs them all; a finish that keeps the frame repairs none, and the removal of another slot only
    its own rows."""
    w, st, run, log = chain
    for f in range(6):
        bound = np.union1d(of(log, "bind", f)[0]["out"]["tracked_rows"], of(log, "bind", f)[0]["out"]["checked_rows"])
        earlier = of(log, "admit", f)[0]["stale"]
        assert len(earlier) == 0                             # every frame starts behind an extract, a removing finish or ms_observation_count
        for name in ("bind", "refresh", "pose"):
            assert np.array_equal(of(log, name, f)[0]["stale"], np.union1d(earlier, bound)), (f, name)
        after = of(log, "finish", f)[0]["stale"]
        if C.FRAME_STAYS[f]:
            assert np.array_equal(after, np.union1d(earlier, bound)) and len(after) > 0
        else:
            assert np.array_equal(after, earlier)
    kept = of(log, "finish", 2)[0]["stale"]
    rem = of(log, "remove")[0]
    assert len(rem["stale"]) > 0 and set(rem["stale"].tolist()) == set(kept.tolist()) - set(rem["out"]["listed_rows"].tolist())
    for e in of(log, "publish"):                                                                           # every publish reads counts that are current
        assert len(e["stale"]) == 0


# ---- sensitivity: one contract broken on the restatement side
def test_a_finish_that_leaves_an_entry_of_the_removed_slot_fails_in_the_same_frame(oracle, monkeypatch):
    real = FF.finish

    def leaky(t, remove, cloud_slot, n_kp, cap_removed=None):
        out = real(t, remove, cloud_slot, n_kp, cap_removed)
        if remove:
            j = int(np.flatnonzero(t["kf_mp"][remove[0]] >= 0)[0])
            out["kf_mp"][remove[0], j] = t["kf_mp"][remove[0], j]
        return out

    monkeypatch.setattr(FF, "finish", leaky)
    with pytest.raises(AssertionError, match=r"step 7 \('finish', 0\).*I5"):
        run_chain(oracle, until=("admit", 1))


def test_a_finish_that_skips_the_n_obs_write_fails_at_the_removal_of_a_keyframe(oracle, monkeypatch):
    """For a frame that is removed at its own finish the write is invisible: the match left n_obs without the frame's observations,
    which is what the finish writes.  The removal of a keyframe that the counts include is where it shows."""
    real = FF.finish

    def lazy(t, remove, cloud_slot, n_kp, cap_removed=None):
        out = real(t, remove, cloud_slot, n_kp, cap_removed)
        out["n_obs"] = t["n_obs"].copy()
        return out

    monkeypatch.setattr(FF, "finish", lazy)
    with pytest.raises(AssertionError, match=r"step \d+ \('remove', \[0\]\).*remove"):
        run_chain(oracle, until=("admit", 3))
