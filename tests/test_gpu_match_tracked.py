"""ms_match_tracked and ms_match_tracked_finish on the device against tests/match_tracked_ref.py, their specification, through
the Python chain.  Every comparison is exact equality (floats by their bits): outcomes, counters, lists and every table, after each stage
of the chain and at its end -- the positions ms_triangulate_lists writes between the two new kernels included, which the chain test prints
the count of before it asserts."""
import ctypes as C

import numpy as np
import pytest

import match_tracked_ref as R
import mi355slam
import triangulate_ref as TR

pytestmark = pytest.mark.gpu


def put(ctx, buf, arr):
    arr = np.ascontiguousarray(arr)
    ctx.check(mi355slam.lib().ms_dev_upload(ctx._h, C.c_void_p(buf.ptr), mi355slam._vp(arr), C.c_size_t(arr.nbytes)), "ms_dev_upload")


class Device:
    """A state of the restatement with its tables on the device."""

    def __init__(self, ctx, sc):
        self.ctx = ctx
        self.table = mi355slam.MapPointTable(ctx, **sc["table"])
        self.kf = mi355slam.KeyframeTable(ctx, sc["kf_mp"])
        self.kp = mi355slam.KeypointTable(ctx, **sc["kp"])
        self.flags, self.live, self.pool = ctx.upload(sc["mp_flags"]), ctx.upload(sc["mp_live"]), ctx.upload(sc["pool"])
        self.tracks = mi355slam.TrackTable(ctx, sc["mp_track"], sc["track_row"], sc["track_base"])
        self.poses = mi355slam.KeyframePoseTable(ctx, sc["poses"])

    def restore(self, sc):
        """Every table the chain writes, as the scene has it."""
        t = sc["table"]
        self.table.update(0, self.table.n, **t)
        for buf, a in ((self.kf.kf_mp, sc["kf_mp"]), (self.flags, sc["mp_flags"]), (self.live, sc["mp_live"]), (self.tracks.mp_track, sc["mp_track"]),
                       (self.tracks.track_row, sc["track_row"])):
            put(self.ctx, buf, a)

    def state(self):
        n = self.table.n
        mp_track, track_row = self.tracks.download()
        table = dict(pos=self.table.pos.download(np.float64, (n, 3)), norm=self.table.norm.download(np.float32, (n, 3)), min_dist=self.table.min_dist.download(np.float32, (n,)),
                     max_dist=self.table.max_dist.download(np.float32, (n,)), desc=self.table.desc.download(np.uint32, (n, 8)))
        return dict(kf_mp=self.kf.download(), mp_flags=self.flags.download(np.uint8, (n,)), mp_live=self.live.download(np.uint8, (n,)), mp_track=mp_track,
                    track_row=track_row, table=table)

    def args(self, sc):
        return (self.table, self.flags, self.live, self.tracks, self.kp, self.pool, self.poses, sc["kf_id"], sc["cams"], sc["focal"], sc["desc_base"])

    def frame(self, sc, frame):
        return dict(slot=frame["slot"], pose=sc["poses"][frame["slot"]], kp_track=frame["kp_track"])

    def walk(self, sc, frame, new_rows, out, slot=None):
        """ms_match_tracked alone (slot: passed in place of the frame's)."""
        s = frame["slot"]
        f = dict(slot=s if slot is None else slot, pose=sc["poses"][s], cam=sc["cams"][s], focal=sc["focal"][s], desc_base=sc["desc_base"][s], level_sigma_sq=sc["S"]["level_sigma_sq"],
                 rel_reprojection_threshold=sc["S"]["rel_reprojection_threshold"], view_cos_limit=sc["view_cos_limit"])
        return self.kf.match_tracked_device(self.table, self.flags, self.live, self.tracks, self.kp, self.pool, f, frame["kp_track"], new_rows, out)

    def free(self):
        for b in (self.table.pos, self.table.norm, self.table.min_dist, self.table.max_dist, self.table.desc, self.kf.kf_mp, self.flags, self.live, self.pool,
                  self.poses.pose):
            b.free()
        self.kp.free(); self.tracks.free()


@pytest.fixture(scope="module")
def dev(ctx):
    d = Device(ctx, R.fixture("desc")[0])
    yield d
    d.free()


@pytest.fixture(scope="module")
def dev_no_desc(ctx):
    d = Device(ctx, R.fixture("no_desc")[0])
    yield d
    d.free()


def walk_buffers(ctx, n_kp, n_new, fill=0xA5):
    out = dict(outcome=ctx.alloc(n_kp + 64), created_rows=ctx.alloc(4 * n_new + 64), created_kp=ctx.alloc(4 * n_new + 64), tracked_rows=ctx.alloc(4 * n_kp + 64),
               checked_rows=ctx.alloc(4 * n_kp + 64))
    for b in out.values():
        put(ctx, b, np.full(b.nbytes, fill, np.uint8))
    return out


def chain(d, name):
    """The whole chain on scene `name`: every stage against the restatement."""
    sc, frame, new_rows, want = R.fixture(name)
    d.restore(sc)
    w = R.walk(sc, frame, new_rows)
    st = w["state"]
    res = d.kf.match_tracked_bind(*d.args(sc), d.frame(sc, frame), new_rows, sc["S"], sc["view_cos_limit"])
    # ---- ms_match_tracked: exact
    assert np.array_equal(res["outcome"], w["outcome"]) and res["counts"].tolist() == w["counts"]
    assert np.array_equal(res["created_rows"], w["created_rows"]) and np.array_equal(res["created_kp"], w["created_kp"])
    for k in ("tracked_rows", "checked_rows"):
        assert np.array_equal(res["bufs"][k].download(np.int32, (len(w[k]),)), w[k]), k
    # ---- FIRST_LAST of the just-tracked rows
    status = R.triangulate_tracked(st, w["tracked_rows"])
    assert np.array_equal(res["status"], status)
    got = d.state()
    moved = w["tracked_rows"][status != TR.NOT_TRIANGULATED]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    same = int((bits(got["table"]["pos"][moved]) == bits(st["table"]["pos"][moved])).all(axis=1).sum())
    print("%s: %d rows triangulated, %d of them bit-equal to the restatement" % (name, len(moved), same))
    assert R.same_state(got, st)
    # ---- ms_match_tracked_finish and the refresh
    refresh_rows = R.finish(st, w["tracked_rows"], w["checked_rows"], w["has_desc"])
    res = d.kf.match_tracked_refresh(res, sc["sf"])
    assert np.array_equal(res["refresh_rows"], refresh_rows) and np.array_equal(refresh_rows, want["refresh_rows"])
    got = d.state()
    assert R.same_state(got, st) and R.same_state(got, want["state"])
    return got


def test_the_scene_end_to_end(dev):
    got = chain(dev, "desc")
    sc = R.fixture("desc")[0]
    assert not np.array_equal(got["kf_mp"], sc["kf_mp"]) and not np.array_equal(got["table"]["desc"], sc["table"]["desc"])


def test_a_frame_without_descriptors(dev_no_desc):
    chain(dev_no_desc, "no_desc")
    assert (R.fixture("no_desc")[3]["outcome"] == R.NO_DESCRIPTORS).sum() >= 5


def test_a_first_trip_without_a_tracked_keypoint(dev):
    chain(dev, "empty_trip")


def test_new_rows_one_short_then_enough(ctx, dev):
    sc, frame, new_rows, want = R.fixture("desc")
    n = want["counts"][0]
    dev.restore(sc)
    out = walk_buffers(ctx, R.N_KP, n)
    rc, counts = dev.walk(sc, frame, new_rows[:n - 1], out)
    assert rc == mi355slam.MS_ERR_CAPACITY and counts.tolist() == want["counts"]
    assert b"creates %d map points, new_rows holds %d" % (n, n - 1) in mi355slam.lib().ms_last_error(ctx._h)
    assert R.same_state(dev.state(), sc)
    assert np.array_equal(out["outcome"].download(np.uint8, (R.N_KP,)), want["outcome"])
    for k in ("created_rows", "created_kp", "tracked_rows", "checked_rows"):
        assert (out[k].download(np.uint8, (out[k].nbytes,)) == 0xA5).all(), k
    rc, counts = dev.walk(sc, frame, new_rows[:n], out)
    w = R.walk(sc, frame, new_rows[:n])
    assert rc == 0 and counts.tolist() == w["counts"] and R.same_state(dev.state(), w["state"])
    assert np.array_equal(out["created_rows"].download(np.int32, (n,)), new_rows[:n])
    for k, m in (("outcome", R.N_KP), ("created_rows", 4 * n), ("created_kp", 4 * n), ("tracked_rows", 4 * w["counts"][1]), ("checked_rows", 4 * w["counts"][2])):
        assert (out[k].download(np.uint8, (out[k].nbytes,))[m:] == 0xA5).all(), k     # nothing behind the lists
    for b in out.values():
        b.free()


@pytest.mark.parametrize("which", ("bound", "live", "octave"))
def test_each_device_violation_leaves_the_tables_alone(ctx, which):
    sc, frame, new_rows, want = R.fixture("desc")
    bad = R.copy_state(sc)
    bad["kp"] = {k: v.copy() for k, v in sc["kp"].items()}
    if which == "bound":                                     # a created keypoint in the third trip whose entry is taken (keyframe.cpp:275)
        bad["kf_mp"][R.CURRENT, int(want["created_kp"][-1])] = 5
    elif which == "live":
        bad["mp_live"][new_rows[1]] = 1
    else:
        bad["kp"]["octave"][R.CURRENT, int(np.flatnonzero(want["outcome"] == R.TRACKED)[-1])] = 8
    w = R.walk(bad, frame, new_rows)
    assert w["rc"] == R.INVALID and w["violations"][which] == 1
    d = Device(ctx, bad)
    out = walk_buffers(ctx, R.N_KP, len(new_rows))
    rc, counts = d.walk(bad, frame, new_rows, out)
    assert rc == mi355slam.MS_ERR_INVALID and b"nothing written" in mi355slam.lib().ms_last_error(ctx._h)
    assert R.same_state(d.state(), bad)
    for k in ("created_rows", "created_kp", "tracked_rows", "checked_rows"):
        assert (out[k].download(np.uint8, (out[k].nbytes,)) == 0xA5).all(), k
    for b in out.values():
        b.free()
    d.free()


def test_host_validation_runs_before_the_device(ctx, dev):
    sc, frame, new_rows, _ = R.fixture("desc")
    dev.restore(sc)
    out = walk_buffers(ctx, R.N_KP, len(new_rows))
    twice = frame["kp_track"].copy()
    twice[np.flatnonzero(twice < 0)[0]] = twice[twice >= 0][0]
    for f, rows, slot, message in ((dict(frame, kp_track=twice), new_rows, None, b"track id %d is listed twice" % twice[twice >= 0][0]),
                                   (frame, np.append(new_rows, new_rows[0]), None, b"new row %d is listed twice" % new_rows[0]),
                                   (frame, new_rows, R.N_KF, b"slot 12 outside [0, 12)")):
        rc, _ = dev.walk(sc, f, rows, out, slot)
        assert rc == mi355slam.MS_ERR_INVALID and message in mi355slam.lib().ms_last_error(ctx._h)
    assert R.same_state(dev.state(), sc)
    assert (out["outcome"].download(np.uint8, (out["outcome"].nbytes,)) == 0xA5).all()
    for b in out.values():
        b.free()


def test_the_same_call_on_a_restored_table_gives_the_same_bits(dev):
    sc, frame, new_rows, _ = R.fixture("desc")
    states, results = [], []
    for _ in range(2):
        dev.restore(sc)
        results.append(dev.kf.match_tracked(*dev.args(sc), dev.frame(sc, frame), new_rows, sc["S"], sc["sf"], sc["view_cos_limit"]))
        states.append(dev.state())
    assert R.same_state(states[0], states[1])
    for k in ("outcome", "created_rows", "created_kp", "counts", "status", "refresh_rows"):
        assert results[0][k].tobytes() == results[1][k].tobytes(), k


def test_no_host_allocation_on_a_second_call_of_equal_size(dev):
    allocs = mi355slam.lib().ms_debug_host_allocs
    allocs.restype = C.c_longlong
    sc, frame, new_rows, _ = R.fixture("desc")
    run = lambda: (dev.restore(sc), dev.kf.match_tracked(*dev.args(sc), dev.frame(sc, frame), new_rows, sc["S"], sc["sf"], sc["view_cos_limit"]))
    run()
    before = allocs()
    run()
    assert allocs() == before


def test_an_empty_frame_and_a_frame_without_tracks(ctx, dev):
    sc, frame, new_rows, _ = R.fixture("desc")
    dev.restore(sc)
    for kp_track in (np.zeros(0, np.int32), np.full(300, -1, np.int32)):
        res = dev.kf.match_tracked(*dev.args(sc), dict(dev.frame(sc, frame), kp_track=kp_track), new_rows, sc["S"], sc["sf"], sc["view_cos_limit"])
        assert res["counts"].tolist() == [0] * 5 and len(res["refresh_rows"]) == 0 and (res["outcome"] == 0).all() and len(res["outcome"]) == len(kp_track)
    assert R.same_state(dev.state(), sc)


def test_finish_walks_more_rows_than_one_trip(ctx, dev):
    """ms_match_tracked_finish alone on the lists of 700 rows of the map (three trips of its one workgroup, the kept count carried across
    them): flags of every kind in every trip, the descriptor rule and the packed rows against their restatement from the same lists."""
    sc = R.fixture("desc")[0]
    dev.restore(sc)
    rng = np.random.default_rng(8)
    n_mp, flags = dev.table.n, sc["mp_flags"]
    observed = np.flatnonzero(sc["mp_live"] & (np.bincount(sc["kf_mp"][sc["kf_mp"] >= 0], minlength=n_mp)[:n_mp] > 0))
    rows_in = rng.permutation(observed)[:700].astype(np.int32)
    checked = rng.permutation(n_mp)[:300].astype(np.int32)
    lists = mi355slam.ObservationLists(ctx, 700, 8000)
    rc, n_rows, n_obs = dev.kf.observation_lists_device(lists, sc["kf_id"], n_mp, dict(source=mi355slam.OBS_FROM_ROWS, drop_empty=1, rows_in=rows_in), dev.kp, sc["desc_base"],
                                                        dev.flags, 8)
    assert (rc, n_rows) == (0, 700)
    L = lists.download(n_rows, n_obs, ("rows", "obs_start", "obs_desc"))
    assert np.array_equal(L["rows"], rows_in)
    for trip in range(3):
        f = flags[rows_in[256 * trip:256 * (trip + 1)]]
        assert (f == 2).sum() >= 5 and (f == 3).sum() >= 5 and (f == 0).sum() >= 5, trip
    want_desc, without = sc["table"]["desc"].copy(), 0
    for i, r in enumerate(rows_in):
        if flags[r] == 2:
            od = L["obs_desc"][L["obs_start"][i]:L["obs_start"][i + 1]]
            have = od[od != -1]
            without += len(have) == 0
            if len(have):
                want_desc[r] = sc["pool"][have[0]]
    assert not np.array_equal(want_desc, sc["table"]["desc"])
    kept = rows_in[(flags[rows_in] & 1) != 0]
    d_checked, d_refresh = ctx.upload(checked), ctx.alloc(4 * 1000 + 64)
    for append, want_rows in ((1, np.concatenate([kept, checked])), (0, kept)):
        dev.restore(sc)
        put(ctx, d_refresh, np.full(d_refresh.nbytes, 0xA5, np.uint8))
        rc, n = dev.table.match_tracked_finish_device(lists, n_rows, dev.flags, dev.pool, d_checked, 300, append, d_refresh, 1000)
        assert (rc, n) == (0, len(want_rows)), mi355slam.lib().ms_last_error(ctx._h)
        assert np.array_equal(d_refresh.download(np.int32, (n,)), want_rows)
        assert (d_refresh.download(np.uint8, (d_refresh.nbytes,))[4 * n:] == 0xA5).all()
        got = dev.state()
        assert np.array_equal(got["table"]["desc"], want_desc)
        got["table"]["desc"] = sc["table"]["desc"]
        assert R.same_state(got, sc)                         # nothing else is written
    rc, n = dev.table.match_tracked_finish_device(lists, n_rows, dev.flags, dev.pool, d_checked, 300, 1, d_refresh, 999)
    assert rc == mi355slam.MS_ERR_CAPACITY
    dev.restore(sc)
    rc, n = dev.table.match_tracked_finish_device(lists, n_rows, dev.flags, None, d_checked, 300, 0, d_refresh, 1000)      # no pool: the descriptors stay
    assert (rc, n) == (0, len(kept)) and R.same_state(dev.state(), sc)
    print("finish: %d rows, %d unsure (%d without a descriptor), %d kept" % (n_rows, int((flags[rows_in] == 2).sum()), without, len(kept)))
    for b in (d_checked, d_refresh):
        b.free()
    lists.free()
