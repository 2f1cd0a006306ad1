"""ms_ba_window_lists and ms_ba_window_apply on the device against tests/ba_window_ref.py, their specification.  Every
comparison is exact equality (floats by their bits); every output buffer, on the host and on the device, carries canary bytes behind its
end.  The observation lists come from the real chain, ms_map_point_union -> ms_observation_lists, on the same tables.  The apply's offsets
scan covers 128 x 256 = 32 768 edges per trip, the gather's 256 x 256 = 65 536 listed observations."""
import ctypes as C

import numpy as np
import pytest

import ba_synth
import ba_window_ref as R
import mi355slam

pytestmark = pytest.mark.gpu
CANARY = 0xA5
HOST_OUT = (("pose", np.float64, 7), ("point", np.float64, 3), ("obs_point", np.int32, 1), ("obs_pose", np.int32, 1), ("obs_uv", np.float64, 2), ("obs_info", np.float64, 1))
TABLES = ("kf_mp", "n_obs", "mp_flags", "mp_pos", "poses")


def put(ctx, buf, arr, byte_offset=0):
    arr = np.ascontiguousarray(arr)
    ctx.check(mi355slam.lib().ms_dev_upload(ctx._h, C.c_void_p(buf.ptr + byte_offset), mi355slam._vp(arr), C.c_size_t(arr.nbytes)), "ms_dev_upload")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def host_canary(n, dtype):
    """n elements and 8 more, every byte the canary."""
    return np.full((n + 8) * np.dtype(dtype).itemsize, CANARY, np.uint8).view(dtype)


def only_canary_behind(a, n):
    return bool((a.view(np.uint8)[n * a.itemsize:] == CANARY).all())


class Device:
    """A scene of the restatement with its tables on the device."""

    def __init__(self, ctx, sc):
        self.ctx, self.sc = ctx, sc
        n = sc["n_mp"]
        self.table = mi355slam.MapPointTable(ctx, sc["mp_pos"], np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 8), np.uint32))
        self.kf = mi355slam.KeyframeTable(ctx, sc["kf_mp"])
        self.kp = mi355slam.KeypointTable(ctx, **sc["kp"])
        self.flags, self.n_obs = ctx.upload(sc["mp_flags"]), ctx.upload(sc["n_obs"])
        self.poses = mi355slam.KeyframePoseTable(ctx, sc["poses"])
        self.lists = {}

    def observation_lists(self, slots):
        """union -> lists over `slots` on the device, once per slot set: (lists, n_rows, n_obs)."""
        key = tuple(int(s) for s in slots)
        if key not in self.lists:
            d_rows = self.ctx.alloc(4 * self.sc["n_mp"])
            n_in = int(self.kf.map_point_union_device(key, [(0, len(key), -1, 1)], self.sc["n_mp"], self.flags, d_rows, None)[0])
            lists = mi355slam.ObservationLists(self.ctx, max(n_in, 1), max(int(self.sc["n_obs"].sum()), 1))
            sel = dict(source=mi355slam.OBS_FROM_ROWS, rows_in=d_rows, n_in=n_in)
            rc, n_rows, n_obs = self.kf.observation_lists_device(lists, self.sc["kf_id"], self.sc["n_mp"], sel, self.kp, None, self.flags, R.N_LEVELS)
            self.ctx.check(rc, "ms_observation_lists")
            d_rows.free()
            self.lists[key] = (lists, n_rows, n_obs)
        return self.lists[key]

    def gather(self, local, current, lists=None, cap_point=None, cap_edge=None):
        """ms_ba_window_lists into canaried host arrays and canaried edge buffers of exactly the capacities.  Returns (rc, window)."""
        lists, n_rows, n_obs = self.observation_lists(local) if lists is None else lists
        cap_point = n_rows if cap_point is None else cap_point
        cap_edge = n_obs if cap_edge is None else cap_edge
        caps = dict(pose=len(local), point=cap_point, obs_point=cap_edge, obs_pose=cap_edge, obs_uv=cap_edge, obs_info=cap_edge)
        out = {k: host_canary(caps[k] * w, dt) for k, dt, w in HOST_OUT}
        edges = mi355slam.BaWindowEdges(self.ctx, cap_edge, guard=64)
        for name in edges._NAMES:
            put(self.ctx, edges[name], np.full(edges[name].nbytes, CANARY, np.uint8))
        rc, n_edge, n_current = self.kf.ba_window_lists_device(self.table, self.poses, lists, n_rows, n_obs, local, current, self.sc["cams"], self.sc["focal"], self.sc["sigma"],
                                                               edges, out, cap_point=cap_point, cap_edge=cap_edge)
        return rc, dict(out=out, edges=edges, lists=lists, n_rows=n_rows, n_obs=n_obs, n_edge=n_edge, n_current=n_current, local_slot=np.asarray(local, np.int32),
                        current_index=current, caps=caps)

    def restore(self, st=None):
        st = R.state_of(self.sc) if st is None else st
        for buf, k in ((self.kf.kf_mp, "kf_mp"), (self.n_obs, "n_obs"), (self.flags, "mp_flags"), (self.table.pos, "mp_pos"), (self.poses.pose, "poses")):
            put(self.ctx, buf, st[k])

    def state(self):
        n = self.sc["n_mp"]
        return dict(kf_mp=self.kf.download(), n_obs=self.n_obs.download(np.int32, (n,)), mp_flags=self.flags.download(np.uint8, (n,)),
                    mp_pos=self.table.pos.download(np.float64, (n, 3)), poses=self.poses.download())

    def free(self):
        for b in (self.table.pos, self.table.norm, self.table.min_dist, self.table.max_dist, self.table.desc, self.kf.kf_mp, self.flags, self.n_obs, self.poses.pose):
            b.free()
        self.kp.free()
        for lists, _, _ in self.lists.values():
            lists.free()


def gathered_equal(w, want):
    """Every host and device output against the restatement's, bit for bit, and nothing written behind them."""
    assert (w["n_rows"], w["n_obs"], w["n_edge"], w["n_current"]) == (want["n_rows"], want["n_obs"], want["n_edge"], want["n_current"])
    used = dict(pose=len(w["local_slot"]), point=w["n_rows"], obs_point=w["n_edge"], obs_pose=w["n_edge"], obs_uv=w["n_edge"], obs_info=w["n_edge"])
    for k, dt, width in HOST_OUT:
        n = used[k] * width
        assert same_bits(w["out"][k][:n], np.ascontiguousarray(want[k], dt).reshape(-1)), k
        assert only_canary_behind(w["out"][k], n), k
    got = w["edges"].download(w["n_edge"])
    for name in w["edges"]._NAMES:
        assert same_bits(got[name], want[name]), name
        assert bool((w["edges"][name].download(np.uint8, (w["edges"][name].nbytes,))[4 * w["n_edge"]:] == CANARY).all()), name
    assert same_bits(w["lists"]["rows"].download(np.int32, (w["n_rows"],)) if w["n_rows"] else np.zeros(0, np.int32), want["rows"])


def nothing_written(w):
    for k, dt, width in HOST_OUT:
        if k != "pose":
            assert only_canary_behind(w["out"][k], 0), k
    assert only_canary_behind(w["out"]["pose"], 0)
    for name in w["edges"]._NAMES:
        assert bool((w["edges"][name].download(np.uint8, (w["edges"][name].nbytes,)) == CANARY).all()), name


@pytest.fixture(scope="module")
def dev(ctx):
    d = Device(ctx, R.cached("base")[0])
    yield d
    d.free()


@pytest.fixture(scope="module")
def big(ctx):
    d = Device(ctx, R.cached("big")[0])
    yield d
    d.free()


@pytest.fixture(scope="module")
def base_window(dev):
    """The base scene's window on the device, gathered once and kept for the apply tests."""
    rc, w = dev.gather(R.BASE_LOCAL, 0)
    dev.ctx.check(rc, "ms_ba_window_lists")
    yield w
    w["edges"].free()


def test_base_scene(dev, base_window):
    sc, want = R.cached("base")
    R.base_conditions(sc, want)
    gathered_equal(base_window, want)
    assert base_window["n_current"] == R.literal_gather(sc, R.BASE_LOCAL, 0)["n_current"]
    rc, again = dev.gather(R.BASE_LOCAL, 0)                  # the same bits on every call
    assert rc == 0
    gathered_equal(again, want)
    again["edges"].free()
    rc, w = dev.gather(R.BASE_LOCAL, 5)                      # another current keyframe: only n_current moves
    assert rc == 0
    gathered_equal(w, R.gather(sc, R.BASE_LOCAL, 5))
    w["edges"].free()


def test_the_binding_runs_the_chain(dev):
    """KeyframeTable.ba_window: union -> lists -> gather with buffers of its own, regrown where a call asks for it."""
    sc, want = R.cached("base")
    lists = mi355slam.ObservationLists(dev.ctx, 4, 16)      # too small: the chain regrows them
    edges = mi355slam.BaWindowEdges(dev.ctx, 8)
    w = dev.kf.ba_window(dev.table, dev.poses, dev.flags, dev.kp, sc["kf_id"], R.BASE_LOCAL, 0, sc["cams"], sc["focal"], sc["sigma"], lists=lists, edges=edges)
    try:
        assert (w["n_rows"], w["n_obs"], w["n_edge"], w["n_current"]) == (want["n_rows"], want["n_obs"], want["n_edge"], want["n_current"])
        for k, dt, _ in HOST_OUT:
            assert same_bits(w[k].reshape(-1), np.ascontiguousarray(want[k], dt).reshape(-1)), k
        got = w["edges"].download(w["n_edge"])
        assert all(same_bits(got[name], want[name]) for name in got)
        pose, point = results(want)
        after, _, _ = R.apply(R.state_of(sc), want, pose, point, None, R.NEIGHBOR)
        rc, erased, n_stale = dev.kf.ba_window_apply(dev.table, dev.poses, dev.flags, dev.n_obs, w, pose, point, None, R.NEIGHBOR)
        assert (rc, len(erased), n_stale) == (0, 0, 0)
        state = dev.state()
        assert all(same_bits(state[k], after[k]) for k in TABLES)
    finally:
        dev.restore()
        w["lists"].free(); w["edges"].free()


def test_second_trip_of_the_offsets_scan(big):
    sc, want = R.cached("big")
    carry = R.big_conditions(sc, want)
    rc, w = big.gather(sc["local"], 0)
    assert rc == 0
    print("72 000 listed observations, %d kept, carry into the second trip %d" % (w["n_edge"], carry))
    gathered_equal(w, want)
    w["edges"].free()


def test_capacity(dev, base_window):
    sc, want = R.cached("base")
    for caps in (dict(cap_edge=want["n_edge"] - 1), dict(cap_point=want["n_rows"] - 1), dict(cap_edge=0), dict(cap_point=0, cap_edge=0)):
        rc, w = dev.gather(R.BASE_LOCAL, 0, **caps)
        assert rc == mi355slam.MS_ERR_CAPACITY, caps
        assert (w["n_edge"], w["n_current"]) == (want["n_edge"], want["n_current"]), caps      # the needed counts
        nothing_written(w)
        w["edges"].free()
    rc, w = dev.gather(R.BASE_LOCAL, 0, cap_point=want["n_rows"], cap_edge=want["n_edge"])     # regrown to exactly what was asked for
    assert rc == 0
    gathered_equal(w, want)
    gathered_equal(base_window, want)
    w["edges"].free()


def test_degenerate_shapes(ctx, dev):
    sc = dev.sc
    lists = dev.observation_lists(R.BASE_LOCAL)[0]
    rc, w = dev.gather(R.BASE_LOCAL, 2, lists=(lists, 0, 0))                     # no rows: poses only
    assert rc == 0 and (w["n_edge"], w["n_current"]) == (0, 0)
    assert same_bits(w["out"]["pose"][:56], R.gather(sc, R.BASE_LOCAL, 2)["pose"].reshape(-1)) and only_canary_behind(w["out"]["pose"], 56)
    for k in ("point", "obs_point", "obs_pose", "obs_uv", "obs_info"):
        assert only_canary_behind(w["out"][k], 0), k
    w["edges"].free()
    rc, w = dev.gather((3,), 0)                              # one local keyframe
    assert rc == 0
    gathered_equal(w, R.gather(sc, (3,), 0))
    assert w["n_edge"] == w["n_current"] > 0
    w["edges"].free()
    # rows none of whose observations is local: the lists of slot 0's rows, gathered for slot 1 alone
    rng = np.random.default_rng(4)
    small = R.finish(dict(n_kf=3, stride=8, n_mp=6, kf_id=np.array([5, 9, 2], np.int32), mp_flags=np.full(6, 3, np.uint8)), rng, [[0, 1, 2], [3, 4], [0, 2, 3]])
    d = Device(ctx, small)
    try:
        rc, w = d.gather((1,), 0, lists=d.observation_lists((0,)))
        assert rc == 0
        want = R.gather(small, (1,), 0, lists=R.lists_of(small, (0,)))
        assert (want["n_rows"], want["n_obs"], want["n_edge"]) == (3, 5, 0)
        gathered_equal(w, want)
        w["edges"].free()
    finally:
        d.free()


def apply_and_compare(d, w, want_window, pose, point, chi2, mode, before=None, expect_rc=0, **kw):
    """ms_ba_window_apply on the device tables against apply() on `before` (the scene's state when None); the tables are put back."""
    before = R.state_of(d.sc) if before is None else before
    want, erased_want, n_stale_want = R.apply(before, want_window, pose, point, chi2, mode)
    erased_buf = host_canary(w["n_edge"], np.int32)
    try:
        rc, erased, n_stale = d.kf.ba_window_apply(d.table, d.poses, d.flags, d.n_obs, w, pose, point, chi2, mode, cap_erased=w["n_edge"], erased_edge=erased_buf, **kw)
        assert rc == expect_rc, (rc, mi355slam.lib().ms_last_error(d.ctx._h))
        got = d.state()
        for k in TABLES:
            assert same_bits(got[k], want[k]), k
        assert n_stale == n_stale_want and same_bits(erased, erased_want) and only_canary_behind(erased_buf, len(erased_want))
    finally:
        d.restore()
    return want, erased_want


def results(want_window, seed=11):
    rng = np.random.default_rng(seed)
    return want_window["pose"] + rng.normal(0, 1e-3, want_window["pose"].shape), want_window["point"] + rng.normal(0, 1e-2, want_window["point"].shape)


def test_apply_local(dev, base_window):
    sc, want_window = R.cached("base")
    chi2 = R.base_chi2(sc, want_window)
    pose, point = results(want_window)
    pose = np.vstack([pose, pose[:1] + 1.0])                 # the fixed extra vertex of stage 2 is ignored
    after, erased = apply_and_compare(dev, base_window, want_window, pose, point, chi2, R.LOCAL)
    R.apply_conditions(sc, want_window, chi2, after)
    listed = np.zeros(sc["n_mp"], bool)
    listed[want_window["rows"]] = True
    assert same_bits(after["mp_pos"][~listed], sc["mp_pos"][~listed]) and same_bits(after["mp_pos"][listed], point)
    other = [s for s in range(sc["n_kf"]) if s not in R.BASE_LOCAL]
    assert same_bits(after["poses"][other], sc["poses"][other])
    assert len(erased) == sum(len(g) for _, _, g in R.BASE_APPLY.values())
    # the pose written for the quaternion that came from the gather reproduces the table's rotation
    got_pose = base_window["out"]["pose"][:56].reshape(8, 7)
    back, _ = apply_and_compare(dev, base_window, want_window, got_pose, want_window["point"], np.zeros(want_window["n_edge"]), R.LOCAL)
    diff, margin = float(np.abs(back["poses"][list(R.BASE_LOCAL)] - sc["poses"][list(R.BASE_LOCAL)]).max()), R.round_trip_margin()
    print("pose -> quaternion -> pose on the device: %.3e, margin %.3e" % (diff, margin))
    assert diff <= margin


def test_apply_capacity_writes_nothing(dev, base_window):
    sc, want_window = R.cached("base")
    chi2 = R.base_chi2(sc, want_window)
    pose, point = results(want_window)
    n = sum(len(g) for _, _, g in R.BASE_APPLY.values())
    erased_buf = host_canary(n, np.int32)
    try:
        rc, needed, _ = dev.kf.ba_window_apply(dev.table, dev.poses, dev.flags, dev.n_obs, base_window, pose, point, chi2, R.LOCAL, cap_erased=n - 1, erased_edge=erased_buf)
        assert rc == mi355slam.MS_ERR_CAPACITY and needed == n and only_canary_behind(erased_buf, 0)
        got, before = dev.state(), R.state_of(sc)
        for k in TABLES:
            assert same_bits(got[k], before[k]), k
        want, erased_want, _ = R.apply(before, want_window, pose, point, chi2, R.LOCAL)
        rc, erased, _ = dev.kf.ba_window_apply(dev.table, dev.poses, dev.flags, dev.n_obs, base_window, pose, point, chi2, R.LOCAL, cap_erased=n, erased_edge=erased_buf)
        assert rc == 0 and same_bits(erased, erased_want) and only_canary_behind(erased_buf, n)
        got = dev.state()
        for k in TABLES:
            assert same_bits(got[k], want[k]), k
    finally:
        dev.restore()


def test_apply_neighbor(dev, base_window):
    sc, want_window = R.cached("base")
    pose, point = results(want_window, seed=12)
    after, erased = apply_and_compare(dev, base_window, want_window, pose, point, None, R.NEIGHBOR)
    before = R.state_of(sc)
    assert len(erased) == 0 and all(same_bits(after[k], before[k]) for k in ("kf_mp", "n_obs", "mp_flags"))
    cur = R.BASE_LOCAL[0]
    others = [s for s in range(sc["n_kf"]) if s != cur]
    assert same_bits(after["poses"][others], before["poses"][others]) and same_bits(after["poses"][cur], np.array(R.matrix_of_pose(pose[0])))
    assert same_bits(after["mp_pos"][want_window["rows"]], point)


def test_apply_on_the_big_scene(big):
    sc, want_window = R.cached("big")
    rc, w = big.gather(sc["local"], 0)
    assert rc == 0
    chi2 = R.big_chi2(want_window)
    pose, point = results(want_window, seed=13)
    _, erased = apply_and_compare(big, w, want_window, pose, point, chi2, R.LOCAL)
    assert want_window["n_edge"] > R.APPLY_TRIP and (erased < R.APPLY_TRIP).any() and (erased >= R.APPLY_TRIP).any() and (np.diff(erased) > 0).all()
    assert same_bits(erased, np.nonzero(chi2 > R.CHI2_THRESHOLD)[0].astype(np.int32))         # complete
    w["edges"].free()


def test_a_stale_table(dev, base_window):
    sc, want_window = R.cached("base")
    chi2 = np.full(want_window["n_edge"], np.inf)
    pose, point = results(want_window, seed=14)
    e = 17
    s, j = int(want_window["edge_slot"][e]), int(want_window["edge_kp"][e])
    before = R.state_of(sc)
    before["kf_mp"][s, j] = 399
    put(dev.ctx, dev.kf.kf_mp, np.array([399], np.int32), 4 * (s * sc["stride"] + j))       # after the gather, on the device
    after, erased = apply_and_compare(dev, base_window, want_window, pose, point, chi2, R.LOCAL, before=before, expect_rc=mi355slam.MS_ERR_INVALID)
    assert e not in erased and len(erased) == want_window["n_edge"] - 1 and after["kf_mp"][s, j] == 399
    assert "no longer names" in mi355slam.lib().ms_last_error(dev.ctx._h).decode()


def test_end_to_end(ctx, dev, base_window):
    """gather -> the two-stage localBundleAdjust schedule (bundle_adjuster.cpp:322-373) -> apply."""
    sc, want_window = R.cached("base")
    built = R.literal_gather(sc, R.BASE_LOCAL, 0)            # the problem as host code builds it from the same scene
    w = base_window
    n_local, n_edge, n_rows = 8, w["n_edge"], w["n_rows"]
    got = {k: w["out"][k][:{"pose": n_local, "point": n_rows}.get(k, n_edge) * width] for k, _, width in HOST_OUT}
    for k, dt, _ in HOST_OUT:
        assert same_bits(got[k], np.ascontiguousarray(built[k], dt).reshape(-1)), k
    pose = got["pose"].reshape(n_local, 7).copy()
    W = np.diag([100.0 ** 2] * 3 + [50.0 ** 2] * 3) * (0.26667 / 0.1)
    meas = [ba_synth._compose(pose[k], ba_synth._inverse(pose[k - 1])) for k in range(1, n_local)]       # the odometry chain of :296-311: newer keyframe first
    prob = dict(pose=pose, pose_fixed=np.zeros(n_local, np.uint8), point=got["point"].reshape(n_rows, 3).copy(), point_fixed=None, obs_pose=got["obs_pose"].copy(),
                obs_point=got["obs_point"].copy(), obs_uv=got["obs_uv"].reshape(n_edge, 2).copy(), obs_info=got["obs_info"].copy(), huber_delta=float(np.sqrt(R.CHI2_THRESHOLD)),
                edge_i=np.arange(0, n_local - 1, dtype=np.int32), edge_j=np.arange(1, n_local, dtype=np.int32), edge_meas=np.array(meas).reshape(-1, 7),
                edge_info=np.tile(W.reshape(1, 36), (n_local - 1, 1)))
    s1 = dict(prob); s1["pose_fixed"] = np.ones(n_local, np.uint8); s1["pose_fixed"][0] = 0
    s2 = dict(prob); s2["pose"] = np.vstack([pose, pose[:1]]); s2["pose_fixed"] = np.concatenate([np.zeros(n_local, np.uint8), [1]]).astype(np.uint8)
    prior = np.zeros((6, 6)); prior[:3, :3] = np.eye(3) * (100 * 100.0) ** 2
    s2["edge_i"] = np.concatenate([prob["edge_i"], [n_local]]).astype(np.int32); s2["edge_j"] = np.concatenate([prob["edge_j"], [0]]).astype(np.int32)
    s2["edge_meas"] = np.vstack([prob["edge_meas"], [[0, 0, 0, 1, 0, 0, 0]]]); s2["edge_info"] = np.vstack([prob["edge_info"], prior.reshape(1, 36)])
    b1 = mi355slam.BundleAdjuster(ctx, [s1], max_iters=8)
    b2 = mi355slam.BundleAdjuster(ctx, [s2], max_iters=8)
    try:
        b1.solve(); b2.copy_state_from(b1, [0]); b2.solve()
        res = b2.download(0)
    finally:
        b1.close(); b2.close()
    print("two-stage solve: chi2 %.1f -> %.1f, %d of %d edges above the threshold" % (res["stats"]["chi2_init"], res["stats"]["chi2_final"],
                                                                                     int((res["chi2"] > R.CHI2_THRESHOLD).sum()), n_edge))
    assert res["pose"].shape == (n_local + 1, 7) and np.isfinite(res["pose"]).all() and np.isfinite(res["point"]).all()
    apply_and_compare(dev, w, want_window, res["pose"], res["point"], res["chi2"], R.LOCAL)
