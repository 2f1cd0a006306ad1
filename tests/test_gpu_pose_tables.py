"""ms_pose_tables_solve on the device against tests/pose_tables_ref.py, its specification: the gathered problem, the solve
and the applied pose, each bit for bit -- the solve against ms_ba_solve_host on the restated problem (same kernel, same inputs in the same
order, no floating-point atomic on a non-zero value in this shape), and with the bar of tests/test_gpu_ba.py against the CPU oracle.  The
scenes are the smallest at which each mechanism can fail: see pose_tables_ref.SCENES."""
import numpy as np
import pytest

import mi355slam
import pose_tables_ref as R
from test_gpu_ba import _check as check_against_the_oracle

pytestmark = pytest.mark.gpu
TABLES = ("kf_mp", "mp_flags", "mp_live", "mp_pos", "poses")
STATS = ("iters", "trials", "stop", "lam", "chi2_init", "chi2_final")
MIN_GAIN = 1e-2                                              # as tests/test_ba_scenes_ref.py: rounding moves a gain ratio by ~1e-12


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


class Device:
    """A scene with its tables on the device."""

    def __init__(self, ctx, sc):
        self.ctx, self.sc = ctx, sc
        n = sc["n_mp"]
        self.table = mi355slam.MapPointTable(ctx, sc["mp_pos"], np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 8), np.uint32))
        self.kf = mi355slam.KeyframeTable(ctx, sc["kf_mp"])
        self.kp = mi355slam.KeypointTable(ctx, **sc["kp"])
        self.flags, self.live = ctx.upload(sc["mp_flags"]), ctx.upload(sc["mp_live"])
        self.poses = mi355slam.KeyframePoseTable(ctx, sc["poses"])

    def solve(self, adj, frame, live=True, want_chi2=True):
        return adj.solve_device(self.kf, self.flags, self.live if live else None, self.table, self.kp, self.poses, frame, want_chi2)

    def state(self):
        n = self.sc["n_mp"]
        return dict(kf_mp=self.kf.download(), mp_flags=self.flags.download(np.uint8, (n,)), mp_live=self.live.download(np.uint8, (n,)),
                    mp_pos=self.table.pos.download(np.float64, (n, 3)), poses=self.poses.download())

    def free(self):
        for b in (self.table.pos, self.table.norm, self.table.min_dist, self.table.max_dist, self.table.desc, self.kf.kf_mp, self.flags, self.live, self.poses.pose):
            b.free()
        self.kp.free()


def host_solve(ctx, prob, max_iters):
    """ms_ba_create / solve / download of the restated problem: what ms_ba_solve_host runs."""
    ba = mi355slam.BundleAdjuster(ctx, [prob], max_iters=max_iters)
    try:
        ba.solve()
        return ba.download(0)
    finally:
        ba.close()


def gathered_equal(got, g):
    assert got["n"] == g["n"]
    for k in ("pose", "point", "obs_point", "obs_pose", "obs_uv", "obs_info"):
        assert same_bits(got[k], g[k]), k


def check_frame(ctx, oracle, sc, frame, g, rc, res, got_problem, after, label=""):
    """Assertions 1 - 4 on one finished call: the gathered problem, the solve against the host path and the oracle, the tables."""
    assert rc == 0, (label, rc, mi355slam.lib().ms_last_error(ctx._h))
    gathered_equal(got_problem, g)
    assert res["n_triangulated"] == g["n"]
    before = {k: np.asarray(sc[k]) for k in TABLES}
    for k in TABLES[:-1]:
        assert same_bits(after[k], before[k]), (label, k)
    ran = g["n"] >= frame["min_visible"]
    assert res["ran"] == ran, label
    if not ran:
        assert same_bits(after["poses"], before["poses"]) and same_bits(res["pose"], g["pose"][0]), label
        return None
    prob = R.problem(frame, g)
    host = host_solve(ctx, prob, frame["max_iters"])
    assert same_bits(res["pose"], host["pose"][0]), (label, res["pose"], host["pose"][0])
    assert same_bits(res["chi2"], host["chi2"]), label
    for k in STATS:
        assert res["stats"][k] == host["stats"][k], (label, k, res["stats"][k], host["stats"][k])
    got = dict(pose=np.vstack([res["pose"], g["pose"][1]]), point=g["point"], chi2=res["chi2"], stats=res["stats"])
    # The trajectory counters (iterations, trials, lambda) are compared while every accept / reject decision of the oracle's own solve stood away
    # from rounding: its smallest gain ratio above MIN_GAIN, the line tests/test_ba_scenes_ref.py draws.  A frame that converges inside its
    # three iterations ends in trials whose gain is 0 / 0, where one ulp decides; its state and chi2 are still held to the oracle's.
    want = oracle.ba_solve(prob, frame["max_iters"], False)
    res["strict"] = want["stats"]["min_abs_gain"] > MIN_GAIN
    check_against_the_oracle(prob, got, want, strict_trajectory=res["strict"])
    want_poses, _ = R.apply(before["poses"], frame, g, res["pose"])
    assert same_bits(after["poses"], want_poses), label
    return host


def run_scene(ctx, oracle, adj, name, frame_changes=None, live=True):
    sc, frame, g = R.cached(name)
    frame = dict(frame, **(frame_changes or {}))
    d = Device(ctx, sc)
    try:
        rc, res = d.solve(adj, frame, live=live)
        return sc, frame, g, res, check_frame(ctx, oracle, sc, frame, g, rc, res, adj.problem(), d.state(), name)
    finally:
        d.free()


@pytest.fixture(scope="module")
def adj(ctx):
    a = mi355slam.PoseAdjuster(ctx, 640, R.W.sigma_levels())
    yield a
    a.close()


@pytest.mark.parametrize("name", ["base", "kp255", "kp256", "kp257", "second_trip_only", "tri192", "tri193"])
def test_scene(ctx, oracle, adj, name):
    sc, frame, g, res, host = run_scene(ctx, oracle, adj, name)
    R.scene_conditions(name, sc, frame, g)
    assert res["ran"] and res["stats"]["chi2_final"] < res["stats"]["chi2_init"] and not same_bits(res["pose"], g["pose"][0])
    assert res["strict"]                                     # these scenes' trajectories are compared step for step
    print("%s: %d of %d keypoints kept, chi2 %.2f -> %.2f" % (name, g["n"], frame["n_kp"], res["stats"]["chi2_init"], res["stats"]["chi2_final"]))


def test_ten_iterations(ctx, oracle, adj):
    sc, frame, g, res, host = run_scene(ctx, oracle, adj, "base", dict(max_iters=10))
    assert res["ran"] and res["stats"]["iters"] > 3


@pytest.mark.parametrize("name", ["kp0", "kp1", "tri0"])
def test_few_points(ctx, oracle, adj, name):
    """Below the threshold nothing is written; with the threshold at the count the problem (the odometry edge and 0 or 1 points) is solved."""
    sc, frame, g, res, _ = run_scene(ctx, oracle, adj, name)
    assert not res["ran"] and g["n"] < frame["min_visible"]
    sc, frame, g, res, host = run_scene(ctx, oracle, adj, name, dict(min_visible=g["n"]))
    assert res["ran"] and host is not None and len(res["chi2"]) == g["n"]


def test_overflow_beyond_the_registers(ctx, oracle):
    """1537 kept keypoints: one more than k_ba_pose_only keeps in registers (PO_OT * PO_K = 1536)."""
    a = mi355slam.PoseAdjuster(ctx, 1600, R.W.sigma_levels())
    try:
        sc, frame, g, res, _ = run_scene(ctx, oracle, a, "overflow")
        R.scene_conditions("overflow", sc, frame, g)
        assert res["ran"] and g["n"] == 1537 and len(res["chi2"]) == 1537
    finally:
        a.close()


def test_without_a_live_array_every_row_is_live(ctx, oracle, adj):
    sc, frame, g = R.cached("base")
    all_live = dict(sc, mp_live=np.ones_like(sc["mp_live"]))
    want = R.gather(all_live, frame)
    assert want["n"] > g["n"]
    d = Device(ctx, sc)
    try:
        rc, res = d.solve(adj, frame, live=False)
        check_frame(ctx, oracle, all_live, frame, want, rc, res, adj.problem(), dict(d.state(), mp_live=all_live["mp_live"]), "no mp_live")
    finally:
        d.free()


def test_threshold_both_sides(ctx, oracle, adj):
    sc, frame, g = R.cached("base")
    d = Device(ctx, sc)
    try:
        rc, res = d.solve(adj, dict(frame, min_visible=g["n"] + 1))
        assert rc == 0 and not res["ran"] and res["n_triangulated"] == g["n"]
        assert same_bits(d.state()["poses"], sc["poses"])
        rc, res = d.solve(adj, dict(frame, min_visible=g["n"]))
        assert rc == 0 and res["ran"]
        after = d.state()["poses"]
        assert not same_bits(after[R.FRAME], sc["poses"][R.FRAME]) and same_bits(after[R.FRAME], np.array(R.matrix_of_pose(res["pose"])))
    finally:
        d.free()


def test_no_previous_keyframe(ctx, adj):
    sc, frame, g = R.cached("base")
    d = Device(ctx, sc)
    try:
        rc, res = d.solve(adj, dict(frame, prev_slot=-1))
        assert rc == 0 and not res["ran"] and res["n_triangulated"] == 0 and adj.problem()["n"] == 0
        assert same_bits(d.state()["poses"], sc["poses"])
    finally:
        d.free()


def changed(sc, **arrays):
    out = dict(sc)
    out.update(arrays)
    return out


def test_octave_outside_the_levels(ctx, oracle, adj):
    sc, frame, g = R.cached("base")
    dropped = np.setdiff1d(np.arange(frame["n_kp"]), g["kept"])
    for j, want_rc in ((int(g["kept"][70]), mi355slam.MS_ERR_INVALID), (int(dropped[70]), 0)):
        for octave in (R.N_LEVELS, -1):
            kp = {k: v.copy() for k, v in sc["kp"].items()}
            kp["octave"][R.FRAME, j] = octave
            bad = changed(sc, kp=kp)
            d = Device(ctx, bad)
            try:
                rc, res = d.solve(adj, frame)
                assert rc == want_rc, (j, octave, rc)
                if want_rc:
                    assert "octave" in mi355slam.lib().ms_last_error(ctx._h).decode() and not res["ran"] and res["n_triangulated"] == g["n"]
                    assert same_bits(d.state()["poses"], sc["poses"])
                else:
                    check_frame(ctx, oracle, bad, frame, g, rc, res, adj.problem(), d.state(), "octave of a dropped keypoint")
            finally:
                d.free()


def test_capacity(ctx, oracle):
    sc, frame, g = R.cached("base")
    d = Device(ctx, sc)
    small = mi355slam.PoseAdjuster(ctx, g["n"] - 1, R.W.sigma_levels())
    exact = mi355slam.PoseAdjuster(ctx, g["n"], R.W.sigma_levels())
    try:
        rc, res = d.solve(small, frame)
        assert rc == mi355slam.MS_ERR_CAPACITY and res["n_triangulated"] == g["n"] and not res["ran"]
        state = d.state()
        for k in TABLES:
            assert same_bits(state[k], sc[k]), k
        rc, res = d.solve(exact, frame)
        check_frame(ctx, oracle, sc, frame, g, rc, res, exact.problem(), d.state(), "exact capacity")
    finally:
        small.close(); exact.close(); d.free()


def test_a_nan_position(ctx, adj):
    sc, frame, g = R.cached("base")
    pos = sc["mp_pos"].copy()
    pos[sc["kf_mp"][R.FRAME, g["kept"][5]], 1] = np.nan
    d = Device(ctx, changed(sc, mp_pos=pos))
    try:
        rc, res = d.solve(adj, frame)
        assert rc == mi355slam.MS_ERR_NUMERIC and not res["ran"] and res["n_triangulated"] == g["n"]
        assert same_bits(d.state()["poses"], sc["poses"])
    finally:
        d.free()


def test_reuse_of_one_handle(ctx, oracle):
    """24 consecutive frames on one handle, the counts growing, shrinking and zero in between: every frame as in test_scene (a stale input
    of a larger earlier frame would show in the solve), and no allocation after the third."""
    counts = [12, 60, 140, 256, 193, 192, 0, 30, 0, 11, 250, 10, 9, 100, 1, 0, 256, 64, 13, 200, 0, 129, 128, 40]
    frames = []
    for i, n in enumerate(counts):
        n_kp = 300 + 13 * i
        sc, frame = R.make_scene(R.mixed(n_kp, n, 40 + i, kept_at=(255, 256)[:min(n, 2)]), seed=300 + i)
        frames.append((Device(ctx, sc), sc, frame, R.gather(sc, frame)))
    a = mi355slam.PoseAdjuster(ctx, 256, R.W.sigma_levels())
    lib = mi355slam.lib()
    lib.ms_debug_host_allocs.restype = mi355slam.C.c_longlong
    try:
        done, allocs = [], []
        for d, sc, frame, g in frames:
            rc, res = d.solve(a, frame)
            done.append((rc, res, a.problem()))
            allocs.append(lib.ms_debug_host_allocs())
        assert len(set(allocs[2:])) == 1, allocs
        for i, ((d, sc, frame, g), (rc, res, prob)) in enumerate(zip(frames, done)):
            assert g["n"] == counts[i]
            check_frame(ctx, oracle, sc, frame, g, rc, res, prob, d.state(), "frame %d" % i)
        strict = [i for i, (_, res, _) in enumerate(done) if res.get("strict")]
        print("frames whose LM trajectory was compared step for step with the oracle:", strict)
        assert len(strict) >= 6
    finally:
        a.close()
        for d, _, _, _ in frames:
            d.free()
