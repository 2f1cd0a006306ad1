"""ms_frame_finish on the device against tests/frame_finish_ref.py, its specification: every table and every output of every
scene bit for bit, canaries behind every buffer, the same bytes on a second run; the capacity return; the no-ops; and cross-checks against
the entry points that were there before -- ms_observation_count, ms_map_cull, ms_pose_tables_solve's gather, and the per-frame chain
ms_match_tracked -> ms_pose_tables_solve -> ms_frame_finish on one reused slot.  The scenes are the smallest at which each mechanism can
fail: see frame_finish_ref.SCENES."""
import ctypes as C

import numpy as np
import pytest

import mi355slam
import frame_finish_ref as R
import pose_tables_ref as PT

pytestmark = pytest.mark.gpu
CAN8, CAN32, PAD = 0x5A, 0x5A5A5A5A, 16
CLOUD = ("cloud_row", "cloud_kp", "cloud_track", "cloud_pos")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def padded(a, dtype):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    return np.concatenate([a, np.full(PAD, CAN8 if dtype == np.uint8 else CAN32, dtype)])


class Device:
    """The tables of a scene on the device, each with a canary behind it."""

    def __init__(self, ctx, t):
        self.ctx, self.t = ctx, t
        self.n_mp, (self.n_kf, self.stride) = len(t["mp_flags"]), t["kf_mp"].shape
        n = self.n_mp
        self.kf = mi355slam.KeyframeTable(ctx, np.vstack([t["kf_mp"], np.full((1, self.stride), CAN32, np.int32)]))
        self.kf.n_kf = self.n_kf                             # the last row is the canary
        self.flags = ctx.upload(padded(t["mp_flags"], np.uint8))
        self.live = None if t["mp_live"] is None else ctx.upload(padded(t["mp_live"], np.uint8))
        self.n_obs = None if t["n_obs"] is None else ctx.upload(padded(t["n_obs"], np.int32))
        self.tracks = None if t["mp_track"] is None else ctx.upload(padded(t["mp_track"], np.int32))
        self.table = mi355slam.MapPointTable(ctx, t["mp_pos"], np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 8), np.uint32))

    def call(self, remove, cloud_slot, n_kp, cap=None, kf_id=None, n_obs=True):
        """The C call with a canary behind every host output.  Returns (rc, outputs cut to their counts)."""
        remove = np.asarray(remove, np.int32)
        cap = min(self.n_mp, len(remove) * self.stride) if cap is None else cap
        kf_id = np.asarray(self.t["kf_id"] if kf_id is None else kf_id, np.int32)
        host = dict(cloud_row=np.full(n_kp + PAD, CAN32, np.int32), cloud_kp=np.full(n_kp + PAD, CAN32, np.int32), cloud_track=np.full(n_kp + PAD, CAN32, np.int32),
                    cloud_pos=np.full(3 * (n_kp + PAD), np.nan), removed_rows=np.full(cap + PAD, CAN32, np.int32), counts=np.full(3 + PAD, CAN32, np.int32))
        A = mi355slam.FrameFinishArgsC(int(cloud_slot), int(n_kp))
        vp = mi355slam._vp
        rc = mi355slam.lib().ms_frame_finish(self.ctx._h, vp(self.kf.kf_mp), self.n_kf, self.stride, vp(self.flags), vp(self.live), vp(self.table.pos), vp(self.tracks),
                                             vp(self.n_obs if n_obs else None), self.n_mp, vp(kf_id), vp(remove), len(remove), C.byref(A),
                                             *[vp(host[k]) for k in CLOUD], vp(host["removed_rows"]), cap, vp(host["counts"]))
        counts = host["counts"][:3].copy()
        assert (host["counts"][3:] == CAN32).all()
        if rc == mi355slam.MS_ERR_INVALID:                   # nothing is written
            assert all((host[k] == CAN32).all() for k in CLOUD[:3] + ("removed_rows", "counts")) and np.isnan(host["cloud_pos"]).all()
            return rc, dict(counts=counts, rc=rc)
        n_cloud, n_removed = int(counts[0]), int(counts[1]) if rc == 0 else 0
        assert 0 <= n_cloud <= n_kp and 0 <= n_removed <= cap
        for k in CLOUD[:3]:
            assert (host[k][n_cloud:] == CAN32).all(), k     # nothing behind the count is written
        assert np.isnan(host["cloud_pos"][3 * n_cloud:]).all() and (host["removed_rows"][n_removed:] == CAN32).all()
        out = {k: host[k][:n_cloud].copy() for k in CLOUD[:3]}
        out.update(cloud_pos=host["cloud_pos"][:3 * n_cloud].reshape(-1, 3).copy(), removed_rows=host["removed_rows"][:n_removed].copy(), counts=counts, rc=rc)
        return rc, out

    def state(self):
        """The tables a call may write, their canaries checked."""
        n = self.n_mp
        kf = self.kf.kf_mp.download(np.int32, (self.n_kf + 1, self.stride))
        assert (kf[-1] == CAN32).all()
        out = dict(kf_mp=kf[:-1])
        for name, buf, dtype in (("mp_flags", self.flags, np.uint8), ("mp_live", self.live, np.uint8), ("n_obs", self.n_obs, np.int32), ("mp_track", self.tracks, np.int32)):
            if buf is None:
                out[name] = None
                continue
            a = buf.download(dtype, (n + PAD,))
            assert (a[n:] == (CAN8 if dtype == np.uint8 else CAN32)).all(), name
            out[name] = a[:n]
        out["mp_pos"] = self.table.pos.download(np.float64, (n, 3)) if n else np.zeros((0, 3))
        return out

    def free(self):
        for b in (self.kf.kf_mp, self.flags, self.live, self.n_obs, self.tracks, self.table.pos, self.table.norm, self.table.min_dist, self.table.max_dist, self.table.desc):
            if b is not None:
                b.free()


def check(got, state, want, t, label=""):
    """Every output and every table against the restatement."""
    assert got["rc"] == want["rc"], (label, got["rc"], want["rc"])
    assert got["counts"].tolist() == want["counts"].tolist(), (label, got["counts"], want["counts"])
    for k in CLOUD + ("removed_rows",):
        assert same_bits(got[k], want[k]), (label, k)
    for k in R.TABLES:
        assert (state[k] is None and want[k] is None) or same_bits(state[k], want[k]), (label, k)
    assert same_bits(state["mp_pos"], t["mp_pos"]) and (t["mp_track"] is None or same_bits(state["mp_track"], t["mp_track"])), label


def run(ctx, t, remove, cloud_slot, n_kp, **kw):
    d = Device(ctx, t)
    try:
        rc, got = d.call(remove, cloud_slot, n_kp, **kw)
        return got, d.state()
    finally:
        d.free()


@pytest.mark.parametrize("name", list(R.SCENES))
def test_scene(ctx, name):
    sc, want = R.cached(name)
    R.scene_conditions(name, sc, want)
    runs = [run(ctx, sc["t"], sc["remove"], sc["cloud_slot"], sc["n_kp"]) for _ in range(2)]
    for got, state in runs:
        check(got, state, want, sc["t"], name)
    for k in runs[0][0]:                                     # the same call on restored tables: the same bytes (implied by the above; stated for itself)
        assert same_bits(runs[0][0][k], runs[1][0][k]), k
    print("%s: cloud %d, removed rows %d, erased entries %d" % ((name,) + tuple(want["counts"])))


def test_without_n_obs_nothing_else_changes(ctx):
    sc, want = R.cached("per_frame")
    got, state = run(ctx, sc["t"], sc["remove"], sc["cloud_slot"], sc["n_kp"], n_obs=False)
    check(got, state, dict(want, n_obs=sc["t"]["n_obs"]), sc["t"])


def test_cap_removed_one_short_then_enough(ctx):
    sc, want = R.cached("per_frame")
    t, n = sc["t"], len(want["removed_rows"])
    short = R.finish(t, sc["remove"], sc["cloud_slot"], sc["n_kp"], cap_removed=n - 1)
    d = Device(ctx, t)
    try:
        rc, got = d.call(sc["remove"], sc["cloud_slot"], sc["n_kp"], cap=n - 1)
        assert rc == mi355slam.MS_ERR_CAPACITY and "removed_rows holds %d" % (n - 1) in mi355slam.lib().ms_last_error(ctx._h).decode()
        check(got, d.state(), short, t, "one short")         # every table keeps its bits, the counts are the needed ones, the cloud is valid
        assert same_bits(d.state()["kf_mp"], t["kf_mp"]) and got["counts"][1] == n
        rc, got = d.call(sc["remove"], sc["cloud_slot"], sc["n_kp"], cap=n)
        check(got, d.state(), want, t, "exact capacity")
    finally:
        d.free()


def test_noops(ctx):
    sc, _ = R.cached("per_frame")
    t = sc["t"]
    for remove, slot, n_kp in (([], -1, 0), ([], -1, 60), ([], 3, 0), ([3], 3, 0), ([3], -1, 0)):
        got, state = run(ctx, t, remove, slot, n_kp)
        check(got, state, R.finish(t, remove, slot, n_kp), t, (remove, slot, n_kp))
    d = Device(ctx, dict(t, mp_live=None))                   # nothing is removed: no live bytes needed
    try:
        rc, got = d.call([], 3, 60)
        check(got, d.state(), R.finish(dict(t, mp_live=None), [], 3, 60), t)
    finally:
        d.free()
    empty = dict(t, mp_flags=np.zeros(0, np.uint8), mp_live=np.zeros(0, np.uint8), mp_pos=np.zeros((0, 3)), mp_track=np.zeros(0, np.int32), n_obs=np.zeros(0, np.int32))
    got, state = run(ctx, empty, [3], 3, 60)                 # n_mp = 0: no entry is valid, the slot is cleared all the same
    check(got, state, R.finish(empty, [3], 3, 60), empty, "n_mp = 0")
    assert got["counts"].tolist() == [0, 0, 0] and (state["kf_mp"][3] == -1).all()


def test_host_validation_runs_before_the_device(ctx):
    sc, _ = R.cached("per_frame")
    d = Device(ctx, sc["t"])
    try:
        for remove, slot, n_kp in (([1], 3, 60), ([3, 3], 3, 60), ([3], 1, 60), ([3], 3, 71), ([4], 3, 60)):
            rc, got = d.call(remove, slot, n_kp)
            assert rc == mi355slam.MS_ERR_INVALID and (got["counts"] == CAN32).all(), (remove, slot, n_kp)      # nothing written, counts included
        state = d.state()
        for k in R.TABLES:
            assert same_bits(state[k], sc["t"][k]), k
    finally:
        d.free()


def test_the_binding_returns_the_same(ctx):
    sc, want = R.cached("two_removed")
    t = sc["t"]
    d = Device(ctx, t)
    try:
        with pytest.raises(mi355slam.MsError, match="removed_rows holds 1"):
            d.kf.frame_finish(d.flags, d.live, d.table, d.tracks, d.n_obs, t["kf_id"], sc["remove"], sc["cloud_slot"], sc["n_kp"], cap_removed=1)
        got = d.kf.frame_finish(d.flags, d.live, d.table, d.tracks, d.n_obs, t["kf_id"], sc["remove"], sc["cloud_slot"], sc["n_kp"])
        check(dict(got, rc=0), d.state(), want, t)
    finally:
        d.free()


def test_nothing_is_allocated_after_warm_up(ctx):
    sc, want = R.cached("per_frame")
    lib = mi355slam.lib()
    lib.ms_debug_host_allocs.restype = C.c_longlong
    devs = [Device(ctx, sc["t"]) for _ in range(4)]
    try:
        allocs = []
        for d in devs:
            rc, got = d.call(sc["remove"], sc["cloud_slot"], sc["n_kp"])
            allocs.append(lib.ms_debug_host_allocs())
            check(got, d.state(), want, sc["t"])
        assert len(set(allocs[1:])) == 1, allocs
    finally:
        for d in devs:
            d.free()


# ---- cross-checks against the entry points that were there before
@pytest.mark.parametrize("name", ["per_frame", "two_removed"])
def test_a_fresh_observation_count_equals_the_written_n_obs(ctx, name):
    sc, want = R.cached(name)
    t = sc["t"]
    d = Device(ctx, t)
    try:
        rc, got = d.call(sc["remove"], sc["cloud_slot"], sc["n_kp"])
        state = d.state()
        kf_id = t["kf_id"].copy()
        kf_id[sc["remove"]] = -1                             # the caller's part
        count, _, _ = d.kf.observation_count(kf_id, d.n_mp, True, False, False)
    finally:
        d.free()
    e = t["kf_mp"][sc["remove"]].reshape(-1)
    touched = np.unique(e[R.valid(t, e)])
    assert len(touched) > 10 and same_bits(count[touched], state["n_obs"][touched])
    rest = np.setdiff1d(np.arange(d.n_mp), touched)
    assert same_bits(state["n_obs"][rest], t["n_obs"][rest])


@pytest.mark.parametrize("name", ["per_frame", "two_removed"])
def test_map_cull_with_the_slot_as_its_single_candidate_leaves_the_same_tables(ctx, name):
    sc, _ = R.cached(name)
    t, slot = sc["t"], sc["remove"][0]
    got, state = run(ctx, t, [slot], -1, 0)
    current = [s for s in range(len(t["kf_id"])) if t["kf_id"][s] >= 0 and s != slot][0]
    kt = mi355slam.KeyframeTable(ctx, t["kf_mp"])
    try:
        settings = dict(current_slot=current, cull_points=0, min_age=0.0, min_obs_for_ba=0, max_critical_ratio=1e300, ratio_float32=0)
        res = kt.cull(t["mp_flags"], t["mp_live"], len(t["mp_flags"]), t["kf_id"], np.arange(len(t["kf_id"]), dtype=np.float64), [slot], None, settings)
        kf_after = kt.download()
    finally:
        kt.kf_mp.free()
    assert res["cand_removed"].tolist() == [1]
    # ms_map_cull also sweeps the STALE entries of empty slots that name a removed row (k_cull_sweep walks the whole table); ms_frame_finish writes the removed
    # slots alone and leaves an empty slot as it is.  So: the same bits in every slot with kf_id >= 0, and in an empty slot exactly that sweep on top.
    used = t["kf_id"] >= 0
    swept = np.where(np.isin(state["kf_mp"], got["removed_rows"]) & ~used[:, None], -1, state["kf_mp"]).astype(np.int32)
    assert same_bits(kf_after[used], state["kf_mp"][used]) and same_bits(kf_after, swept)
    assert same_bits(res["mp_live"], state["mp_live"]) and same_bits(res["mp_flags"], state["mp_flags"])
    assert sorted(res["removed_rows"].tolist()) == sorted(got["removed_rows"].tolist()) and len(got["removed_rows"]) > 2
    touched = np.unique(t["kf_mp"][slot][R.valid(t, t["kf_mp"][slot])])
    assert same_bits(res["n_obs"][touched], state["n_obs"][touched])


@pytest.mark.parametrize("name", ["per_frame", "two_removed"])
def test_the_cloud_is_what_the_pose_adjustment_gathered(ctx, name):
    sc, want = R.cached(name)
    t, slot = sc["t"], sc["cloud_slot"]
    n_kf, stride = t["kf_mp"].shape
    prev = [s for s in range(n_kf) if t["kf_id"][s] >= 0 and s != slot][0]
    zeros = np.zeros((n_kf, stride), np.float32)
    d = Device(ctx, t)
    kp = mi355slam.KeypointTable(ctx, zeros, zeros, np.zeros((n_kf, stride), np.int32), zeros)
    poses = mi355slam.KeyframePoseTable(ctx, np.tile(np.eye(3, 4).reshape(12), (n_kf, 1)))
    adj = mi355slam.PoseAdjuster(ctx, stride, PT.W.sigma_levels())
    try:
        frame = dict(slot=slot, prev_slot=prev, n_kp=sc["n_kp"], cam=(500.0, 500.0, 320.0, 240.0, 640, 480), focal=500, edge_meas=[0, 0, 0, 1, 0, 0, 0], edge_info=np.eye(6),
                     min_visible=10 ** 6, max_iters=0, huber_delta=1.0)      # the threshold keeps the solver from running: the gather is what is compared
        rc, res = adj.solve_device(d.kf, d.flags, d.live, d.table, kp, poses, frame, False)
        assert rc == 0 and not res["ran"], (rc, mi355slam.lib().ms_last_error(ctx._h))
        prob = adj.problem()
        rc, got = d.call(sc["remove"], slot, sc["n_kp"])
    finally:
        adj.close(); kp.free(); poses.pose.free(); d.free()
    assert prob["n"] == res["n_triangulated"] == got["counts"][0] > 3 and same_bits(prob["point"], got["cloud_pos"])


# ---- the per-frame chain on one reused slot
def test_three_frames_through_match_tracked_pose_adjust_and_finish(ctx):
    """Three consecutive frames that do not become keyframes, in the slot of a pose_tables_ref scene: ms_match_tracked binds the tracked keypoints and creates
    rows for the new tracks, ms_pose_tables_solve adjusts the pose, ms_frame_finish returns the cloud and takes the frame out again.  ms_match_tracked
    turns a frame away whose slot still holds a valid entry, so each later frame also needs the slot the way the finish left it."""
    sc, frame0, g = PT.cached("base")
    FRAME, n_kp, stride, n_old = PT.FRAME, frame0["n_kp"], sc["stride"], sc["n_mp"]
    n_free, base = 700, 5000
    n_mp = n_old + n_free                                    # free rows behind the scene's, for the points the frames create
    bound = np.asarray(sc["kf_mp"][FRAME], np.int64)         # what the scene binds the frame's keypoints to: their tracks
    kf_mp = sc["kf_mp"].copy()
    kf_mp[FRAME] = -1                                        # the frame has not been matched yet
    flags = np.r_[sc["mp_flags"], np.zeros(n_free, np.uint8)]
    live = np.r_[sc["mp_live"], np.zeros(n_free, np.uint8)]
    pos = np.vstack([sc["mp_pos"], np.zeros((n_free, 3))])
    true = sc["true"]
    Rf, cf = true["R"][FRAME], true["c"][FRAME]
    to_cam = cf - pos
    norm = (to_cam / np.linalg.norm(to_cam, axis=1, keepdims=True)).astype(np.float32)
    rng = np.random.default_rng(5)
    table = mi355slam.MapPointTable(ctx, pos, norm, np.zeros(n_mp, np.float32), np.full(n_mp, 1e6, np.float32), rng.integers(0, 2 ** 32, (n_mp, 8), dtype=np.uint32))
    kt = mi355slam.KeyframeTable(ctx, kf_mp)
    kp = mi355slam.KeypointTable(ctx, **sc["kp"])
    poses = mi355slam.KeyframePoseTable(ctx, sc["poses"])
    d_flags, d_live, d_nobs = ctx.upload(flags), ctx.upload(live), ctx.upload(np.full(n_mp, -5, np.int32))
    pool = ctx.upload(rng.integers(0, 2 ** 32, (stride, 8), dtype=np.uint32))
    n_track = n_mp + 3 * stride
    tracks = mi355slam.TrackTable(ctx, np.r_[base + np.arange(n_old), np.full(n_free, -1)], np.r_[np.arange(n_old), np.full(n_track - n_old, -1)], base)
    adj = mi355slam.PoseAdjuster(ctx, stride, PT.W.sigma_levels())
    out = dict(outcome=ctx.alloc(n_kp), created_rows=ctx.alloc(4 * n_free), created_kp=ctx.alloc(4 * n_free), tracked_rows=ctx.alloc(4 * n_kp), checked_rows=ctx.alloc(4 * n_kp))
    new_rows = np.arange(n_old, n_mp, dtype=np.int32)        # the same free rows for every frame: the finish gives them back
    true_pose = np.concatenate([Rf, (-Rf @ cf)[:, None]], 1).reshape(12)
    ok = (bound[:n_kp] >= 0) & (bound[:n_kp] < n_old)
    try:
        for f in range(3):
            kf_id = sc["kf_id"].copy()
            kf_id[FRAME] = 9 + f                             # a new frame in the same slot
            before, _, _ = kt.observation_count(kf_id, n_mp, True, False, False)
            live_before = d_live.download(np.uint8, (n_mp,))
            # tracked keypoints carry the track of the row the scene binds them to; the others a track nobody has seen yet
            kp_track = np.where(ok, base + bound[:n_kp], base + n_mp + f * stride + np.arange(n_kp)).astype(np.int32)
            mt = dict(slot=FRAME, pose=true_pose, cam=sc["cams"][FRAME], focal=int(sc["focal"][FRAME]), desc_base=0, level_sigma_sq=PT.W.sigma_levels(),
                      rel_reprojection_threshold=0.05, view_cos_limit=0.5)
            rc, counts = kt.match_tracked_device(table, d_flags, d_live, tracks, kp, pool, mt, kp_track, new_rows, out)
            assert rc == 0, (f, rc, mi355slam.lib().ms_last_error(ctx._h))
            n_created, n_tracked, n_checked = (int(v) for v in counts[:3])
            created = out["created_rows"].download(np.int32, (n_created,))
            # 150 keypoints are bound to live TRIANGULATED rows and lie where the true pose projects them (0.3 px of noise, 1 cm on the positions): a third may fail a check
            assert n_created >= (~ok).sum() and n_checked >= 100 and n_created + n_tracked + n_checked > n_kp // 2, (f, counts)
            rc, res = adj.solve_device(kt, d_flags, d_live, table, kp, poses, dict(frame0, n_kp=n_kp), False)
            assert rc == 0 and res["ran"] and res["n_triangulated"] >= n_checked, (f, rc, res)
            prob = adj.problem()
            got = kt.frame_finish(d_flags, d_live, table, tracks.mp_track, d_nobs, kf_id, [FRAME], FRAME, n_kp)
            assert got["counts"][0] == res["n_triangulated"] and same_bits(got["cloud_pos"], prob["point"]), f
            assert same_bits(got["cloud_track"], (base + got["cloud_row"]).astype(np.int32))
            assert got["counts"][2] == n_created + n_tracked + n_checked
            assert (kt.download_slot(FRAME) == -1).all(), f
            assert set(created.tolist()) <= set(got["removed_rows"].tolist())                # a point only this frame saw goes with it
            live_after = d_live.download(np.uint8, (n_mp,))
            assert not live_after[n_old:].any() and not (live_after & ~live_before).any()
            after, _, _ = kt.observation_count(kf_id, n_mp, True, False, False)
            stayed = live_after != 0
            assert stayed.sum() > 100 and same_bits(after[stayed], before[stayed]), f
            n_obs = d_nobs.download(np.int32, (n_mp,))
            listed = np.unique(np.r_[got["removed_rows"], got["cloud_row"]])
            assert same_bits(n_obs[listed], after[listed])
            print("frame %d: created %d, tracked %d, checked %d; cloud %d, removed rows %d" % (f, n_created, n_tracked, n_checked, got["counts"][0], got["counts"][1]))
    finally:
        adj.close(); kp.free(); tracks.free()
        for b in list(out.values()) + [table.pos, table.norm, table.min_dist, table.max_dist, table.desc, kt.kf_mp, poses.pose, d_flags, d_live, d_nobs, pool]:
            b.free()
