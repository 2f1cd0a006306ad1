"""ms_map_extract on the device against tests/map_extract_ref.py, its specification: every destination array and output of
every scene bit for bit on a destination pre-filled with a pattern, canaries behind every destination buffer, every SOURCE array compared
before and after, the same bytes on a second run; the capacity return; no active slots; the full copy; and cross-checks against the entry
points that were there before, run on the DESTINATION tables -- ms_observation_count, ms_covisibility, and the per-frame chain
ms_match_tracked -> ms_pose_tables_solve -> ms_frame_finish, which gives on the extraction what it gives on the whole map.  The scenes are
the smallest at which each part can fail: see map_extract_ref.SCENES."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mi355slam
import covis_ref
import map_extract_ref as R
import pose_tables_ref as PT

pytestmark = pytest.mark.gpu
FILL, CANARY, PAD = 0x5A, 0xA5, 64
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slam-module_amd", "csrc")
SRC_NAMES = mi355slam.MAP_EXTRACT_SRC


def with_canary(a):
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.full(PAD, CANARY, np.uint8)])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Device:
    """The source tables of a scene and a destination filled with a pattern, each buffer with a canary behind it."""

    def __init__(self, ctx, t, z, outputs=True):
        self.ctx, self.t, self.z = ctx, t, z
        self.src_bytes = {k: with_canary(t[k]) for k in SRC_NAMES if t.get(k) is not None}
        self.src = {k: ctx.upload(v) for k, v in self.src_bytes.items()}
        self.kf = table_on(ctx, self.src["kf_mp"], z["n_kf"], z["stride"])
        self.before = R.fresh_dst(t, z, FILL, outputs)
        self.dst = {k: ctx.upload(with_canary(v)) for k, v in self.before.items()}

    def call(self, active, kf_id=None):
        t = self.t
        n_kp = None if t["desc_pool"] is None else np.take(np.asarray(t["n_kp"], np.int32), np.asarray(active, np.int64), mode="clip")
        src = {k: v for k, v in self.src.items() if k != "kf_mp"}
        return self.kf.map_extract_device(src, self.dst, self.z, t["kf_id"] if kf_id is None else kf_id, active, None if t["desc_pool"] is None else t["desc_base"], n_kp)

    def state(self):
        """The destination arrays, their canaries checked."""
        out = {}
        for k, v in self.before.items():
            raw = self.dst[k].download(np.uint8, (v.nbytes + PAD,))
            assert (raw[v.nbytes:] == CANARY).all(), k
            out[k] = raw[:v.nbytes].view(v.dtype).reshape(v.shape)
        return out

    def source_untouched(self):
        return all(same_bits(self.src[k].download(np.uint8, v.shape), v) for k, v in self.src_bytes.items())

    def free(self):
        for b in list(self.src.values()) + list(self.dst.values()):
            b.free()


def table_on(ctx, buf, n_kf, stride):
    """A KeyframeTable over a kf_mp that is on the device already."""
    kt = mi355slam.KeyframeTable.__new__(mi355slam.KeyframeTable)
    kt.ctx, kt.kf_mp, kt.n_kf, kt.stride = ctx, buf, n_kf, stride
    return kt


def check(rc, out, state, want, label=""):
    assert rc == want["rc"], (label, rc, want["rc"])
    assert out["counts"].tolist() == want["counts"].tolist(), (label, out["counts"], want["counts"])
    assert same_bits(out["dst_desc_base"], want["dst_desc_base"]), label
    for k in state:
        assert same_bits(state[k], want[k]), (label, k)


def run(ctx, t, z, active, outputs=True, **kw):
    d = Device(ctx, t, z, outputs)
    try:
        rc, out = d.call(active, **kw)
        state = d.state()
        assert d.source_untouched()
        return rc, out, state, R.extract(t, active, z, d.before)
    finally:
        d.free()


@pytest.mark.parametrize("name", list(R.SCENES))
def test_scene(ctx, name):
    sc, z, want0 = R.cached(name)
    R.scene_conditions(name, sc, z, want0)
    if name == "second_trip":                                # the trip of block_offsets is the workgroup size the unit passes it
        k_block = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(CSRC, "map_extract.hip")).read()).group(1))
        scan = open(os.path.join(CSRC, "ms_scan.h")).read()
        assert "i0 += BLOCK" in scan.split("block_offsets(")[1] and k_block == sc["k_block"] and z["n_mp"] > k_block * k_block
    runs = [run(ctx, sc["t"], z, sc["active"], sc.get("outputs", True)) for _ in range(2)]
    for rc, out, state, want in runs:
        check(rc, out, state, want, name)
        assert rc == 0 and want["counts"].tolist() == want0["counts"].tolist()
    for k in runs[0][2]:                                     # the same call again: the same bytes (implied by the above; stated for itself)
        assert same_bits(runs[0][2][k], runs[1][2][k]), k
    print("%s: rows %d, entries kept %d, dropped %d, tracks %d, descriptors %d" % ((name,) + tuple(want0["counts"])))


def test_capacity_one_short_then_enough(ctx):
    sc, z, want = R.cached("every_kind")
    n = int(want["counts"][0])
    rc, out, state, short = run(ctx, sc["t"], dict(z, n_mp_dst=n - 1), sc["active"])
    assert rc == mi355slam.MS_ERR_CAPACITY and "the destination holds %d" % (n - 1) in mi355slam.lib().ms_last_error(ctx._h).decode()
    check(rc, out, state, short, "one short")
    assert out["counts"][0] == n and all((v.view(np.uint8) == FILL).all() for v in state.values())      # the needed number; nothing of the destination is written
    rc, out, state, exact = run(ctx, sc["t"], dict(z, n_mp_dst=n), sc["active"])
    check(rc, out, state, exact, "exact capacity")
    assert rc == 0 and state["mp_live"].all()


def test_no_active_slots_and_an_empty_source(ctx):
    sc, z, _ = R.cached("every_kind")
    rc, out, state, want = run(ctx, sc["t"], z, [])
    check(rc, out, state, want, "n_active = 0")
    assert rc == 0 and out["counts"].tolist() == [0] * 5 and (state["kf_mp"] == -1).all() and not state["mp_live"].any() and (state["row_dst"] == -1).all()
    t = sc["t"]
    empty = dict(t, **{k: t[k][:0] for k in R.ROW_FIELDS + ("mp_live",)})
    rc, out, state, want = run(ctx, empty, R.sizes(empty, 5, 20, 14), sc["active"])      # n_mp = 0: no entry is valid
    check(rc, out, state, want, "n_mp = 0")
    assert rc == 0 and out["counts"].tolist() == [0, 0, 0, 0, 12] and (state["kf_mp"] == -1).all()


@pytest.mark.parametrize("name", ["every_kind", "optional_absent"])
def test_the_full_copy(ctx, name):
    sc, _, _ = R.cached(name)
    t = sc["t"]
    active = R.occupied(t)
    e = np.asarray(t["kf_mp"], np.int64)[active].reshape(-1)
    listed = np.unique(e[R.present(t, e)])
    z = R.sizes(t, len(active) + 1, len(listed) + 3, 0 if t["desc_pool"] is None else len(t["desc_pool"]))
    rc, out, state, want = run(ctx, t, z, active)
    check(rc, out, state, want, name)
    assert rc == 0 and same_bits(state["row_src"][:len(listed)], listed.astype(np.int32)) and out["counts"][0] == len(listed)      # every live row that a keyframe lists


def test_nothing_is_allocated_after_warm_up(ctx):
    sc, z, _ = R.cached("every_kind")
    lib = mi355slam.lib()
    lib.ms_debug_host_allocs.restype = C.c_longlong
    allocs = []
    for _ in range(4):
        d = Device(ctx, sc["t"], z)
        try:
            rc, out = d.call(sc["active"])
            allocs.append(lib.ms_debug_host_allocs())
            check(rc, out, d.state(), R.extract(sc["t"], sc["active"], z, d.before))
        finally:
            d.free()
    assert len(set(allocs[1:])) == 1, allocs


def test_host_validation_runs_before_the_device(ctx):
    sc, z, _ = R.cached("every_kind")
    d = Device(ctx, sc["t"], z)
    try:
        for active, text in (([4, 0, 6], "active slot 6 outside [0, 6)"), ([4, 0, 4], "active slot 4 is listed twice"), ([4, 3], "active slot 3 is empty"),
                             ([0, 1, 2, 4, 5, 0], "6 active slots for a destination of 5 slots")):
            rc, out = d.call(active)
            assert rc == mi355slam.MS_ERR_INVALID and text in mi355slam.lib().ms_last_error(ctx._h).decode(), (active, rc)
            assert not out["counts"].any() and not out["dst_desc_base"].any()                            # the host outputs are not written either
        assert all((v.view(np.uint8) == FILL).all() for v in d.state().values()) and d.source_untouched()
    finally:
        d.free()


def test_the_binding_returns_the_same(ctx):
    sc, z, want = R.cached("every_kind")
    d = Device(ctx, sc["t"], z)
    try:
        src = {k: v for k, v in d.src.items() if k != "kf_mp"}
        t = sc["t"]
        got = d.kf.map_extract(src, z, t["kf_id"], sc["active"], t["desc_base"], t["n_kp"][sc["active"]])
        for k in want:
            if k != "rc":
                assert same_bits(got[k], want[k]), k
        with pytest.raises(mi355slam.MsError, match="the destination holds 10"):
            d.kf.map_extract(src, dict(z, n_mp_dst=10), t["kf_id"], sc["active"], t["desc_base"], t["n_kp"][sc["active"]])
    finally:
        d.free()


# ---- consistency with the entry points that were there before, on the DESTINATION tables
@pytest.mark.parametrize("name", ["every_kind", "second_trip"])
def test_observation_count_and_covisibility_on_the_destination(ctx, name):
    sc, z, want = R.cached(name)
    t, active = sc["t"], sc["active"]
    d = Device(ctx, t, z)
    try:
        rc, out = d.call(active)
        assert rc == 0
        state = d.state()
        kt = table_on(ctx, d.dst["kf_mp"], z["n_kf_dst"], z["stride"])
        kf_id = np.full(z["n_kf_dst"], -1, np.int32)
        kf_id[:len(active)] = t["kf_id"][active]
        count, _, _ = kt.observation_count(kf_id, z["n_mp_dst"], True, False, False)
        assert same_bits(count, state["n_obs"]) and count.sum() == out["counts"][1] > 0
        queries = [(i, -1, -1, 1, 0) for i in range(len(active))]
        got, _, _ = kt.covisibility(queries, z["n_mp_dst"])
    finally:
        d.free()
    # the source's count restricted to active rows: the same query on the source table with every other entry taken out
    e = np.asarray(t["kf_mp"], np.int64)
    keep = R.present(t, e) & (state["row_dst"][np.where(R.present(t, e), e, 0)] >= 0)
    ref, _, _ = covis_ref.covisibility(np.where(keep, e, -1).astype(np.int32), z["n_mp"], None, [(s, -1, -1, 1, 0) for s in active])
    ref = np.asarray(ref)[:, active]
    assert same_bits(np.ascontiguousarray(got[:, :len(active)]), np.ascontiguousarray(ref.astype(np.int32))) and ref.sum() > 0 and not got[:, len(active):].any()


def test_the_front_end_on_the_extracted_map_equals_the_front_end_on_the_whole_map(ctx):
    """One frame that does not become a keyframe, in the slot of a pose_tables_ref scene, through ms_match_tracked -> ms_pose_tables_solve ->
    ms_frame_finish: once on the source tables (the scene's three slots, an inactive fourth keyframe and free rows behind) and once on their
    extraction with the three slots active.  The scene states, and the test asserts, that every row a tracked keypoint names is observed by an
    active slot and by no inactive one.  Compared bit for bit: the 27 numbers of the pose result (the solver's pose [7], the slot's row of the pose
    table [12], lambda and the two chi2, iterations / trials / stopped_early / ran / n_triangulated), the cloud's keypoints, tracks and positions;
    the cloud's rows through row_src."""
    sc, frame0, g = PT.cached("base")
    FRAME, PREV, n_kp, stride, n_old = PT.FRAME, PT.PREV, frame0["n_kp"], sc["stride"], sc["n_mp"]
    n_free, base, n_kf = 700, 5000, 4
    n_mp = n_old + n_free
    rng = np.random.default_rng(6)
    bound = np.asarray(sc["kf_mp"][FRAME], np.int64)[:n_kp]
    kf_mp = np.vstack([sc["kf_mp"], np.full((1, stride), -1, np.int32)])
    kf_mp[FRAME] = -1                                        # the frame has not been matched yet
    seen = np.zeros(n_old, bool)                             # by the two keyframes that stay active
    for s in (0, PREV):
        e = kf_mp[s][(kf_mp[s] >= 0) & (kf_mp[s] < n_old)]
        seen[e] = True
    ok = (bound >= 0) & (bound < n_old)
    ok[ok] = seen[bound[ok]]                                 # the tracked keypoints: bound to rows an active keyframe observes
    unseen = np.nonzero(~seen)[0]                            # the inactive keyframe observes rows nobody active does: they stay behind
    kf_mp[3, :len(unseen)] = unseen
    kf_id = np.array([4, 9, 7, 5], np.int32)
    active = [0, PREV, FRAME]                                # ascending KfId: 4, 7, 9
    assert ok.sum() > 100 and len(unseen) > 50 and not np.isin(bound[ok], kf_mp[3]).any() and seen[bound[ok]].all()
    flags = np.r_[sc["mp_flags"], np.zeros(n_free, np.uint8)]
    live = np.r_[sc["mp_live"], np.zeros(n_free, np.uint8)]
    pos = np.vstack([sc["mp_pos"], np.zeros((n_free, 3))])
    true = sc["true"]
    Rf, cf = true["R"][FRAME], true["c"][FRAME]
    to_cam = cf - pos
    norm = (to_cam / np.linalg.norm(to_cam, axis=1, keepdims=True)).astype(np.float32)
    n_track = n_mp + stride
    kp4 = {k: np.vstack([v, np.zeros((1, stride), v.dtype)]) for k, v in sc["kp"].items()}
    t = dict(kf_mp=kf_mp, kf_id=kf_id, mp_flags=flags, mp_live=live, mp_pos=pos, mp_norm=norm, mp_min_dist=np.zeros(n_mp, np.float32), mp_max_dist=np.full(n_mp, 1e6, np.float32),
             mp_desc=rng.integers(0, 2 ** 32, (n_mp, 8), dtype=np.uint32), mp_track=np.r_[base + np.arange(n_old), np.full(n_free, -1)].astype(np.int32),
             kp_x=kp4["x"], kp_y=kp4["y"], kp_octave=kp4["octave"], kp_depth=kp4["depth"], kf_pose=np.vstack([sc["poses"], np.eye(3, 4).reshape(1, 12)]),
             track_row=np.r_[np.arange(n_old), np.full(n_track - n_old, -1)].astype(np.int32), track_base=base,
             desc_pool=rng.integers(0, 2 ** 32, (stride, 8), dtype=np.uint32), desc_base=np.array([-1, 0, -1, -1], np.int32), n_kp=np.array([0, n_kp, 0, 0], np.int32))
    n_rows = int(R.extract(t, active, R.sizes(t, 3, n_mp, stride))["counts"][0])
    z = R.sizes(t, 3, n_rows + n_free, stride)
    assert 0 < n_rows < n_old - 50
    d = Device(ctx, t, z)
    adj = mi355slam.PoseAdjuster(ctx, stride, PT.W.sigma_levels())
    outs = [dict(outcome=ctx.alloc(n_kp), created_rows=ctx.alloc(4 * n_free), created_kp=ctx.alloc(4 * n_free), tracked_rows=ctx.alloc(4 * n_kp), checked_rows=ctx.alloc(4 * n_kp))
            for _ in range(2)]
    try:
        rc, ext = d.call(active)
        assert rc == 0 and ext["counts"][0] == n_rows and ext["dst_desc_base"].tolist() == [-1, -1, 0]
        row_src = d.state()["row_src"]
        true_pose = np.concatenate([Rf, (-Rf @ cf)[:, None]], 1).reshape(12)
        kp_track = np.where(ok, base + bound, base + n_mp + np.arange(n_kp)).astype(np.int32)      # the others carry a track nobody has seen yet
        results = []
        for which, bufs, rows, slots in (("source", d.src, n_mp, dict(frame=FRAME, prev=PREV, first_free=n_old)), ("extraction", d.dst, z["n_mp_dst"], dict(frame=2, prev=1, first_free=n_rows))):
            kt = table_on(ctx, bufs["kf_mp"], n_kf if which == "source" else 3, stride)
            table, kp = mi355slam.MapPointTable.__new__(mi355slam.MapPointTable), mi355slam.KeypointTable.__new__(mi355slam.KeypointTable)
            table.ctx, table.n = ctx, rows
            table.pos, table.norm, table.min_dist, table.max_dist, table.desc = (bufs[k] for k in ("mp_pos", "mp_norm", "mp_min_dist", "mp_max_dist", "mp_desc"))
            kp.ctx, kp.n_kf, kp.stride = ctx, kt.n_kf, stride
            kp.x, kp.y, kp.octave, kp.depth = (bufs[k] for k in R.KP_FIELDS)
            tracks = mi355slam.TrackTable.__new__(mi355slam.TrackTable)
            tracks.ctx, tracks.track_base, tracks.n_mp, tracks.n_track, tracks.mp_track, tracks.track_row = ctx, base, rows, n_track, bufs["mp_track"], bufs["track_row"]
            poses = mi355slam.KeyframePoseTable.__new__(mi355slam.KeyframePoseTable)
            poses.ctx, poses.n, poses.pose = ctx, kt.n_kf, bufs["kf_pose"]
            pool = bufs["desc_pool"]
            pool.shape = (stride, 8)
            out = outs[which == "extraction"]
            mt = dict(slot=slots["frame"], pose=true_pose, cam=sc["cams"][FRAME], focal=int(sc["focal"][FRAME]), desc_base=0, level_sigma_sq=PT.W.sigma_levels(),
                      rel_reprojection_threshold=0.05, view_cos_limit=0.5)
            new_rows = np.arange(slots["first_free"], rows, dtype=np.int32)
            rc, counts = kt.match_tracked_device(table, bufs["mp_flags"], bufs["mp_live"], tracks, kp, pool, mt, kp_track, new_rows, out)
            assert rc == 0, (which, rc, mi355slam.lib().ms_last_error(ctx._h))
            rc, res = adj.solve_device(kt, bufs["mp_flags"], bufs["mp_live"], table, kp, poses, dict(frame0, slot=slots["frame"], prev_slot=slots["prev"], n_kp=n_kp), False)
            assert rc == 0 and res["ran"], (which, rc, res)
            row12 = mi355slam._download_i32_at(bufs["kf_pose"], 96 * slots["frame"], 24)
            ids = kf_id.copy() if which == "source" else kf_id[active].copy()
            n_obs = ctx.upload(np.zeros(rows, np.int32))
            got = kt.frame_finish(bufs["mp_flags"], bufs["mp_live"], table, bufs["mp_track"], n_obs, ids, [slots["frame"]], slots["frame"], n_kp)
            n_obs.free()
            outcome = out["outcome"].download(np.uint8, (n_kp,))
            results.append(dict(counts=counts, res=res, row12=row12, cloud=got, outcome=outcome))
        a, b = results
        assert a["counts"].tolist() == b["counts"].tolist() and same_bits(a["outcome"], b["outcome"]) and a["counts"][2] > 30, (a["counts"], b["counts"])
        assert same_bits(a["res"]["pose"], b["res"]["pose"]) and same_bits(a["row12"], b["row12"])
        sa, sb = a["res"]["stats"], b["res"]["stats"]
        assert all(np.float64(sa[k]).tobytes() == np.float64(sb[k]).tobytes() for k in sa) and a["res"]["n_triangulated"] == b["res"]["n_triangulated"] > 30
        for k in ("cloud_kp", "cloud_track", "cloud_pos"):
            assert same_bits(a["cloud"][k], b["cloud"][k]), k
        rb = b["cloud"]["cloud_row"]
        assert len(rb) > 30 and (rb < n_rows).all() and same_bits(a["cloud"]["cloud_row"], row_src[rb]) and not np.array_equal(a["cloud"]["cloud_row"], rb)
    finally:
        adj.close()
        for o in outs:
            for b_ in o.values():
                b_.free()
        d.free()
