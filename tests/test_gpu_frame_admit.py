"""ms_frame_admit on the device against tests/frame_admit_ref.py, its specification: every table and every host output bit for
bit, canaries behind every buffer, the same bytes on a second run.  Small shapes: a 6 x 8 table with every kind of drop and of depth; a frame
that reaches the kernel's third trip with the drops on both sides of the first trip's end; the capacity rule at its limit; an occupied row; no
features; no keep, mask or image; the depth rule against ms_keyframe_admit's on the same points; the slot against the one the upload path
leaves, and ms_match_tracked behind it; no allocation after warm-up."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frame_admit_ref as R
import match_tracked_ref as MT
import mi355slam

pytestmark = pytest.mark.gpu
CAN, PAD = 0x5A, 16
F = np.float32
POSE = np.arange(12, dtype=np.float64) * 0.25 - 1.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIP = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(ROOT, "slam-module_amd", "csrc", "frame_admit.hip")).read()).group(1))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def with_canary(a):
    return np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.full(PAD, CAN, np.uint8)])


class Dev:
    """The tables, the depth image and the mask on the device, each with a canary behind it."""

    def __init__(self, ctx, tables, image=None, mask=None):
        self.ctx, self.t, self.image, self.mask = ctx, tables, image, mask
        self.n_kf, self.stride = tables["kf_mp"].shape
        self.tab = {k: ctx.upload(with_canary(tables[k])) for k in R.TABLES}
        self.rasters = dict(image=image, mask=mask)
        self.rbuf = {k: ctx.upload(with_canary(a)) for k, a in self.rasters.items() if a is not None}

    def args(self, slot, pose=POSE):
        a = dict(slot=slot, pose=pose)
        if self.image is not None:
            a.update(depth_image=self.rbuf["image"], depth_height=self.image.shape[0], depth_width=self.image.shape[1])
        if self.mask is not None:
            a.update(valid_mask=self.rbuf["mask"], mask_height=self.mask.shape[0], mask_width=self.mask.shape[1])
        return a

    def call(self, feat, slot, n_mp=50, cap_kp=None, pose=POSE):
        """The C call with a canary behind every host output.  Returns (rc, counts, kp_track, kp_feature), the two cut to n_kp."""
        A = mi355slam._frame_admit_args(self.args(slot, pose))
        arrs, n = mi355slam._frame_admit_features(feat)
        cap = n if cap_kp is None else cap_kp
        trk, ftr = (np.full(4 * (cap + PAD), CAN, np.uint8).view(np.int32) for _ in range(2))
        counts = np.full(4 + PAD, -77, np.int32)
        vp = mi355slam._vp
        rc = mi355slam.lib().ms_frame_admit(self.ctx._h, vp(self.tab["kf_mp"]), self.n_kf, self.stride, n_mp, vp(self.tab["kp_x"]), vp(self.tab["kp_y"]), vp(self.tab["kp_octave"]),
                                            vp(self.tab["kp_depth"]), vp(self.tab["kf_pose"]), *[vp(a) for a in arrs], n, C.byref(A), vp(trk), vp(ftr), cap, vp(counts))
        assert (counts[4:] == -77).all()
        m = int(counts[0]) if rc == 0 else 0
        for a in (trk, ftr):
            assert (a.view(np.uint8)[4 * m:] == CAN).all()   # nothing behind n_kp is written, nothing at all on a refusal
        return rc, counts[:4].copy(), trk[:m].copy(), ftr[:m].copy()

    def state(self):
        """Every table, with its canary and the rasters' bytes checked."""
        out = {}
        for k, b in self.tab.items():
            raw = b.download(np.uint8, (self.t[k].nbytes + PAD,))
            assert (raw[self.t[k].nbytes:] == CAN).all(), k
            out[k] = raw[:self.t[k].nbytes].view(self.t[k].dtype).reshape(self.t[k].shape)
        for k, b in self.rbuf.items():
            assert same_bits(b.download(np.uint8, (self.rasters[k].nbytes + PAD,)), with_canary(self.rasters[k])), k
        return out

    def free(self):
        for b in list(self.tab.values()) + list(self.rbuf.values()):
            b.free()


def admit_and_check(ctx, tables, feat, slot, image=None, mask=None, n_mp=50, cap_kp=None, runs=2):
    """One call on fresh buffers against the restatement, and a second one on fresh buffers that must give the same bytes.  Returns the
    restatement's (rc, tables, outputs)."""
    want_rc, want_t, want = R.frame_admit(tables, n_mp, feat, slot, POSE, image, mask, cap_kp)
    seen = []
    for _ in range(runs):
        dev = Dev(ctx, tables, image, mask)
        try:
            rc, counts, trk, ftr = dev.call(feat, slot, n_mp, cap_kp)
            assert rc == want_rc, (rc, want_rc, mi355slam.lib().ms_last_error(ctx._h))
            assert counts.tolist() == want["counts"].tolist(), (counts, want["counts"])
            state = dev.state()
            for k in R.TABLES:                               # the touched slot, every other slot, every table
                assert same_bits(state[k], want_t[k]), k
            assert same_bits(trk, want["kp_track"]) and same_bits(ftr, want["kp_feature"])
            seen.append((counts, trk, ftr, state))
        finally:
            dev.free()
    for a, b in zip(seen, seen[1:]):
        assert all(same_bits(x, y) for x, y in zip(a[:3], b[:3])) and all(same_bits(a[3][k], b[3][k]) for k in R.TABLES)
    return want_rc, want_t, want


def grid_features(n, seed, width=40):
    """n features, one per pixel of a grid `width` wide (so that a mask byte names one feature), with every kind of depth"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    depth = rng.uniform(0.5, 9, n).astype(F)
    depth[rng.random(n) < 0.4] = -1
    depth[rng.random(n) < 0.05] = np.nan
    return dict(x=(i % width + rng.uniform(-0.4, 0.4, n)).astype(F), y=(i // width + rng.uniform(-0.4, 0.4, n)).astype(F),
                id=(rng.permutation(3 * n + 5)[:n] + 1000).astype(np.int32), depth=depth, keep=None)


def pixel_of(feat, i):
    return int(R.rint_i32(feat["y"][i:i + 1])[0]), int(R.rint_i32(feat["x"][i:i + 1])[0])


# ---- (a)
def test_every_kind_of_drop_and_of_depth_on_a_small_table(ctx):
    tables = R.empty_tables(6, 8, seed=1)
    tables["kf_mp"][:] = np.arange(48, dtype=np.int32).reshape(6, 8) % 50      # other slots are bound
    tables["kf_mp"][3] = [-1, 50, -1, 1 << 30, -9, -1, 77, -2**31]              # the slot's row: stale -1 and out-of-range entries, none valid
    mask = np.ones((10, 12), np.uint8)
    mask[2, 3] = 0
    image = (np.arange(24, dtype=F).reshape(4, 6) + F(100))                    # smaller than the mask: a kept position can lie outside it
    #            kept >= 0   keep   masked  kept <0 image  keep   kept <0 outside the image   kept NaN
    feat = dict(x=np.array([1.0, 2.0, 2.6, 4.5, 0.0, 7.5, 5.0], F), y=np.array([1.0, 2.0, 2.4, 2.5, 0.0, 3.0, 3.0], F), id=np.array([30, 31, 32, 33, 34, 35, 36], np.int32),
                depth=np.array([2.5, 1.0, 1.0, -1.0, -1.0, -3.0, np.nan], F), keep=np.array([1, 0, 1, 1, 0, 1, 1], np.uint8))
    rc, T, out = admit_and_check(ctx, tables, feat, 3, image, mask)
    assert rc == 0 and out["counts"].tolist() == [4, 2, 1, 1] and out["kp_feature"].tolist() == [0, 3, 5, 6] and out["kp_track"].tolist() == [30, 33, 35, 36]
    d = T["kp_depth"][3]
    assert d[0] == F(2.5) and d[1] == image[2, 4] and d[2] == -1 and np.isnan(d[3])       # round(4.5) = 4 and round(2.5) = 2, to even; column 8 is outside
    assert (T["kf_mp"][3] == -1).all() and (T["kp_octave"][3, :4] == 0).all() and same_bits(T["kp_x"][3, 4:], tables["kp_x"][3, 4:])
    # a position outside the MASK's raster is invalid; without an image every negative depth is -1
    feat2 = dict(feat, x=np.array([1.0, 2.0, 12.0, 4.5, 0.0, 7.5, -0.6], F), keep=None)
    rc, T, out = admit_and_check(ctx, tables, feat2, 3, None, mask)
    assert rc == 0 and out["counts"].tolist() == [5, 0, 2, 0] and out["kp_feature"].tolist() == [0, 1, 3, 4, 5] and T["kp_depth"][3, :5].tolist() == [2.5, 1.0, -1.0, -1.0, -1.0]


# ---- (b)
def test_ranks_cross_the_trip_boundary(ctx):
    n, stride = 2 * TRIP + 37, 1024
    feat = grid_features(n, 5)
    feat["keep"] = np.ones(n, np.uint8)
    feat["keep"][[TRIP - 1, TRIP + 1]] = 0
    h = (n + 39) // 40 + 1
    mask = np.ones((h, 41), np.uint8)
    mask[pixel_of(feat, TRIP)] = 0
    image = np.random.default_rng(6).uniform(1, 20, (h - 3, 30)).astype(F)     # some positions lie outside it
    tables = R.empty_tables(3, stride, seed=2)
    rc, T, out = admit_and_check(ctx, tables, feat, 1, image, mask)
    assert rc == 0 and out["counts"][:3].tolist() == [n - 3, 2, 1] and 0 < out["counts"][3] < n
    # the keypoints on both sides of every trip's end
    assert out["kp_feature"][TRIP - 3:TRIP + 1].tolist() == [TRIP - 3, TRIP - 2, TRIP + 2, TRIP + 3]
    assert out["kp_feature"][2 * TRIP - 4:2 * TRIP - 2].tolist() == [2 * TRIP - 1, 2 * TRIP] and out["kp_feature"][-1] == n - 1
    # a drop in the first lane and in the last lane of a trip, and a trip without a kept feature
    feat["keep"][:] = 1
    feat["keep"][[0, TRIP - 1, 2 * TRIP - 1, 2 * TRIP]] = 0
    feat["keep"][TRIP:2 * TRIP] = 0
    rc, T, out = admit_and_check(ctx, tables, feat, 2, image, None)
    assert rc == 0 and out["counts"][0] == n - TRIP - 3 and out["kp_feature"][TRIP - 3:TRIP].tolist() == [TRIP - 2, 2 * TRIP + 1, 2 * TRIP + 2]


# ---- (c)
def test_the_capacity_rule_at_its_limit(ctx):
    stride = 9
    feat = grid_features(11, 7)
    feat["keep"] = np.ones(11, np.uint8)
    feat["keep"][[2, 6]] = 0                                 # n_kp == stride exactly
    tables = R.empty_tables(3, stride, seed=3)
    tables["kf_mp"][1, 8] = -4
    rc, T, out = admit_and_check(ctx, tables, feat, 1)
    assert rc == 0 and out["counts"][0] == stride
    feat["keep"][6] = 1                                      # one more
    rc, T, out = admit_and_check(ctx, tables, feat, 1)
    assert rc == R.CAPACITY and out["counts"][0] == stride + 1 and all(same_bits(T[k], tables[k]) for k in R.TABLES)
    feat["keep"][6] = 0
    rc, T, out = admit_and_check(ctx, tables, feat, 1, cap_kp=stride - 1)      # the host outputs are one short
    assert rc == R.CAPACITY and out["counts"][0] == stride and all(same_bits(T[k], tables[k]) for k in R.TABLES)
    assert b"9 keypoints" in mi355slam.lib().ms_last_error(ctx._h)
    rc, T, out = admit_and_check(ctx, tables, feat, 1, cap_kp=stride)
    assert rc == 0


# ---- (d)
def test_a_valid_entry_in_the_row_refuses_the_frame(ctx):
    feat = grid_features(5, 8)
    tables = R.empty_tables(4, 8, seed=4)
    tables["kf_mp"][2, 7] = 49                               # behind every keypoint of the frame, the last row of the map
    rc, T, out = admit_and_check(ctx, tables, feat, 2, n_mp=50)
    assert rc == R.INVALID and all(same_bits(T[k], tables[k]) for k in R.TABLES) and b"slot 2 is not empty, 1 of its entries" in mi355slam.lib().ms_last_error(ctx._h)
    assert admit_and_check(ctx, tables, feat, 2, n_mp=49)[0] == 0              # the same entry is stale on a smaller map
    tables["kf_mp"][2] = np.arange(8)
    assert admit_and_check(ctx, tables, feat, 2, n_mp=50)[0] == R.INVALID
    assert admit_and_check(ctx, tables, feat, 1, n_mp=50)[0] == 0              # the neighbour is free


# ---- (e), (f)
def test_no_features_and_no_keep_mask_or_image(ctx):
    none = dict(x=np.zeros(0, F), y=np.zeros(0, F), id=np.zeros(0, np.int32), depth=np.zeros(0, F), keep=None)
    tables = R.empty_tables(3, 5, seed=5)
    tables["kf_mp"][0] = [-1, 60, -3, 1 << 29, -1]
    rc, T, out = admit_and_check(ctx, tables, none, 0)
    assert rc == 0 and out["counts"].tolist() == [0, 0, 0, 0] and (T["kf_mp"][0] == -1).all() and same_bits(T["kf_pose"][0], POSE)
    assert all(same_bits(T[k], tables[k]) for k in ("kp_x", "kp_y", "kp_octave", "kp_depth"))
    feat = grid_features(5, 9)
    feat["depth"][:3] = [-1, np.nan, 4.0]
    rc, T, out = admit_and_check(ctx, tables, feat, 2)
    assert rc == 0 and out["counts"].tolist() == [5, 0, 0, 0] and T["kp_depth"][2, 0] == -1 and np.isnan(T["kp_depth"][2, 1]) and T["kp_depth"][2, 2] == 4.0
    assert same_bits(out["kp_track"], feat["id"])
    big = grid_features(1, 10)                               # one feature, a stride of one
    assert admit_and_check(ctx, R.empty_tables(2, 1, seed=6), big, 1)[0] == 0


# ---- (g)
def test_the_depth_rule_is_the_one_of_keyframe_admit(ctx):
    n, stride = 300, 320
    feat = grid_features(n, 11)
    feat["keep"] = (np.random.default_rng(12).random(n) > 0.1).astype(np.uint8)
    image = np.random.default_rng(13).uniform(1, 20, (6, 33)).astype(F)
    tables = R.empty_tables(3, stride, seed=7)
    kept = np.flatnonzero(feat["keep"])
    m = len(kept)
    kt = mi355slam.KeyframeTable(ctx, tables["kf_mp"]); kp = mi355slam.KeypointTable(ctx, tables["kp_x"], tables["kp_y"], tables["kp_octave"], tables["kp_depth"])
    poses = mi355slam.KeyframePoseTable(ctx, tables["kf_pose"])
    d_image, pool, out = ctx.upload(image), ctx.alloc(32 * stride), mi355slam.AdmitFrame(ctx, stride)
    up = lambda a: ctx.upload(np.ascontiguousarray(a))
    view_bufs = [up(np.array([m], np.int32)), up(feat["x"][kept]), up(feat["y"][kept]), up(np.zeros(m, F)), up(np.zeros(m, np.int32)), up(np.zeros((m, 8), np.uint32)),
                 up(feat["id"][kept])]
    try:
        img = dict(depth_image=d_image, depth_height=image.shape[0], depth_width=image.shape[1])
        a = mi355slam.frame_admit(ctx, kt, 50, kp, poses, feat, dict(dict(slot=1, pose=POSE), **img))
        view = mi355slam.keypoints_view(m, *view_bufs)
        b = mi355slam.keyframe_admit(ctx, view, 0, kt, 50, kp, pool, poses, dict(dict(slot=2, desc_base=0, pose=POSE, cam=(500.0, 500.0, 20.0, 4.0, 40, 8), track_ids=feat["id"],
                                                                                      track_depth=feat["depth"]), **img), out, host=("kp_track",))
        assert a["counts"][0] == b["counts"][0] == m and same_bits(a["kp_track"], b["kp_track"])
        shape = (3, stride)
        for name, dt in (("x", F), ("y", F), ("depth", F)):
            rows = getattr(kp, name).download(dt, shape)
            assert same_bits(rows[1, :m], rows[2, :m]), name
            assert same_bits(rows[1, m:], tables["kp_" + name][1, m:])
        depth = kp.depth.download(F, shape)[1, :m]
        assert np.isnan(depth).any() and (depth == -1).any() and a["counts"][3] > 10 and same_bits(a["depth"][:m], depth)
    finally:
        for b_ in view_bufs + [d_image, pool, kt.kf_mp, poses.pose]:
            b_.free()
        kp.free(); out.free()


# ---- (h)
def test_the_slot_equals_the_one_the_upload_path_leaves_and_match_tracked_reads_it(ctx):
    n, stride, n_kf, slot, n_mp, base, window = 40, 48, 4, 2, 20, 1000, 200
    feat = grid_features(n, 14)
    feat["id"] = (base + np.random.default_rng(15).permutation(window)[:n]).astype(np.int32)
    feat["keep"] = np.ones(n, np.uint8)
    feat["keep"][[3, 17]] = 0
    image = np.random.default_rng(16).uniform(1, 20, (3, 30)).astype(F)
    tables = R.empty_tables(n_kf, stride, seed=8)
    tables["kf_mp"][slot, :6] = [-1, 25, -1, 1 << 20, -1, 20]                   # stale entries of an earlier frame
    rc, want_t, want = R.frame_admit(tables, n_mp, feat, slot, POSE, image)
    m = int(want["counts"][0])
    assert rc == 0 and m == n - 2
    # the map: ten live rows that are not triangulated, each the map point of one of the frame's tracks (or of a dropped feature's)
    rows = np.arange(10)
    owners = np.concatenate([want["kp_track"][::5][:8], feat["id"][[3, 17]]])
    mp_track, track_row = np.full(n_mp, -1, np.int32), np.full(window, -1, np.int32)
    mp_track[rows] = owners
    track_row[owners - base] = rows
    mp_live, mp_flags = (np.arange(n_mp) < 10).astype(np.uint8), np.zeros(n_mp, np.uint8)
    sigma = mi355slam.level_sigma_sq(8, 1.2)
    states, outcomes = [], []
    for path in ("admit", "upload"):
        kt = mi355slam.KeyframeTable(ctx, tables["kf_mp"]); kp = mi355slam.KeypointTable(ctx, tables["kp_x"], tables["kp_y"], tables["kp_octave"], tables["kp_depth"])
        poses = mi355slam.KeyframePoseTable(ctx, tables["kf_pose"])
        table = mi355slam.MapPointTable(ctx, np.zeros((n_mp, 3)), np.zeros((n_mp, 3), F), np.zeros(n_mp, F), np.ones(n_mp, F), np.zeros((n_mp, 8), np.uint32))
        tracks = mi355slam.TrackTable(ctx, mp_track, track_row, base)
        flags, live, d_image = ctx.upload(mp_flags), ctx.upload(mp_live), ctx.upload(image)
        out = dict(outcome=ctx.alloc(stride), created_rows=ctx.alloc(4 * n_mp), created_kp=ctx.alloc(4 * n_mp), tracked_rows=ctx.alloc(4 * stride))
        try:
            if path == "admit":
                res = mi355slam.frame_admit(ctx, kt, n_mp, kp, poses, feat, dict(slot=slot, pose=POSE, depth_image=d_image, depth_height=3, depth_width=30))
                kp_track = res["kp_track"]
            else:                                            # the mirror's clear, update and poses.update: the host compaction and depth fill, then six uploads
                kept = np.flatnonzero(feat["keep"])
                depth, _ = R.depth_of(feat["x"][kept], feat["y"][kept], feat["depth"][kept], image)
                row = {k: tables["kp_" + k][slot].copy() for k in ("x", "y", "octave", "depth")}
                row["x"][:m], row["y"][:m], row["octave"][:m], row["depth"][:m] = feat["x"][kept], feat["y"][kept], 0, depth
                kt.update(slot, [])
                kp.update(slot, **row)
                poses.update(slot, 1, POSE)
                kp_track = feat["id"][kept]
            shape = (n_kf, stride)
            states.append(dict(kf_mp=kt.download(), kp_x=kp.x.download(F, shape), kp_y=kp.y.download(F, shape), kp_octave=kp.octave.download(np.int32, shape),
                               kp_depth=kp.depth.download(F, shape), kf_pose=poses.download()))
            frame = dict(slot=slot, pose=POSE, cam=(500.0, 500.0, 20.0, 4.0, 40, 8), focal=500, desc_base=-1, level_sigma_sq=sigma, rel_reprojection_threshold=0.05)
            rc, counts = kt.match_tracked_device(table, flags, live, tracks, kp, None, frame, kp_track, np.arange(10, n_mp, dtype=np.int32), out)
            assert rc == 0, mi355slam.lib().ms_last_error(ctx._h)
            outcomes.append((counts, out["outcome"].download(np.uint8, (stride,))[:m], out["tracked_rows"].download(np.int32, (stride,))[:counts[1]], kt.download()))
        finally:
            for b in [kt.kf_mp, poses.pose, flags, live, d_image, tracks.mp_track, tracks.track_row] + list(out.values()):
                b.free()
            kp.free()
    for k in R.TABLES:
        assert same_bits(states[0][k], states[1][k]) and same_bits(states[0][k], want_t[k]), k
    # the outcomes of the restatement of matchTrackedFeatures on the restated tables with the restated kp_track
    scene = dict(kf_mp=want_t["kf_mp"], mp_flags=mp_flags, mp_live=mp_live, mp_track=mp_track, track_row=track_row, track_base=base, desc_base=np.full(n_kf, -1, np.int32),
                 S=dict(level_sigma_sq=sigma), kp=dict(octave=want_t["kp_octave"]), table={})
    w = MT.walk(scene, dict(slot=slot, kp_track=want["kp_track"]), np.arange(10, n_mp, dtype=np.int32))
    assert w["rc"] == 0 and (w["outcome"] == MT.TRACKED).sum() == 8 and (w["outcome"] == MT.NO_DESCRIPTORS).sum() == m - 8
    for counts, outcome, tracked, kf_mp in outcomes:
        assert counts.tolist() == w["counts"] and same_bits(outcome, w["outcome"]) and same_bits(tracked, w["tracked_rows"]) and same_bits(kf_mp, w["state"]["kf_mp"])


# ---- (i)
def test_nothing_is_allocated_after_warm_up(ctx):
    lib = mi355slam.lib()
    lib.ms_debug_host_allocs.restype = C.c_longlong
    n, stride, n_slots = 500, 512, 4
    feat = grid_features(n, 17)
    feat["keep"] = (np.random.default_rng(18).random(n) > 0.05).astype(np.uint8)
    t = R.empty_tables(n_slots, stride, seed=9)
    kt = mi355slam.KeyframeTable(ctx, t["kf_mp"]); kp = mi355slam.KeypointTable(ctx, t["kp_x"], t["kp_y"], t["kp_octave"], t["kp_depth"])
    poses = mi355slam.KeyframePoseTable(ctx, t["kf_pose"])
    tables = dict(kf_mp=kt.kf_mp, kp_x=kp.x, kp_y=kp.y, kp_octave=kp.octave, kp_depth=kp.depth, kf_pose=poses.pose)
    try:
        allocs, tracks = [], []
        for i in range(23):
            rc, res = mi355slam.frame_admit_device(ctx, tables, n_slots, stride, 50, feat, dict(slot=i % n_slots, pose=POSE))
            allocs.append(lib.ms_debug_host_allocs())
            assert rc == 0 and res["counts"][0] == feat["keep"].sum()
            tracks.append(res["kp_track"])
        assert len(set(allocs[3:])) == 1, allocs             # flat over 20 calls after three warm-ups
        assert all(same_bits(tracks[0], x) for x in tracks)
        x = kp.x.download(F, (n_slots, stride))
        assert all(same_bits(x[0, :res["counts"][0]], x[k, :res["counts"][0]]) for k in range(n_slots))
    finally:
        kp.free(); kt.kf_mp.free(); poses.pose.free()
