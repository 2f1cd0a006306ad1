"""ms_loop_usable_mask, ms_loop_pairs and ms_loop_sim3_lists on the device against tests/loop_chain_ref.py, their specification.
Every output is compared bit for bit; every device buffer the test hands over ends in a canary that must survive the call, every host output
array is followed by a guard that must keep its fill.  tests/test_loop_chain_ref.py asserts on the restatement that the scenes hold the
conditions relied on here (every drop reason in every trip of the walk, a first trip without a kept pair, an empty candidate between two
others, a 257th candidate behind a non-zero carry)."""
import ctypes as C

import numpy as np
import pytest

import mi355slam
import loop_chain_ref as R

pytestmark = pytest.mark.gpu

CANARY = 64
FILL = 0x77
TABLES = ("mp_flags", "mp_live", "mp_pos", "kf_pose", "kp_x", "kp_y", "kp_octave")
INVALID, CAPACITY = mi355slam.MS_ERR_INVALID, mi355slam.MS_ERR_CAPACITY


class Dev:
    """An array on the device with CANARY bytes of 0xA5 behind it."""

    def __init__(self, ctx, arr):
        self.host = np.ascontiguousarray(arr)
        raw = np.concatenate([self.host.view(np.uint8).reshape(-1), np.full(CANARY, 0xA5, np.uint8)])
        self.buf = ctx.upload(raw)

    def get(self):
        raw = self.buf.download(np.uint8, (self.host.nbytes + CANARY,))
        assert (raw[self.host.nbytes:] == 0xA5).all(), "canary overwritten"
        return raw[:self.host.nbytes].view(self.host.dtype).reshape(self.host.shape).copy()

    def free(self):
        self.buf.free()


class Tables:
    """The tables of a scene on the device; close() checks that the calls left every one of them as it was."""

    def __init__(self, ctx, t):
        self.t = t
        self.kt = mi355slam.KeyframeTable(ctx, t["kf_mp"])
        self.d = {k: Dev(ctx, t[k]) for k in TABLES}

    def __getitem__(self, k):
        return self.d[k].buf

    def close(self):
        assert np.array_equal(self.kt.download(), self.t["kf_mp"])
        for k in TABLES:
            assert np.array_equal(self.d[k].get().view(np.uint8), np.ascontiguousarray(self.t[k]).view(np.uint8)), k
            self.d[k].free()
        self.kt.kf_mp.free()


def filled(spec, n, extra=()):
    """Host output arrays of n entries, every byte FILL, each a view into a block with a guard of CANARY bytes behind it."""
    out, blocks = {}, {}
    for k, dt, w in tuple(spec) + tuple(extra):
        shape = w if isinstance(w, tuple) else ((n, w) if w > 1 else (n,))
        nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
        blocks[k] = np.full(nbytes + CANARY, FILL, np.uint8)
        out[k] = blocks[k][:nbytes].view(dt).reshape(shape)
    return out, blocks


def untouched(blocks, names=None, first=None):
    """The guards, and for `names` the whole arrays (or their entries from `first` on), still hold the fill."""
    for k, b in blocks.items():
        assert (b[-CANARY:] == FILL).all(), k + ": guard overwritten"
    for k in names or ():
        b = blocks[k][:-CANARY]
        assert (b[(first or {}).get(k, 0):] == FILL).all(), k


def pairs(ctx, S, T, matched=None, cap=None):
    """One ms_loop_pairs call.  Returns (rc, n_pairs, out, blocks, the context's message)."""
    matched = S["matched"] if matched is None else matched
    cap = S["want"]["n_pairs"] if cap is None else cap
    n_cand = len(S["cand_slot"])
    dm = [Dev(ctx, m if len(m) else np.zeros(1, np.int32)) for m in matched]
    out, blocks = filled(mi355slam.LOOP_PAIRS_OUT, cap, (("pair_start", np.int32, (n_cand + 1,)), ("cur_pose", np.float64, (12,)), ("cand_pose", np.float64, (max(n_cand, 1), 12))))
    a = mi355slam.LoopPairsArgs(mp_live=T["mp_live"], mp_pos=T["mp_pos"], n_mp=S["n_mp"], kf_pose=T["kf_pose"], kp_octave=T["kp_octave"], cur=S["cur"], n_kp_cur=S["n_kp_cur"],
                                cand_slot=S["cand_slot"], n_kp_cand=S["n_kp_cand"], matched=[d.buf for d in dm], level_sigma_sq=S["level_sigma_sq"], cap_pairs=cap, out=out)
    why = ""
    try:
        rc, n, _ = T.kt.loop_pairs(a)
        if rc:
            why = mi355slam.lib().ms_last_error(ctx._h).decode()
    except mi355slam.MsError as e:                           # every code but MS_ERR_CAPACITY raises
        rc, n, why = e.rc, None, mi355slam.lib().ms_last_error(ctx._h).decode()
    for d, m in zip(dm, matched):
        assert np.array_equal(d.get()[:len(m)], m)
        d.free()
    return rc, n, out, blocks, why


def assert_pairs(out, blocks, w, n):
    assert n == w["n_pairs"] and np.array_equal(out["pair_start"], w["pair_start"])
    for k in R.PAIR_ARRAYS:
        assert np.array_equal(out[k][:n].view(np.uint8), w[k].view(np.uint8)), k
    assert np.array_equal(out["cur_pose"].view(np.uint8), w["cur_pose"].view(np.uint8)) and np.array_equal(out["cand_pose"].view(np.uint8), w["cand_pose"].view(np.uint8))
    sizes = {k: n * w_ * np.dtype(dt).itemsize for k, dt, w_ in mi355slam.LOOP_PAIRS_OUT}
    untouched(blocks, sizes, sizes)


def sim3_lists(ctx, S, T, kp1, kp2, start):
    out, blocks = filled(mi355slam.LOOP_SIM3_OUT, len(kp1))
    a = mi355slam.LoopSim3ListsArgs(mp_live=T["mp_live"], mp_pos=T["mp_pos"], n_mp=S["n_mp"], kf_pose=T["kf_pose"], kp_x=T["kp_x"], kp_y=T["kp_y"], kp_octave=T["kp_octave"],
                                    cur=S["cur"], n_kp_cur=S["n_kp_cur"], cand_slot=S["cand_slot"], n_kp_cand=S["n_kp_cand"], cams=T.t["cams"],
                                    level_sigma_sq=S["level_sigma_sq"], kp1=kp1, kp2=kp2, match_start=start, out=out)
    try:
        T.kt.loop_sim3_lists(a)
    except mi355slam.MsError as e:
        return e.rc, out, blocks, mi355slam.lib().ms_last_error(ctx._h).decode()
    return 0, out, blocks, ""


def assert_sim3(out, blocks, w):
    for k in R.SIM3_ARRAYS:
        assert np.array_equal(out[k].view(np.uint8), w[k].view(np.uint8)), k
    untouched(blocks)


# base: three trips of the walk over 600 keypoints, candidates of 600, 0, 257, 1 and 256 keypoints; cands257: the offsets scan's second trip
# (DESIGN 9.10), keyframes of 8 keypoints; small: one trip
@pytest.mark.parametrize("name", R.SCENES)
def test_scene_matches_the_restatement(ctx, name):
    S = R.gpu_scene(name)
    T = Tables(ctx, S["tables"])
    rc, n, out, blocks, why = pairs(ctx, S, T)
    assert rc == 0, why
    assert_pairs(out, blocks, S["want"], n)
    kp1, kp2, start = R.keypoint_lists(S, S["lists"])
    rc, out, blocks, why = sim3_lists(ctx, S, T, kp1, kp2, start)
    assert rc == 0, why
    assert_sim3(out, blocks, S["want_sim3"])
    T.close()


@pytest.mark.parametrize("name", ("base", "small"))
def test_masks_of_every_slot_in_one_call(ctx, name):
    S = R.gpu_scene(name)
    t = S["tables"]
    T = Tables(ctx, t)
    slots = np.concatenate([[S["cur"], S["cur"]], S["cand_slot"]]).astype(np.int32)
    n_kp = np.concatenate([[S["n_kp_cur"], S["n_kp_cur"]], S["n_kp_cand"]]).astype(np.int32)
    require = np.array([0, 1] + [1] * len(S["cand_slot"]), np.int32)
    masks = [Dev(ctx, np.full(max(n, 1) + 3, FILL, np.uint8)) for n in n_kp]
    rows = [None if s == 2 else Dev(ctx, np.full(max(n, 1) + 3, 0x77777777, np.int32)) for s, n in enumerate(n_kp)]
    T.kt.loop_usable_mask(mi355slam.LoopMaskArgs(mp_flags=T["mp_flags"], mp_live=T["mp_live"], n_mp=S["n_mp"], slots=slots, n_kp=n_kp, require_triangulated=require,
                                                 usable=[m.buf for m in masks], tri_row=[None if r is None else r.buf for r in rows]))
    for s, (slot, n) in enumerate(zip(slots, n_kp)):
        u, r = R.usable_mask_tables(t, slot, n, require[s])
        got = masks[s].get()
        assert np.array_equal(got[:n], u) and (got[n:] == FILL).all(), s
        if rows[s] is not None:
            got = rows[s].get()
            assert np.array_equal(got[:n], r) and (got[n:] == 0x77777777).all(), s
    # without mp_live every row is live: the stale entries count again; without tri_row and require no flags are needed
    m2 = Dev(ctx, np.full(S["n_kp_cur"], FILL, np.uint8))
    T.kt.loop_usable_mask(mi355slam.LoopMaskArgs(mp_flags=None, mp_live=None, n_mp=S["n_mp"], slots=[S["cur"]], n_kp=[S["n_kp_cur"]], require_triangulated=[0], usable=[m2.buf]))
    assert np.array_equal(m2.get(), ((t["kf_mp"][S["cur"], :S["n_kp_cur"]] >= 0)).astype(np.uint8))
    with pytest.raises(mi355slam.MsError, match="loop mask: slot"):
        T.kt.loop_usable_mask(mi355slam.LoopMaskArgs(mp_flags=None, mp_live=None, n_mp=S["n_mp"], slots=[S["cur"]], n_kp=[S["n_kp_cur"]], require_triangulated=[1], usable=[m2.buf]))
    for b in masks + [r for r in rows if r is not None] + [m2]:
        b.free()
    T.close()


def test_zero_sizes(ctx):
    S = dict(R.gpu_scene("small"))
    T = Tables(ctx, S["tables"])
    none = [np.full(S["n_kp_cur"], -1, np.int32) for _ in S["cand_slot"]]
    rc, n, out, blocks, why = pairs(ctx, S, T, matched=none, cap=0)
    assert rc == 0 and n == 0 and not out["pair_start"].any(), why
    assert np.array_equal(out["cand_pose"], S["want"]["cand_pose"])
    for kw in (dict(cand_slot=np.zeros(0, np.int32), n_kp_cand=np.zeros(0, np.int32), matched=[]), dict(n_kp_cur=0, matched=[np.zeros(0, np.int32)] * 2)):
        Z = dict(S, **kw)
        rc, n, out, blocks, why = pairs(ctx, Z, T, matched=Z["matched"], cap=4)
        assert rc == 0 and n == 0 and not out["pair_start"].any(), why
        untouched(blocks, [k for k, _, _ in mi355slam.LOOP_PAIRS_OUT] + ["cur_pose", "cand_pose"])
    rc, out, blocks, why = sim3_lists(ctx, S, T, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(len(S["cand_slot"]) + 1, np.int32))
    assert rc == 0, why
    T.close()


def violated(S, which):
    """(tables, matched, the sim3 lists) of scene S with one device-detected condition broken."""
    t, w = {k: v.copy() for k, v in S["tables"].items()}, S["want"]
    matched = [m.copy() for m in S["matched"]]
    kp1, kp2, start = R.keypoint_lists(S, S["lists"])
    c = 1
    e = int(w["pair_start"][c])                              # candidate 1's first pair
    assert w["pair_start"][c + 1] > e
    if which == "matched at n_kp_cand":
        matched[c][int(np.flatnonzero(matched[c] < 0)[0])] = S["n_kp_cand"][c]
    elif which == "matched below -1":
        matched[0][3] = -2
    elif which == "octave at n_levels, current keyframe":
        t["kp_octave"][S["cur"], w["kp1"][e]] = S["n_levels"]
    elif which == "octave at n_levels, candidate":
        t["kp_octave"][S["cand_slot"][c], w["kp2"][e]] = S["n_levels"]
    elif which == "negative octave":
        t["kp_octave"][S["cand_slot"][c], w["kp2"][e]] = -1
    elif which == "listed keypoint without a row":
        t["kf_mp"][S["cur"], kp1[0]] = -1
    elif which == "listed keypoint with a dead row":
        t["mp_live"][t["kf_mp"][S["cand_slot"][0], kp2[0]]] = 0
    elif which == "listed keypoint outside its keyframe":
        kp2[len(kp2) - 1] = S["n_kp_cand"][-1]
    elif which == "listed keypoint negative":
        kp1[1] = -1
    return t, matched, (kp1, kp2, start)


@pytest.mark.parametrize("which", ("matched at n_kp_cand", "matched below -1", "octave at n_levels, current keyframe", "octave at n_levels, candidate", "negative octave"))
def test_each_violation_of_the_pairs_writes_nothing(ctx, which):
    S = R.gpu_scene("small")
    t, matched, _ = violated(S, which)
    T = Tables(ctx, t)
    rc, n, out, blocks, why = pairs(ctx, S, T, matched=matched)
    assert rc == INVALID and why.startswith("loop pairs: ") and "violations on the device" in why, (rc, why)
    untouched(blocks, list(blocks))
    T.close()


@pytest.mark.parametrize("which", ("octave at n_levels, current keyframe", "listed keypoint without a row", "listed keypoint with a dead row",
                                   "listed keypoint outside its keyframe", "listed keypoint negative"))
def test_each_violation_of_the_sim3_lists_writes_nothing(ctx, which):
    S = R.gpu_scene("small")
    t, _, (kp1, kp2, start) = violated(S, which)
    if which.startswith("octave"):                           # an octave of a LISTED keypoint
        t = {k: v.copy() for k, v in S["tables"].items()}
        t["kp_octave"][S["cur"], kp1[0]] = S["n_levels"]
    T = Tables(ctx, t)
    rc, out, blocks, why = sim3_lists(ctx, S, T, kp1, kp2, start)
    assert rc == INVALID and why.startswith("loop sim3 lists: ") and "violations on the device" in why, (rc, why)
    untouched(blocks, list(blocks))
    T.close()


def test_capacity_reports_the_needed_sizes_and_leaves_the_arrays(ctx):
    S = R.gpu_scene("base")
    w = S["want"]
    T = Tables(ctx, S["tables"])
    rc, n, out, blocks, why = pairs(ctx, S, T, cap=w["n_pairs"] - 1)
    assert rc == CAPACITY and n == w["n_pairs"] and np.array_equal(out["pair_start"], w["pair_start"]), (rc, why)
    untouched(blocks, [k for k, _, _ in mi355slam.LOOP_PAIRS_OUT] + ["cur_pose", "cand_pose"])
    rc, n, out, blocks, why = pairs(ctx, S, T, cap=w["n_pairs"])
    assert rc == 0, why
    assert_pairs(out, blocks, w, n)
    rc, n, out, blocks, why = pairs(ctx, S, T, cap=w["n_pairs"] + 1000)                    # the same bits at a larger capacity
    assert rc == 0, why
    assert_pairs(out, blocks, w, n)
    T.close()


def test_two_calls_give_the_same_bits_and_the_workspace_only_grows(ctx):
    allocs = mi355slam.lib().ms_debug_host_allocs
    allocs.restype = C.c_longlong
    big, small = R.gpu_scene("base"), R.gpu_scene("small")
    Tb, Ts = Tables(ctx, big["tables"]), Tables(ctx, small["tables"])
    lists_b, lists_s = R.keypoint_lists(big, big["lists"]), R.keypoint_lists(small, small["lists"])
    pairs(ctx, big, Tb)
    sim3_lists(ctx, big, Tb, *lists_b)
    first = (pairs(ctx, small, Ts), sim3_lists(ctx, small, Ts, *lists_s))
    before = allocs()
    second = (pairs(ctx, small, Ts), sim3_lists(ctx, small, Ts, *lists_s))
    again = pairs(ctx, big, Tb)
    assert allocs() == before
    assert first[0][0] == second[0][0] == 0 and first[1][0] == second[1][0] == 0 and again[0] == 0
    for k in first[0][3]:
        assert np.array_equal(first[0][3][k], second[0][3][k]), k
    for k in first[1][2]:
        assert np.array_equal(first[1][2][k], second[1][2][k]), k
    assert_pairs(second[0][2], second[0][3], small["want"], second[0][1])
    assert_pairs(again[2], again[3], big["want"], again[1])
    Tb.close(); Ts.close()


def test_the_chain_feeds_the_solvers_the_restatements_arrays(ctx):
    """ms_loop_usable_mask -> ms_match_loop_closure -> ms_loop_pairs -> ms_loop_ransac -> matchMapPointsSim3 (keyframe_matcher.cpp:633-686 on
    the rows ms_loop_usable_mask left in tri_row: the gate and the scoring of both directions on the device, the mutual check here, as the
    table form of the C++ mirror runs it) -> ms_loop_sim3_lists -> ms_sim3_optimize, with `matched` never leaving the device; the solvers'
    results equal those of the same solvers fed by the restatement's arrays."""
    S, t, frames = R.chain_scene()
    T = Tables(ctx, t)
    n, cands = S["stride"], list(S["cand_slot"])
    slots = [S["cur"]] + cands
    masks = [Dev(ctx, np.full(n, FILL, np.uint8)) for _ in slots]
    rows = [Dev(ctx, np.full(n, 0x77777777, np.int32)) for _ in slots]
    T.kt.loop_usable_mask(mi355slam.LoopMaskArgs(mp_flags=T["mp_flags"], mp_live=T["mp_live"], n_mp=S["n_mp"], slots=slots, n_kp=[n] * 3, require_triangulated=[0, 1, 1],
                                                 usable=[m.buf for m in masks], tri_row=[r.buf for r in rows]))
    tri = [r.get() for r in rows]
    fr = [mi355slam.FrameOnDevice(ctx, f["desc"], f["angle"], np.zeros(n, np.uint8), f["bucket"]) for f in frames]
    for f, m in zip(fr, masks):                              # the matcher reads the masks where ms_loop_usable_mask wrote them
        f.struct.usable = m.buf.ptr
    A1 = (mi355slam.MatchFrame * 2)(fr[0].struct, fr[0].struct)
    A2 = (mi355slam.MatchFrame * 2)(fr[1].struct, fr[2].struct)
    dm = [Dev(ctx, np.full(n, 0x77777777, np.int32)) for _ in cands]
    nm = ctx.alloc(8)
    ctx.check(mi355slam.lib().ms_match_loop_closure(ctx._h, A1, A2, 2, C.c_float(0.75), 1, (C.c_void_p * 2)(*[d.buf.ptr for d in dm]), C.c_void_p(nm.ptr)), "ms_match_loop_closure")
    ctx.sync()
    matched = [d.get() for d in dm]
    assert all((m >= 0).sum() > 200 for m in matched)
    w = R.pairs_tables(S, t, matched)
    out, blocks = filled(mi355slam.LOOP_PAIRS_OUT, w["n_pairs"], (("pair_start", np.int32, (3,)), ("cur_pose", np.float64, (12,)), ("cand_pose", np.float64, (2, 12))))
    rc, total, _ = T.kt.loop_pairs(mi355slam.LoopPairsArgs(mp_live=T["mp_live"], mp_pos=T["mp_pos"], n_mp=S["n_mp"], kf_pose=T["kf_pose"], kp_octave=T["kp_octave"], cur=0,
                                                             n_kp_cur=n, cand_slot=cands, n_kp_cand=[n, n], matched=[d.buf for d in dm], level_sigma_sq=S["level_sigma_sq"],
                                                             cap_pairs=w["n_pairs"], out=out))
    assert rc == 0, mi355slam.lib().ms_last_error(ctx._h).decode()
    assert_pairs(out, blocks, w, total)
    cam = tuple(t["cams"][0][:4]) + (640, 480)
    rng = np.random.default_rng(5)
    samples = [mi355slam.draw_samples(int(b - a), 60, rng) for a, b in zip(w["pair_start"], w["pair_start"][1:])]

    def ransac(src):
        return mi355slam.loop_ransac(ctx, [dict(pts1=src["pts1"][a:b], pts2=src["pts2"][a:b], thr1=src["thr1"][a:b], thr2=src["thr2"][a:b], cam1=cam, cam2=cam, n_iter=60,
                                                samples=samples[c], min_inliers=15) for c, (a, b) in enumerate(zip(w["pair_start"], w["pair_start"][1:]))])

    got, want = ransac(out), ransac(w)
    for g, x in zip(got, want):
        assert g["ok"] and g["count"] > 100
        for k in ("ok", "count", "best_iter"):
            assert g[k] == x[k], k
        for k in ("R12", "t12", "union", "best"):
            assert np.array_equal(g[k], x[k]), k
        assert g["scale12"] == x["scale12"]
    sf = mi355slam.scale_factors(S["n_levels"], 1.2)
    mpt = S["mp_table"]
    table = mi355slam.MapPointTable(ctx, mpt["pos"], mpt["norm"], mpt["min_dist"], mpt["max_dist"], mpt["desc"])
    pk = [mi355slam.ProjectionKeyframe(ctx, t["kp_x"][s], t["kp_y"][s], frames[s]["desc"], t["kp_octave"][s]) for s in slots]

    def match_map_points_sim3(c, g, taken1, taken2):
        P1, P2 = t["kf_pose"][0].reshape(3, 4), t["kf_pose"][cands[c]].reshape(3, 4)
        R12, t12, s12 = g["R12"], g["t12"], float(g["scale12"])
        poses = ((R12.T @ P1[:, :3] / s12, R12.T @ (P1[:, 3] - t12) / s12),                          # transform12^-1 * kf1.poseCW (:650)
                 (s12 * R12 @ P2[:, :3], s12 * R12 @ P2[:, 3] + t12))                                # transform12 * kf2.poseCW (:661)
        best = []
        for (Rv, tv), mps, taken, kf in zip(poses, (tri[0], tri[1 + c]), (taken1, taken2), (pk[1 + c], pk[0])):
            owner = np.flatnonzero(~taken & (mps >= 0))
            view = dict(R=Rv, t=tv, cam=cam, threshold=7.5, mode=mi355slam.GATE_SIM3, indices=mps[owner])
            m = np.full(n, -1, np.int32)
            m[owner] = mi355slam.find_matches_transformed(ctx, kf, table, view, sf, 1.2)
            best.append(m)
        fwd, bwd = best
        return [(i1, int(fwd[i1])) for i1 in range(n) if fwd[i1] >= 0 and bwd[fwd[i1]] == i1]      # :672-685

    kp1, kp2, start = [], [], [0]
    for c, g in enumerate(got):
        a = int(w["pair_start"][c])
        inl = a + np.flatnonzero(g["union"])
        taken1, taken2 = np.zeros(n, bool), np.zeros(n, bool)
        taken1[out["kp1"][inl]] = True; taken2[out["kp2"][inl]] = True
        more = match_map_points_sim3(c, g, taken1, taken2)
        assert len(more) > 10 and all(i1 == i2 for i1, i2 in more)                                  # keypoint k is world point k on both sides
        assert any(matched[c][i1] < 0 for i1, _ in more)                                             # among them points the BoW matcher left out
        kp1 += list(out["kp1"][inl]) + [i1 for i1, _ in more]
        kp2 += list(out["kp2"][inl]) + [i2 for _, i2 in more]
        start.append(len(kp1))
    kp1, kp2, start = np.array(kp1, np.int32), np.array(kp2, np.int32), np.array(start, np.int32)
    ws = R.sim3_lists_tables(S, t, kp1, kp2, start)
    rc, so, sblocks, why = sim3_lists(ctx, S, T, kp1, kp2, start)
    assert rc == 0, why
    assert_sim3(so, sblocks, ws)

    def optimise(src):
        return mi355slam.sim3_optimize(ctx, [dict({k: src[k][a:b] for k in ("pts1", "pts2", "obs1", "obs2", "info1", "info2")}, huber_delta=float(np.float32(np.sqrt(10.0))),
                                                  R12=g["R12"], t12=g["t12"], scale12=float(g["scale12"])) for g, a, b in zip(got, start, start[1:])], chi2=True)

    for g, x in zip(optimise(so), optimise(ws)):
        assert g["iters"] > 0 and np.isfinite(g["chi2_final"]) and g["chi2_final"] <= g["chi2_init"]
        for k in g:
            assert np.array_equal(np.asarray(g[k]), np.asarray(x[k])), k
    for b in masks + rows + dm:
        b.free()
    nm.free()
    for b in [table.pos, table.norm, table.min_dist, table.max_dist, table.desc] + [b for k in pk for b in (k.d_sx, k.d_sy, k.d_si, k.d_desc, k.d_oct)]:
        b.free()
    for f in fr:
        for b in f.bufs.values():
            b.free()
    T.close()
