"""ms_bound_mask and ms_search_bind on the device against tests/search_bind_ref.py, their specification.  Every table and every
output is compared bit for bit with the `tables` form; every buffer the test hands over ends in a canary that must survive the call.
tests/test_search_bind_ref.py asserts on the restatement that the scenes hold the conditions relied on here (every outcome code in every trip
of the walk, the rescan of the band scene in more than one pass, a first trip without a stepped query)."""
import ctypes as C

import numpy as np
import pytest

import mi355slam
import project_gate_ref as G
import search_bind_ref as R

pytestmark = pytest.mark.gpu

CANARY = 64
LISTS = ("top_idx", "top_dist", "top_octave", "n_scored")
QUERIES = ("kept_entry", "q_x", "q_y", "q_radius", "q_min_octave", "q_max_octave", "q_desc")
OUTPUTS = ("match_kp", "outcome", "usable")


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


def run(ctx, S, null=(), skip=None, **changed):
    """One ms_search_bind call on fresh copies of scene S (with `changed` inputs).  skip None: the mask comes from ms_bound_mask.  Returns
    (result or None, the MsError or None, dict of the tables and outputs after the call)."""
    S = dict(S, **{k: v for k, v in changed.items() if k not in LISTS})
    L = dict(S["want"]["lists"], **{k: v for k, v in changed.items() if k in LISTS})
    n_kp, count = S["n_kp"], S["count"]
    t = mi355slam.KeyframeTable(ctx, S["kf_mp"])
    k = S["kf"]
    kf = mi355slam.ProjectionKeyframe(ctx, k["x"], k["y"], k["desc"], k["octave"])
    d = {name: Dev(ctx, S[name]) for name in ("mp_live", "n_obs") + QUERIES}
    d.update({name: Dev(ctx, L[name]) for name in LISTS})
    d["skip"] = Dev(ctx, np.full(n_kp, 0x77, np.uint8) if skip is None else skip)
    if skip is None:
        t.bound_mask(S["slot"], n_kp, S["n_mp"], d["skip"].buf)
    d.update(match_kp=Dev(ctx, np.full(count, 12345, np.int32)), outcome=Dev(ctx, np.full(count, 0x77, np.uint8)), usable=Dev(ctx, np.ones(n_kp, np.uint8)))
    a = mi355slam.SearchBindArgs(n_mp=S["n_mp"], kf=kf, mp_index=S["mp_index"], first=S["first"], count=count, n_kept=S["n_kept"], slot=S["slot"],
                                 **{name: (None if name in null else b.buf) for name, b in d.items()})
    res = err = None
    try:
        res = t.search_bind(a)
    except mi355slam.MsError as ex:
        err = ex
    got = dict(kf_mp=t.download(), **{name: b.get() for name, b in d.items()})
    for name in ("mp_live",) + QUERIES + LISTS:                   # what the call only reads
        assert np.array_equal(got[name], d[name].host), name
    for b in list(d.values()) + [t.kf_mp, kf.d_sx, kf.d_sy, kf.d_si, kf.d_desc, kf.d_oct]:
        b.free()
    return res, err, got


def assert_same(S, res, got, null=()):
    w = S["want"]
    assert np.array_equal(got["kf_mp"], w["kf_mp"]) and np.array_equal(got["n_obs"], w["n_obs"])
    assert np.array_equal(got["skip"], w["skip"])
    for name in OUTPUTS:
        if name in null:
            assert np.array_equal(got[name], np.full(len(got[name]), {"match_kp": 12345, "outcome": 0x77, "usable": 1}[name])), name
        else:
            assert np.array_equal(got[name], w[name]), name
    assert res.n_matched == w["n_matched"] and np.array_equal(res.counts, w["counts"])


def test_bound_mask_is_the_complement_of_unbound_mask(ctx):
    S = R.gpu_scene("clustered")
    t = mi355slam.KeyframeTable(ctx, S["kf_mp"])
    for slot in range(S["n_kf"]):
        for n_kp in (S["n_kp"], S["stride"], 1, 0):
            a, b = Dev(ctx, np.full(max(n_kp, 1), 0x77, np.uint8)), Dev(ctx, np.full(max(n_kp, 1), 0x77, np.uint8))
            t.bound_mask(slot, n_kp, S["n_mp"], a.buf)
            t.unbound_mask([slot], [n_kp], S["n_mp"], [b.buf])
            ga, gb = a.get(), b.get()
            assert np.array_equal(ga[:n_kp], R.bound_mask(S["kf_mp"], slot, n_kp, S["n_mp"])) and np.array_equal(ga[:n_kp], 1 - gb[:n_kp])
            assert (ga[n_kp:] == 0x77).all()
            a.free(); b.free()
    t.kf_mp.free()


# clustered: three trips of the walk; kp1100 / kp2100: the marks' second and third trip; band: a rescan of three passes; lead: a first trip
# in which no query is stepped, so the second trip starts from an empty carry
@pytest.mark.parametrize("name", ("clustered", "kp1100", "kp2100", "band", "lead"))
def test_scene_matches_the_restatement(ctx, name):
    S = R.gpu_scene(name)
    res, err, got = run(ctx, S)
    assert err is None, err
    assert_same(S, res, got)


@pytest.mark.parametrize("left_out", OUTPUTS)
def test_each_optional_output_left_out_once(ctx, left_out):
    S = R.gpu_scene("small")
    res, err, got = run(ctx, S, null=(left_out,))
    assert err is None, err
    assert_same(S, res, got, null=(left_out,))


def test_no_kept_query_binds_nothing(ctx):
    S = R.gpu_scene("small")
    res, err, got = run(ctx, S, n_kept=0)
    assert err is None, err
    assert np.array_equal(got["kf_mp"], S["kf_mp"]) and np.array_equal(got["n_obs"], S["n_obs"])
    assert (got["match_kp"] == -1).all() and (got["outcome"] == 0).all() and (got["usable"] == 1).all()
    assert res.n_matched == 0 and not res.counts.any()


def violated(S, which):
    """The inputs of run() that break one condition of the pre-pass."""
    w, first, count, K = S["want"], S["first"], S["count"], S["slot"]
    ke, mi, ti, skip, kf_mp, live = S["kept_entry"].copy(), S["mp_index"].copy(), w["lists"]["top_idx"].copy(), w["skip"].copy(), S["kf_mp"].copy(), S["mp_live"].copy()
    bound = np.flatnonzero(skip)
    free = np.setdiff1d(np.flatnonzero(skip == 0), ti.reshape(-1))
    if which == "kept_entry behind the slice":
        ke[3] = first + count
    elif which == "kept_entry in front of the slice":
        ke[0] = first - 1
    elif which == "top_idx at n_kp":
        ti[5, 1] = S["n_kp"]
    elif which == "top_idx below -1":
        ti[2, 3] = -2
    elif which == "top_idx marked by skip":
        ti[7, 0] = bound[0]
    elif which == "skip marks a free keypoint":
        skip[free[0]] = 1
    elif which == "skip misses a bound keypoint":
        skip[bound[1]] = 0
    elif which == "row not live":
        live[mi[ke[4]]] = 0
    elif which == "row listed by the slot":
        kf_mp[K, bound[2]] = mi[ke[4]]
    elif which == "entry named twice":
        ke[9] = ke[8]
    elif which == "row named twice":
        mi[ke[9]] = mi[ke[8]]
    return dict(kept_entry=ke, mp_index=mi, top_idx=ti, skip=skip, kf_mp=kf_mp, mp_live=live)


@pytest.mark.parametrize("which", ("kept_entry behind the slice", "kept_entry in front of the slice", "top_idx at n_kp", "top_idx below -1", "top_idx marked by skip",
                                   "skip marks a free keypoint", "skip misses a bound keypoint", "row not live", "row listed by the slot", "entry named twice",
                                   "row named twice"))
def test_each_pre_pass_violation_leaves_the_tables_as_they_were(ctx, which):
    S = R.gpu_scene("small")
    ch = violated(S, which)
    res, err, got = run(ctx, S, **ch)
    assert res is None and err is not None and "1 violations on the device" in str(err), err
    assert np.array_equal(got["kf_mp"], ch["kf_mp"]) and np.array_equal(got["n_obs"], S["n_obs"])
    assert (got["match_kp"] == -1).all() and (got["outcome"] == 0).all() and (got["usable"] == 1).all()


def test_host_validation_runs_in_front_of_the_device(ctx):
    S = R.gpu_scene("small")
    mi = S["mp_index"].copy()
    mi[S["first"] + 2] = S["n_mp"]
    res, err, got = run(ctx, S, mp_index=mi)
    assert res is None and "entry %d is row %d outside [0, %d)" % (S["first"] + 2, S["n_mp"], S["n_mp"]) in str(err)
    assert np.array_equal(got["kf_mp"], S["kf_mp"]) and (got["match_kp"] == 12345).all()


def test_two_calls_give_the_same_bits_and_the_workspace_only_grows(ctx):
    allocs = mi355slam.lib().ms_debug_host_allocs
    allocs.restype = C.c_longlong
    big, small = R.gpu_scene("kp1100"), R.gpu_scene("small")
    ra, _, a = run(ctx, big)
    before = allocs()
    rb, _, b = run(ctx, big)
    rs, err, s = run(ctx, small)                             # and a smaller one
    assert allocs() == before
    assert err is None
    assert_same(small, rs, s)
    for name in ("kf_mp", "n_obs", "skip") + OUTPUTS:
        assert np.array_equal(a[name], b[name]), name
    assert ra.n_matched == rb.n_matched and np.array_equal(ra.counts, rb.counts)


def test_the_whole_chain_on_real_geometry(ctx):
    """ms_bound_mask -> ms_project_gate -> ms_projection_topk -> ms_search_bind with everything staying on the device, against
    search_by_projection of project_gate_ref; then ms_unbound_mask of K against the keypoints that are bound now."""
    sc, kfh, S = R.matcher_scene()
    t, view, n_kp, n_mp, K = sc["table"], sc["views"][0], S["n_kp"], S["n_mp"], S["slot"]
    table = mi355slam.MapPointTable(ctx, t["pos"], t["norm"], t["min_dist"], t["max_dist"], t["desc"])
    kf = mi355slam.ProjectionKeyframe(ctx, kfh["x"], kfh["y"], kfh["desc"], kfh["octave"])
    kt = mi355slam.KeyframeTable(ctx, S["kf_mp"])
    skip = Dev(ctx, np.full(n_kp, 0x77, np.uint8))
    kt.bound_mask(K, n_kp, n_mp, skip.buf)
    out, n_kept, V = mi355slam.project_gate_device(ctx, table, [view], sc["sf"], sc["scale_factor"], per_entry=False)
    nq, ne = int(n_kept[0]), len(view["indices"])
    ti, td, to, ns = ctx.alloc(16 * nq + 16), ctx.alloc(8 * nq + 16), ctx.alloc(16 * nq + 16), ctx.alloc(4 * nq + 16)
    vp = mi355slam._vp
    ctx.check(mi355slam.lib().ms_projection_topk(ctx._h, vp(kf.d_sx), vp(kf.d_sy), vp(kf.d_si), kf.n, vp(kf.d_desc), vp(kf.d_oct), vp(skip.buf), vp(out["q_x"]),
                                                 vp(out["q_y"]), vp(out["q_radius"]), vp(out["q_min_octave"]), vp(out["q_max_octave"]), vp(out["q_desc"]), nq,
                                                 vp(ti), vp(td), vp(to), vp(ns), None), "ms_projection_topk")
    live, n_obs = Dev(ctx, S["mp_live"]), Dev(ctx, S["n_obs"])
    match_kp, outcome, usable = Dev(ctx, np.full(ne, 12345, np.int32)), Dev(ctx, np.full(ne, 0x77, np.uint8)), Dev(ctx, (1 - S["bound"]).astype(np.uint8))
    res = kt.search_bind(mi355slam.SearchBindArgs(mp_live=live.buf, n_obs=n_obs.buf, n_mp=n_mp, kept_entry=out["kept_entry"], q_x=out["q_x"], q_y=out["q_y"],
                                                  q_radius=out["q_radius"], q_min_octave=out["q_min_octave"], q_max_octave=out["q_max_octave"], q_desc=out["q_desc"],
                                                  top_idx=ti, top_dist=td, top_octave=to, n_scored=ns, skip=skip.buf, kf=kf, mp_index=view["indices"], first=0,
                                                  count=ne, n_kept=nq, slot=K, match_kp=match_kp.buf, outcome=outcome.buf, usable=usable.buf))
    bound = S["bound"].copy()
    want = G.search_by_projection(kfh, bound, t, view, sc["sf"], sc["scale_factor"])
    m = match_kp.get()
    assert [(int(e), int(m[e])) for e in sc["ref"][0]["kept"] if m[e] >= 0] == want and res.n_matched == len(want) >= 50
    w = R.tables(S)
    assert nq == S["n_kept"] and np.array_equal(kt.download(), w["kf_mp"]) and np.array_equal(n_obs.get(), w["n_obs"]) and np.array_equal(m, w["match_kp"])
    assert np.array_equal(outcome.get(), w["outcome"]) and np.array_equal(res.counts, w["counts"])
    mask = Dev(ctx, np.full(n_kp, 0x77, np.uint8))
    kt.unbound_mask([K], [n_kp], n_mp, [mask.buf])
    assert np.array_equal(mask.get(), 1 - bound) and np.array_equal(usable.get(), 1 - bound)
    for b in [skip, live, n_obs, match_kp, outcome, usable, mask, ti, td, to, ns, kt.kf_mp] + list(out.values()):
        b.free()

