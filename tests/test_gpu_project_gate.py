"""ms_project_gate on the device against tests/project_gate_ref.py, its specification.

status, x, y, dist, the kept order and n_kept are bit-equal to the restatement everywhere; level and radius are bit-equal outside near_level
(entries whose quotient log(ratio) / log(scale_factor) lies within 1e-5 of an integer, where two conforming logf may disagree); inside it the
level is a neighbour and the radius is the formula at the level returned.  tests/test_project_gate_ref.py holds near_level under 0.1 % of
every draw used here."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import mi355slam
import project_gate_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
U32 = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
DRAWS = R.gpu_test_draws()


def scene_of(draw):
    seed, counts, modes, special = draw
    sc = R.make_views(np.random.default_rng(seed), counts, modes, special=special)
    assert np.array_equal(sc["sf"], mi355slam.scale_factors(8, 1.2))
    return sc


def upload(ctx, t):
    return mi355slam.MapPointTable(ctx, t["pos"], t["norm"], t["min_dist"], t["max_dist"], t["desc"])


def check(sc, entries, per_view):
    ref, near = sc["ref"], sc["near_level"]
    cat = lambda k, dt: np.concatenate([r[k] for r in ref] + [np.zeros(0, dt)])
    assert np.array_equal(entries["status"], cat("status", np.uint8))
    for k in ("x", "y", "dist"):
        assert np.array_equal(U32(entries[k]), U32(cat(k, F))), k
    lv, rad = cat("level", np.int32), cat("radius", F)
    assert np.array_equal(entries["level"][~near], lv[~near]) and np.array_equal(U32(entries["radius"][~near]), U32(rad[~near]))
    assert (np.abs(entries["level"][near] - lv[near]) <= 1).all()
    at = 0
    for v, (r, view, got) in enumerate(zip(ref, sc["views"], per_view)):
        n = len(view["indices"])
        e = {k: a[at:at + n] for k, a in entries.items()}
        nr = r["near_level"]
        if nr.any():                                           # the radius is the formula at the level returned
            want = R.radius_of(view["mode"], e["level"][nr], view["threshold"], r["cos"][nr], sc["sf"]).astype(F)
            assert np.array_equal(U32(e["radius"][nr]), U32(want))
        k = r["kept"]
        assert np.array_equal(got["kept"], k), v
        assert np.array_equal(U32(got["q_x"]), U32(e["x"][k])) and np.array_equal(U32(got["q_y"]), U32(e["y"][k])) and np.array_equal(U32(got["q_radius"]), U32(e["radius"][k]))
        assert np.array_equal(got["q_desc"], sc["table"]["desc"][np.asarray(view["indices"])[k]])
        if view["mode"] == R.SIM3:
            assert np.array_equal(got["q_min_octave"], e["level"][k] - 1) and np.array_equal(got["q_max_octave"], e["level"][k])
        else:
            assert (got["q_min_octave"] == R.NO_WINDOW[0]).all() and (got["q_max_octave"] == R.NO_WINDOW[1]).all()
        at += n


@pytest.mark.parametrize("draw", DRAWS, ids=["seed%d" % d[0] for d in DRAWS])
def test_gates_equal_the_restatement(ctx, draw):
    sc = scene_of(draw)
    table = upload(ctx, sc["table"])
    entries, per_view = mi355slam.project_gate(ctx, table, sc["views"], sc["sf"], 1.2)
    check(sc, entries, per_view)


def edge_scene():
    """Constructed points (identity pose, camera centre at the origin, fx = fy = 320 so that x / z = -1 lands on u = 0 exactly), every mode."""
    cam = (320.0, 320.0, 320.0, 240.0, 640, 480)
    below = None
    for k in range(1, 16):                                     # x / z just below 1 whose u is the largest double below the width
        if 320.0 * (1.0 - k * 2.0 ** -53) + 320.0 == np.nextafter(640.0, 0.0):
            below = 1.0 - k * 2.0 ** -53
            break
    assert below is not None
    c998 = F(0.998)
    rows = [  # pos, norm, min, max
        ((0, 0, 0), (0, 0, -1), 0, 9), ((0, 0, -4), (0, 0, -1), 0, 9),                       # z = 0, z < 0
        ((-4, 0, 4), (1, 0, -1), 0, 9), ((4 * below, 0, 4), (-1, 0, -1), 0, 9), ((4, 0, 4), (-1, 0, -1), 0, 9),    # u = 0, just below the width, = width
        ((0, 0, 4), (0, 0, -1), 4, 9), ((0, 0, 4), (0, 0, -1), 1, 4),                        # dist = min, dist = max
        ((0, 0, 4), (0, 0, -1), float(np.nextafter(F(4), F(5))), 9), ((0, 0, 4), (0, 0, -1), 1, float(np.nextafter(F(4), F(0)))),
        ((0, 0, 4), (np.sqrt(0.75), 0, -0.5), 1, 9),                                         # cosine exactly at the limit
        ((0, 0, 4), (np.sqrt(0.75), 0, float(np.nextafter(F(-0.5), F(0)))), 1, 9),
        ((0, 0, 4), (0, 0, -float(c998)), 1, 9), ((0, 0, 4), (0, 0, -float(np.nextafter(c998, F(1)))), 1, 9),     # around 0.998f
        ((0, 0, 4), (0, 0, -float(np.nextafter(c998, F(0)))), 1, 9),
        ((0, 0, 4), (0, 0, 0), 1, 9),                                                        # zero normal
        ((0, 0, 4), (0, 0, -1), 1, 4), ((0, 0, 4), (0, 0, -1), 1, 4 * 1.2 ** 7.5), ((0, 0, 4), (0, 0, -1), 1, 4 * 1.2 ** 30), ((0, 0, 4), (0, 0, -1), 1, np.inf),   # level clamps
        ((0, 0, 1e-60), (0, 0, -1), 0, 1), ((0, 0, 1e-60), (0, 0, -1), 0, 0),                # dist = 0: ratio +inf, ratio NaN
        ((np.nan, 0, 4), (0, 0, -1), 0, 9), ((0, 0, np.inf), (0, 0, -1), 0, np.inf), ((np.inf, 0, 4), (0, 0, -1), 0, 9), ((0, 0, 1e300), (0, 0, -1), 0, np.inf),
        ((0, 0, 4), (np.nan, 0, -1), 1, 9),
    ]
    t = dict(pos=np.array([r[0] for r in rows], np.float64), norm=np.array([r[1] for r in rows], F), min_dist=np.array([r[2] for r in rows], F),
             max_dist=np.array([r[3] for r in rows], F), desc=np.arange(8 * len(rows), dtype=np.uint32).reshape(-1, 8))
    views = [dict(R=np.eye(3), t=np.zeros(3), cam=cam, threshold=10.0, view_cos_limit=0.5, mode=m, indices=np.arange(len(rows), dtype=np.int32))
             for m in (R.SEARCH, R.FUSE, R.SIM3)]
    return R.regate(dict(table=t, views=views, sf=R.scale_factors(8, 1.2), scale_factor=1.2))


def test_constructed_edge_points(ctx):
    sc = edge_scene()
    # what the restatement says about them, spelled out: rows 0-4 visibility, 5-8 distance bounds, 9-10 the cosine limit, 11-13 around 0.998f,
    # 14 zero normal, 15-18 level clamps, 19-20 dist = 0, 21-24 non-finite positions, 25 a NaN normal (no comparison rejects it)
    want = {R.SEARCH: [1, 1, 0, 0, 1, 0, 0, 2, 2, 0, 4, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0],
            R.FUSE: [1, 1, 0, 0, 1, 0, 0, 2, 2, 0, 4, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0],
            R.SIM3: [1, 1, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 1, 1, 1, 0, 0]}
    for r, view in zip(sc["ref"], sc["views"]):
        assert r["status"].tolist() == want[view["mode"]]
        assert r["level"][15:20].tolist() == [0, 7, 7, 7, 7] and r["dist"][19] == 0
    search = sc["ref"][0]
    assert search["level"][20] == 0 and search["dist"][20] == 0                         # ratio 0 / 0
    assert search["radius"][12] == F(0.625) * search["radius"][11] and search["radius"][11] == search["radius"][13]      # only above 0.998f
    entries, per_view = mi355slam.project_gate(ctx, upload(ctx, sc["table"]), sc["views"], sc["sf"], 1.2)
    check(sc, entries, per_view)
    # a scale factor below 1 turns every quotient negative: the lower clamp
    low = R.regate(dict(sc, sf=R.scale_factors(8, 0.8), scale_factor=0.8))
    assert all((r["level"][r["kept"]] == 0).all() for r in low["ref"])
    check(low, *mi355slam.project_gate(ctx, upload(ctx, low["table"]), low["views"], low["sf"], 0.8))


def test_batch_position_and_repeat(ctx):
    sc = scene_of(DRAWS[-1])                                   # the mixed-mode call
    table = upload(ctx, sc["table"])
    e1, v1 = mi355slam.project_gate(ctx, table, sc["views"], sc["sf"], 1.2)
    before = mi355slam.lib().ms_debug_host_allocs()
    e2, v2 = mi355slam.project_gate(ctx, table, sc["views"], sc["sf"], 1.2)
    assert mi355slam.lib().ms_debug_host_allocs() == before
    same = lambda a, b: all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)
    assert same(e1, e2) and all(same(a, b) for a, b in zip(v1, v2))
    at = 0
    order = [3, 5, 0, 1, 4, 2]                                  # every view alone, and the batch in another order
    eo, vo = mi355slam.project_gate(ctx, table, [sc["views"][i] for i in order], sc["sf"], 1.2)
    starts = np.cumsum([0] + [len(sc["views"][i]["indices"]) for i in order])
    for v, view in enumerate(sc["views"]):
        n = len(view["indices"])
        ea, va = mi355slam.project_gate(ctx, table, [view], sc["sf"], 1.2)
        o = starts[order.index(v)]
        for k in e1:
            assert np.array_equal(ea[k].view(np.uint8), e1[k][at:at + n].view(np.uint8)) and np.array_equal(eo[k][o:o + n].view(np.uint8), ea[k].view(np.uint8))
        assert same(va[0], v1[v]) and same(vo[order.index(v)], v1[v])
        at += n


def test_table_update_reuploads_a_range(ctx):
    sc = scene_of(DRAWS[8])                                    # SEARCH, 1000 entries
    t = sc["table"]
    table = upload(ctx, dict(t, pos=np.zeros_like(t["pos"]), max_dist=np.zeros_like(t["max_dist"])))
    table.update(0, 700, pos=t["pos"][:700], max_dist=t["max_dist"][:700])
    table.update(700, table.n - 700, pos=t["pos"][700:], max_dist=t["max_dist"][700:])
    check(sc, *mi355slam.project_gate(ctx, table, sc["views"], sc["sf"], 1.2))


def raw_call(ctx, table, V, idx, n_views, sf, scale_factor, n_levels=None, n_mp=None):
    """ms_project_gate with sentinel-filled outputs: (rc, True when no output byte and no n_kept entry changed)."""
    ne = len(idx)
    sizes = [ne, 4 * ne, 4 * ne, 4 * ne, 4 * ne, 4 * ne, 4 * ne, 4 * ne, 4 * ne, 4 * ne, 4 * ne, 4 * ne, 32 * ne]
    bufs = [ctx.upload(np.full(n + 16, 0xA5, np.uint8)) for n in sizes]
    n_kept = np.full(max(n_views, 1), -77, np.int32)
    sf = np.ascontiguousarray(sf, F)
    vp = mi355slam._vp
    rc = mi355slam.lib().ms_project_gate(ctx._h, vp(table.pos), vp(table.norm), vp(table.min_dist), vp(table.max_dist), vp(table.desc), table.n if n_mp is None else n_mp,
                                         vp(idx), ne, V, n_views, vp(sf), len(sf) if n_levels is None else n_levels, C.c_float(scale_factor), *[vp(b) for b in bufs], vp(n_kept))
    ctx.sync()
    clean = all((b.download(np.uint8, (b.nbytes,)) == 0xA5).all() for b in bufs) and (n_kept == -77).all()
    return rc, clean


def test_bad_arguments_are_rejected_with_nothing_written(ctx):
    sc = scene_of(DRAWS[-1])
    table = upload(ctx, sc["table"])
    pack = lambda: mi355slam.gate_views_pack(sc["views"])
    nv = len(sc["views"])
    V, idx = pack()
    assert raw_call(ctx, table, V, idx, nv, sc["sf"], 1.2) == (0, False)                       # the good call writes
    cases = []
    V, idx = pack(); V[3].mode = 3; cases.append(("mode", V, idx, {}))
    V, idx = pack(); V[0].mode = -1; cases.append(("mode", V, idx, {}))
    V, idx = pack(); idx = idx.copy(); idx[700] = table.n; cases.append(("index", V, idx, {}))
    V, idx = pack(); idx = idx.copy(); idx[5] = -1; cases.append(("index", V, idx, {}))
    V, idx = pack(); V[5].count += 1; cases.append(("slice", V, idx, {}))
    V, idx = pack(); V[0].first = -1; cases.append(("slice", V, idx, {}))
    V, idx = pack(); V[2].count = -1; cases.append(("slice", V, idx, {}))
    V, idx = pack(); V[3].first -= 1; cases.append(("overlap", V, idx, {}))
    V, idx = pack(); V[4].cam.width = 0; cases.append(("camera", V, idx, {}))
    V, idx = pack(); V[4].cam.height = -3; cases.append(("camera", V, idx, {}))
    for bad in (0.0, -1.2, 1.0, float("nan")):
        V, idx = pack(); cases.append(("scale factor %r" % bad, V, idx, dict(scale_factor=bad)))
    V, idx = pack(); cases.append(("levels", V, idx, dict(n_levels=0)))
    for what, V, idx, kw in cases:
        rc, clean = raw_call(ctx, table, V, idx, nv, sc["sf"], kw.get("scale_factor", 1.2), n_levels=kw.get("n_levels"))
        assert rc == -1 and clean, what
    V, idx = pack()
    rc, clean = raw_call(ctx, table, V, idx, nv, np.ones(33, F), 1.2)
    assert rc == -4 and clean
    rc, clean = raw_call(ctx, table, (mi355slam.GateViewC * 4097)(), np.zeros(0, np.int32), 4097, sc["sf"], 1.2)
    assert rc == -4 and clean
    # not errors: no entries, no views
    rc, clean = raw_call(ctx, table, (mi355slam.GateViewC * 1)(mi355slam.GateViewC(cam=mi355slam.Pinhole(1, 1, 0, 0, 1, 1))), np.zeros(0, np.int32), 1, sc["sf"], 1.2)
    assert rc == 0 and not clean
    assert raw_call(ctx, table, (mi355slam.GateViewC * 1)(), np.zeros(0, np.int32), 0, sc["sf"], 1.2) == (0, True)


@pytest.fixture(scope="module")
def matcher_scene():
    sc, kfs, bound = R.make_matcher_scene()
    assert np.array_equal(sc["sf"], mi355slam.scale_factors(8, 1.2))
    return sc, kfs, bound


def test_search_by_projection_end_to_end(ctx, matcher_scene):
    sc, kfs, bound0 = matcher_scene
    want_bound = bound0.copy()
    want = R.search_by_projection(kfs[0], want_bound, sc["table"], sc["views"][0], sc["sf"], 1.2)
    kf = mi355slam.ProjectionKeyframe(ctx, kfs[0]["x"], kfs[0]["y"], kfs[0]["desc"], kfs[0]["octave"])
    bound = bound0.copy()
    got = mi355slam.search_by_projection(ctx, kf, upload(ctx, sc["table"]), sc["views"][0], bound, sc["sf"], 1.2)
    assert len(want) > 40 and 120 < bound0.sum() < 180
    assert got == want and np.array_equal(bound, want_bound)


def test_sim3_direction_end_to_end(ctx, matcher_scene):
    sc, kfs, _ = matcher_scene
    want = R.find_matches_transformed(kfs[1], sc["table"], sc["views"][1], sc["sf"], 1.2)
    kf = mi355slam.ProjectionKeyframe(ctx, kfs[1]["x"], kfs[1]["y"], kfs[1]["desc"], kfs[1]["octave"])
    got = mi355slam.find_matches_transformed(ctx, kf, upload(ctx, sc["table"]), sc["views"][1], sc["sf"], 1.2)
    assert (want >= 0).sum() > 40 and np.array_equal(got, want)


def test_mirror_overloads_equal_their_sequential_restatements():
    import test_project_gate_abi
    out = subprocess.run([test_project_gate_abi.build_smoke(), "--gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "gpu ok 4 functions" in out.stdout
