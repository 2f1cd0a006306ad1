"""ms_observation_count and ms_map_cull on the device against tests/map_cull_ref.py, their specification.  Integer work and one
float64 subtraction: every comparison is exact equality.  Out-of-range entries here are n_mp and n_mp + 1 only (besides -1)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import map_cull_ref as R
import mi355slam

pytestmark = pytest.mark.gpu

SCENE = R.make_scene()
N_KF, STRIDE, N_MP = SCENE["kf_mp"].shape + (SCENE["n_mp"],)
WANT = {}                                                    # settings -> the restatement on the scene, computed once


def want(s, n_cand=None):
    key = (tuple(sorted(s.items())), n_cand)
    if key not in WANT:
        WANT[key] = R.run_scene(SCENE, s, n_cand)
    return WANT[key]


def run(ctx, kf_mp, flags, live, n_mp, kf_id, kf_t, cand, keep, s, **kw):
    """One cull on a fresh table; returns the result dict with the table downloaded into it."""
    t = mi355slam.KeyframeTable(ctx, kf_mp)
    try:
        out = t.cull(flags, live, n_mp, kf_id, kf_t, cand, keep, s, **kw)
        out["kf_mp"] = t.download() if len(kf_mp) else np.zeros(kf_mp.shape, np.int32)
    finally:
        t.kf_mp.free()
    return out


def run_scene(ctx, s, n_cand=None, with_flags=True, **kw):
    n = len(SCENE["cand"]) if n_cand is None else n_cand
    return run(ctx, SCENE["kf_mp"], SCENE["mp_flags"] if with_flags else None, SCENE["mp_live"], N_MP, SCENE["kf_id"], SCENE["kf_t"], SCENE["cand"][:n],
               SCENE["cand_keep"][:n], s, **kw)


def assert_same_cull(got, w):
    assert np.array_equal(got["cand_removed"], w["cand_removed"]) and got["n_removed_kf"] == w["n_removed_kf"]
    assert got["removed_rows"].dtype == np.int32 and np.array_equal(got["removed_rows"], w["removed_rows"])      # n_removed_rows is its length
    if got["removed_why"] is not None:
        assert np.array_equal(got["removed_why"], w["removed_why"])
    assert np.array_equal(got["kf_mp"], w["kf_mp"])
    assert np.array_equal(got["mp_live"], w["mp_live"])
    if w["mp_flags"] is not None:
        assert np.array_equal(got["mp_flags"], w["mp_flags"])
    if got["n_obs"] is not None:
        assert np.array_equal(got["n_obs"], w["n_obs"])


def test_scene_counts(ctx):
    t = mi355slam.KeyframeTable(ctx, SCENE["kf_mp"])
    w = R.observation_count(SCENE["kf_mp"], N_MP, SCENE["kf_id"])
    got = t.observation_count(SCENE["kf_id"], N_MP)
    for g, x in zip(got, w):
        assert g.dtype == np.int32 and np.array_equal(g, x)
    assert got[0].max() >= 8 and (got[0] == 0).sum() >= 40 and (got[1] != got[2]).any()
    for left_out in range(3):                                # each optional output left out once
        flags = [i != left_out for i in range(3)]
        part = t.observation_count(SCENE["kf_id"], N_MP, *flags)
        for i in range(3):
            assert (part[i] is None) if i == left_out else np.array_equal(part[i], w[i])
    assert np.array_equal(t.download(), SCENE["kf_mp"])      # the table is only read
    t.kf_mp.free()


@pytest.mark.parametrize("ratio_float32", (0, 1))
@pytest.mark.parametrize("cull_points", (0, 1))
def test_scene_cull(ctx, cull_points, ratio_float32):
    s = R.scene_settings(cull_points, ratio_float32)
    w = want(s)
    got = run_scene(ctx, s)
    assert_same_cull(got, w)
    assert got["n_removed_kf"] >= 1 and len(got["removed_rows"]) >= 5
    if cull_points == 0:                                     # the flags are optional then
        assert_same_cull(dict(run_scene(ctx, s, with_flags=False), mp_flags=None), dict(w, mp_flags=None))


def test_scene_cull_where_float32_decides_otherwise(ctx):
    a, b = R.find_ratio_pair(SCENE, R.scene_settings())
    wa, wb = want(a), want(b)
    assert not np.array_equal(wa["cand_removed"], wb["cand_removed"])
    assert_same_cull(run_scene(ctx, a), wa)
    assert_same_cull(run_scene(ctx, b), wb)


def test_scene_cull_without_candidates_and_without_optional_outputs(ctx):
    s = R.scene_settings()
    got = run_scene(ctx, s, n_cand=0)
    assert_same_cull(got, want(s, 0))
    assert got["n_removed_kf"] == 0 and len(got["cand_removed"]) == 0 and set(got["removed_why"].tolist()) == {R.EMPTY, R.AGED}
    bare = run_scene(ctx, s, want_n_obs=False, want_why=False)
    assert bare["n_obs"] is None and bare["removed_why"] is None
    assert_same_cull(bare, want(s))


def random_case(rng, n_kf, stride, n_mp):
    """Entries drawn from -1, the valid rows and the two out-of-range values n_mp, n_mp + 1; rows may repeat within a slot; candidates in
    shuffled order."""
    kf_mp = rng.integers(-1, n_mp + 2, (n_kf, stride)).astype(np.int32)
    kf_mp[rng.random((n_kf, stride)) < 0.3] = -1
    kf_id = rng.permutation(3 * n_kf)[:n_kf].astype(np.int32)
    kf_id[rng.random(n_kf) < 0.1] = -1
    current = int(rng.integers(0, n_kf))
    kf_id[current] = 3 * n_kf
    kf_t = np.round(rng.normal(0, 8, n_kf), 2)
    others = [k for k in range(n_kf) if k != current and kf_id[k] >= 0]
    cand = rng.permutation(others)[:min(len(others), 20)].astype(np.int32)
    keep = (rng.random(len(cand)) < 0.2).astype(np.uint8)
    flags = rng.integers(0, 4, n_mp).astype(np.uint8)
    live = ((rng.random(n_mp) < 0.85) * rng.integers(1, 256, n_mp)).astype(np.uint8)
    return kf_mp, flags, live, kf_id, kf_t, cand, keep, current


# one entry, one row; a stride beyond two trips of the walk's 1024 lanes; rows and slots at the edge of a wave and a block; one more than those;
# and no rows at all
SHAPES = [(1, 1, 1), (3, 2049, 300), (65, 64, 256), (64, 257, 1025), (7, 33, 0)]


@pytest.mark.parametrize("n_kf,stride,n_mp", SHAPES)
def test_random_tables(ctx, n_kf, stride, n_mp):
    rng = np.random.default_rng(1000 * n_kf + stride + n_mp)
    kf_mp, flags, live, kf_id, kf_t, cand, keep, current = random_case(rng, n_kf, stride, n_mp)
    t = mi355slam.KeyframeTable(ctx, kf_mp)
    for g, x in zip(t.observation_count(kf_id, n_mp), R.observation_count(kf_mp, n_mp, kf_id)):
        assert np.array_equal(g, x)
    t.kf_mp.free()
    # a stride of 2049 with 300 rows lists every row many times: the thresholds follow the counts so that both outcomes occur
    typical = int(np.median(R.observation_count(kf_mp, n_mp, kf_id)[0])) if n_mp else 0
    removed = 0
    for ratio_float32, ratio in ((0, 0.5), (1, 0.7)):
        s = R.settings(current, 1, min_age=2.0, min_obs_for_ba=typical, max_critical_ratio=ratio, ratio_float32=ratio_float32)
        w = R.map_cull(kf_mp, flags, live, n_mp, kf_id, kf_t, cand, keep, s)
        got = run(ctx, kf_mp, flags, live, n_mp, kf_id, kf_t, cand, keep, s)
        assert_same_cull(got, w)
        # rows and slots not named by the result are byte-identical to the input
        rows = np.zeros(n_mp, bool)
        rows[got["removed_rows"]] = True
        assert np.array_equal(got["mp_live"][~rows], live[~rows]) and np.array_equal(got["mp_flags"][~rows], flags[~rows])
        slots = np.zeros(n_kf, bool)
        slots[cand[got["cand_removed"] != 0]] = True
        untouched = ~np.append(rows, [False, False])[np.where(kf_mp >= 0, kf_mp, n_mp)] & ~slots[:, None]
        assert np.array_equal(got["kf_mp"][untouched], kf_mp[untouched])
        removed += got["n_removed_kf"]
    if n_mp >= 256:
        assert removed >= 1


def test_same_bits_on_a_second_run_and_a_small_call_after_the_scene(ctx):
    s = R.scene_settings()
    first, second = run_scene(ctx, s), run_scene(ctx, s)
    for key in ("kf_mp", "mp_live", "mp_flags", "n_obs", "removed_rows", "removed_why", "cand_removed"):
        assert first[key].tobytes() == second[key].tobytes(), key
    assert_same_cull(second, want(s))
    # two slots, five rows: positions the scene call marked must not show
    kf_mp = np.array([[0, 1, 4], [1, -1, 5]], np.int32)
    flags, live = np.array([0, 0, 1, 0, 0], np.uint8), np.array([1, 1, 1, 1, 0], np.uint8)
    kf_id, kf_t = np.array([7, 3], np.int32), np.array([10.0, 2.0])
    for cur, cand in ((0, [1]), (1, [0])):
        s2 = R.settings(cur, 1, min_age=1.0, min_obs_for_ba=1, max_critical_ratio=0.75)
        w = R.map_cull(kf_mp, flags, live, 5, kf_id, kf_t, cand, None, s2)
        assert_same_cull(run(ctx, kf_mp, flags, live, 5, kf_id, kf_t, cand, None, s2), w)
    t = mi355slam.KeyframeTable(ctx, kf_mp)
    for g, x in zip(t.observation_count(kf_id, 5), R.observation_count(kf_mp, 5, kf_id)):
        assert np.array_equal(g, x)
    t.kf_mp.free()


def test_invalid_and_capacity_are_errors_and_nothing_is_written(ctx):
    t = mi355slam.KeyframeTable(ctx, SCENE["kf_mp"])
    flags, live = ctx.upload(SCENE["mp_flags"]), ctx.upload(SCENE["mp_live"])
    d_rows = ctx.alloc(4 * N_MP)
    s = R.scene_settings()
    args = lambda **kw: dict(dict(kf_id=SCENE["kf_id"], kf_t=SCENE["kf_t"], cand=SCENE["cand"], s=s), **kw)
    bad_id = SCENE["kf_id"].copy(); bad_id[3] = bad_id[4]
    bad_t = SCENE["kf_t"].copy(); bad_t[7] = np.inf
    for a in (args(cand=[R.CURRENT]), args(cand=[30, 30]), args(cand=[13]), args(cand=[N_KF]), args(kf_id=bad_id), args(kf_t=bad_t),
              args(s=dict(s, current_slot=13)), args(s=dict(s, min_age=float("nan"))), args(s=dict(s, min_obs_for_ba=-1))):
        with pytest.raises(mi355slam.MsError, match="map cull"):
            t.cull_device(flags, live, N_MP, a["kf_id"], a["kf_t"], a["cand"], None, a["s"], None, d_rows, None)
    with pytest.raises(mi355slam.MsError, match="no mp_flags"):
        t.cull_device(None, live, N_MP, SCENE["kf_id"], SCENE["kf_t"], SCENE["cand"], None, s, None, d_rows, None)
    with pytest.raises(mi355slam.MsError, match="caps"):
        t.cull_device(flags, live, 1 << 24, SCENE["kf_id"], SCENE["kf_t"], SCENE["cand"], None, s, None, d_rows, None)
    with pytest.raises(mi355slam.MsError, match="listed twice"):
        t.observation_count(bad_id, N_MP)
    assert np.array_equal(t.download(), SCENE["kf_mp"]) and np.array_equal(live.download(), SCENE["mp_live"]) and np.array_equal(flags.download(), SCENE["mp_flags"])
    for b in (flags, live, d_rows, t.kf_mp):
        b.free()


def test_workspace_only_grows(ctx):
    allocs = mi355slam.lib().ms_debug_host_allocs
    allocs.restype = C.c_longlong
    s = R.scene_settings()
    t = mi355slam.KeyframeTable(ctx, SCENE["kf_mp"])
    run_scene(ctx, s)                                        # the first of two equal calls
    t.observation_count(SCENE["kf_id"], N_MP)
    before = allocs()
    run_scene(ctx, s)
    t.observation_count(SCENE["kf_id"], N_MP)
    run_scene(ctx, s, n_cand=3, want_n_obs=False)            # and smaller ones
    assert allocs() == before
    t.kf_mp.free()


def test_mirror_smoke_on_the_device():
    import test_map_cull_abi
    out = subprocess.check_output([test_map_cull_abi.build_smoke(), "--gpu"], text=True)
    for line in ("cullMap ok ratioFloat32 0", "cullMap ok ratioFloat32 1", "chain ok ratioFloat32 0", "chain ok ratioFloat32 1", "observationCounts ok"):
        assert line in out, out
