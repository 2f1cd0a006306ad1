"""ms_observation_lists on the device against tests/obs_lists_ref.py, its specification: integer work and copies, so every output
array is compared for exact equality (floats by their bits).  Out-of-range entries: -1, n_mp, n_mp + 1 and INT32_MIN."""
import ctypes as C

import numpy as np
import pytest

import map_refresh_ref as MR
import mi355slam
import obs_lists_ref as R
import test_gpu_triangulate as TT
import triangulate_ref as TR

pytestmark = pytest.mark.gpu

GUARD = 256                                                  # bytes behind every output buffer that no call may touch
ARRAYS = R.ROW_ARRAYS + R.OBS_ARRAYS


class Scene:
    """A scene of the restatement with its tables on the device."""

    def __init__(self, ctx, scene):
        self.ctx, self.s = ctx, scene
        self.table = mi355slam.KeyframeTable(ctx, scene["kf_mp"])
        self.kp = mi355slam.KeypointTable(ctx, **scene["kp"])
        self.flags = ctx.upload(scene["mp_flags"])

    def lists(self, cap_rows, cap_obs):
        L = mi355slam.ObservationLists(self.ctx, cap_rows, cap_obs, guard=GUARD)
        for name, dt in L._ROW + L._OBS:                     # a pattern everywhere: what a call leaves alone shows
            b = L[name]
            pattern = np.full(b.nbytes, 0xA5, np.uint8)      # held until the upload has returned
            self.ctx.check(mi355slam.lib().ms_dev_upload(self.ctx._h, C.c_void_p(b.ptr), mi355slam._vp(pattern), C.c_size_t(b.nbytes)), "ms_dev_upload")
        return L

    def call(self, L, sel, n_levels=R.N_LEVELS, **kw):
        return self.table.observation_lists_device(L, self.s["kf_id"], self.s["n_mp"], sel, self.kp, self.s["desc_base"], self.flags, n_levels, **kw)

    def free(self):
        self.table.kf_mp.free(); self.kp.free(); self.flags.free()


@pytest.fixture(scope="module")
def scene_a(ctx):
    s = Scene(ctx, R.scene_a())
    yield s
    s.free()


@pytest.fixture(scope="module")
def scene_b(ctx):
    s = Scene(ctx, R.scene_b())
    yield s
    s.free()


def guards(L, cap_rows=None, cap_obs=None):
    """The bytes behind the capacities of every buffer."""
    cr, co = L.cap_rows if cap_rows is None else cap_rows, L.cap_obs if cap_obs is None else cap_obs
    out = {}
    for name, dt in L._ROW + L._OBS:
        used = np.dtype(dt).itemsize * (co if (name, dt) in L._OBS else cr + (name == "obs_start"))
        out[name] = L[name].download(np.uint8, (L[name].nbytes,))[used:]
    return out


def assert_guards(L, **kw):
    for name, g in guards(L, **kw).items():
        assert len(g) >= GUARD and (g == 0xA5).all(), name


def assert_same_lists(got, want):
    for name in ARRAYS:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w), name


def check(scene, sel, n_levels=R.N_LEVELS, slack=(3, 5)):
    want = R.run_scene(scene.s, sel, n_levels)
    L = scene.lists(want["n_rows"] + slack[0], want["n_obs"] + slack[1])
    try:
        rc, n_rows, n_obs = scene.call(L, sel, n_levels)
        assert (rc, n_rows, n_obs) == (0, want["n_rows"], want["n_obs"]), mi355slam.lib().ms_last_error(scene.ctx._h)
        assert_same_lists(L.download(n_rows, n_obs), want)
        assert_guards(L)
    finally:
        L.free()
    return want


SELECTIONS_A = [(src, flt, drop) for src in (R.FROM_ROWS, R.FROM_SLOT) for flt in (R.ALL, R.REFRESH, R.RETRIANGULATE) for drop in (0, 1)]


@pytest.mark.parametrize("source,flt,drop", SELECTIONS_A)
def test_scene_a_lists_equal_the_restatement(scene_a, source, flt, drop):
    rng = np.random.default_rng(5)
    n_mp = scene_a.s["n_mp"]
    # every row once in shuffled order, then repeats, and the invalid values in between
    rows_in = np.concatenate([rng.permutation(n_mp), [-1, n_mp, R.INT32_MIN, n_mp + 1], rng.integers(0, n_mp, 200)]).astype(np.int32)
    rows_in = np.insert(rows_in, [10, 500], [n_mp, -1]).astype(np.int32)
    sel = R.select(source, flt, drop, R.A_CURRENT if source == R.FROM_SLOT else -1, rows_in if source == R.FROM_ROWS else None)
    want = check(scene_a, sel)
    if source == R.FROM_ROWS and flt == R.ALL:
        assert want["n_rows"] == (n_mp if not drop else int((want["n_obs_row"] > 0).sum()))
        assert {0, 1, 2, 63, 64, 65} <= set(R.run_scene(scene_a.s, R.select(R.FROM_ROWS, rows_in=rows_in))["n_obs_row"].tolist())
    if source == R.FROM_SLOT and flt == R.ALL:
        assert {1, 2, 63, 64} <= set(want["n_obs_row"].tolist())


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 1003))
def test_row_counts(scene_a, n):
    rows_in = np.random.default_rng(n).permutation(scene_a.s["n_mp"])[:n].astype(np.int32)
    want = check(scene_a, R.select(R.FROM_ROWS, rows_in=rows_in))
    assert want["n_rows"] == n


def test_scene_b_long_lists_and_a_whole_map_selection(scene_b):
    n_mp = scene_b.s["n_mp"]
    want = check(scene_b, R.select(R.FROM_ROWS, rows_in=np.arange(n_mp, dtype=np.int32)))
    assert want["n_rows"] == n_mp > 256 * 256                # the block totals are scanned in more than one trip
    assert {300, 1025, 1100} <= set(want["n_obs_row"].tolist())
    check(scene_b, R.select(R.FROM_ROWS, R.RETRIANGULATE, 1, rows_in=np.arange(n_mp, dtype=np.int32)[::-1]))
    check(scene_b, R.select(R.FROM_SLOT, R.ALL, 0, 17))


def test_same_bytes_on_every_call_and_at_any_capacity(scene_a, scene_b):
    for scene, sel in ((scene_a, R.select(R.FROM_SLOT, R.ALL, 0, R.A_CURRENT)), (scene_b, R.select(R.FROM_ROWS, rows_in=np.arange(4000, dtype=np.int32)))):
        want = R.run_scene(scene.s, sel)
        nr, no = want["n_rows"], want["n_obs"]
        L, big = scene.lists(nr, no), scene.lists(3 * nr + 7, 4 * no + 9)
        first = None
        for lists in (L, L, big):
            assert scene.call(lists, sel) == (0, nr, no)
            got = lists.download(nr, no)
            assert_same_lists(got, want)
            first = first or got
            assert all(got[k].tobytes() == first[k].tobytes() for k in ARRAYS)
            assert_guards(lists)
        L.free(); big.free()


def test_capacity_one_short_reports_the_needed_counts_and_writes_nothing_behind(scene_a):
    sel = R.select(R.FROM_SLOT, R.ALL, 0, R.A_CURRENT)
    want = R.run_scene(scene_a.s, sel)
    nr, no = want["n_rows"], want["n_obs"]
    L = scene_a.lists(nr, no)
    for cr, co in ((nr, no - 1), (nr - 1, no), (0, 0)):
        assert scene_a.call(L, sel, cap_rows=cr, cap_obs=co) == (mi355slam.MS_ERR_CAPACITY, nr, no)
        assert_guards(L, cap_rows=cr, cap_obs=co)
    assert scene_a.call(L, sel) == (0, nr, no)
    assert_same_lists(L.download(nr, no), want)
    L.free()


def test_a_small_call_after_a_large_one_sees_nothing_stale(scene_a, scene_b):
    big = R.select(R.FROM_ROWS, rows_in=np.arange(scene_b.s["n_mp"], dtype=np.int32))
    wb = R.run_scene(scene_b.s, big)
    L = scene_b.lists(wb["n_rows"], wb["n_obs"])
    assert scene_b.call(L, big)[0] == 0
    small = R.select(R.FROM_ROWS, R.ALL, 0, rows_in=np.array([902, 7, 955, 902, 3], np.int32))
    ws = R.run_scene(scene_a.s, small)
    assert scene_a.call(L, small) == (0, ws["n_rows"], ws["n_obs"])
    assert_same_lists(L.download(ws["n_rows"], ws["n_obs"]), ws)
    L.free()


def test_a_slot_that_lists_a_row_twice_selects_it_once(scene_a):
    slot, row = R.A_TWICE
    want = check(scene_a, R.select(R.FROM_SLOT, R.ALL, 0, slot))
    assert (want["rows"] == row).sum() == 1 and (scene_a.s["kf_mp"][slot] == row).sum() == 2


def test_empty_cases_return_zero_counts(ctx, scene_a):
    L = scene_a.lists(4, 4)
    assert scene_a.call(L, R.select(R.FROM_ROWS, rows_in=np.zeros(0, np.int32))) == (0, 0, 0)
    assert scene_a.call(L, R.select(R.FROM_ROWS, rows_in=np.array([-1, scene_a.s["n_mp"]], np.int32))) == (0, 0, 0)
    kf_mp = np.full((3, 5), -1, np.int32)
    t = mi355slam.KeyframeTable(ctx, kf_mp)
    kp = mi355slam.KeypointTable(ctx, *[np.zeros((3, 5), dt) for dt in (np.float32, np.float32, np.int32, np.float32)])
    ids = np.array([4, 2, 9], np.int32)
    assert t.observation_lists_device(L, ids, 10, R.select(R.FROM_SLOT, slot=1), kp, np.zeros(3, np.int32), None) == (0, 0, 0)       # an all-empty slot
    assert t.observation_lists_device(L, ids, 0, R.select(R.FROM_SLOT, slot=1), kp, np.zeros(3, np.int32), None) == (0, 0, 0)        # n_mp = 0
    rc, n_rows, n_obs = t.observation_lists_device(L, ids, 10, R.select(R.FROM_ROWS, rows_in=np.array([3, 3, 1], np.int32)), kp, None, None)
    assert (rc, n_rows, n_obs) == (0, 2, 0)                  # rows without observations are kept unless drop_empty says otherwise
    got = L.download(2, 0, ("rows", "obs_start", "n_obs_row", "first_octave"))
    assert got["rows"].tolist() == [3, 1] and got["obs_start"].tolist() == [0, 0, 0] and got["first_octave"].tolist() == [0, 0]
    assert_guards(L)
    t.kf_mp.free(); kp.free(); L.free()


def test_octave_violation_is_reported_and_stored_in_range(ctx):
    s = R.scene_a()
    s["kp"] = dict(s["kp"], octave=s["kp"]["octave"].copy())
    sel = R.select(R.FROM_SLOT, R.ALL, 0, R.A_CURRENT)
    j = int(np.nonzero(s["kf_mp"][R.A_CURRENT] == 903)[0][0])           # row 903 is observed by the current slot alone: its first observation
    s["kp"]["octave"][R.A_CURRENT, j] = R.N_LEVELS
    want = R.run_scene(s, sel)
    assert want["violations"] == 1 and want["obs_octave"].max() == R.N_LEVELS - 1
    scene = Scene(ctx, s)
    L = scene.lists(want["n_rows"], want["n_obs"])
    rc, n_rows, n_obs = scene.call(L, sel)
    assert (rc, n_rows, n_obs) == (mi355slam.MS_ERR_INVALID, want["n_rows"], want["n_obs"])
    assert b"octave" in mi355slam.lib().ms_last_error(ctx._h)
    got = L.download(n_rows, n_obs)
    assert_same_lists(got, want)                             # complete, with the clamped value
    assert got["obs_octave"].min() >= 0 and got["obs_octave"].max() < R.N_LEVELS and got["first_octave"].max() < R.N_LEVELS
    assert scene.call(L, sel, n_levels=0)[0] == 0            # no levels given: gathered as it is
    assert L.download(n_rows, n_obs)["obs_octave"].max() == R.N_LEVELS
    L.free(); scene.free()


def _allocs():
    f = mi355slam.lib().ms_debug_host_allocs
    f.restype = C.c_longlong
    return f()


def test_workspace_is_flat_over_repeated_calls(scene_a):
    own = mi355slam.Context(0)
    try:
        scene = Scene(own, scene_a.s)
        sel = R.select(R.FROM_ROWS, rows_in=np.arange(scene.s["n_mp"], dtype=np.int32))
        want = R.run_scene(scene.s, sel)
        L = scene.lists(want["n_rows"], want["n_obs"])
        rows_dev = own.upload(sel["rows_in"])
        dsel = dict(sel, rows_in=rows_dev, n_in=len(sel["rows_in"]))
        small = dict(R.select(R.FROM_SLOT, R.REFRESH, 1, R.A_CURRENT))
        rose = []
        for s in (dsel, dsel, small, dsel):
            before = _allocs()
            assert scene.call(L, s)[0] == 0
            rose.append(_allocs() - before)
        print("allocations per call:", rose)
        assert rose[0] >= 1 and rose[1:] == [0, 0, 0]
        rows_dev.free(); L.free(); scene.free()
    finally:
        own.close()


# ---- the consumers: ms_triangulate_lists and ms_map_refresh_lists against ms_triangulate and ms_map_refresh, bit for bit ----

def as_tables(prob, n_kf, per_obs, fill):
    """The CSR lists of a fixture (rows, obs_start, obs_kf; one keyframe may observe a row more than once) re-expressed as kf_mp and tables
    parallel to it: observation o of row r becomes the next free keypoint of slot obs_kf[o], so the (slot, j) order of a row's
    observations is the fixture's order.  per_obs: name -> per-observation array; fill: name -> the value of unused keypoints.
    Returns kf_mp, the tables, and (slot, j) per observation."""
    start, okf = np.asarray(prob["obs_start"]), np.asarray(prob["obs_kf"])
    n_obs = int(start[-1])
    stride = max(int(np.bincount(okf[:n_obs], minlength=n_kf).max()), 1)
    kf_mp = np.full((n_kf, stride), -1, np.int32)
    tables = {k: np.full((n_kf, stride), fill[k], np.asarray(v).dtype) for k, v in per_obs.items()}
    used, js = np.zeros(n_kf, np.int64), np.zeros(n_obs, np.int64)
    row_of = np.repeat(np.asarray(prob["rows"]), np.diff(start))
    for o in range(n_obs):
        k = okf[o]
        js[o] = used[k]
        used[k] += 1
    kf_mp[okf[:n_obs], js] = row_of
    for name, v in per_obs.items():
        tables[name][okf[:n_obs], js] = np.asarray(v)[:n_obs]
    return kf_mp, tables, js


def bits(a):
    return a.tobytes()


@pytest.fixture(scope="module")
def tri_setup(ctx):
    """The triangulation fixture as device tables, its lists built on the device, and the entry state of positions and flags."""
    want = TR.fixture(TR.TME, True)
    sc, prob = want["scene"], want["prob"]
    n_kf, n_mp = len(sc["poses"]), TR.N_MP
    kf_mp, tables, _ = as_tables(prob, n_kf, dict(x=prob["obs_x"], y=prob["obs_y"], octave=prob["obs_octave"], depth=prob["obs_depth"]),
                                 dict(x=0.0, y=0.0, octave=0, depth=-1.0))
    flags_in = sc["mp_flags"].copy()
    flags_in[prob["rows"]] = (flags_in[prob["rows"]] & 1) | (prob["was_triangulated"] << 1)       # bit 1 = the fixture's was_triangulated
    table = mi355slam.KeyframeTable(ctx, kf_mp)
    kp = mi355slam.KeypointTable(ctx, tables["x"], tables["y"], tables["octave"], tables["depth"])
    d_flags = ctx.upload(flags_in)
    lists, n_rows, n_obs = table.observation_lists(np.arange(n_kf, dtype=np.int32), n_mp, R.select(R.FROM_ROWS, rows_in=prob["rows"]), kp, None, d_flags, 8)
    got = lists.download(n_rows, n_obs)
    for a, b in (("rows", "rows"), ("obs_start", "obs_start"), ("was_triangulated", "was_triangulated"), ("obs_kf", "obs_kf"), ("obs_x", "obs_x"), ("obs_y", "obs_y"),
                 ("obs_octave", "obs_octave"), ("obs_depth", "obs_depth")):
        assert bits(got[a]) == bits(np.ascontiguousarray(prob[b])), a        # the device lists ARE the fixture's lists
    dev = TT.Device(ctx)
    yield dict(want=want, sc=sc, lists=lists, n_rows=n_rows, n_obs=n_obs, got=got, dev=dev, flags_in=flags_in, d_flags=d_flags)
    lists.free(); table.kf_mp.free(); kp.free(); d_flags.free()
    del dev


@pytest.mark.parametrize("with_depth", (True, False))
@pytest.mark.parametrize("mode", (TR.TME, TR.MIDPOINT, TR.FIRST_LAST))
def test_triangulate_lists_equals_triangulate_bit_for_bit(ctx, tri_setup, mode, with_depth):
    T = tri_setup
    sc, dev, got = T["sc"], T["dev"], T["got"]
    S = TR.settings()
    prob = {k: got[k] for k in ("rows", "was_triangulated", "obs_start", "obs_kf", "obs_x", "obs_y", "obs_octave")}
    prob["obs_depth"] = got["obs_depth"] if with_depth else None
    results = []
    for path in ("host", "device"):
        dev.table.update(0, TR.N_MP, pos=sc["mp_pos"])
        ctx.check(mi355slam.lib().ms_dev_upload(ctx._h, C.c_void_p(dev.flags.ptr), mi355slam._vp(T["flags_in"]), C.c_size_t(TR.N_MP)), "ms_dev_upload")
        if path == "host":
            out = dev.table.triangulate(dev.poses, sc["cams"], sc["focal"], prob, S, mode, flags=dev.flags)
        else:
            out = dev.table.triangulate_lists(dev.poses, sc["cams"], sc["focal"], T["lists"], T["n_rows"], T["n_obs"], S, mode, flags=dev.flags, with_depth=with_depth)
        results.append(out + (dev.table.pos.download(np.float64, (TR.N_MP, 3)), dev.flags.download(np.uint8, (TR.N_MP,))))
    for a, b in zip(*results):
        assert a.dtype == b.dtype and bits(a) == bits(b)
    status, pos, flags = results[1][0], results[1][3], results[1][4]
    assert len(set(status.tolist())) >= 2                    # points that triangulate and points that do not
    other = np.setdiff1d(np.arange(TR.N_MP), got["rows"])
    assert len(other) and bits(pos[other]) == bits(sc["mp_pos"][other]) and bits(flags[other]) == bits(T["flags_in"][other])


@pytest.fixture(scope="module")
def refresh_setup(ctx):
    """The refresh fixture as device tables (descriptors: a pool laid out slot by slot), its lists on the device."""
    sc = dict(MR.make_refresh_scene())
    rng = np.random.default_rng(77)
    # Two more keyframes, slots 40 and 41, WITHOUT descriptors: they observe entries 20 .. 49 after the fixture's keyframes (rows with and
    # without gaps in their descriptor lists), and slot 40 alone observes one more row (no descriptor at all: medoid -1).  The fixture's 40
    # keyframes all have descriptors, so its lists of 256 and 257 observations stay the largest that fits and the first that does not (-2).
    old = sc["prob"]
    n_kf = len(sc["kf_pose"]) + 2
    sc["kf_pose"] = np.concatenate([sc["kf_pose"], np.stack([MR.random_pose(rng) for _ in range(2)])])
    per_row = [list(old["obs_kf"][a:b]) for a, b in zip(old["obs_start"][:-1], old["obs_start"][1:])]
    for e in range(20, 50):
        per_row[e] += [n_kf - 2] if e < 40 else [n_kf - 2, n_kf - 1]
    per_row.append([n_kf - 2])
    n_mp = len(sc["table"]["pos"])
    extra = int(np.setdiff1d(np.arange(n_mp), old["rows"])[0])
    start = np.zeros(len(per_row) + 1, np.int32)
    start[1:] = np.cumsum([len(l) for l in per_row])
    prob = dict(rows=np.append(old["rows"], extra).astype(np.int32), obs_start=start, obs_kf=np.concatenate(per_row).astype(np.int32),
                first_octave=np.append(old["first_octave"], 3).astype(np.int32))
    src = np.full(int(start[-1]), -1, np.int64)              # the fixture's descriptor index of an observation it has, -1 for the added ones
    for e, (a, b) in enumerate(zip(old["obs_start"][:-1], old["obs_start"][1:])):
        src[start[e]:start[e] + (b - a)] = old["obs_desc"][a:b]
    n_obs = int(prob["obs_start"][-1])
    octave = rng.integers(0, len(sc["sf"]), n_obs).astype(np.int32)
    octave[prob["obs_start"][:-1]] = prob["first_octave"]    # a row's first observation carries the fixture's octave
    kf_mp, tables, js = as_tables(prob, n_kf, dict(octave=octave), dict(octave=0))
    stride = kf_mp.shape[1]
    base = (np.arange(n_kf) * stride).astype(np.int32)
    base[n_kf - 2:] = -1
    pool = rng.integers(0, 2 ** 32, (n_kf * stride, 8), dtype=np.uint64).astype(np.uint32)
    has = src >= 0                                           # the fixture's descriptors where it has some: near-duplicates, so medoids are contested
    pool[np.asarray(prob["obs_kf"])[:n_obs][has] * stride + js[has]] = sc["pool"][src[has]]
    table = mi355slam.KeyframeTable(ctx, kf_mp)
    zeros = np.zeros((n_kf, stride), np.float32)
    kp = mi355slam.KeypointTable(ctx, zeros, zeros, tables["octave"], zeros)
    flags_in = rng.integers(0, 4, n_mp).astype(np.uint8)
    lists, n_rows, n_obs_dev = table.observation_lists(np.arange(n_kf, dtype=np.int32), n_mp, R.select(R.FROM_ROWS, R.ALL, 1, rows_in=prob["rows"]), kp, base, flags_in,
                                                       len(sc["sf"]))
    got = lists.download(n_rows, n_obs_dev)
    for name in ("rows", "obs_start", "obs_kf", "first_octave"):
        assert bits(got[name]) == bits(np.ascontiguousarray(prob[name])), name
    n_desc = np.add.reduceat((got["obs_desc"] >= 0).astype(np.int64), got["obs_start"][:-1])
    assert n_desc.max() > MR.MEDOID_MAX_OBS and (n_desc == 0).any() and ((n_desc > 0) & (n_desc < got["n_obs_row"])).any()     # the -2 and -1 cases, and rows with gaps
    yield dict(sc=sc, lists=lists, n_rows=n_rows, n_obs=n_obs_dev, got=got, pool=pool, flags_in=flags_in, n_mp=n_mp, prob=prob)
    lists.free(); table.kf_mp.free(); kp.free()


def _refresh_state(ctx, T, with_desc, path, promote=0, want_medoid=True):
    sc = T["sc"]
    table = mi355slam.MapPointTable(ctx, **sc["table"])
    poses = mi355slam.KeyframePoseTable(ctx, sc["kf_pose"])
    pool = ctx.upload(T["pool"]) if with_desc else None
    flags = ctx.upload(T["flags_in"])
    if path == "host":
        prob = {k: T["got"][k] for k in ("rows", "obs_start", "obs_kf", "first_octave")}
        prob["obs_desc"] = T["got"]["obs_desc"] if with_desc else None
        medoid = mi355slam.map_refresh(ctx, table, poses, prob, sc["sf"], pool)
    else:
        medoid = table.refresh_lists(poses, T["lists"], T["n_rows"], T["n_obs"], sc["sf"], pool, promote, flags, want_medoid)
    n = T["n_mp"]
    out = dict(medoid=medoid, norm=table.norm.download(np.float32, (n, 3)), min_dist=table.min_dist.download(np.float32, (n,)),
               max_dist=table.max_dist.download(np.float32, (n,)), desc=table.desc.download(np.uint32, (n, 8)), pos=table.pos.download(np.float64, (n, 3)),
               flags=flags.download(np.uint8, (n,)))
    for b in (table.pos, table.norm, table.min_dist, table.max_dist, table.desc, poses.pose, pool, flags):
        if b is not None:
            b.free()
    return out


@pytest.mark.parametrize("with_desc", (True, False))
def test_refresh_lists_equals_map_refresh_bit_for_bit(ctx, refresh_setup, with_desc):
    T = refresh_setup
    host, device = _refresh_state(ctx, T, with_desc, "host"), _refresh_state(ctx, T, with_desc, "device")
    for name in host:
        assert host[name].dtype == device[name].dtype and bits(host[name]) == bits(device[name]), name
    if with_desc:
        assert {-2, -1} <= set(device["medoid"].tolist()) and (device["medoid"] > 0).any()
    else:
        assert (device["medoid"] == -1).all()
    other = np.setdiff1d(np.arange(T["n_mp"]), T["got"]["rows"])
    for name in ("norm", "min_dist", "max_dist", "desc"):
        assert len(other) and bits(device[name][other]) == bits(np.ascontiguousarray(T["sc"]["table"][name])[other]), name
    assert bits(device["flags"]) == bits(T["flags_in"])      # promote_min_obs = 0: untouched
    no_medoid = _refresh_state(ctx, T, with_desc, "device", want_medoid=False)
    assert no_medoid["medoid"] is None and all(bits(no_medoid[k]) == bits(device[k]) for k in device if k != "medoid")


def test_refresh_lists_promotes_the_status(ctx, refresh_setup):
    T = refresh_setup
    plain, promoted = _refresh_state(ctx, T, True, "device"), _refresh_state(ctx, T, True, "device", promote=3)
    want = T["flags_in"].copy()
    want[T["got"]["rows"]] = np.where(T["got"]["n_obs_row"] >= 3, 3, 2)
    assert bits(promoted["flags"]) == bits(want) and {2, 3} <= set(promoted["flags"][T["got"]["rows"]].tolist())
    assert all(bits(plain[k]) == bits(promoted[k]) for k in plain if k != "flags")


def test_consumer_workspaces_are_flat_over_repeated_calls(refresh_setup):
    own = mi355slam.Context(0)
    try:
        sc, prob = refresh_setup["sc"], refresh_setup["prob"]
        n_kf, n_mp = len(sc["kf_pose"]), len(sc["table"]["pos"])
        kf_mp, tables, _ = as_tables(prob, n_kf, dict(octave=np.zeros(int(prob["obs_start"][-1]), np.int32)), dict(octave=0))
        stride = kf_mp.shape[1]
        zeros = np.zeros((n_kf, stride), np.float32)
        table, kp = mi355slam.KeyframeTable(own, kf_mp), mi355slam.KeypointTable(own, zeros + 300, zeros + 200, tables["octave"], zeros - 1)
        mpt, poses = mi355slam.MapPointTable(own, **sc["table"]), mi355slam.KeyframePoseTable(own, sc["kf_pose"])
        pool = own.upload(np.random.default_rng(3).integers(0, 2 ** 32, (n_kf * stride, 8), dtype=np.uint64).astype(np.uint32))
        flags = own.upload(np.zeros(n_mp, np.uint8))
        ids, base = np.arange(n_kf, dtype=np.int32), (np.arange(n_kf) * stride).astype(np.int32)
        cams = np.tile(np.array([500.0, 500.0, 320.0, 240.0, 640, 480]), (n_kf, 1))
        focal = np.full(n_kf, 500, np.int32)
        lists = mi355slam.ObservationLists(own, len(prob["rows"]), int(prob["obs_start"][-1]))
        d_all, d_few = own.upload(prob["rows"]), own.upload(prob["rows"][20:60])
        rose = []
        for d_rows, n_in in ((d_all, len(prob["rows"])), (d_all, len(prob["rows"])), (d_few, 40), (d_all, len(prob["rows"]))):
            before = _allocs()
            rc, n_rows, n_obs = table.observation_lists_device(lists, ids, n_mp, dict(R.select(R.FROM_ROWS, R.ALL, 1), rows_in=d_rows, n_in=n_in), kp, base, flags, 8)
            assert rc == 0 and n_rows == n_in
            mpt.refresh_lists(poses, lists, n_rows, n_obs, sc["sf"], pool, 3, flags)
            mpt.triangulate_lists(poses, cams, focal, lists, n_rows, n_obs, TR.settings(), TR.TME, flags=flags)
            rose.append(_allocs() - before)
        print("allocations per round of three calls:", rose)
        assert rose[0] >= 3 and rose[1:] == [0, 0, 0]
    finally:
        own.close()
