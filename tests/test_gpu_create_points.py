"""ms_create_points_lists, ms_create_points_bind and ms_unbound_mask on the device against tests/create_points_ref.py, their specification
(DESIGN 9.13).  Every comparison is exact equality (floats by their bits): lists, counters, masks and every table, for each entry point
alone against the staged restatement and for the whole chain, after every adjacent keyframe, against the sequential one -- the positions
ms_triangulate_lists writes between the two new kernels included, which the chain test prints the count of before it asserts.  Every output
buffer carries canary bytes behind its end."""
import ctypes as C

import numpy as np
import pytest

import create_points_ref as R
import mi355slam
import triangulate_ref as TR

pytestmark = pytest.mark.gpu
CANARY = 0xA5
N_LEVELS = 8


def put(ctx, buf, arr):
    arr = np.ascontiguousarray(arr)
    ctx.check(mi355slam.lib().ms_dev_upload(ctx._h, C.c_void_p(buf.ptr), mi355slam._vp(arr), C.c_size_t(arr.nbytes)), "ms_dev_upload")


def canary(ctx, nbytes):
    b = ctx.alloc(nbytes + 64)
    put(ctx, b, np.full(b.nbytes, CANARY, np.uint8))
    return b


def untouched_behind(buf, nbytes):
    return bool((buf.download(np.uint8, (buf.nbytes,))[nbytes:] == CANARY).all())


class Device:
    """A scene of the restatement with its tables, masks and matcher frames on the device."""

    def __init__(self, ctx, sc):
        self.ctx, self.sc = ctx, sc
        self.table = mi355slam.MapPointTable(ctx, **sc["table"])
        self.kf = mi355slam.KeyframeTable(ctx, sc["kf_mp"])
        self.kp = mi355slam.KeypointTable(ctx, **sc["kp"])
        self.flags, self.live, self.pool = ctx.upload(sc["mp_flags"]), ctx.upload(sc["mp_live"]), ctx.upload(sc["pool"])
        self.n_obs, self.mp_track = ctx.upload(sc["n_obs"]), ctx.upload(sc["mp_track"])
        self.poses = mi355slam.KeyframePoseTable(ctx, sc["poses"])
        n_mp = len(sc["mp_live"])
        self.frames = {}
        for s in range(len(sc["kf_id"])):
            n = int(sc["n_kp"][s])
            self.frames[s] = mi355slam.FrameOnDevice(ctx, R.descriptors(sc, s), sc["angle"][s, :n], R.unbound_mask(sc["kf_mp"], n_mp, s, n), sc["node"][s, :n],
                                                     octave=sc["kp"]["octave"][s, :n], bearing=R.bearings(sc, s))

    def restore(self, st=None, masks=None):
        """Every table the chain writes, as the state has it (the scene when None); the masks from the state's kf_mp unless given."""
        st = self.sc if st is None else st
        self.table.update(0, self.table.n, **st["table"])
        for buf, a in ((self.kf.kf_mp, st["kf_mp"]), (self.flags, st["mp_flags"]), (self.live, st["mp_live"]), (self.n_obs, st["n_obs"]), (self.mp_track, st["mp_track"])):
            put(self.ctx, buf, a)
        for s, f in self.frames.items():
            put(self.ctx, f.bufs["usable"], R.unbound_mask(st["kf_mp"], self.table.n, s, f.n) if masks is None else masks[s])

    def state(self):
        n = self.table.n
        table = dict(pos=self.table.pos.download(np.float64, (n, 3)), norm=self.table.norm.download(np.float32, (n, 3)), min_dist=self.table.min_dist.download(np.float32, (n,)),
                     max_dist=self.table.max_dist.download(np.float32, (n,)), desc=self.table.desc.download(np.uint32, (n, 8)))
        return dict(kf_mp=self.kf.download(), mp_flags=self.flags.download(np.uint8, (n,)), mp_live=self.live.download(np.uint8, (n,)),
                    n_obs=self.n_obs.download(np.int32, (n,)), mp_track=self.mp_track.download(np.int32, (n,)), table=table)

    def masks(self):
        return {s: f.bufs["usable"].download(np.uint8, (f.n,)) for s, f in self.frames.items()}

    def chain_args(self):
        sc = self.sc
        return (self.table, self.flags, self.live, self.kp, self.pool, self.poses, sc["kf_id"], sc["cams"], sc["focal"], sc["desc_base"])

    def create(self, adjacent, free_rows, **kw):
        sc = self.sc
        return self.kf.create_points(*self.chain_args(), R.CURRENT, adjacent, self.frames, free_rows, sc["S"], sc["sf"], sc["thr_deg"], n_obs=self.n_obs,
                                     mp_track=self.mp_track, pose_host=sc["poses"], **kw)

    def lists_call(self, lists, adj, matched, new_rows, kp1, kp2, desc_base=None, **kw):
        sc = self.sc
        d_matched = self.ctx.upload(matched if len(matched) else np.zeros(1, np.int32))
        try:
            return self.kf.create_points_lists_device(lists, self.live, self.table.n, sc["kf_id"], self.kp, sc["desc_base"] if desc_base is None else desc_base, R.CURRENT,
                                                      adj, d_matched, len(matched), int(sc["n_kp"][adj]), new_rows, N_LEVELS, kp1, kp2, **kw)
        finally:
            d_matched.free()

    def free(self):
        for b in (self.table.pos, self.table.norm, self.table.min_dist, self.table.max_dist, self.table.desc, self.kf.kf_mp, self.flags, self.live, self.pool,
                  self.n_obs, self.mp_track, self.poses.pose):
            b.free()
        self.kp.free()
        for f in self.frames.values():
            for b in f.bufs.values():
                b.free()


@pytest.fixture(scope="module")
def dev(ctx):
    d = Device(ctx, R.fixture()[0])
    yield d
    d.free()


@pytest.fixture(scope="module")
def staged():
    sc, free_rows = R.fixture()[:2]
    return R.staged(sc, R.CURRENT, R.ADJACENT, free_rows)


def guarded_lists(ctx, cap_rows, cap_obs):
    lists = mi355slam.ObservationLists(ctx, cap_rows, cap_obs, guard=64)
    for name, _ in lists._ROW + lists._OBS:
        put(ctx, lists[name], np.full(lists[name].nbytes, CANARY, np.uint8))
    return lists


def lists_equal(lists, n, want):
    """Every array of the device lists against the restatement's, bit for bit, and nothing written behind them."""
    got = lists.download(n, 2 * n)
    for name, dt in lists._ROW + lists._OBS:
        assert got[name].tobytes() == np.ascontiguousarray(want[name], dt).tobytes(), name
        used = np.dtype(dt).itemsize * (2 * n if (name, dt) in lists._OBS else n + (name == "obs_start"))
        assert untouched_behind(lists[name], used), name


def test_unbound_mask_against_the_table(ctx, dev):
    sc = dev.sc
    n_mp = 10
    kf = mi355slam.KeyframeTable(ctx, np.array([[-1, n_mp, n_mp - 1, 0, 11, -2 ** 31, 2 ** 31 - 1, 3], [0, 1, 2, -1, -1, n_mp, 9, 10]], np.int32))
    masks = [canary(ctx, 8), canary(ctx, 5)]
    kf.unbound_mask([1, 0], [8, 5], n_mp, masks)
    assert masks[0].download(np.uint8, (8,)).tolist() == [0, 0, 0, 1, 1, 1, 0, 1] and untouched_behind(masks[0], 8)
    assert masks[1].download(np.uint8, (5,)).tolist() == [1, 1, 0, 0, 1] and untouched_behind(masks[1], 5)
    kf.unbound_mask([], [], n_mp, [])
    kf.unbound_mask([0], [0], n_mp, [masks[0]])
    assert masks[0].download(np.uint8, (8,)).tolist() == [0, 0, 0, 1, 1, 1, 0, 1]
    # the scene's six slots in one launch, in a shuffled order
    st = R.fixture()[2]
    dev.restore(st)
    slots = [4, 0, 5, 2, 1, 3]
    out = [canary(ctx, int(sc["n_kp"][s])) for s in slots]
    dev.kf.unbound_mask(slots, sc["n_kp"][slots], dev.table.n, out)
    for s, b in zip(slots, out):
        n = int(sc["n_kp"][s])
        assert np.array_equal(b.download(np.uint8, (n,)), R.unbound_mask(st["kf_mp"], dev.table.n, s, n)) and untouched_behind(b, n), s
    assert (R.unbound_mask(st["kf_mp"], dev.table.n, R.CURRENT, 300) == 0).sum() > 100
    for b in masks + out + [kf.kf_mp]:
        b.free()


@pytest.mark.parametrize("index", (0, 1, 3), ids=("younger_adjacent", "older_adjacent", "third_adjacent"))
def test_lists_alone_against_the_staged_restatement(ctx, dev, staged, index):
    sc, free_rows = R.fixture()[:2]
    before = sc if index == 0 else staged[1][[i for i in range(index) if staged[1][i] is not None][-1]]["state"]
    want = staged[1][index]
    n = want["n_matches"]
    free = [r for r in free_rows.tolist() if not before["mp_live"][r]]
    dev.restore(before)
    lists, kp1, kp2 = guarded_lists(ctx, n + 3, 2 * n + 5), canary(ctx, 4 * n), canary(ctx, 4 * n)
    rc, got_n = dev.lists_call(lists, want["slot"], want["matched"], free, kp1, kp2)
    assert (rc, got_n) == (0, n), mi355slam.lib().ms_last_error(ctx._h)
    lists_equal(lists, n, want["lists"])
    assert np.array_equal(kp1.download(np.int32, (n,)), want["match_kp1"]) and untouched_behind(kp1, 4 * n)
    assert np.array_equal(kp2.download(np.int32, (n,)), want["match_kp2"]) and untouched_behind(kp2, 4 * n)
    assert R.same_state(dev.state(), before)                 # no table is written
    # an adjacent keyframe without descriptors in the pool: obs_desc -1 on its side
    base = sc["desc_base"].copy()
    base[want["slot"]] = -1
    rc, got_n = dev.lists_call(lists, want["slot"], want["matched"], free, kp1, kp2, desc_base=base)
    _, _, L, _, _, _ = R.lists_of(dict(before, kp=sc["kp"], n_kp=sc["n_kp"], kf_id=sc["kf_id"], S=sc["S"], desc_base=base), R.CURRENT, want["slot"], want["matched"], free)
    assert (rc, got_n) == (0, n) and (L["obs_desc"] == -1).sum() == n
    lists_equal(lists, n, L)
    for b in (kp1, kp2):
        b.free()
    lists.free()


def after_triangulation(sc, staged, index):
    """(state before the adjacent, state after its lists and triangulation, its staged result)."""
    free_rows = R.fixture()[1]
    before = sc if index == 0 else staged[1][[i for i in range(index) if staged[1][i] is not None][-1]]["state"]
    want = staged[1][index]
    st = R.copy_state(dict(sc, **{k: before[k] for k in R.TABLES}, table=before["table"]))
    R.triangulate_lists(st, want["lists"], TR.TME)
    return before, st, want


@pytest.mark.parametrize("index", (0, 1), ids=("younger_adjacent", "older_adjacent"))
def test_bind_alone_against_the_staged_restatement(ctx, dev, staged, index):
    sc = dev.sc
    before, st, want = after_triangulation(sc, staged, index)
    n, adj = want["n_matches"], want["slot"]
    masks = (before if index else dict(masks={s: R.unbound_mask(sc["kf_mp"], dev.table.n, s, int(sc["n_kp"][s])) for s in dev.frames}))["masks"]
    dev.restore(st, masks)
    lists = guarded_lists(ctx, n, 2 * n)
    for name, dt in lists._ROW + lists._OBS:
        put(ctx, lists[name], np.ascontiguousarray(want["lists"][name], dt))
    kp1, kp2 = ctx.upload(want["match_kp1"]), ctx.upload(want["match_kp2"])
    out = dict(created_rows=canary(ctx, 4 * n), created_kp1=canary(ctx, 4 * n), created_kp2=canary(ctx, 4 * n))
    n1, n2 = dev.frames[R.CURRENT].n, dev.frames[adj].n
    rc, n_created = dev.kf.create_points_bind_device(dev.table, dev.flags, dev.live, dev.pool, R.CURRENT, adj, lists, kp1, kp2, n, n1, n2,
                                                     dev.frames[R.CURRENT].bufs["usable"], dev.frames[adj].bufs["usable"], dev.n_obs, dev.mp_track, out)
    assert (rc, n_created) == (0, len(want["created_rows"])), mi355slam.lib().ms_last_error(ctx._h)
    assert 0 < n_created < n
    for k in out:
        assert np.array_equal(out[k].download(np.int32, (n_created,)), want[k]) and untouched_behind(out[k], 4 * n_created), k
    assert R.same_state(dev.state(), want["state"]) and R.same_masks(dev.masks(), want["state"]["masks"])
    # without a pool, masks, n_obs, mp_track and packed lists: the descriptors and those arrays stay
    dev.restore(st, masks)
    rc, n_created = dev.kf.create_points_bind_device(dev.table, dev.flags, dev.live, None, R.CURRENT, adj, lists, kp1, kp2, n, n1, n2)
    assert (rc, n_created) == (0, len(want["created_rows"]))
    got, w = dev.state(), want["state"]
    assert np.array_equal(got["kf_mp"], w["kf_mp"]) and np.array_equal(got["mp_live"], w["mp_live"]) and np.array_equal(got["table"]["desc"], st["table"]["desc"])
    assert np.array_equal(got["n_obs"], st["n_obs"]) and np.array_equal(got["mp_track"], st["mp_track"]) and R.same_masks(dev.masks(), masks)
    # a keypoint index past its frame's keypoints is found on the device before anything is written
    dev.restore(st, masks)
    put(ctx, kp2, np.append(want["match_kp2"][:-1], n2).astype(np.int32))
    rc, _ = dev.kf.create_points_bind_device(dev.table, dev.flags, dev.live, dev.pool, R.CURRENT, adj, lists, kp1, kp2, n, n1, n2, dev.frames[R.CURRENT].bufs["usable"],
                                             dev.frames[adj].bufs["usable"], dev.n_obs, dev.mp_track, out)
    assert rc == mi355slam.MS_ERR_INVALID and b"1 entries name a row, a keypoint or a descriptor outside the tables" in mi355slam.lib().ms_last_error(ctx._h)
    assert R.same_state(dev.state(), st) and R.same_masks(dev.masks(), masks)
    for b in [kp1, kp2] + list(out.values()):
        b.free()
    lists.free()


def run_chain(dev, step_by_step, **kw):
    """The chain over the fixture's adjacents; step_by_step compares everything with the sequential restatement after every adjacent."""
    sc, free_rows, st, results, _ = R.fixture()
    dev.restore()
    if not step_by_step:
        return dev.create(R.ADJACENT, free_rows, **kw), dev.state(), dev.masks()
    free, out = free_rows.tolist(), []
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    for adj, want in zip(R.ADJACENT, results):
        res = dev.create([adj], free, **kw)[0]
        out.append(res)
        if want is None:
            assert res is None
            continue
        assert res["slot"] == want["slot"] and res["n_matches"] == want["n_matches"]
        for k in ("match_kp1", "match_kp2", "rows", "status", "reason", "created_rows", "created_kp1", "created_kp2"):
            assert np.array_equal(res[k], want[k]), (adj, k)
        got, w = dev.state(), want["state"]
        rows = want["created_rows"]
        same = int((bits(got["table"]["pos"][rows]) == bits(w["table"]["pos"][rows])).all(axis=1).sum())
        print("adjacent %d: %d matches, %d created, %d of their positions bit-equal to the restatement" % (adj, want["n_matches"], len(rows), same))
        assert R.same_state(got, w), adj
        assert R.same_masks(dev.masks(), w["masks"]), adj
        taken = set(rows.tolist())
        free = [r for r in free if r not in taken]
    return out, dev.state(), dev.masks()


def test_the_chain_after_every_adjacent_against_the_sequential_restatement(dev):
    _, state, masks = run_chain(dev, True)
    sc, _, st, results, counts = R.fixture()
    assert R.same_state(state, st) and not R.same_state(state, sc) and counts["created"] == int(state["mp_live"].sum() - sc["mp_live"].sum())


def test_the_chain_twice_and_at_exact_capacity_gives_the_same_bits(ctx, dev):
    st, results = R.fixture()[2:4]
    runs = [run_chain(dev, False), run_chain(dev, False), run_chain(dev, False, exact_capacity=True, lists=mi355slam.ObservationLists(ctx, 1, 2))]
    for res, state, masks in runs:
        assert R.same_state(state, st) and R.same_state(state, runs[0][1]) and R.same_masks(masks, runs[0][2])
        for a, b, want in zip(res, runs[0][0], results):
            assert (a is None) == (b is None) == (want is None)
            for k in () if a is None else ("match_kp1", "match_kp2", "rows", "status", "reason", "created_rows", "created_kp1", "created_kp2"):
                assert a[k].tobytes() == b[k].tobytes() == want[k].tobytes(), k


def test_new_rows_one_short_reports_the_count_and_writes_nothing(ctx, dev, staged):
    sc, free_rows = R.fixture()[:2]
    want = staged[1][0]
    n = want["n_matches"]
    dev.restore()
    lists, kp1, kp2 = guarded_lists(ctx, n, 2 * n), canary(ctx, 4 * n), canary(ctx, 4 * n)
    for rows, caps, message in ((free_rows[:n - 1], {}, b"%d matches; new_rows holds %d" % (n, n - 1)), (free_rows, dict(cap_rows=n - 1), b"the lists %d rows" % (n - 1)),
                                (free_rows, dict(cap_obs=2 * n - 1), b"and %d observations" % (2 * n - 1))):
        rc, got_n = dev.lists_call(lists, want["slot"], want["matched"], rows, kp1, kp2, **caps)
        assert (rc, got_n) == (mi355slam.MS_ERR_CAPACITY, n) and message in mi355slam.lib().ms_last_error(ctx._h)
        assert R.same_state(dev.state(), sc)
        for name, _ in lists._ROW + lists._OBS:
            assert untouched_behind(lists[name], 0), name
        assert untouched_behind(kp1, 0) and untouched_behind(kp2, 0)
    rc, got_n = dev.lists_call(lists, want["slot"], want["matched"], free_rows[:n], kp1, kp2)      # exactly enough of both
    assert (rc, got_n) == (0, n)
    lists_equal(lists, n, want["lists"])
    for b in (kp1, kp2):
        b.free()
    lists.free()


@pytest.mark.parametrize("which", ("bound_current", "bound_adjacent", "live", "range", "twice", "octave"))
def test_each_device_violation_leaves_every_table_alone(ctx, which, staged):
    sc, free_rows = R.fixture()[:2]
    want = staged[1][0]
    adj, matched = want["slot"], want["matched"].copy()
    j = int(want["match_kp1"][-1])                           # a match of the second trip
    assert j >= R.TRIP
    bad = R.copy_state(sc)
    bad["kp"] = {k: v.copy() for k, v in sc["kp"].items()}
    if which == "bound_current":                             # keyframe.cpp:275
        bad["kf_mp"][R.CURRENT, j] = 5
    elif which == "bound_adjacent":
        bad["kf_mp"][adj, matched[j]] = 0
    elif which == "live":
        bad["mp_live"][free_rows[want["n_matches"] - 1]] = 1
    elif which == "range":
        matched[j] = sc["n_kp"][adj]
    elif which == "twice":
        matched[j] = matched[int(want["match_kp1"][0])]
    else:
        bad["kp"]["octave"][adj, matched[j]] = N_LEVELS
    rc_ref, _, _, _, _, v = R.lists_of(bad, R.CURRENT, adj, matched, free_rows)
    assert rc_ref == R.INVALID and sum(v.values()) == 1
    d = Device(ctx, bad)
    lists, kp1, kp2 = guarded_lists(ctx, 128, 256), canary(ctx, 512), canary(ctx, 512)
    rc, _ = d.lists_call(lists, adj, matched, free_rows, kp1, kp2)
    assert rc == mi355slam.MS_ERR_INVALID and b"nothing written" in mi355slam.lib().ms_last_error(ctx._h)
    assert R.same_state(d.state(), bad)
    for name, _ in lists._ROW + lists._OBS:
        assert untouched_behind(lists[name], 0), name
    assert untouched_behind(kp1, 0) and untouched_behind(kp2, 0)
    for b in (kp1, kp2):
        b.free()
    lists.free()
    d.free()


def test_no_keypoints_and_no_matches_return_zero_counts(ctx, dev):
    sc, free_rows = R.fixture()[:2]
    dev.restore()
    lists, kp1, kp2 = guarded_lists(ctx, 4, 8), canary(ctx, 16), canary(ctx, 16)
    rc, n = dev.lists_call(lists, 3, np.zeros(0, np.int32), free_rows, kp1, kp2)
    assert (rc, n) == (0, 0) and untouched_behind(lists["obs_start"], 0)
    rc, n = dev.lists_call(lists, 3, np.full(300, -1, np.int32), free_rows, kp1, kp2)
    assert (rc, n) == (0, 0) and lists["obs_start"].download(np.int32, (1,)).tolist() == [0] and untouched_behind(lists["obs_start"], 4)
    assert untouched_behind(lists["rows"], 0) and untouched_behind(kp1, 0)
    rc, n_created = dev.kf.create_points_bind_device(dev.table, dev.flags, dev.live, dev.pool, R.CURRENT, 3, lists, kp1, kp2, 0, 300, 280)
    assert (rc, n_created) == (0, 0) and R.same_state(dev.state(), sc)
    res = dev.create([R.EMPTY_SLOT], free_rows)[0]
    assert res["n_matches"] == 0 and len(res["created_rows"]) == 0 and len(res["status"]) == 0 and R.same_state(dev.state(), sc)
    for b in (kp1, kp2):
        b.free()
    lists.free()
