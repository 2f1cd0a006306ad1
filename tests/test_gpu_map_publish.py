"""ms_map_publish on the device against tests/map_publish_ref.py, its specification: every host output and the record state bit
for bit, canaries behind every buffer, every table left as it was.  Small shapes: 40 rows x 4 slots x 8 with every class of row; a map that ends
37 rows into its second workgroup; one whose block-offsets scan takes a second trip; both capacities exact and one short; four calls with the
state carried; positions at rounding ties, a denormal, infinities, -0.0 and a NaN; ms_map_cull in front; every optional input left out; the same
bytes on a second run; no allocation after warm-up."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_publish_ref as R
import mi355slam

pytestmark = pytest.mark.gpu
CAN, PAD = 0x5A, 16
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(ROOT, "slam-module_amd", "csrc", "map_publish.hip")).read()).group(1))
TABLES = ("mp_pos", "mp_norm", "mp_flags", "mp_live", "n_obs", "mp_color", "kf_mp", "kf_pose")
BOTH = R.VIEW | R.RECORD


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def with_canary(a):
    return np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.full(PAD, CAN, np.uint8)])


def scene(n_mp, n_kf, stride, seed, live_p=0.8, flag_p=(0.2, 0.3, 0.5), obs4_p=0.5):
    """random tables holding every class of row: free rows with stale flags, live rows with flags 0 / 2 / 3, n_obs 3 and 4 (and more)"""
    rng = np.random.default_rng(seed)
    t = dict(mp_pos=rng.normal(size=(n_mp, 3)) * 10, mp_norm=rng.normal(size=(n_mp, 3)).astype(F), mp_flags=rng.choice(np.array([0, 2, 3], np.uint8), n_mp, p=flag_p),
             mp_live=(rng.random(n_mp) < live_p).astype(np.uint8), n_obs=np.where(rng.random(n_mp) < obs4_p, 4 + rng.integers(0, 3, n_mp), 3).astype(np.int32),
             mp_color=rng.integers(0, 256, (n_mp, 3)).astype(np.uint8), kf_mp=rng.integers(-1, max(n_mp, 1), (n_kf, stride)).astype(np.int32),
             kf_pose=rng.normal(size=(n_kf, 12)))
    t["kf_mp"][rng.random((n_kf, stride)) < 0.3] = -1
    return t


class Dev:
    """The tables, the local list and the record state on the device, each with a canary behind it."""

    def __init__(self, ctx, t, rec_pos, rec_state, local_rows=None):
        self.ctx, self.t, self.n_mp = ctx, t, len(t["mp_flags"])
        self.n_kf, self.stride = t["kf_mp"].shape
        self.tab = {k: ctx.upload(with_canary(t[k])) for k in TABLES if t.get(k) is not None}
        self.local = None if local_rows is None else np.asarray(local_rows, np.int32)
        if self.local is not None:
            self.tab["local_rows"] = ctx.upload(with_canary(self.local))
        self.set_record(rec_pos, rec_state)

    def set_record(self, rec_pos, rec_state):
        for k in ("rec_pos", "rec_state"):
            if k in self.tab:
                self.tab[k].free()
        self.tab["rec_pos"], self.tab["rec_state"] = self.ctx.upload(with_canary(rec_pos)), self.ctx.upload(with_canary(rec_state))

    def update(self, **arrays):
        """the tables edited between two calls"""
        for k, a in arrays.items():
            self.t[k] = a
            self.tab[k].free()
            self.tab[k] = self.ctx.upload(with_canary(a))

    def call(self, what, current_slot=-1, min_record_obs=4, kf_list=(), cap_pub=None, cap_ev=None, leave_out=()):
        """The C call with a canary behind every host output.  Returns (rc, out), the arrays cut to the counts (to nothing on a refusal)."""
        cp, ce = (self.n_mp if c is None else c for c in (cap_pub, cap_ev))
        lst = np.asarray(kf_list, np.int32)
        raw = {k: np.full((cap * w + PAD) * np.dtype(dt).itemsize, CAN, np.uint8).view(dt) for spec, cap in ((R.PUB, cp), (R.EV, ce)) for k, dt, w in spec}
        raw["pose_wc"] = np.full(4 * (16 * len(lst) + PAD), CAN, np.uint8).view(F)
        counts = np.full(8 + PAD, -77, np.int32)
        vp = mi355slam._vp
        p = lambda k: vp(None if k in leave_out else self.tab.get(k))
        A = mi355slam.MapPublishArgsC(what, current_slot, min_record_obs)
        rc = mi355slam.lib().ms_map_publish(
            self.ctx._h, p("mp_pos"), p("mp_norm"), p("mp_flags"), p("mp_live"), p("n_obs"), p("mp_color"), self.n_mp, p("kf_mp"), self.n_kf, self.stride, p("kf_pose"),
            p("local_rows"), 0 if self.local is None or "local_rows" in leave_out else len(self.local), p("rec_pos"), p("rec_state"), C.byref(A), vp(lst), len(lst),
            *[vp(raw[k]) for k, _, _ in R.PUB], cp, *[vp(raw[k]) for k, _, _ in R.EV], ce, vp(raw["pose_wc"]), vp(counts))
        assert (counts[8:] == -77).all()
        n = {"p": int(counts[0]) if rc == 0 else 0, "e": int(counts[1]) if rc == 0 else 0}
        out = dict(counts=counts[:8].copy())
        for k, dt, w in R.PUB + R.EV:
            m = n[k[0]] * w
            assert (raw[k][m:].view(np.uint8) == CAN).all(), k     # nothing behind n_pub / n_ev is written, nothing at all on a refusal
            out[k] = raw[k][:m].reshape((-1, w) if w > 1 else (-1,)).copy()
        m = 16 * len(lst) if rc == 0 else 0
        assert (raw["pose_wc"][m:].view(np.uint8) == CAN).all()
        out["pose_wc"] = raw["pose_wc"][:m].reshape(-1, 4, 4).copy()
        return rc, out

    def record(self):
        out = []
        for k, dt, shape in (("rec_pos", F, (self.n_mp, 3)), ("rec_state", np.uint8, (self.n_mp,))):
            nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
            raw = self.tab[k].download(np.uint8, (nbytes + PAD,))
            assert (raw[nbytes:] == CAN).all(), k
            out.append(raw[:nbytes].view(dt).reshape(shape))
        return out

    def tables_untouched(self):
        for k in TABLES:
            if self.t.get(k) is not None:
                assert same_bits(self.tab[k].download(np.uint8, (self.t[k].nbytes + PAD,)), with_canary(self.t[k])), k
        if self.local is not None:
            assert same_bits(self.tab["local_rows"].download(np.uint8, (self.local.nbytes + PAD,)), with_canary(self.local))

    def free(self):
        for b in self.tab.values():
            b.free()


def check(ctx, dev, rec_pos, rec_state, what, current_slot=-1, min_record_obs=4, kf_list=(), cap_pub=None, cap_ev=None, leave_out=()):
    """One call against the restatement: the code, the head, every output, the record state, the tables.  Returns the restatement's
    (rc, out, rec_pos, rec_state)."""
    t = {k: (None if k in leave_out else v) for k, v in dev.t.items()}
    local = () if dev.local is None or "local_rows" in leave_out else dev.local
    want_rc, want, new_pos, new_state = R.map_publish(t, rec_pos, rec_state, what, current_slot, min_record_obs, local, kf_list, dev.n_mp if cap_pub is None else cap_pub,
                                                      dev.n_mp if cap_ev is None else cap_ev)
    rc, out = dev.call(what, current_slot, min_record_obs, kf_list, cap_pub, cap_ev, leave_out)
    assert rc == want_rc, (rc, want_rc, mi355slam.lib().ms_last_error(ctx._h))
    assert out["counts"].tolist() == want["counts"].tolist(), (out["counts"], want["counts"])
    if rc == 0:
        for k, _, _ in R.PUB + R.EV:
            assert same_bits(out[k], want[k]), k
        assert same_bits(out["pose_wc"], want["pose_wc"])
    got_pos, got_state = dev.record()
    assert same_bits(got_pos, new_pos) and same_bits(got_state, new_state)
    dev.tables_untouched()
    return want_rc, want, new_pos, new_state


def some_recorded(t, seed):
    """a record state in which every state meets every class of row: 0 / 1 / 2, the recorded positions equal to the row's or not"""
    rng = np.random.default_rng(seed)
    n_mp = len(t["mp_flags"])
    state = rng.integers(0, 3, n_mp).astype(np.uint8)
    pos = np.where(rng.random((n_mp, 1)) < 0.5, t["mp_pos"].astype(F), F(1.5)).astype(F)
    return pos, state


# ---- (a)
def test_every_class_of_row_on_a_small_map(ctx):
    t = scene(40, 4, 8, 1)
    t["mp_live"][:12] = [0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1, 1]
    t["mp_flags"][:12] = [0, 3, 2, 0, 2, 3, 0, 2, 3, 3, 3, 2]  # free rows with stale flags; live with 0 / 2 / 3
    t["n_obs"][:12] = [4, 4, 3, 4, 3, 4, 3, 4, 3, 9, 4, 4]
    t["kf_mp"][3] = [4, -1, 8, 8, 40, 1, -2**31, 11]            # the current slot: a repeat, a free row, entries that are not VALID
    local = [5, 7, 7, 40, -1, 1 << 30, 2, 10]                   # a repeat, invalid entries, a free row
    pos, state = some_recorded(t, 2)
    state[:12] = [1, 0, 2, 1, 1, 1, 0, 2, 0, 1, 1, 0]
    pos[10] = t["mp_pos"][10].astype(F)                         # recorded where it is: no event
    pos[[3, 5]] = F(99)                                         # recorded elsewhere: MOVED
    dev = Dev(ctx, t, pos, state, local)
    try:
        rc, want, _, _ = check(ctx, dev, pos, state, BOTH, 3, 4, [2, 0, 3])
        assert rc == 0
        k = {int(r): i for i, r in enumerate(want["pub_row"])}
        assert want["pub_bits"][k[4]] == 2 and want["pub_bits"][k[5]] == 1 and want["pub_bits"][k[7]] == 1 and want["pub_bits"][k[8]] == 2 and want["pub_bits"][k[11]] == 2
        assert want["pub_bits"][k[10]] == 1 and 1 not in k and 2 not in k and 3 not in k and want["pub_status"][k[4]] == 2 and want["pub_status"][k[5]] == 0
        e = {int(r): int(kind) for r, kind in zip(want["ev_row"], want["ev_kind"])}
        assert e[0] == R.REMOVED and e[9] == R.REMOVED and e[5] == R.MOVED and e[7] == R.NEW and e[11] == R.NEW and e[3] == R.MOVED
        assert not {1, 2, 4, 6, 8, 10} & set(e)
        assert want["counts"][7] == int(((t["mp_flags"] & 3) == 0)[t["mp_live"] != 0].sum()) > 0
    finally:
        dev.free()


# ---- (b), (c)
@pytest.mark.parametrize("n_mp, live_p, flag_p, obs4_p", [(T + 37, 0.8, (0.2, 0.3, 0.5), 0.5), (T * T + T + 37, 0.02, (0.5, 0.2, 0.3), 0.3)], ids=["T+37", "T*T+T+37 sparse"])
def test_block_ends_and_the_second_trip_of_the_offsets_scan(ctx, n_mp, live_p, flag_p, obs4_p):
    t = scene(n_mp, 3, 64, 3, live_p, flag_p, obs4_p)
    # kept and dropped rows on both sides of the first block's end, and the last row kept
    t["mp_live"][[T - 2, T - 1, T, T + 1, n_mp - 1]] = 1
    t["mp_flags"][[T - 2, T - 1, T, T + 1, n_mp - 1]] = [3, 0, 2, 0, 3]
    t["n_obs"][[T - 2, T - 1, T, T + 1, n_mp - 1]] = [3, 5, 4, 3, 4]
    pos, state = some_recorded(t, 4)
    if n_mp > T * T:                                          # sparse events too: only few rows were ever recorded
        state[np.random.default_rng(5).random(n_mp) < 0.97] = 0
    state[[T - 2, T - 1, T, T + 1, n_mp - 1]] = [1, 0, 1, 0, 0]
    local = np.random.default_rng(6).integers(0, n_mp, 300)
    dev = Dev(ctx, t, pos, state, local)
    try:
        rc, want, _, _ = check(ctx, dev, pos, state, BOTH, 1, 4, [1])
        assert rc == 0 and want["counts"][0] > 2 and want["counts"][1] > 2 and want["pub_row"][-1] == n_mp - 1 and want["ev_row"][-1] == n_mp - 1
        assert T - 2 in want["pub_row"] and T in want["pub_row"] and T - 1 in want["ev_row"] and T - 1 not in want["pub_row"]
        if n_mp > T * T:
            assert -(-n_mp // T) > T                          # more workgroups than one trip of the scan holds
    finally:
        dev.free()


# ---- (d)
def test_both_capacities_exact_and_one_short(ctx):
    t = scene(T + 37, 3, 16, 7)
    pos, state = some_recorded(t, 8)
    dev = Dev(ctx, t, pos, state, [1, 2, 3])
    try:
        rc, want, _, _ = R.map_publish(t, pos, state, BOTH, 2, 4, [1, 2, 3], [0])
        n_pub, n_ev = int(want["counts"][0]), int(want["counts"][1])
        assert n_pub > 10 and n_ev > 10
        for cp, ce in ((n_pub - 1, n_ev), (n_pub, n_ev - 1), (0, 0)):
            rc, out, p2, s2 = check(ctx, dev, pos, state, BOTH, 2, 4, [0], cp, ce)
            assert rc == R.CAPACITY and out["counts"][:2].tolist() == [n_pub, n_ev] and p2 is pos and s2 is state      # the needed numbers; nothing moved
            assert b"published rows" in mi355slam.lib().ms_last_error(ctx._h)
        rc, _, pos, state = check(ctx, dev, pos, state, BOTH, 2, 4, [0], n_pub, n_ev)
        assert rc == 0
        rc, out, _, _ = check(ctx, dev, pos, state, BOTH, 2, 4, [0], n_pub, 0)      # the events are recorded: the second call has none
        assert rc == 0 and out["counts"][1] == 0
    finally:
        dev.free()


# ---- (e)
def test_four_calls_with_the_state_carried(ctx):
    n_mp = 2 * T + 5
    t = scene(n_mp, 3, 32, 9)
    pos, state = R.empty_record(n_mp)
    dev = Dev(ctx, t, pos, state, np.arange(0, n_mp, 7))
    try:
        rc, out, pos, state = check(ctx, dev, pos, state, BOTH, 0)
        assert out["counts"][2] == out["counts"][1] > 0                        # all NEW
        rc, out, pos, state = check(ctx, dev, pos, state, BOTH, 0)
        assert out["counts"][1] == 0 and out["counts"][0] > 0                   # a repeated call gives no event
        rng = np.random.default_rng(10)
        moved = rng.random(n_mp) < 0.2
        mp_pos = np.where(moved[:, None], t["mp_pos"] + 0.5, t["mp_pos"])
        n_obs = np.where(rng.random(n_mp) < 0.2, 7 - t["n_obs"], t["n_obs"]).astype(np.int32)      # 3 <-> 4
        dev.update(mp_pos=mp_pos, n_obs=n_obs)
        rc, out, pos, state = check(ctx, dev, pos, state, BOTH, 1)
        assert out["counts"][2] > 0 and out["counts"][3] > 0 and out["counts"][4] == 0
        live = np.where(rng.random(n_mp) < 0.3, 1 - t["mp_live"], t["mp_live"]).astype(np.uint8)     # rows removed, and free rows taken
        dev.update(mp_live=live)
        rc, out, pos, state = check(ctx, dev, pos, state, BOTH, 2)
        assert out["counts"][4] > 0 and out["counts"][2] > 0
        dev.update(mp_live=(t["mp_live"] | (state == 2)).astype(np.uint8))                        # removed rows taken again: NEW (rule 1 with state 2)
        rc, out, pos, state = check(ctx, dev, pos, state, R.RECORD, 2)
        assert out["counts"][2] > 0 and out["counts"][0] == 0 and len(out["pub_row"]) == 0
    finally:
        dev.free()


# ---- (f)
def test_rounding_ties_a_denormal_infinities_minus_zero_and_a_nan(ctx):
    t = scene(16, 2, 4, 11)
    t["mp_live"][:], t["mp_flags"][:], t["n_obs"][:] = 1, 3, 4
    tie = lambda lo: float(F(lo)) + float(np.spacing(F(lo))) / 2     # halfway between two floats: to even
    t["mp_pos"][0] = [tie(1.0), tie(1.0 + 2.0 ** -23), -tie(3.0)]
    t["mp_pos"][1] = [1e-40, -1e-45, 0.7e-45]                         # float denormals; the last is halfway below the smallest
    t["mp_pos"][2] = [np.inf, -np.inf, 1e300]
    t["mp_pos"][3] = [-0.0, 0.0, -0.0]
    t["mp_pos"][4] = [np.nan, 1.0, 2.0]
    t["mp_pos"][5] = [3.4028235677973366e38, 3.4028234663852886e38, -3.5e38]      # the first rounds to inf, the second is FLT_MAX
    t["mp_pos"][6] = [0.1, 0.2, 0.3]
    pos, state = R.empty_record(16)
    state[3] = 1                                                      # recorded at +0.0, +0.0, +0.0
    dev = Dev(ctx, t, pos, state)
    try:
        rc, want, pos, state = check(ctx, dev, pos, state, BOTH)
        assert want["pub_pos"][0].tolist() == [1.0, float(F(1.0 + 2.0 ** -22)), -3.0] and want["pub_pos"][1][0] != 0 and want["pub_pos"][2].tolist() == [np.inf, -np.inf, np.inf]
        assert 3 not in want["ev_row"] and want["counts"][2] == 15
        assert np.signbit(want["pub_pos"][3][0]) and pos[3].tobytes() == np.zeros(3, F).tobytes()       # the view shows -0.0, the record keeps +0.0
        for _ in range(2):                                            # the NaN moves on every call, nothing else ever does
            rc, want, pos, state = check(ctx, dev, pos, state, BOTH)
            assert want["ev_row"].tolist() == [4] and want["ev_kind"].tolist() == [R.MOVED] and np.isnan(want["ev_pos"][0, 0])
    finally:
        dev.free()


# ---- (g)
def test_removed_for_exactly_the_rows_ms_map_cull_removes(ctx):
    n_mp, n_kf, stride = T + 37, 4, 32
    t = scene(n_mp, n_kf, stride, 12, live_p=1.0)
    t["kf_mp"][t["kf_mp"] % 5 == 0] = -1                          # a fifth of the rows has no observation left
    t["n_obs"][:] = 5                                             # the first call records every row
    pos, state = R.empty_record(n_mp)
    dev = Dev(ctx, t, pos, state)
    try:
        rc, out, pos, state = check(ctx, dev, pos, state, R.RECORD)
        assert out["counts"][2] == n_mp
        kt = mi355slam.KeyframeTable(ctx, t["kf_mp"])
        flags, live = ctx.upload(t["mp_flags"]), ctx.upload(t["mp_live"])
        d_n, d_rows = ctx.alloc(4 * n_mp), ctx.alloc(4 * n_mp)
        settings = dict(current_slot=n_kf - 1, cull_points=1, min_age=1e9, min_obs_for_ba=0, max_critical_ratio=1.0, ratio_float32=0)
        _, n_rows, _ = kt.cull_device(flags, live, n_mp, np.arange(n_kf), np.arange(n_kf, dtype=np.float64), [], None, settings, d_n, d_rows, None)
        removed = np.sort(d_rows.download(np.int32, (n_rows,)))
        assert n_rows > 10
        dev.update(mp_flags=flags.download(np.uint8, (n_mp,)), mp_live=live.download(np.uint8, (n_mp,)), n_obs=d_n.download(np.int32, (n_mp,)),
                   kf_mp=kt.kf_mp.download(np.int32, (n_kf, stride)))
        rc, out, pos, state = check(ctx, dev, pos, state, BOTH, n_kf - 1)
        gone = out["ev_row"][out["ev_kind"] == R.REMOVED]
        assert same_bits(gone, removed) and out["counts"][4] == n_rows and (out["ev_pos"][out["ev_kind"] == R.REMOVED] == 0).all()
        assert not set(removed.tolist()) & set(out["pub_row"].tolist())
        for b in (flags, live, d_n, d_rows, kt.kf_mp):
            b.free()
    finally:
        dev.free()


# ---- (h)
def test_view_alone_record_alone_and_every_optional_input_left_out(ctx):
    t = scene(T + 37, 3, 16, 13)
    pos, state = some_recorded(t, 14)
    dev = Dev(ctx, t, pos, state, [3, 4, 5, T, T + 1])
    try:
        rc, out, p2, s2 = check(ctx, dev, pos, state, R.VIEW, 1, 4, [0, 2], leave_out=("n_obs", "rec_pos", "rec_state"))
        assert rc == 0 and out["counts"][0] > 0 and out["counts"][1] == 0 and same_bits(p2, pos) and same_bits(s2, state)
        rc, out, _, _ = check(ctx, dev, pos, state, R.VIEW, 1, 4, [0, 2], leave_out=("mp_color",))
        assert (out["pub_color"] == 0).all() and out["counts"][5] > 0 and out["counts"][6] > 0
        rc, out, _, _ = check(ctx, dev, pos, state, R.VIEW, 1, leave_out=("local_rows",))
        assert out["counts"][5] == 0 and out["counts"][6] > 0 and out["pose_wc"].size == 0
        rc, out, _, _ = check(ctx, dev, pos, state, R.VIEW, -1)
        assert out["counts"][5] > 0 and out["counts"][6] == 0
        rc, out, _, _ = check(ctx, dev, pos, state, R.RECORD, 1, 4, [2], leave_out=("mp_color",))
        assert rc == 0 and out["counts"][0] == 0 and out["counts"][1] > 0 and out["counts"][5:].tolist() == [0, 0, 0]
    finally:
        dev.free()
    # an empty map with a keyframe list: the poses alone; nothing at all: no launch, zero counts
    e = scene(0, 2, 4, 15)
    dev = Dev(ctx, e, *R.empty_record(0))
    try:
        rc, out, _, _ = check(ctx, dev, *R.empty_record(0), BOTH, 1, 4, [1, 0])
        assert rc == 0 and out["counts"].tolist() == [0] * 8 and out["pose_wc"].shape == (2, 4, 4)
        rc, out, _, _ = check(ctx, dev, *R.empty_record(0), BOTH, 1)
        assert rc == 0 and out["counts"].tolist() == [0] * 8
    finally:
        dev.free()


# ---- (i)
def test_the_same_bytes_on_fresh_state_and_nothing_allocated_after_warm_up(ctx):
    lib = mi355slam.lib()
    lib.ms_debug_host_allocs.restype = C.c_longlong
    t = scene(4 * T + 3, 5, 64, 16)
    local = np.arange(0, 4 * T, 3)
    seen = []
    for run in range(2):
        allocs = []
        pos, state = some_recorded(t, 17)
        dev = Dev(ctx, t, pos, state, local)
        try:
            rc, out = dev.call(BOTH, 4, 4, [0, 1, 2, 3, 4])
            assert rc == 0
            seen.append([out[k] for k in sorted(out)] + dev.record())
            for i in range(23):                              # the record is current now: the calls differ in their answer's size, not in their workspace
                rc, again = dev.call(BOTH if i % 2 else R.VIEW, 4, 4, [0, 1, 2, 3, 4])
                allocs.append(lib.ms_debug_host_allocs())
                assert rc == 0 and again["counts"][1] == 0 and same_bits(again["pub_pos"], out["pub_pos"])
            assert len(set(allocs[3:])) == 1, allocs          # flat over 20 calls after three warm-ups
        finally:
            dev.free()
    assert all(same_bits(a, b) for a, b in zip(*seen))
