"""CPU checks of the surface of the device createNewMapPoints: the library exports the three calls and their *_check twins with
the header's signatures, Python binds them, and the host-only halves that run in front of any device call turn every MS_ERR_INVALID case
away with its message, hold every capacity cap and accept the empty cases.  The checks dereference HOST arguments only, so host arrays stand
in for the device tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mi355slam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_create_points_lists", "ms_create_points_lists_check", "ms_create_points_bind", "ms_create_points_bind_check", "ms_unbound_mask", "ms_unbound_mask_check")
INVALID, CAPACITY = mi355slam.MS_ERR_INVALID, mi355slam.MS_ERR_CAPACITY
MAX_KF, MAX_STRIDE, MAX_MP, MAX_QUERIES = 65536, 8192, 1 << 24, 4096


def test_library_exports_the_calls_and_python_binds_them():
    for name in NAMES:
        assert hasattr(mi355slam.lib(), name), name
    for name in ("create_points_lists_device", "create_points_bind_device", "create_points", "unbound_mask"):
        assert callable(getattr(mi355slam.KeyframeTable, name)), name
    assert callable(mi355slam.create_E21)
    mk = open(os.path.join(ROOT, "slam-module_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bcreate_points\.hip\b", mk, flags=re.M)


def test_the_check_twins_take_the_arguments_of_the_calls():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355slam.h")).read(), flags=re.S)

    def declaration(name):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        return [" ".join(p.split()).replace("const ", "") for p in m.group(1).split(",")]

    for name in ("ms_create_points_lists", "ms_create_points_bind", "ms_unbound_mask"):
        call, check = declaration(name), declaration(name + "_check")
        assert call[0] == "ms_ctx *ctx" and call[1:] == check[:-2] and check[-2:] == ["char *why", "size_t why_bytes"], name


def test_the_kernels_use_the_shared_scan_and_workspace():
    src = open(os.path.join(ROOT, "slam-module_amd", "csrc", "create_points.hip")).read()
    assert '#include "ms_scan.h"' in src and "block_rank<kBlock>" in src and "MS_WS_CREATE_POINTS" in src
    assert "MS_WS_CREATE_POINTS" in open(os.path.join(ROOT, "slam-module_amd", "csrc", "ms_internal.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "__shfl_up" not in code and not re.search(r"atomic(Add|CAS|Exch|Min|Max)\s*\(", code)         # no third scan; one LDS atomicOr and nothing else


def arrays(n_kf=3, stride=8, n_mp=10):
    a = lambda n, dt: np.zeros(max(n, 1), dt)
    return dict(kf_mp=np.full(n_kf * stride, -1, np.int32), mp_live=a(n_mp, np.uint8), mp_flags=a(n_mp, np.uint8), kp_x=a(n_kf * stride, np.float32),
                kp_y=a(n_kf * stride, np.float32), kp_octave=a(n_kf * stride, np.int32), kp_depth=a(n_kf * stride, np.float32), matched=a(stride, np.int32),
                mp_desc=a(8 * n_mp + 8, np.uint32), desc_pool=a(64 * 8 + 8, np.uint32), n_obs=a(n_mp, np.int32), mp_track=a(n_mp, np.int32),
                match_kp1=a(stride, np.int32), match_kp2=a(stride, np.int32), usable=a(stride, np.uint8), created=a(stride, np.int32))


class Lists:
    """One call of ms_create_points_lists_check: 3 slots x 8, 10 map points, current slot 1 (5 keypoints), adjacent slot 2 (8 keypoints)."""

    def __init__(self):
        self.n_kf, self.stride, self.n_mp = 3, 8, 10
        self.arrays = arrays()
        self.kf_id, self.desc_base = np.array([4, 9, 7], np.int32), np.array([0, 8, -1], np.int32)
        self.cur, self.adj, self.n_kp1, self.n_kp2, self.n_levels = 1, 2, 5, 8, 8
        self.new_rows, self.n_new = np.array([9, 4, 7], np.int32), 3
        self.cap_rows, self.cap_obs = 4, 8
        self.lists = {k: np.zeros(16, np.float32 if k in ("obs_x", "obs_y", "obs_depth") else np.int32) for k, _ in mi355slam.ObsListsC._fields_}
        self.null_lists = self.null_count = False

    def run(self):
        p = lambda k: mi355slam._vp(self.arrays.get(k))
        L = mi355slam.ObsListsC(*[None if self.lists.get(k) is None else self.lists[k].ctypes.data for k, _ in mi355slam.ObsListsC._fields_])
        n, why = C.c_int32(0), C.create_string_buffer(512)
        rc = mi355slam.lib().ms_create_points_lists_check(p("kf_mp"), self.n_kf, self.stride, p("mp_live"), self.n_mp, mi355slam._vp(self.kf_id), p("kp_x"), p("kp_y"),
                                                          p("kp_octave"), p("kp_depth"), mi355slam._vp(self.desc_base), self.cur, self.adj, p("matched"), self.n_kp1,
                                                          self.n_kp2, mi355slam._vp(self.new_rows), self.n_new, self.n_levels, None if self.null_lists else C.byref(L),
                                                          self.cap_rows, self.cap_obs, p("match_kp1"), p("match_kp2"), None if self.null_count else C.byref(n), why,
                                                          C.c_size_t(512))
        return rc, why.value.decode()


def change(c, **kw):
    for k, v in kw.items():
        if k in c.arrays:
            c.arrays[k] = v
        elif k.startswith("L_"):
            c.lists[k[2:]] = v
        else:
            setattr(c, k, v)


def test_a_valid_lists_call_and_the_empty_cases_pass():
    assert Lists().run() == (0, "")
    c = Lists(); change(c, n_kp1=0, matched=None)
    assert c.run() == (0, "")
    c = Lists(); change(c, n_new=0, new_rows=None)
    assert c.run() == (0, "")
    c = Lists(); change(c, n_kp1=8, n_kp2=8)                 # n_kp == stride
    assert c.run() == (0, "")
    c = Lists(); change(c, match_kp1=None, match_kp2=None, n_levels=0, cap_rows=0, cap_obs=0)
    assert c.run() == (0, "")
    c = Lists(); change(c, desc_base=None, L_obs_desc=None, kp_depth=None, L_obs_depth=None, kp_x=None, L_obs_x=None)       # an output and its table, both absent
    assert c.run() == (0, "")


LISTS_INVALID = [
    (dict(cur=-1), "slot -1 outside [0, 3)"), (dict(cur=3), "slot 3 outside [0, 3)"), (dict(adj=-1), "slot -1 outside [0, 3)"), (dict(adj=3), "slot 3 outside [0, 3)"),
    (dict(adj=1), "the current and the adjacent keyframe are both slot 1"),
    (dict(kf_id=np.array([4, -1, 7], np.int32)), "slot 1 has kf_id -1"), (dict(kf_id=np.array([4, 9, -5], np.int32)), "slot 2 has kf_id -5"),
    (dict(kf_id=np.array([4, 7, 7], np.int32)), "slots 1 and 2 both have kf_id 7"),
    (dict(new_rows=np.array([9, 4, 9], np.int32)), "new row 9 is listed twice"), (dict(new_rows=np.array([9, 10, 7], np.int32)), "new row 10 outside [0, 10)"),
    (dict(new_rows=np.array([-1, 4, 7], np.int32)), "new row -1 outside [0, 10)"),
    (dict(n_kp1=9), "9 keypoints in a table of stride 8"), (dict(n_kp2=9), "9 keypoints in a table of stride 8"),
    (dict(n_levels=33), "33 levels outside [0, 32]"), (dict(n_levels=-1), "negative size"),
    (dict(stride=0), "stride 0"), (dict(n_mp=-1), "negative size"), (dict(n_new=-1), "negative size"), (dict(cap_rows=-1), "negative size"), (dict(n_kp1=-1), "negative size"),
    (dict(null_count=True), "missing array (n_matches or kf_id)"), (dict(kf_id=None), "missing array (n_matches or kf_id)"),
    (dict(kf_mp=None), "missing array (kf_mp or mp_live)"), (dict(mp_live=None), "missing array (kf_mp or mp_live)"),
    (dict(matched=None), "missing array (matched)"), (dict(new_rows=None), "missing array (new_rows)"),
    (dict(null_lists=True), "missing array (rows or obs_start)"), (dict(L_rows=None), "missing array (rows or obs_start)"), (dict(L_obs_start=None), "missing array (rows or obs_start)"),
    (dict(kp_x=None), "an output is asked for whose table is missing"), (dict(kp_octave=None), "an output is asked for whose table is missing"),
    (dict(kp_depth=None), "an output is asked for whose table is missing"), (dict(desc_base=None), "an output is asked for whose table is missing"),
]


@pytest.mark.parametrize("fields,message", LISTS_INVALID, ids=[m[:40] + "/" + ",".join(f) for f, m in LISTS_INVALID])
def test_each_invalid_lists_case_is_turned_away_with_its_message(fields, message):
    c = Lists()
    change(c, **fields)
    rc, why = c.run()
    assert rc == INVALID and why.startswith("create points lists: ") and message in why, why


@pytest.mark.parametrize("fields", [dict(n_kf=MAX_KF + 1), dict(stride=MAX_STRIDE + 1), dict(n_mp=MAX_MP)], ids=lambda f: next(iter(f)))
def test_each_capacity_cap_of_lists(fields):
    """The sizes alone are past the caps: the check reads no table, so the small arrays still stand in."""
    c = Lists()
    change(c, **fields)
    rc, why = c.run()
    assert rc == CAPACITY and "caps 65536 / 8192 / below 16777216" in why
    c = Lists()
    change(c, **{k: v - 1 for k, v in fields.items()})
    assert c.run() == (0, "")


def bind(n_kf=3, stride=8, n_mp=10, n_pool=64, cur=1, adj=2, n_matches=4, n_kp1=5, n_kp2=8, lists=True, **null):
    arr = arrays()
    L = mi355slam.ObsListsC(*[None] * len(mi355slam.ObsListsC._fields_))
    keep = [np.zeros(8, np.int32), np.zeros(16, np.int32)]
    L.rows, L.obs_desc = (None if null.get(k) else a.ctypes.data for k, a in zip(("rows", "obs_desc"), keep))

    def p(k, name=None):
        if null.get(name or k):
            return C.c_void_p(0)
        return C.c_void_p((arr[k].ctypes.data + 15) // 16 * 16 + int(null.get("shift_" + k, 0)))

    n, why = C.c_int32(0), C.create_string_buffer(512)
    rc = mi355slam.lib().ms_create_points_bind_check(p("kf_mp"), n_kf, stride, p("mp_flags"), p("mp_live"), p("mp_desc"), p("n_obs"), p("mp_track"), n_mp, p("desc_pool"), n_pool,
                                                     cur, adj, C.byref(L) if lists else None, p("match_kp1"), p("match_kp2"), n_matches, n_kp1, n_kp2, p("usable", "usable1"),
                                                     p("usable", "usable2"), p("created", "created_rows"), p("created", "created_kp1"), p("created", "created_kp2"),
                                                     None if null.get("n_created") else C.byref(n), why, C.c_size_t(512))
    return rc, why.value.decode()


def test_bind_check():
    assert bind() == (0, "")
    assert bind(n_matches=0, lists=False, match_kp1=True, match_kp2=True) == (0, "")
    assert bind(n_obs=True, mp_track=True, usable1=True, usable2=True, created_rows=True, created_kp1=True, created_kp2=True) == (0, "")      # every optional array absent
    assert bind(desc_pool=True, mp_desc=True) == (0, "") and bind(obs_desc=True, mp_desc=True) == (0, "")                                    # no descriptor half
    for kw, message in ((dict(cur=3), "slot 3 outside [0, 3)"), (dict(adj=-1), "slot -1 outside [0, 3)"), (dict(adj=1), "both slot 1"), (dict(stride=0), "stride 0"),
                        (dict(n_matches=-1), "negative size"), (dict(n_mp=-1), "negative size"), (dict(n_kp2=-1), "negative size"),
                        (dict(n_kp1=9), "9 keypoints in a table of stride 8"), (dict(n_kp2=9), "9 keypoints in a table of stride 8"), (dict(n_created=True), "missing array (n_created)"),
                        (dict(kf_mp=True), "missing array (kf_mp, mp_flags or mp_live)"), (dict(mp_flags=True), "missing array (kf_mp, mp_flags or mp_live)"),
                        (dict(mp_live=True), "missing array (kf_mp, mp_flags or mp_live)"), (dict(lists=False), "missing array (rows, match_kp1 or match_kp2)"),
                        (dict(rows=True), "missing array (rows, match_kp1 or match_kp2)"), (dict(match_kp1=True), "missing array (rows, match_kp1 or match_kp2)"),
                        (dict(match_kp2=True), "missing array (rows, match_kp1 or match_kp2)"), (dict(mp_desc=True), "missing array (mp_desc)"),
                        (dict(shift_mp_desc=4), "16-byte aligned"), (dict(shift_desc_pool=8), "16-byte aligned")):
        rc, why = bind(**kw)
        assert rc == INVALID and why.startswith("create points bind: ") and message in why, (kw, why)
    for kw in (dict(n_kf=MAX_KF + 1), dict(stride=MAX_STRIDE + 1), dict(n_mp=MAX_MP), dict(n_matches=MAX_STRIDE + 1)):
        rc, why = bind(**kw)
        assert rc == CAPACITY and "caps 65536 / 8192 / below 16777216 / 8192" in why, (kw, why)
    assert bind(n_matches=MAX_STRIDE) == (0, "")


def mask(n_kf=3, stride=8, n_mp=10, slots=(2, 0), n_kp=(8, 3), null=(), kf_mp=True, n_slots=None):
    arr = arrays()
    s, k = np.array(slots, np.int32), np.array(n_kp, np.int32)
    bufs = [np.zeros(8, np.uint8) for _ in slots]
    ptrs = (C.c_void_p * max(len(slots), 1))(*[None if i in null else b.ctypes.data for i, b in enumerate(bufs)])
    why = C.create_string_buffer(512)
    rc = mi355slam.lib().ms_unbound_mask_check(mi355slam._vp(arr["kf_mp"] if kf_mp else None), n_kf, stride, n_mp, mi355slam._vp(s) if len(s) else None,
                                               mi355slam._vp(k) if len(k) else None, ptrs, len(slots) if n_slots is None else n_slots, why, C.c_size_t(512))
    return rc, why.value.decode()


def test_unbound_mask_check():
    assert mask() == (0, "") and mask(slots=(), n_kp=()) == (0, "") and mask(n_kp=(0, 3), null=(0,)) == (0, "")
    for kw, message in ((dict(slots=(3, 0)), "slot 3 outside [0, 3)"), (dict(slots=(-1, 0)), "slot -1 outside [0, 3)"), (dict(n_kp=(9, 3)), "9 keypoints in a table of stride 8"),
                        (dict(n_kp=(8, -1)), "-1 keypoints"), (dict(null=(1,)), "missing array (usable of slot 0)"), (dict(kf_mp=False), "missing array (kf_mp, slots, n_kp or usable)"),
                        (dict(stride=0), "stride 0"), (dict(n_slots=-1), "negative size")):
        rc, why = mask(**kw)
        assert rc == INVALID and why.startswith("unbound mask: ") and message in why, (kw, why)
    for kw in (dict(n_kf=MAX_KF + 1), dict(stride=MAX_STRIDE + 1), dict(n_mp=MAX_MP)):
        rc, why = mask(**kw)
        assert rc == CAPACITY and "caps 65536 / 8192 / below 16777216 / 4096" in why, (kw, why)
