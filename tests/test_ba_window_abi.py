"""CPU checks of the surface of the device BA window: the library exports ms_ba_window_lists, ms_ba_window_apply and their
*_check twins with the header's signatures, Python binds them, and the host-only halves that run in front of any device call turn every
MS_ERR_INVALID case away with its message, hold the capacity caps and accept the empty cases.  The checks dereference HOST arguments only,
so host arrays stand in for the device tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mi355slam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_ba_window_lists", "ms_ba_window_lists_check", "ms_ba_window_apply", "ms_ba_window_apply_check")
INVALID, CAPACITY = mi355slam.MS_ERR_INVALID, mi355slam.MS_ERR_CAPACITY
MAX_KF, MAX_STRIDE, MAX_MP, MAX_ROWS, MAX_OBS = 65536, 8192, 1 << 24, 1 << 24, 1 << 22


def header():
    return open(os.path.join(ROOT, "include", "mi355slam.h")).read()


def test_library_exports_the_calls_and_python_binds_them():
    for name in NAMES:
        assert hasattr(mi355slam.lib(), name), name
    for name in ("ba_window_lists_device", "ba_window", "ba_window_apply"):
        assert callable(getattr(mi355slam.KeyframeTable, name)), name
    assert [k for k, _ in mi355slam.BaWindowDevC._fields_] == ["edge_slot", "edge_kp", "edge_point"]
    mk = open(os.path.join(ROOT, "slam-module_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bba_window\.hip\b", mk, flags=re.M)


def test_the_header_declares_the_struct_and_the_modes_the_binding_uses():
    hdr = header()
    m = re.search(r"typedef struct \{([^}]*)\} ms_ba_window_dev;", hdr)
    assert m and re.sub(r"/\*.*?\*/", "", m.group(1)).split() == ["int32_t", "*edge_slot,", "*edge_kp,", "*edge_point;"]
    for name, value in (("MS_BA_APPLY_LOCAL", mi355slam.BA_APPLY_LOCAL), ("MS_BA_APPLY_NEIGHBOR", mi355slam.BA_APPLY_NEIGHBOR)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), hdr), name


def test_the_check_twins_take_the_arguments_of_the_calls():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)

    def declaration(name):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        return [" ".join(p.split()).replace("const ", "") for p in m.group(1).split(",")]

    for name, n_args in (("ms_ba_window_lists", 26), ("ms_ba_window_apply", 25)):
        call, check = declaration(name), declaration(name + "_check")
        assert call[0] == "ms_ctx *ctx" and call[1:] == check[:-2] and check[-2:] == ["char *why", "size_t why_bytes"], name
        assert len(call) == n_args, (name, len(call))        # what the binding passes, argument for argument
    src = open(os.path.join(ROOT, "slam-module_amd", "mi355slam", "__init__.py")).read()
    for name, n_args in (("ms_ba_window_lists", 26), ("ms_ba_window_apply", 25)):
        m = re.search(r"lib\(\)\.%s\((.*?)\)\n" % name, src, flags=re.S)
        depth, count = 0, 1
        for ch in m.group(1):
            depth += ch in "(["
            depth -= ch in ")]"
            count += ch == "," and depth == 0
        assert count == n_args, (name, count)


def test_the_kernels_use_the_shared_scan_and_workspace():
    src = open(os.path.join(ROOT, "slam-module_amd", "csrc", "ba_window.hip")).read()
    assert '#include "ms_scan.h"' in src and "block_rank<kBlock>" in src and "block_offsets<kBlock>" in src and "MS_WS_BA_WINDOW" in src and "ms_pinned(" in src
    assert "MS_WS_BA_WINDOW" in open(os.path.join(ROOT, "slam-module_amd", "csrc", "ms_internal.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "__shfl_up" not in code and re.findall(r"atomic\w*\s*\(", code) == ["atomicSub("]        # no scan of its own; the integer decrement and no other atomic


class Lists:
    """One call of ms_ba_window_lists_check: 5 slots, 20 map points, 6 listed rows with 14 observations, 3 local slots."""

    def __init__(self):
        self.n_kf, self.n_mp, self.n_rows, self.n_obs = 5, 20, 6, 14
        self.arrays = dict(kf_pose=np.zeros(60), mp_pos=np.zeros(60), pose=np.zeros(21), point=np.zeros(18), obs_point=np.zeros(14, np.int32), obs_pose=np.zeros(14, np.int32),
                           obs_uv=np.zeros(28), obs_info=np.zeros(14), focal=np.full(5, 500, np.int32), sigma=np.array([1, 1.44, 2.0736], np.float32),
                           local=np.array([4, 0, 2], np.int32))
        self.lists = {k: np.zeros(16, np.float32 if k in ("obs_x", "obs_y", "obs_depth") else np.int32) for k, _ in mi355slam.ObsListsC._fields_}
        self.window = {k: np.zeros(14, np.int32) for k, _ in mi355slam.BaWindowDevC._fields_}
        self.cams = [[500.0, 501.0, 320.0, 240.0, 640, 480] for _ in range(5)]
        self.n_local, self.current, self.n_levels, self.cap_point, self.cap_edge = 3, 0, 3, 6, 14
        self.null_lists = self.null_window = self.null_cams = self.null_n_edge = self.null_n_current = False

    def run(self):
        p = lambda k: mi355slam._vp(self.arrays.get(k))
        L = mi355slam.ObsListsC(*[None if self.lists.get(k) is None else self.lists[k].ctypes.data for k, _ in mi355slam.ObsListsC._fields_])
        Wd = mi355slam.BaWindowDevC(*[None if self.window.get(k) is None else self.window[k].ctypes.data for k, _ in mi355slam.BaWindowDevC._fields_])
        K = (mi355slam.Pinhole * 5)(*[mi355slam.Pinhole(c[0], c[1], c[2], c[3], int(c[4]), int(c[5])) for c in self.cams])
        n_edge, n_current, why = C.c_int32(0), C.c_int32(0), C.create_string_buffer(512)
        rc = mi355slam.lib().ms_ba_window_lists_check(p("kf_pose"), self.n_kf, p("mp_pos"), self.n_mp, None if self.null_lists else C.byref(L), self.n_rows, self.n_obs,
                                                      p("local"), self.n_local, self.current, None if self.null_cams else K, p("focal"), p("sigma"), self.n_levels,
                                                      p("pose"), p("point"), p("obs_point"), p("obs_pose"), p("obs_uv"), p("obs_info"), self.cap_point, self.cap_edge,
                                                      None if self.null_window else C.byref(Wd), None if self.null_n_edge else C.byref(n_edge),
                                                      None if self.null_n_current else C.byref(n_current), why, C.c_size_t(512))
        return rc, why.value.decode()


def change(c, **kw):
    for k, v in kw.items():
        if k in c.arrays:
            c.arrays[k] = v
        elif k.startswith("L_"):
            c.lists[k[2:]] = v
        elif k.startswith("W_"):
            c.window[k[2:]] = v
        elif k.startswith("cam"):
            slot, field = int(k[3]), "fx fy cx cy".split().index(k[5:])
            c.cams[slot][field] = v
        else:
            setattr(c, k, v)


def test_a_valid_lists_call_and_the_empty_cases_pass():
    assert Lists().run() == (0, "")
    c = Lists(); change(c, n_rows=0, n_obs=0, null_lists=True, mp_pos=None, cap_point=0, cap_edge=0, point=None, obs_point=None, obs_pose=None, obs_uv=None, obs_info=None,
                        null_window=True)
    assert c.run() == (0, "")                                # poses only
    c = Lists(); change(c, n_obs=0, L_obs_kf=None, L_obs_x=None)
    assert c.run() == (0, "")
    c = Lists(); change(c, n_local=1, local=np.array([3], np.int32))
    assert c.run() == (0, "")
    c = Lists(); change(c, cap_point=0, cap_edge=0, point=None, obs_uv=None, null_window=True)     # a call that asks for the counts
    assert c.run() == (0, "")
    c = Lists(); change(c, cam1_fx=-1.0, cam3_fy=float("nan"))                                     # cameras of slots that are not local are not read
    assert c.run() == (0, "")
    c = Lists(); change(c, n_levels=32, sigma=np.ones(32, np.float32))
    assert c.run() == (0, "")


nan, inf = float("nan"), float("inf")
LISTS_INVALID = [
    (dict(local=np.array([4, 5, 2], np.int32)), "local slot 5 outside [0, 5)"), (dict(local=np.array([-1, 0, 2], np.int32)), "local slot -1 outside [0, 5)"),
    (dict(local=np.array([4, 0, 4], np.int32)), "local slot 4 is listed twice"),
    (dict(current=-1), "current index -1 outside [0, 3)"), (dict(current=3), "current index 3 outside [0, 3)"), (dict(n_local=0), "current index 0 outside [0, 0)"),
    (dict(cam4_fx=0.0), "the camera of local slot 4 has fx 0"), (dict(cam0_fy=-2.0), "the camera of local slot 0 has fx 500, fy -2"),
    (dict(cam2_fx=nan), "the camera of local slot 2 has fx nan"), (dict(cam2_fy=inf), "the camera of local slot 2 has fx 500, fy inf"),
    (dict(cam0_cx=nan), "the camera of local slot 0 has cx nan"),
    (dict(n_levels=0), "0 levels outside [1, 32]"), (dict(n_levels=33), "33 levels outside [1, 32]"), (dict(n_levels=-1), "-1 levels outside [1, 32]"),
    (dict(sigma=np.array([1, 0, 2], np.float32)), "level_sigma_sq[1] = 0"), (dict(sigma=np.array([1, 2, -1], np.float32)), "level_sigma_sq[2] = -1"),
    (dict(sigma=np.array([nan, 2, 1], np.float32)), "level_sigma_sq[0] = nan"), (dict(sigma=np.array([1, inf, 1], np.float32)), "level_sigma_sq[1] = inf"),
    (dict(n_kf=-1), "negative size"), (dict(n_mp=-1), "negative size"), (dict(n_rows=-1), "negative size"), (dict(n_obs=-1), "negative size"), (dict(n_local=-1), "negative size"),
    (dict(cap_point=-1), "negative size"), (dict(cap_edge=-1), "negative size"),
    (dict(null_n_edge=True), "missing array (n_edge or n_current)"), (dict(null_n_current=True), "missing array (n_edge or n_current)"),
    (dict(kf_pose=None), "missing array (kf_pose, kf_cam, kf_focal, level_sigma_sq or pose)"), (dict(null_cams=True), "missing array (kf_pose, kf_cam, kf_focal, level_sigma_sq or pose)"),
    (dict(focal=None), "missing array (kf_pose, kf_cam, kf_focal, level_sigma_sq or pose)"), (dict(sigma=None), "missing array (kf_pose, kf_cam, kf_focal, level_sigma_sq or pose)"),
    (dict(pose=None), "missing array (kf_pose, kf_cam, kf_focal, level_sigma_sq or pose)"),
    (dict(mp_pos=None), "missing array (mp_pos, rows or obs_start)"), (dict(null_lists=True), "missing array (mp_pos, rows or obs_start)"),
    (dict(L_rows=None), "missing array (mp_pos, rows or obs_start)"), (dict(L_obs_start=None), "missing array (mp_pos, rows or obs_start)"),
    (dict(L_obs_kf=None), "missing array (obs_kf, obs_kp, obs_x, obs_y or obs_octave)"), (dict(L_obs_kp=None), "missing array (obs_kf, obs_kp, obs_x, obs_y or obs_octave)"),
    (dict(L_obs_x=None), "missing array (obs_kf, obs_kp, obs_x, obs_y or obs_octave)"), (dict(L_obs_y=None), "missing array (obs_kf, obs_kp, obs_x, obs_y or obs_octave)"),
    (dict(L_obs_octave=None), "missing array (obs_kf, obs_kp, obs_x, obs_y or obs_octave)"), (dict(n_rows=0), "missing array (obs_kf, obs_kp, obs_x, obs_y or obs_octave)"),
    (dict(point=None), "missing array (point)"),
    (dict(obs_point=None), "missing array (obs_point, obs_pose, obs_uv, obs_info or the window's edge arrays)"),
    (dict(obs_info=None), "missing array (obs_point, obs_pose, obs_uv, obs_info or the window's edge arrays)"),
    (dict(null_window=True), "missing array (obs_point, obs_pose, obs_uv, obs_info or the window's edge arrays)"),
    (dict(W_edge_kp=None), "missing array (obs_point, obs_pose, obs_uv, obs_info or the window's edge arrays)"),
    (dict(local=None), "missing array (local_slot)"),
]


@pytest.mark.parametrize("fields,message", LISTS_INVALID, ids=[m[:36] + "/" + ",".join(f) for f, m in LISTS_INVALID])
def test_each_invalid_lists_case_is_turned_away_with_its_message(fields, message):
    c = Lists()
    change(c, **fields)
    rc, why = c.run()
    assert rc == INVALID and why.startswith("ba window lists: ") and message in why, why


@pytest.mark.parametrize("fields", [dict(n_kf=MAX_KF + 1), dict(n_mp=MAX_MP), dict(n_rows=MAX_ROWS + 1), dict(n_obs=MAX_OBS + 1)], ids=lambda f: next(iter(f)))
def test_each_capacity_cap_of_lists(fields):
    c = Lists()
    change(c, **fields)
    rc, why = c.run()
    assert rc == CAPACITY and "caps 65536 / below 16777216 / 16777216 / 4194304" in why
    c = Lists()
    change(c, **{k: v - 1 for k, v in fields.items()})
    assert c.run() == (0, "")


def apply(n_kf=5, stride=8, n_mp=20, n_pose=4, n_edge=14, n_rows=6, n_local=3, current=0, mode=0, cap_erased=14, local=(4, 0, 2), window=True, **null):
    arr = dict(kf_mp=np.zeros(40, np.int32), mp_pos=np.zeros(60), mp_flags=np.zeros(20, np.uint8), n_obs=np.zeros(20, np.int32), kf_pose=np.zeros(60), pose=np.zeros(28),
               point=np.zeros(18), chi2=np.zeros(14), rows=np.zeros(6, np.int32), local=np.array(local, np.int32), erased=np.zeros(14, np.int32))
    keep = {k: np.zeros(14, np.int32) for k, _ in mi355slam.BaWindowDevC._fields_}
    Wd = mi355slam.BaWindowDevC(*[None if null.get(k) else keep[k].ctypes.data for k, _ in mi355slam.BaWindowDevC._fields_])
    p = lambda k: C.c_void_p(0) if null.get(k) else mi355slam._vp(arr[k])
    n_erased, n_stale, why = C.c_int32(0), C.c_int32(0), C.create_string_buffer(512)
    rc = mi355slam.lib().ms_ba_window_apply_check(p("kf_mp"), n_kf, stride, p("mp_pos"), p("mp_flags"), p("n_obs"), n_mp, p("kf_pose"), p("pose"), n_pose, p("point"), p("chi2"),
                                                  C.byref(Wd) if window else None, n_edge, p("rows"), n_rows, C.c_void_p(0) if null.get("null_local") else p("local"), n_local, current, mode, p("erased"), cap_erased,
                                                  None if null.get("n_erased") else C.byref(n_erased), None if null.get("n_stale") else C.byref(n_stale), why, C.c_size_t(512))
    return rc, why.value.decode()


def test_apply_check():
    assert apply() == (0, "") and apply(n_pose=3) == (0, "")
    assert apply(mode=1, kf_mp=True, mp_flags=True, n_obs=True, chi2=True, window=False, erased=True, cap_erased=0) == (0, "")       # NEIGHBOR reads none of them
    assert apply(n_edge=0, chi2=True, window=False, cap_erased=0, erased=True) == (0, "")
    assert apply(n_rows=0, n_edge=0, mp_pos=True, point=True, rows=True, chi2=True) == (0, "")
    assert apply(n_local=1, local=(3,), n_pose=1) == (0, "")
    for kw, message in ((dict(mode=2), "mode 2"), (dict(mode=-1), "mode -1"), (dict(n_pose=2), "2 poses for 3 local keyframes"), (dict(stride=0), "stride 0"),
                        (dict(local=(4, 5, 2)), "local slot 5 outside [0, 5)"), (dict(local=(4, 2, 2)), "local slot 2 is listed twice"),
                        (dict(current=3), "current index 3 outside [0, 3)"), (dict(current=-1), "current index -1 outside [0, 3)"),
                        (dict(n_kf=-1), "negative size"), (dict(n_mp=-1), "negative size"), (dict(n_pose=-1), "negative size"), (dict(n_edge=-1), "negative size"),
                        (dict(n_rows=-1), "negative size"), (dict(n_local=-1), "negative size"), (dict(cap_erased=-1), "negative size"),
                        (dict(n_erased=True), "missing array (n_erased or n_stale)"), (dict(n_stale=True), "missing array (n_erased or n_stale)"),
                        (dict(kf_pose=True), "missing array (kf_pose or pose)"), (dict(pose=True), "missing array (kf_pose or pose)"),
                        (dict(mp_pos=True), "missing array (mp_pos, point or rows)"), (dict(point=True), "missing array (mp_pos, point or rows)"),
                        (dict(rows=True), "missing array (mp_pos, point or rows)"),
                        (dict(kf_mp=True), "missing array (kf_mp, mp_flags or n_obs)"), (dict(mp_flags=True), "missing array (kf_mp, mp_flags or n_obs)"),
                        (dict(n_obs=True), "missing array (kf_mp, mp_flags or n_obs)"),
                        (dict(chi2=True), "missing array (chi2 or the window's edge arrays)"), (dict(window=False), "missing array (chi2 or the window's edge arrays)"),
                        (dict(edge_point=True), "missing array (chi2 or the window's edge arrays)"), (dict(n_rows=0), "14 edges without a row"),
                        (dict(erased=True), "missing array (erased_edge)"), (dict(null_local=True), "missing array (local_slot)")):
        rc, why = apply(**kw)
        assert rc == INVALID and why.startswith("ba window apply: ") and message in why, (kw, why)
    for kw in (dict(n_kf=MAX_KF + 1), dict(stride=MAX_STRIDE + 1), dict(n_mp=MAX_MP), dict(n_rows=MAX_ROWS + 1), dict(n_edge=MAX_OBS + 1)):
        rc, why = apply(**kw)
        assert rc == CAPACITY and "caps 65536 / 8192 / below 16777216 / 16777216 / 4194304" in why, (kw, why)
    assert apply(n_edge=MAX_OBS) == (0, "")
