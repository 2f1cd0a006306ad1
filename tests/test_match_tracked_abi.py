"""CPU checks of the surface of the device matchTrackedFeatures: the library exports the four calls, ms_tracked_frame has the
layout ctypes gives it, and the host-only halves that run in front of any device call -- ms_match_tracked_check and
ms_match_tracked_finish_check -- turn every MS_ERR_INVALID case away with its message, hold every capacity cap and accept the empty cases.
The checks dereference HOST arguments only, so host arrays stand in for the device tables."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mi355slam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_match_tracked", "ms_match_tracked_check", "ms_match_tracked_finish", "ms_match_tracked_finish_check")
INVALID, CAPACITY = mi355slam.MS_ERR_INVALID, mi355slam.MS_ERR_CAPACITY
MAX_KF, MAX_STRIDE, MAX_MP, MAX_WINDOW = 65536, 8192, 1 << 24, 1 << 24


def test_library_exports_the_calls_and_python_binds_them():
    for name in NAMES:
        assert hasattr(mi355slam.lib(), name), name
    for name in ("match_tracked", "match_tracked_device", "match_tracked_bind", "match_tracked_refresh"):
        assert callable(getattr(mi355slam.KeyframeTable, name)), name
    assert callable(mi355slam.TrackTable) and callable(mi355slam.MapPointTable.match_tracked_finish_device)
    mk = open(os.path.join(ROOT, "slam-module_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmatch_tracked\.hip\b", mk, flags=re.M)


def test_the_check_twins_take_the_arguments_of_the_calls():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355slam.h")).read(), flags=re.S)

    def declaration(name):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        return [" ".join(p.split()).replace("const ", "") for p in m.group(1).split(",")]

    call, check = declaration("ms_match_tracked"), declaration("ms_match_tracked_check")
    packed = ["int32_t *created_rows", "int32_t *created_kp", "int32_t *tracked_rows", "int32_t *checked_rows"]
    assert [p for p in call[1:] if p not in packed] == check[:-2] and check[-2:] == ["char *why", "size_t why_bytes"]
    call, check = declaration("ms_match_tracked_finish"), declaration("ms_match_tracked_finish_check")
    assert call[1:] == check[:-2] and check[-2:] == ["char *why", "size_t why_bytes"]


def test_struct_layout_matches_the_header(tmp_path):
    T = mi355slam.TrackedFrameC
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mi355slam.h"', "int main(void) {", 'printf("%zu", sizeof(ms_tracked_frame));']
    lines += ['printf(" %%zu", offsetof(ms_tracked_frame, %s));' % f for f, _ in T._fields_]
    lines += ['printf("\\n%d %d %d %d\\n", MS_TRACKED_MAX_WINDOW, MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP);', "return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    got = [int(x) for x in out[0].split()]
    assert got[0] == C.sizeof(T) and got[1:] == [getattr(T, f).offset for f, _ in T._fields_]
    assert [int(x) for x in out[1].split()] == [MAX_WINDOW, MAX_KF, MAX_STRIDE, MAX_MP]


class Call:
    """One call of ms_match_tracked_check: 3 slots x 8, 10 map points, a window of 6 track ids from 100, a frame of 5 keypoints in slot 1."""

    def __init__(self):
        self.n_kf, self.stride, self.n_mp, self.n_pool, self.n_track = 3, 8, 10, 64, 6
        a = lambda n, dt: np.zeros(max(n, 1), dt)
        self.arrays = dict(kf_mp=np.full(24, -1, np.int32), mp_flags=a(10, np.uint8), mp_live=a(10, np.uint8), mp_pos=a(30, np.float64), mp_norm=a(30, np.float32),
                           mp_min_dist=a(10, np.float32), mp_max_dist=a(10, np.float32), mp_desc=a(80 + 8, np.uint32), mp_track=a(10, np.int32), kp_x=a(24, np.float32),
                           kp_y=a(24, np.float32), kp_octave=a(24, np.int32), desc_pool=a(64 * 8 + 8, np.uint32), track_row=a(6, np.int32), outcome=a(5, np.uint8),
                           counts=a(5, np.int32))
        self.sigma = np.array([1.0, 1.44, 2.07, 2.99], np.float32)
        self.frame = dict(slot=1, pose=np.eye(3, 4).reshape(12), cam=(450.0, 450.0, 320.0, 240.0, 640, 480), focal=450, desc_base=8, track_base=100, sigma=True,
                          n_levels=4, rel=0.004, cos=0.5, null=False)
        self.kp_track = np.array([100, -1, 105, 103, -1], np.int32)
        self.new_rows = np.array([9, 4, 7], np.int32)
        self.n_kp, self.n_new = 5, 3
        self.align = {}                                      # array name -> byte offset added to its pointer

    def ptr(self, name):
        a = self.arrays.get(name)
        if a is None:
            return C.c_void_p(0)
        base = a.ctypes.data
        if name in ("mp_desc", "desc_pool"):                 # numpy gives 16-byte alignment or better for these sizes; make it exact, then shift on request
            base = (base + 15) // 16 * 16 + self.align.get(name, 0)
        return C.c_void_p(base)

    def run(self):
        f = self.frame
        Fr = mi355slam.TrackedFrameC(f["slot"], (C.c_double * 12)(*f["pose"]), mi355slam.Pinhole(*f["cam"]), f["focal"], f["desc_base"], f["track_base"],
                                     self.sigma.ctypes.data if f["sigma"] else None, f["n_levels"], f["rel"], f["cos"])
        why = C.create_string_buffer(512)
        p = self.ptr
        rc = mi355slam.lib().ms_match_tracked_check(p("kf_mp"), self.n_kf, self.stride, p("mp_flags"), p("mp_live"), p("mp_pos"), p("mp_norm"), p("mp_min_dist"),
                                                    p("mp_max_dist"), p("mp_desc"), p("mp_track"), self.n_mp, p("kp_x"), p("kp_y"), p("kp_octave"), p("desc_pool"),
                                                    self.n_pool, p("track_row"), self.n_track, None if f["null"] else C.byref(Fr),
                                                    mi355slam._vp(self.kp_track), self.n_kp, mi355slam._vp(self.new_rows), self.n_new, p("outcome"), p("counts"), why,
                                                    C.c_size_t(512))
        return rc, why.value.decode()


def test_a_valid_call_and_the_empty_cases_pass():
    assert Call().run() == (0, "")
    c = Call(); c.n_kp = 0; c.kp_track = None; c.arrays["outcome"] = None
    assert c.run() == (0, "")
    c = Call(); c.n_new = 0; c.new_rows = None
    assert c.run() == (0, "")
    c = Call(); c.frame["desc_base"] = -1; c.arrays["desc_pool"] = None; c.n_pool = 0
    assert c.run() == (0, "")
    c = Call(); c.n_kp = 8                                   # n_kp == stride
    c.kp_track = np.array([100, -1, 105, 103, -1, -7, 101, 102], np.int32)
    c.arrays["outcome"] = np.zeros(8, np.uint8)
    assert c.run() == (0, "")


def change(c, **kw):
    for k, v in kw.items():
        if k in c.frame:
            c.frame[k] = v
        elif k in c.arrays:
            c.arrays[k] = v
        else:
            setattr(c, k, v)


INVALID_CASES = [
    (dict(slot=-1), "slot -1 outside [0, 3)"), (dict(slot=3), "slot 3 outside [0, 3)"),
    (dict(kp_track=np.array([100, 103, 105, 103, -1], np.int32)), "track id 103 is listed twice"),
    (dict(kp_track=np.array([100, 106, -1, -1, -1], np.int32)), "keypoint 1: track id 106 outside the window [100, 100 + 6)"),
    (dict(kp_track=np.array([99, -1, -1, -1, -1], np.int32)), "keypoint 0: track id 99 outside the window"),
    (dict(new_rows=np.array([9, 4, 9], np.int32)), "new row 9 is listed twice"),
    (dict(new_rows=np.array([9, 10, 7], np.int32)), "new row 10 outside [0, 10)"),
    (dict(new_rows=np.array([-1, 4, 7], np.int32)), "new row -1 outside [0, 10)"),
    (dict(rel=float("nan")), "is not finite"), (dict(cos=float("inf")), "is not finite"),
    (dict(n_levels=0), "0 levels outside [1, 32]"), (dict(n_levels=33), "33 levels outside [1, 32]"),
    (dict(sigma=False), "missing array (level_sigma_sq)"), (dict(null=True), "missing array (frame or counts)"), (dict(counts=None), "missing array (frame or counts)"),
    (dict(n_kp=9), "9 keypoints in a table of stride 8"),
    (dict(stride=0), "stride 0"), (dict(n_mp=-1), "negative size"), (dict(n_new=-1), "negative size"), (dict(n_track=-1), "negative size"),
    (dict(kf_mp=None), "missing array (kf_mp or the keypoint table)"), (dict(kp_octave=None), "missing array (kf_mp or the keypoint table)"),
    (dict(mp_track=None), "missing array (the map-point table)"), (dict(mp_live=None), "missing array (the map-point table)"),
    (dict(mp_norm=None), "missing array (the map-point table)"), (dict(track_row=None), "missing array (track_row)"),
    (dict(outcome=None), "missing array (kp_track or outcome)"), (dict(kp_track=None), "missing array (kp_track or outcome)"),
    (dict(new_rows=None), "missing array (new_rows)"),
    (dict(cam=(450.0, 450.0, 320.0, 240.0, 0, 480)), "bad camera"), (dict(cam=(0.0, 450.0, 320.0, 240.0, 640, 480)), "bad camera"),
    (dict(cam=(450.0, float("inf"), 320.0, 240.0, 640, 480)), "bad camera"),
    (dict(desc_base=60), "descriptors [60, 60 + 5) outside the pool of 64"), (dict(desc_pool=None), "outside the pool of 0"),
    (dict(align=dict(mp_desc=4)), "16-byte aligned"), (dict(align=dict(desc_pool=8)), "16-byte aligned"),
]


@pytest.mark.parametrize("fields,message", INVALID_CASES, ids=[m[:40] + "/" + ",".join(f) for f, m in INVALID_CASES])
def test_each_invalid_case_is_turned_away_with_its_message(fields, message):
    c = Call()
    change(c, **fields)
    rc, why = c.run()
    assert rc == INVALID and why.startswith("match tracked: ") and message in why, why


def test_non_finite_level_sigma_is_invalid():
    c = Call()
    c.sigma[2] = np.inf
    rc, why = c.run()
    assert rc == INVALID and "level_sigma_sq[2] is not finite" in why


@pytest.mark.parametrize("fields", [dict(n_kf=MAX_KF + 1), dict(stride=MAX_STRIDE + 1), dict(n_mp=MAX_MP), dict(n_track=MAX_WINDOW + 1)], ids=lambda f: next(iter(f)))
def test_each_capacity_cap(fields):
    """The sizes alone are past the caps: the check reads no table, so the small arrays still stand in."""
    c = Call()
    change(c, **fields)
    rc, why = c.run()
    assert rc == CAPACITY and "caps 65536 / 8192 / below 16777216 / 16777216" in why
    c = Call()
    change(c, **{k: v - 1 for k, v in fields.items()})
    assert c.run() == (0, "")


def finish(n_rows=3, n_checked=2, append=1, cap=5, n_mp=10, lists=True, **null):
    i32 = lambda n: np.zeros(max(n, 1), np.int32)
    L = mi355slam.ObsListsC(*[None] * len(mi355slam.ObsListsC._fields_))
    keep = [i32(n_rows), i32(n_rows + 1), i32(8)]
    L.rows, L.obs_start, L.obs_desc = (None if null.get(k) else a.ctypes.data for k, a in zip(("rows", "obs_start", "obs_desc"), keep))
    arr = dict(mp_flags=np.zeros(10, np.uint8), desc_pool=np.zeros(64, np.uint32), mp_desc=np.zeros(96, np.uint32), checked_rows=i32(n_checked), refresh_rows=i32(cap))
    p = lambda k: C.c_void_p(0) if null.get(k) else C.c_void_p((arr[k].ctypes.data + 15) // 16 * 16 + int(null.get("shift_" + k, 0)))
    n_refresh = C.c_int32(0)
    why = C.create_string_buffer(512)
    rc = mi355slam.lib().ms_match_tracked_finish_check(C.byref(L) if lists else None, n_rows, p("mp_flags"), p("desc_pool"), p("mp_desc"), n_mp, p("checked_rows"), n_checked,
                                                       append, p("refresh_rows"), cap, None if null.get("n_refresh") else C.byref(n_refresh), why, C.c_size_t(512))
    return rc, why.value.decode()


def test_finish_check():
    assert finish() == (0, "")
    assert finish(n_rows=0, n_checked=0, cap=0, lists=False, refresh_rows=True, checked_rows=True, mp_flags=True) == (0, "")
    assert finish(append=0, cap=3) == (0, "")                # the checked rows are not appended: the tracked rows alone must fit
    assert finish(desc_pool=True, mp_desc=True) == (0, "")   # no descriptor half
    for kw, message in ((dict(n_rows=-1), "negative size"), (dict(cap=-1), "negative size"), (dict(n_refresh=True), "missing array (n_refresh)"),
                        (dict(lists=False), "missing array (rows, obs_start or mp_flags)"), (dict(rows=True), "missing array (rows, obs_start or mp_flags)"),
                        (dict(obs_start=True), "missing array (rows, obs_start or mp_flags)"), (dict(mp_flags=True), "missing array (rows, obs_start or mp_flags)"),
                        (dict(mp_desc=True), "missing array (mp_desc)"), (dict(checked_rows=True), "missing array (checked_rows)"),
                        (dict(refresh_rows=True), "missing array (refresh_rows)"), (dict(shift_mp_desc=4), "16-byte aligned"), (dict(shift_desc_pool=8), "16-byte aligned")):
        rc, why = finish(**kw)
        assert rc == INVALID and why.startswith("match tracked finish: ") and message in why, (kw, why)
    for kw in (dict(cap=4), dict(append=0, cap=2), dict(n_rows=MAX_STRIDE + 1, cap=3 * MAX_STRIDE), dict(n_checked=MAX_STRIDE + 1, cap=3 * MAX_STRIDE), dict(n_mp=MAX_MP)):
        rc, why = finish(**kw)
        assert rc == CAPACITY and "refresh_rows holds" in why, (kw, why)
