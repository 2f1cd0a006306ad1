"""CPU checks of the surface of the bind step: the header declares the calls, the library exports them, Python binds them, and
the host-only halves that run in front of any device call -- ms_bound_mask_check and ms_search_bind_check -- turn every MS_ERR_INVALID case
away with its message, hold every cap and accept the zero sizes.  The checks dereference HOST arguments only, so host arrays stand in for the
device tables."""
import ctypes as C
import os
import re

import numpy as np

import mi355slam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_bound_mask", "ms_bound_mask_check", "ms_search_bind", "ms_search_bind_check")
INVALID, CAPACITY = mi355slam.MS_ERR_INVALID, mi355slam.MS_ERR_CAPACITY
MAX_KF, MAX_STRIDE, MAX_MP, MAX_ENTRIES = 65536, 8192, 1 << 24, 1 << 24
DEVICE = ("kept_entry", "q_x", "q_y", "q_radius", "q_min_octave", "q_max_octave", "q_desc", "top_idx", "top_dist", "top_octave", "n_scored", "skip",
          "sorted_x", "sorted_y", "sorted_idx", "t_desc", "t_octave")


def test_library_exports_the_calls_and_python_binds_them():
    for name in NAMES:
        assert hasattr(mi355slam.lib(), name), name
    for name in ("bound_mask", "search_bind"):
        assert callable(getattr(mi355slam.KeyframeTable, name)), name
    assert set(DEVICE) - {"sorted_x", "sorted_y", "sorted_idx", "t_desc", "t_octave"} < set(mi355slam.SearchBindArgs.FIELDS)
    mk = open(os.path.join(ROOT, "slam-module_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bsearch_bind\.hip\b", mk, flags=re.M)


def test_the_check_twins_take_the_arguments_of_the_calls():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355slam.h")).read(), flags=re.S)

    def declaration(name):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        return [" ".join(p.split()).replace("const ", "") for p in m.group(1).split(",")]

    call, check = declaration("ms_bound_mask"), declaration("ms_bound_mask_check")
    assert call[1:] == check[:-2] and check[-2:] == ["char *why", "size_t why_bytes"]
    call, check = declaration("ms_search_bind"), declaration("ms_search_bind_check")
    outputs = ["int32_t *match_kp", "uint8_t *outcome", "uint8_t *usable"]
    assert [p for p in call[1:] if p not in outputs] == check[:-2] and check[-2:] == ["char *why", "size_t why_bytes"]
    assert len(call) == 35 and [p.split("*")[-1].split()[-1] for p in call[7:24]] == list(DEVICE)


def test_caps_match_the_header(tmp_path):
    import subprocess
    src, exe = tmp_path / "caps.c", tmp_path / "caps"
    src.write_text('#include <stdio.h>\n#include "mi355slam.h"\nint main(void) { printf("%d %d %d %d %d\\n", MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, '
                   "MS_GATE_MAX_ENTRIES, MS_HAMMING_THR_HIGH); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == [MAX_KF, MAX_STRIDE, MAX_MP, MAX_ENTRIES, 100]


class Call:
    """One call of either check: 3 slots x 8, 10 map points, a keyframe of 6 keypoints in slot 1; a slice of 5 entries from entry 2 on, 3 kept."""

    def __init__(self):
        self.n_kf, self.stride, self.n_mp, self.n_kp, self.slot = 3, 8, 10, 6, 1
        self.first, self.count, self.n_kept = 2, 5, 3
        a = lambda n, dt: np.zeros(max(n, 1), dt)
        self.arrays = dict(kf_mp=np.full(24, -1, np.int32), mp_live=a(10, np.uint8), n_obs=a(10, np.int32), n_matched=a(1, np.int32), counts=a(6, np.int32),
                           mp_index=np.array([77, -3, 4, 2, 9, 0, 7, 55], np.int32), **{k: a(64, np.uint32) for k in DEVICE})

    def ptr(self, name):
        v = self.arrays.get(name)
        if isinstance(v, int):
            return C.c_void_p(v)
        return C.c_void_p(0) if v is None else C.c_void_p(v.ctypes.data)

    def mask(self):
        why = C.create_string_buffer(512)
        rc = mi355slam.lib().ms_bound_mask_check(self.ptr("kf_mp"), self.n_kf, self.stride, self.n_mp, self.slot, self.n_kp, self.ptr("skip"), why, C.c_size_t(512))
        return rc, why.value.decode()

    def bind(self, why_bytes=512):
        p, why = self.ptr, C.create_string_buffer(512)
        rc = mi355slam.lib().ms_search_bind_check(p("kf_mp"), self.n_kf, self.stride, p("mp_live"), p("n_obs"), self.n_mp, *[p(k) for k in DEVICE], self.n_kp,
                                                  p("mp_index"), self.first, self.count, self.n_kept, self.slot, p("n_matched"), p("counts"),
                                                  why if why_bytes else None, C.c_size_t(why_bytes))
        return rc, why.value.decode()


def changed(**kw):
    c = Call()
    for k, v in kw.items():
        if k in c.arrays:
            c.arrays[k] = v
        else:
            assert hasattr(c, k), k
            setattr(c, k, v)
    return c


def test_valid_calls_and_the_zero_sizes_pass():
    assert Call().mask() == (0, "") and Call().bind() == (0, "")
    assert changed(n_kp=0, skip=None).mask() == (0, "") and changed(n_kp=8).mask() == (0, "") and changed(n_mp=0).mask() == (0, "")
    assert changed(n_kept=0, **{k: None for k in DEVICE}).bind() == (0, "")                                     # no kept query: no list is needed
    assert changed(count=0, n_kept=0, mp_index=None, **{k: None for k in DEVICE}).bind() == (0, "")
    assert changed(q_min_octave=None).bind() == (0, "") and changed(q_max_octave=None).bind() == (0, "")       # no window on that side
    assert changed(n_kept=5).bind() == (0, "")                                                                  # n_kept == count; the entries outside the slice are not read
    assert changed(n_kp=0, skip=None, sorted_x=None, sorted_y=None, sorted_idx=None, t_desc=None, t_octave=None).bind() == (0, "")      # a keyframe without keypoints


def test_every_invalid_mask_call_is_turned_away_and_every_cap_holds():
    cases = [(dict(n_kf=-1), "negative size"), (dict(n_mp=-1), "negative size"), (dict(n_kp=-1), "negative size"), (dict(stride=0), "stride 0"),
             (dict(kf_mp=None), "missing array (kf_mp)"), (dict(skip=None), "missing array (skip)"), (dict(slot=3), "slot 3 outside [0, 3)"),
             (dict(slot=-1), "slot -1 outside [0, 3)"), (dict(n_kp=9), "9 keypoints for a stride of 8")]
    for kw, text in cases:
        rc, why = changed(**kw).mask()
        assert rc == INVALID and text in why and why.startswith("bound mask: "), (kw, rc, why)
    for kw, text in ((dict(n_kf=MAX_KF + 1), "65537 slots"), (dict(stride=MAX_STRIDE + 1), "stride 8193"), (dict(n_mp=MAX_MP), "16777216 map points")):
        rc, why = changed(**kw).mask()
        assert rc == CAPACITY and text in why, (kw, rc, why)
    for kw in (dict(n_kf=MAX_KF), dict(stride=MAX_STRIDE), dict(n_mp=MAX_MP - 1)):
        assert changed(**kw).mask() == (0, "")


def test_every_invalid_bind_call_is_turned_away_with_its_message():
    cases = [
        (dict(n_kf=-1), "negative size"), (dict(n_mp=-1), "negative size"), (dict(n_kp=-1), "negative size"), (dict(stride=0), "stride 0"),
        (dict(first=-1), "negative size (first -1"), (dict(count=-1), "negative size"), (dict(n_kept=-1), "negative size"),
        (dict(kf_mp=None), "missing array (kf_mp)"), (dict(slot=3), "slot 3 outside [0, 3)"), (dict(slot=-1), "slot -1 outside"),
        (dict(n_kp=9), "9 keypoints for a stride of 8"), (dict(n_kept=6), "n_kept 6 for a slice of 5"),
        (dict(n_matched=None), "missing array (n_matched or counts)"), (dict(counts=None), "missing array (n_matched or counts)"),
        (dict(mp_live=None), "missing array (mp_live or n_obs)"), (dict(n_obs=None), "missing array (mp_live or n_obs)"), (dict(mp_index=None), "missing array (mp_index)"),
        (dict(mp_index=np.array([77, -3, 4, 2, 10, 0, 7, 55], np.int32)), "entry 4 is row 10 outside [0, 10)"),
        (dict(mp_index=np.array([77, -3, 4, 2, 9, 0, -1, 55], np.int32)), "entry 6 is row -1 outside [0, 10)"),
        (dict(first=1), "entry 1 is row -3 outside [0, 10)"),
    ]
    cases += [(dict(**{k: None}), "missing array (a list of the gate or of the scoring)") for k in DEVICE[:11] if k not in ("q_min_octave", "q_max_octave")]
    cases += [(dict(**{k: None}), "missing array (skip or a keyframe array)") for k in DEVICE[11:]]
    for kw, text in cases:
        rc, why = changed(**kw).bind()
        assert rc == INVALID and text in why and why.startswith("search bind: "), (kw, rc, why)
    c = Call()
    for k in ("q_desc", "t_desc"):
        rc, why = changed(**{k: c.arrays[k].ctypes.data + 4}).bind()
        assert rc == INVALID and "16-byte aligned" in why, (k, rc, why)
    assert changed(stride=0).bind(why_bytes=0)[0] == INVALID                                                    # no buffer for the message


def test_every_cap_of_the_bind_call_holds():
    big = [(dict(n_kf=MAX_KF + 1), "65537 slots"), (dict(stride=MAX_STRIDE + 1), "stride 8193"), (dict(n_mp=MAX_MP), "16777216 map points"),
           (dict(count=MAX_ENTRIES, first=0), "cap below 16777216 entries"), (dict(first=MAX_ENTRIES - 5), "cap below 16777216 entries")]
    for kw, text in big:
        rc, why = changed(**kw).bind()
        assert rc == CAPACITY and text in why, (kw, rc, why)
    for kw in (dict(n_kf=MAX_KF), dict(stride=MAX_STRIDE)):
        assert changed(**kw).bind() == (0, "")
    assert changed(n_mp=MAX_MP - 1).bind() == (0, "")
    rc, why = changed(first=MAX_ENTRIES - 6, n_kept=6).bind()                                                   # the last slice below the cap passes the capacity check
    assert rc == INVALID and "n_kept 6" in why
