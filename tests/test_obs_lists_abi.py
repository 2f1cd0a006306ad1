"""CPU checks of the surface of the observation lists: the header declares ms_observation_lists, ms_triangulate_lists,
ms_map_refresh_lists and ms_observation_lists_check with the signatures the bindings use, the library exports them, the two structs have
the layout ctypes gives them (a C program that includes the header prints it), and ms_observation_lists_check -- the host-only half that
runs in front of any device call -- turns every MS_ERR_INVALID case away with a message and accepts the empty cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mi355slam
import obs_lists_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_observation_lists", "ms_triangulate_lists", "ms_map_refresh_lists", "ms_observation_lists_check")


def declaration(name):
    hdr = open(os.path.join(ROOT, "include", "mi355slam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_calls_with_these_signatures():
    lists = declaration("ms_observation_lists")
    assert lists == ["ms_ctx *ctx", "const int32_t *kf_mp", "int n_kf", "int stride", "int n_mp", "const int32_t *kf_id", "const uint8_t *mp_flags",
                     "const float *kp_x", "const float *kp_y", "const int32_t *kp_octave", "const float *kp_depth", "const int32_t *kf_desc_base",
                     "const ms_obs_select *select", "int n_levels", "const ms_obs_lists *lists", "int cap_rows", "int cap_obs", "int32_t *n_rows", "int32_t *n_obs"]
    check = declaration("ms_observation_lists_check")
    assert [p.replace("const int32_t *n_", "int32_t *n_") for p in check] == lists[1:] + ["char *why", "size_t why_bytes"]
    assert declaration("ms_triangulate_lists") == ["ms_ctx *ctx", "double *mp_pos", "uint8_t *mp_flags", "int n_mp", "const double *kf_pose", "int n_kf",
                                                   "const ms_pinhole *kf_cam", "const int32_t *kf_focal", "const ms_obs_lists *lists", "int n_rows", "int n_obs",
                                                   "const ms_tri_settings *settings", "int mode", "uint8_t *status", "uint8_t *reason", "int32_t *n_pass"]
    assert declaration("ms_map_refresh_lists") == ["ms_ctx *ctx", "const double *mp_pos", "float *mp_norm", "float *mp_min_dist", "float *mp_max_dist", "uint32_t *mp_desc",
                                                   "int n_mp", "const double *kf_pose", "int n_kf", "const uint32_t *desc_pool", "int n_pool", "const ms_obs_lists *lists",
                                                   "int n_rows", "int n_obs", "const float *scale_factors", "int n_levels", "int promote_min_obs", "uint8_t *mp_flags",
                                                   "int32_t *medoid"]


def test_library_exports_the_calls_and_python_binds_them():
    for name in NAMES:
        assert hasattr(mi355slam.lib(), name), name
    assert callable(mi355slam.KeyframeTable.observation_lists) and callable(mi355slam.KeyframeTable.observation_lists_device)
    assert callable(mi355slam.MapPointTable.triangulate_lists) and callable(mi355slam.MapPointTable.refresh_lists)
    assert (mi355slam.OBS_FROM_ROWS, mi355slam.OBS_FROM_SLOT, mi355slam.OBS_ALL, mi355slam.OBS_REFRESH, mi355slam.OBS_RETRIANGULATE) == \
           (R.FROM_ROWS, R.FROM_SLOT, R.ALL, R.REFRESH, R.RETRIANGULATE)
    mk = open(os.path.join(ROOT, "slam-module_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bobs_lists\.hip\b", mk, flags=re.M)


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    fields = {"ms_obs_select": [f for f, _ in mi355slam.ObsSelectC._fields_], "ms_obs_lists": [f for f, _ in mi355slam.ObsListsC._fields_]}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mi355slam.h"', "int main(void) {"]
    for s, fs in fields.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (s, s))
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (s, f) for f in fs]
        lines.append('printf("\\n");')
    lines.append('printf("codes %d %d %d %d %d %d %d\\n", MS_OBS_FROM_ROWS, MS_OBS_FROM_SLOT, MS_OBS_ALL, MS_OBS_REFRESH, MS_OBS_RETRIANGULATE, MS_ERR_INVALID, MS_ERR_CAPACITY);')
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    for line, (name, T) in zip(out, (("ms_obs_select", mi355slam.ObsSelectC), ("ms_obs_lists", mi355slam.ObsListsC))):
        got = line.split()
        assert got[0] == name and int(got[1]) == C.sizeof(T)
        assert [int(x) for x in got[2:]] == [getattr(T, f).offset for f, _ in T._fields_]
    assert out[2].split()[1:] == [str(v) for v in (0, 1, 0, 1, 2, mi355slam.MS_ERR_INVALID, mi355slam.MS_ERR_CAPACITY)]


class Call:
    """One call of ms_observation_lists_check on host arrays (it dereferences kf_id and the structs only); fields are replaced per case."""

    def __init__(self):
        self.kf_mp = np.full((4, 6), -1, np.int32)
        self.n_kf, self.stride, self.n_mp = 4, 6, 10
        self.kf_id = np.array([5, -1, 2, 9], np.int32)
        self.flags = np.zeros(10, np.uint8)
        self.kp = {k: np.zeros((4, 6), np.int32 if k == "octave" else np.float32) for k in ("x", "y", "octave", "depth")}
        self.base = np.zeros(4, np.int32)
        self.rows_in = np.arange(3, dtype=np.int32)
        self.select = dict(source=R.FROM_ROWS, filter=R.ALL, drop_empty=0, slot=-1, n_in=3)
        self.n_levels, self.cap_rows, self.cap_obs = 8, 4, 4
        self.out = {f: np.zeros(8, np.int32) for f, _ in mi355slam.ObsListsC._fields_}
        self.counts = True
        self.no_select = self.no_lists = False

    def run(self):
        vp = mi355slam._vp
        s = self.select
        S = mi355slam.ObsSelectC(s["source"], s["filter"], s["drop_empty"], s["slot"], None if self.rows_in is None else self.rows_in.ctypes.data, s["n_in"])
        L = mi355slam.ObsListsC(*[None if self.out[f] is None else self.out[f].ctypes.data for f, _ in mi355slam.ObsListsC._fields_])
        n_rows, n_obs = C.c_int32(-7), C.c_int32(-7)
        why = C.create_string_buffer(256)
        rc = mi355slam.lib().ms_observation_lists_check(vp(self.kf_mp), self.n_kf, self.stride, self.n_mp, vp(self.kf_id), vp(self.flags), vp(self.kp["x"]),
                                                        vp(self.kp["y"]), vp(self.kp["octave"]), vp(self.kp["depth"]), vp(self.base),
                                                        None if self.no_select else C.byref(S), self.n_levels, None if self.no_lists else C.byref(L), self.cap_rows,
                                                        self.cap_obs, C.byref(n_rows) if self.counts else None, C.byref(n_obs) if self.counts else None, why,
                                                        C.c_size_t(256))
        assert (n_rows.value, n_obs.value) == (-7, -7)       # the validation writes nothing
        return rc, why.value.decode()


def _set(**kw):
    def f(c):
        for k, v in kw.items():
            setattr(c, k, v)
    return f


def _sel(**kw):
    return lambda c: c.select.update(kw)


def _drop(where, key):
    return lambda c: getattr(c, where).__setitem__(key, None)


INVALID = [
    ("slot below 0", _sel(source=R.FROM_SLOT, slot=-1), "slot"),
    ("slot at n_kf", _sel(source=R.FROM_SLOT, slot=4), "slot"),
    ("slot with kf_id < 0", _sel(source=R.FROM_SLOT, slot=1), "empty"),
    ("kf_id listed twice", _set(kf_id=np.array([5, -1, 5, 9], np.int32)), "twice"),
    ("refresh filter without flags", lambda c: (_sel(filter=R.REFRESH)(c), _set(flags=None)(c), _drop("out", "was_triangulated")(c)), "mp_flags"),
    ("retriangulate filter without flags", lambda c: (_sel(filter=R.RETRIANGULATE)(c), _set(flags=None)(c), _drop("out", "was_triangulated")(c)), "mp_flags"),
    ("was_triangulated without flags", _set(flags=None), "mp_flags"),
    ("stride 0", _set(stride=0), "stride"),
    ("negative n_kf", _set(n_kf=-1), "negative"),
    ("negative n_mp", _set(n_mp=-1), "negative"),
    ("negative n_in", _sel(n_in=-1), "negative"),
    ("negative cap_rows", _set(cap_rows=-1), "negative"),
    ("negative cap_obs", _set(cap_obs=-1), "negative"),
    ("negative n_levels", _set(n_levels=-1), "negative"),
    ("no kf_mp", _set(kf_mp=None), "missing"),
    ("no kf_id", _set(kf_id=None), "missing"),
    ("no selection", _set(no_select=True), "missing"),
    ("no lists", _set(no_lists=True), "missing"),
    ("no counts", _set(counts=False), "missing"),
    ("no rows_in", _set(rows_in=None), "rows_in"),
    ("no rows", _drop("out", "rows"), "missing"),
    ("no obs_start", _drop("out", "obs_start"), "missing"),
    ("obs_x without kp_x", _drop("kp", "x"), "missing"),
    ("obs_y without kp_y", _drop("kp", "y"), "missing"),
    ("octaves without kp_octave", _drop("kp", "octave"), "missing"),
    ("obs_depth without kp_depth", _drop("kp", "depth"), "missing"),
    ("obs_desc without kf_desc_base", _set(base=None), "missing"),
    ("bad source", _sel(source=2), "source"),
    ("bad filter", _sel(filter=3), "filter"),
    ("negative filter", _sel(filter=-1), "filter"),
]


@pytest.mark.parametrize("name,change,word", INVALID, ids=[c[0] for c in INVALID])
def test_check_rejects(name, change, word):
    c = Call()
    change(c)
    rc, why = c.run()
    assert rc == mi355slam.MS_ERR_INVALID and why.startswith("observation lists: ") and word in why, (rc, why)


def test_check_accepts_the_valid_and_the_empty_cases():
    assert Call().run() == (0, "")
    for change in (_sel(n_in=0), lambda c: (_sel(n_in=0)(c), _set(rows_in=None)(c)), _set(n_mp=0), _sel(source=R.FROM_SLOT, slot=2), _set(n_levels=0),
                   lambda c: (_set(cap_rows=0, cap_obs=0)(c), _drop("out", "rows")(c)), lambda c: (_set(n_kf=0, kf_mp=None, kf_id=None)(c)),
                   lambda c: [_drop("out", f)(c) for f, _ in mi355slam.ObsListsC._fields_ if f not in ("rows", "obs_start")] and
                   [_drop("kp", k)(c) for k in ("x", "y", "octave", "depth")] and _set(base=None, flags=None)(c)):
        c = Call()
        change(c)
        assert c.run() == (0, ""), change
