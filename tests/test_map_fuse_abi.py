"""CPU checks of the surface of the fuse step: the header declares the calls, the library exports them, Python binds them,
ms_fuse_view has the layout ctypes gives it, and the host-only halves that run in front of any device call -- ms_map_fuse_check and
ms_map_replace_pairs_check -- turn every MS_ERR_INVALID case away with its message, hold every cap and accept the zero sizes.  The checks
dereference HOST arguments only, so host arrays stand in for the device tables."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import mi355slam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_map_fuse", "ms_map_fuse_check", "ms_map_replace_pairs", "ms_map_replace_pairs_check")
INVALID, CAPACITY = mi355slam.MS_ERR_INVALID, mi355slam.MS_ERR_CAPACITY
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "map_fuse_smoke")
MAX_KF, MAX_STRIDE, MAX_MP, MAX_WINDOW, MAX_VIEWS, MAX_ENTRIES = 65536, 8192, 1 << 24, 1 << 24, 4096, 1 << 24


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "map_fuse_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_links_and_the_validation_runs_without_a_device():
    out = subprocess.check_output([build_smoke(), "--no-gpu"], text=True)
    assert "link ok 1" in out
    m = re.search(r"no-gpu ok (\d+) fuse cases", out)
    assert m and int(m.group(1)) >= 10, out


def test_library_exports_the_calls_and_python_binds_them():
    for name in NAMES:
        assert hasattr(mi355slam.lib(), name), name
    for name in ("fuse", "replace_pairs"):
        assert callable(getattr(mi355slam.KeyframeTable, name)), name
    mk = open(os.path.join(ROOT, "slam-module_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmap_fuse\.hip\b", mk, flags=re.M)


def test_the_check_twins_take_the_arguments_of_the_calls():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355slam.h")).read(), flags=re.S)

    def declaration(name):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        return [" ".join(p.split()).replace("const ", "") for p in m.group(1).split(",")]

    call, check = declaration("ms_map_fuse"), declaration("ms_map_fuse_check")
    per_entry = ["uint8_t *outcome", "int32_t *kp", "int32_t *other", "int32_t *erased_rows", "int32_t *erased_into"]
    assert [p for p in call[1:] if p not in per_entry] == check[:-2] and check[-2:] == ["char *why", "size_t why_bytes"]
    call, check = declaration("ms_map_replace_pairs"), declaration("ms_map_replace_pairs_check")
    assert [p for p in call[1:] if p not in per_entry[3:]] == check[:-2] and check[-2:] == ["char *why", "size_t why_bytes"]


def test_struct_layout_and_caps_match_the_header(tmp_path):
    T = mi355slam.FuseViewC
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mi355slam.h"', "int main(void) {", 'printf("%zu", sizeof(ms_fuse_view));']
    lines += ['printf(" %%zu", offsetof(ms_fuse_view, %s));' % f for f, _ in T._fields_]
    lines += ['printf("\\n%d %d %d %d %d %d\\n", MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, MS_TRACKED_MAX_WINDOW, MS_GATE_MAX_VIEWS, MS_GATE_MAX_ENTRIES);',
              "return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    got = [int(x) for x in out[0].split()]
    assert got[0] == C.sizeof(T) == 12 and got[1:] == [getattr(T, f).offset for f, _ in T._fields_] == [0, 4, 8]
    assert [int(x) for x in out[1].split()] == [MAX_KF, MAX_STRIDE, MAX_MP, MAX_WINDOW, MAX_VIEWS, MAX_ENTRIES]


class Call:
    """One call of either check: 3 slots x 8, 10 map points, a window of 6 tracks; two views over 7 entries with a gap; 3 pairs."""

    def __init__(self):
        self.n_kf, self.stride, self.n_mp, self.n_track, self.track_base = 3, 8, 10, 6, 100
        a = lambda n, dt: np.zeros(max(n, 1), dt)
        self.arrays = dict(kf_mp=np.full(24, -1, np.int32), mp_flags=a(10, np.uint8), mp_live=a(10, np.uint8), n_obs=a(10, np.int32), mp_track=a(10, np.int32),
                           track_row=a(6, np.int32), kept_entry=a(7, np.int32), top_idx=a(28, np.int32), top_dist=a(28, np.uint16),
                           mp_index=np.array([4, 2, 9, 0, 2, 7, 3], np.int32), n_kept=np.array([2, 3], np.int32), n_erased=a(1, np.int32), counts=a(8, np.int32),
                           views_done=a(1, np.int32), pairs=np.array([1, 2, 2, 3, 5, 5], np.int32), outcome=a(3, np.uint8))
        self.views = [(1, 0, 3), (2, 4, 3)]
        self.n_entries, self.n_views, self.n_pairs, self.max_dist, self.source_slot = 7, 2, 3, 50, 0
        self.no_views = False

    def ptr(self, name):
        a = self.arrays.get(name)
        return C.c_void_p(0) if a is None else C.c_void_p(a.ctypes.data)

    def tables(self):
        p = self.ptr
        return (p("kf_mp"), self.n_kf, self.stride, p("mp_flags"), p("mp_live"), p("n_obs"), self.n_mp, p("mp_track"), p("track_row"), self.track_base, self.n_track)

    def fuse(self):
        p, why = self.ptr, C.create_string_buffer(512)
        V = (mi355slam.FuseViewC * max(len(self.views), 1))(*[mi355slam.FuseViewC(*v) for v in self.views])
        rc = mi355slam.lib().ms_map_fuse_check(*self.tables(), p("kept_entry"), p("top_idx"), p("top_dist"), p("mp_index"), self.n_entries, None if self.no_views else V,
                                               p("n_kept"), self.n_views, self.max_dist, self.source_slot, p("n_erased"), p("counts"), p("views_done"), why, C.c_size_t(512))
        return rc, why.value.decode()

    def pairs(self):
        p, why = self.ptr, C.create_string_buffer(512)
        rc = mi355slam.lib().ms_map_replace_pairs_check(*self.tables(), p("pairs"), self.n_pairs, p("outcome"), p("n_erased"), why, C.c_size_t(512))
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
    assert Call().fuse() == (0, "") and Call().pairs() == (0, "")
    assert changed(n_views=0, views=[], no_views=True, n_kept=None).fuse() == (0, "")
    assert changed(n_entries=0, views=[(1, 0, 0), (2, 0, 0)], n_kept=np.zeros(2, np.int32), mp_index=None, kept_entry=None, top_idx=None, top_dist=None).fuse() == (0, "")
    assert changed(views=[(1, 0, 3), (2, 3, 0)], n_kept=np.array([3, 0], np.int32)).fuse() == (0, "")           # an empty view; n_kept == count
    assert changed(mp_track=None, track_row=None, n_track=0).fuse() == (0, "")
    assert changed(mp_track=None, track_row=None, n_track=0).pairs() == (0, "")
    assert changed(source_slot=-1).fuse() == (0, "") and changed(max_dist=0).fuse() == (0, "") and changed(max_dist=256).fuse() == (0, "")
    assert changed(n_pairs=0, pairs=None, outcome=None).pairs() == (0, "")
    assert changed(n_mp=0, mp_flags=None, mp_live=None, n_obs=None, mp_track=None, track_row=None, n_track=0, n_entries=0, views=[(1, 0, 0)], n_views=1,
                   n_kept=np.zeros(1, np.int32)).fuse() == (0, "")
    assert changed(n_kf=0, kf_mp=None, n_views=0, views=[], n_kept=None, source_slot=-1).fuse() == (0, "")
    assert changed(views=[(1, 4, 3), (1, 0, 3)]).fuse() == (0, "")                                              # slices in any order, a slot walked twice
    assert changed(views=[(1, 0, 3), (2, 3, 4)], mp_index=np.array([4, 2, 9, 2, 4, 7, 3], np.int32)).fuse() == (0, "")      # a row in two views


def test_every_invalid_fuse_call_is_turned_away_with_its_message():
    cases = [
        (dict(n_kf=-1), "negative size"), (dict(n_mp=-1), "negative size"), (dict(n_track=-1), "negative size"),
        (dict(n_entries=-1), "negative size"), (dict(n_views=-1), "negative size"),
        (dict(stride=0), "stride 0"),
        (dict(kf_mp=None), "missing array"), (dict(mp_flags=None), "missing array"), (dict(mp_live=None), "missing array"), (dict(n_obs=None), "missing array"),
        (dict(mp_index=None), "missing array"), (dict(kept_entry=None), "missing array"), (dict(top_idx=None), "missing array"), (dict(top_dist=None), "missing array"),
        (dict(n_kept=None), "missing array"), (dict(no_views=True), "missing array"), (dict(n_erased=None), "missing array"), (dict(counts=None), "missing array"),
        (dict(views_done=None), "missing array"),
        (dict(mp_track=None), "one track table without the other"), (dict(track_row=None), "one track table without the other"),
        (dict(max_dist=-1), "max_dist -1 outside [0, 256]"), (dict(max_dist=257), "max_dist 257 outside [0, 256]"),
        (dict(source_slot=3), "source slot 3 outside [-1, 3)"), (dict(source_slot=-2), "source slot -2 outside [-1, 3)"),
        (dict(views=[(3, 0, 3), (2, 4, 3)]), "view 0: slot 3 outside [0, 3)"), (dict(views=[(1, 0, 3), (-1, 4, 3)]), "view 1: slot -1 outside [0, 3)"),
        (dict(views=[(1, 0, 3), (2, 5, 3)]), "view 1: slice [5, 5 + 3) outside [0, 7)"), (dict(views=[(1, -1, 3), (2, 4, 3)]), "view 0: slice [-1,"),
        (dict(views=[(1, 0, -3), (2, 4, 3)]), "view 0: slice"), (dict(views=[(1, 0, 3), (2, 8, 0)]), "view 1: slice [8,"),
        (dict(views=[(1, 0, 3), (2, 2, 3)]), "the slices of views 0 and 1 overlap"), (dict(views=[(1, 3, 3), (2, 0, 4)]), "the slices of views 1 and 0 overlap"),
        (dict(n_kept=np.array([4, 3], np.int32)), "view 0: n_kept 4 for a slice of 3"), (dict(n_kept=np.array([2, -1], np.int32)), "view 1: n_kept -1"),
        (dict(mp_index=np.array([4, 2, 10, 0, 2, 7, 3], np.int32)), "view 0: entry 2 is row 10 outside [0, 10)"),
        (dict(mp_index=np.array([4, 2, 9, 0, 2, -1, 3], np.int32)), "view 1: entry 5 is row -1 outside [0, 10)"),
        (dict(mp_index=np.array([4, 2, 4, 0, 2, 7, 3], np.int32)), "view 0 lists row 4 twice"),
        (dict(mp_index=np.array([4, 2, 9, 0, 3, 7, 3], np.int32)), "view 1 lists row 3 twice"),
    ]
    for kw, text in cases:
        rc, why = changed(**kw).fuse()
        assert rc == INVALID and text in why and why.startswith("map fuse: "), (kw, rc, why)
    assert changed(mp_index=np.array([4, 2, 9, 10, 2, 7, 3], np.int32)).fuse() == (0, "")                      # an entry of no slice is not read
    assert mi355slam.lib().ms_map_fuse_check(*Call().tables(), *([None] * 4), 0, None, None, 0, 50, -1, *Call().tables()[3:6], None, C.c_size_t(0)) == 0
    c = changed(stride=0)                                                                                       # no buffer for the message
    assert mi355slam.lib().ms_map_fuse_check(*c.tables(), *([None] * 4), 0, None, None, 0, 50, -1, *c.tables()[3:6], None, C.c_size_t(0)) == INVALID


def test_every_cap_of_the_fuse_call_holds():
    big = [(dict(n_kf=MAX_KF + 1), "65537 slots"), (dict(stride=MAX_STRIDE + 1), "stride 8193"), (dict(n_mp=MAX_MP), "16777216 map points"),
           (dict(n_track=MAX_WINDOW + 1), "a track window of 16777217"), (dict(n_views=MAX_VIEWS + 1), "4097 views"), (dict(n_entries=MAX_ENTRIES), "16777216 entries")]
    for kw, text in big:
        rc, why = changed(**kw).fuse()
        assert rc == CAPACITY and text in why, (kw, rc, why)
    # at the caps the sizes pass the capacity checks (the arrays here are too small for them, so stop at the first thing read behind the caps)
    for kw in (dict(n_kf=MAX_KF), dict(stride=MAX_STRIDE), dict(n_track=MAX_WINDOW)):
        assert changed(**kw).fuse() == (0, "")
    rc, why = changed(n_mp=MAX_MP - 1).fuse()
    assert (rc, why) == (0, "")
    rc, why = changed(n_views=MAX_VIEWS, max_dist=-1).fuse()
    assert rc == INVALID and "max_dist" in why
    rc, why = changed(n_entries=MAX_ENTRIES - 1, max_dist=-1).fuse()
    assert rc == INVALID and "max_dist" in why


def test_every_invalid_pairs_call_is_turned_away_and_every_cap_holds():
    cases = [
        (dict(n_kf=-1), "negative size"), (dict(n_pairs=-1), "negative size (-1 pairs)"), (dict(stride=0), "stride 0"),
        (dict(kf_mp=None), "missing array"), (dict(mp_live=None), "missing array"), (dict(mp_flags=None), "missing array"), (dict(n_obs=None), "missing array"),
        (dict(pairs=None), "missing array"), (dict(outcome=None), "missing array"), (dict(n_erased=None), "missing array"),
        (dict(mp_track=None), "one track table without the other"), (dict(track_row=None), "one track table without the other"),
        (dict(pairs=np.array([1, 2, 2, 10, 5, 5], np.int32)), "pair 1: row 10 outside [0, 10)"),
        (dict(pairs=np.array([1, 2, 2, 3, -1, 5], np.int32)), "pair 2: row -1 outside [0, 10)"),
    ]
    for kw, text in cases:
        rc, why = changed(**kw).pairs()
        assert rc == INVALID and text in why and why.startswith("map replace pairs: "), (kw, rc, why)
    for kw, text in ((dict(n_kf=MAX_KF + 1), "65537 slots"), (dict(stride=MAX_STRIDE + 1), "stride 8193"), (dict(n_mp=MAX_MP), "16777216 map points"),
                     (dict(n_track=MAX_WINDOW + 1), "a track window of 16777217"), (dict(n_pairs=MAX_ENTRIES), "16777216 pairs")):
        rc, why = changed(**kw).pairs()
        assert rc == CAPACITY and text in why, (kw, rc, why)
    assert changed(n_kf=MAX_KF).pairs() == (0, "") and changed(n_track=MAX_WINDOW).pairs() == (0, "")
