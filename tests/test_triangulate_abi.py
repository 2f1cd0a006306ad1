"""CPU checks of the surface of the map-point triangulator (ms_triangulate): the header declares it, the library exports it, the Python
binding and the host mirror's triangulateMapPoints are there (tests/triangulate_smoke.cpp compiles and links), the constants and struct
sizes agree, and every MS_ERR_INVALID case is turned away, with its message, by ms_triangulate_check -- the host-only half of the call,
which runs in front of any device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mi355slam
import triangulate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "triangulate_smoke")
NAMES = ("ms_triangulate", "ms_triangulate_check")
MS_ERR_INVALID, MS_ERR_CAPACITY = -1, -4


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "triangulate_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355slam.h")).read(), flags=re.S)


def test_header_declares_the_triangulator():
    code = header()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert re.search(r"}\s*ms_tri_settings\s*;", code)


def test_constants_and_struct_sizes():
    code = header()

    def define(name):
        return eval(re.search(r"#define\s+%s\s+(.+)" % name, code).group(1))
    assert (define("MS_TRI_TME"), define("MS_TRI_MIDPOINT"), define("MS_TRI_FIRST_LAST")) == (R.TME, R.MIDPOINT, R.FIRST_LAST) == (0, 1, 2)
    assert (mi355slam.TRI_TME, mi355slam.TRI_MIDPOINT, mi355slam.TRI_FIRST_LAST) == (0, 1, 2)
    assert (define("MS_TRI_MAX_LEVELS"), define("MS_TRI_MAX_ROWS"), define("MS_TRI_MAX_OBS")) == (32, 1 << 24, 1 << 22)
    assert (mi355slam.TRI_MAX_LEVELS, mi355slam.TRI_MAX_ROWS, mi355slam.TRI_MAX_OBS) == (32, 1 << 24, 1 << 22)
    assert C.sizeof(mi355slam.TriSettingsC) == 40 and C.sizeof(mi355slam.Pinhole) == 40              # the C layout of the two host structs
    assert mi355slam.TriSettingsC.min_angle_two_obs.offset == 16 and mi355slam.TriSettingsC.dense_stereo_depth.offset == 36
    assert R.FLAG_OF_STATUS == (0, 2, 3) and R.GROUP == 16
    src = open(os.path.join(ROOT, "slam-module_amd", "csrc", "triangulate.hip")).read()
    assert "kSweeps = %d;" % R.JACOBI_SWEEPS in src and "kPivotRel = 1e-10;" in src and R.PIVOT_REL == 1e-10 and "kChi2Inv2D = 5.991;" in src


def test_library_exports_the_triangulator_and_python_binds_it():
    for name in NAMES:
        assert hasattr(mi355slam.lib(), name), name
    assert callable(mi355slam.MapPointTable.triangulate)


def test_makefile_builds_the_new_source():
    mk = open(os.path.join(ROOT, "slam-module_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\btriangulate\.hip\b", mk, flags=re.M)


def test_mirror_links_and_rejects_without_a_device():
    out = subprocess.check_output([build_smoke(), "--no-gpu"], text=True)
    assert "link ok 1" in out
    m = re.search(r"no-gpu ok (\d+) cases", out)
    assert m and int(m.group(1)) >= 25, out


# ---------------------------------------------------------------------------------------------------- ms_triangulate_check
class Call:
    """A valid call of three entries (2, 0 and 3 observations) that a test breaks in one place."""

    def __init__(self):
        self.n_mp, self.n_kf, self.mode = 10, 3, R.TME
        self.pos, self.pose = np.zeros(30), np.zeros(36)     # stand-ins: the check never reads the device arrays
        self.cam = (mi355slam.Pinhole * 3)(*[mi355slam.Pinhole(500.0, 500.0, 320.0, 240.0, 640, 480) for _ in range(3)])
        self.focal = np.array([500, 500, 500], np.int32)
        self.rows, self.was = np.array([4, 2, 9], np.int32), np.array([0, 1, 0], np.uint8)
        self.start = np.array([0, 2, 2, 5], np.int32)
        self.kf, self.octave = np.array([0, 1, 0, 1, 2], np.int32), np.array([0, 7, 3, 3, 1], np.int32)
        self.x, self.y = np.arange(5, dtype=np.float32), np.arange(5, dtype=np.float32)
        self.sigma = R.settings()["level_sigma_sq"].copy()
        self.S = mi355slam.TriSettingsC(self.sigma.ctypes.data, 8, 1.0, 3.0, 0.004, 0)
        self.n_rows = 3
        self.settings = C.byref(self.S)

    def check(self):
        why = C.create_string_buffer(256)
        vp = mi355slam._vp
        rc = mi355slam.lib().ms_triangulate_check(vp(self.pos), self.n_mp, vp(self.pose), self.n_kf, self.cam, vp(self.focal), vp(self.rows), vp(self.was),
                                                  self.n_rows, vp(self.start), vp(self.kf), vp(self.x), vp(self.y), vp(self.octave), self.settings,
                                                  self.mode, why, C.c_size_t(256))
        return rc, why.value.decode()


def broken(**changes):
    c = Call()
    for name, (index, value) in changes.items():
        if index is None:
            setattr(c, name, value)
        elif name == "cam":
            setattr(c.cam[index[0]], index[1], value)
        elif name == "S":
            setattr(c.S, index, value)
        else:
            getattr(c, name)[index] = value
    return c.check()


def test_a_valid_call_and_the_empty_ones_pass():
    assert Call().check() == (0, "")
    c = Call()
    c.n_rows, c.pos, c.pose, c.rows, c.was, c.kf = 0, None, None, None, None, None
    assert c.check() == (0, "")                              # n_rows = 0
    c = Call()
    c.start[:] = 0
    c.kf = c.x = c.y = c.octave = None
    assert c.check() == (0, "")                              # empty lists only: no observation array is needed
    c = Call()
    c.cam[2].width = 0
    c.kf[4] = 1
    assert c.check() == (0, "")                              # a camera no observation names is not read


INVALID = {
    "row beyond the table": (dict(rows=(1, 10)), r"row entry 1: row 10 outside \[0, 10\)"),
    "row -1": (dict(rows=(0, -1)), r"row entry 0: row -1 outside \[0, 10\)"),
    "row listed twice": (dict(rows=(2, 4)), r"row 4 is listed twice"),
    "slot beyond the table": (dict(kf=(3, 3)), r"observation 3: keyframe slot 3 outside \[0, 3\)"),
    "slot -1": (dict(kf=(0, -1)), r"observation 0: keyframe slot -1 outside \[0, 3\)"),
    "obs_start not starting at 0": (dict(start=(0, 1)), r"obs_start\[0\] = 1"),
    "obs_start decreasing": (dict(start=(2, 1)), r"obs_start decreases at row entry 1"),
    "octave n_levels": (dict(octave=(1, 8)), r"observation 1: octave 8 outside \[0, 8\)"),
    "octave -1": (dict(octave=(4, -1)), r"observation 4: octave -1 outside \[0, 8\)"),
    "width 0": (dict(cam=((1, "width"), 0)), r"keyframe slot 1: bad camera \(0 x 480"),
    "height 0": (dict(cam=((2, "height"), 0)), r"keyframe slot 2: bad camera \(640 x 0"),
    "fx 0": (dict(cam=((0, "fx"), 0.0)), r"keyframe slot 0: bad camera .*fx 0,"),
    "fy negative": (dict(cam=((0, "fy"), -500.0)), r"keyframe slot 0: bad camera .*fy -500"),
    "fx NaN": (dict(cam=((1, "fx"), float("nan"))), r"keyframe slot 1: bad camera .*fx nan"),
    "fy infinite": (dict(cam=((1, "fy"), float("inf"))), r"keyframe slot 1: bad camera .*fy inf"),
    "cx NaN": (dict(cam=((1, "cx"), float("nan"))), r"keyframe slot 1: bad camera"),
    "mode 3": (dict(mode=(None, 3)), r"mode 3"),
    "mode -1": (dict(mode=(None, -1)), r"mode -1"),
    "NaN two-observation angle": (dict(S=("min_angle_two_obs", float("nan"))), r"a setting is not finite"),
    "infinite multiple-observation angle": (dict(S=("min_angle_multiple_obs", float("inf"))), r"a setting is not finite"),
    "NaN threshold": (dict(S=("rel_reprojection_threshold", float("nan"))), r"a setting is not finite"),
    "infinite sigma": (dict(sigma=(3, np.inf)), r"level_sigma_sq\[3\] is not finite"),
    "n_levels 0": (dict(S=("n_levels", 0)), r"n_levels 0 outside \[1, 32\]"),
    "n_levels 33": (dict(S=("n_levels", 33)), r"n_levels 33 outside \[1, 32\]"),
    "negative n_mp": (dict(n_mp=(None, -1)), r"bad arguments"),
    "negative n_kf": (dict(n_kf=(None, -1)), r"bad arguments"),
    "negative n_rows": (dict(n_rows=(None, -1)), r"bad arguments"),
    "missing positions": (dict(pos=(None, None)), r"missing array"),
    "missing poses": (dict(pose=(None, None)), r"missing array"),
    "missing cameras": (dict(cam=(None, None)), r"missing array"),
    "missing focal lengths": (dict(focal=(None, None)), r"missing array"),
    "missing rows": (dict(rows=(None, None)), r"missing array"),
    "missing was_triangulated": (dict(was=(None, None)), r"missing array"),
    "missing obs_start": (dict(start=(None, None)), r"missing array"),
    "missing obs_kf": (dict(kf=(None, None)), r"missing array"),
    "missing obs_x": (dict(x=(None, None)), r"missing array"),
    "missing obs_y": (dict(y=(None, None)), r"missing array"),
    "missing obs_octave": (dict(octave=(None, None)), r"missing array"),
    "missing settings": (dict(settings=(None, None)), r"missing settings"),
    "missing sigmas": (dict(S=("level_sigma_sq", None)), r"missing settings"),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_call_is_rejected_with_its_message(case):
    changes, message = INVALID[case]
    rc, why = broken(**changes)
    assert rc == MS_ERR_INVALID and why.startswith("triangulate: ") and re.search(message, why), (rc, why)


def test_capacity_is_its_own_error():
    c = Call()
    c.start[3] = (1 << 22) + 1
    rc, why = c.check()
    assert rc == MS_ERR_CAPACITY and re.search(r"4194305 observations, at most 4194304", why)
    c = Call()
    c.n_rows = (1 << 24) + 1
    rc, why = c.check()
    assert rc == MS_ERR_CAPACITY and re.search(r"16777217 rows, at most 16777216", why)
