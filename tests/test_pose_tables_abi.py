"""CPU checks of the surface of poseBundleAdjust on the device map tables: the library exports the ms_pose_tables_* calls with
the header's signatures, Python binds them with the header's struct layouts, and ms_pose_tables_solve_check, the host-only half that runs
in front of any device call, turns every MS_ERR_INVALID case away with its message, holds the capacity caps and accepts the valid cases.
The check dereferences HOST arguments only, so host arrays stand in for the device tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mi355slam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_pose_tables_create", "ms_pose_tables_destroy", "ms_pose_tables_solve", "ms_pose_tables_solve_check", "ms_pose_tables_problem")
INVALID, CAPACITY = mi355slam.MS_ERR_INVALID, mi355slam.MS_ERR_CAPACITY
MAX_KF, MAX_STRIDE, MAX_MP = 65536, 8192, 1 << 24


def header():
    return open(os.path.join(ROOT, "include", "mi355slam.h")).read()


def test_library_exports_the_calls_and_python_binds_them():
    for name in NAMES:
        assert hasattr(mi355slam.lib(), name), name
    for name in ("solve_device", "solve", "problem", "close"):
        assert callable(getattr(mi355slam.PoseAdjuster, name)), name
    mk = open(os.path.join(ROOT, "slam-module_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bpose_tables\.hip\b", mk, flags=re.M)


def test_the_header_declares_the_structs_the_binding_uses():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)

    def members(name):
        m = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr)
        assert m, name
        out = []
        for decl in m.group(1).split(";"):
            words = decl.split()
            if words:
                out += [w.strip(",").split("[")[0] for w in words[1:]]
        return out

    assert members("ms_pose_tables_frame") == [k for k, _ in mi355slam.PoseTablesFrameC._fields_]
    assert members("ms_pose_tables_out") == [k for k, _ in mi355slam.PoseTablesOutC._fields_]
    assert C.sizeof(mi355slam.PoseTablesFrameC) == 12 + 4 + 40 + 8 + 8 * 43 + 8 + 8         # three ints (+ padding), the camera, focal (+ padding), the edge, two ints, huber


def test_the_check_twin_takes_the_arguments_of_the_call():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)

    def declaration(name):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        return [" ".join(p.split()).replace("const ", "") for p in m.group(1).split(",")]

    call, check = declaration("ms_pose_tables_solve"), declaration("ms_pose_tables_solve_check")
    assert call[0] == "ms_pose_tables *h" and call[-1] == "double *chi2"
    assert call[1:-1] == check[:-2] and check[-2:] == ["char *why", "size_t why_bytes"]
    assert len(call) == 15                                   # what the binding passes, argument for argument


def test_the_kernels_share_the_scan_and_the_window_helpers():
    src = open(os.path.join(ROOT, "slam-module_amd", "csrc", "pose_tables.hip")).read()
    assert '#include "ms_scan.h"' in src and '#include "ba_window_dev.h"' in src and "block_rank<kBlock>" in src and "ms_pinned(" in src
    win = open(os.path.join(ROOT, "slam-module_amd", "csrc", "ba_window.hip")).read()
    assert '#include "ba_window_dev.h"' in win and "quat_of_matrix(const" not in win and "write_pose(const" not in win      # one definition, in the header
    code = re.sub(r"//[^\n]*", "", src)
    assert "__shfl_up" not in code and not re.findall(r"atomic\w*\s*\(", code)                   # no scan of its own, no atomic
    assert "hipMemcpyHostToDevice" not in code.split('extern "C" int ms_pose_tables_solve(')[1].split('extern "C"')[0]      # a frame uploads nothing


class Call:
    """One call of ms_pose_tables_solve_check: 4 slots x 32, 50 map points, the frame in slot 1 behind the keyframe in slot 3."""

    def __init__(self):
        self.n_kf, self.stride, self.n_mp = 4, 32, 50
        self.arrays = dict(kf_mp=np.full(128, -1, np.int32), mp_flags=np.zeros(50, np.uint8), mp_live=np.ones(50, np.uint8), mp_pos=np.zeros(150), kp_x=np.zeros(128, np.float32),
                           kp_y=np.zeros(128, np.float32), kp_octave=np.zeros(128, np.int32), kf_pose=np.zeros(48))
        self.frame = dict(slot=1, prev_slot=3, n_kp=20, cam=[500.0, 501.0, 320.0, 240.0, 640, 480], focal=500, edge_meas=np.array([0, 0, 0, 1, 0.1, 0, 0]),
                          edge_info=np.eye(6).reshape(36), min_visible=10, max_iters=10, huber_delta=2.4477)
        self.null_frame = self.null_out = False

    def run(self):
        p = lambda k: mi355slam._vp(self.arrays.get(k))
        F, O = mi355slam.pose_tables_frame(self.frame), mi355slam.PoseTablesOutC()
        why = C.create_string_buffer(512)
        rc = mi355slam.lib().ms_pose_tables_solve_check(p("kf_mp"), self.n_kf, self.stride, p("mp_flags"), p("mp_live"), p("mp_pos"), self.n_mp, p("kp_x"), p("kp_y"),
                                                        p("kp_octave"), p("kf_pose"), None if self.null_frame else C.byref(F), None if self.null_out else C.byref(O), why,
                                                        C.c_size_t(512))
        return rc, why.value.decode()


def test_valid_calls_pass():
    c = Call()
    assert c.run() == (0, "")
    c.arrays["mp_live"] = None                               # every row is live
    assert c.run() == (0, "")
    c.frame["prev_slot"] = -1                                # no previous keyframe: the call answers ran = 0 itself
    assert c.run() == (0, "")
    c = Call()
    c.frame.update(n_kp=0, max_iters=0, min_visible=0, huber_delta=0.0)
    assert c.run() == (0, "")
    c.frame["n_kp"] = c.stride
    assert c.run() == (0, "")
    c = Call()
    c.n_mp = 0
    c.arrays.update(mp_flags=None, mp_live=None, mp_pos=None)
    assert c.run() == (0, "")


def edit(path, value):
    def go(c):
        if path[0] == "frame":
            if len(path) == 3:
                v = np.array(c.frame[path[1]], np.float64)
                v[path[2]] = value
                c.frame[path[1]] = v
            else:
                c.frame[path[1]] = value
        elif path[0] == "array":
            c.arrays[path[1]] = value
        else:
            setattr(c, path[0], value)
    return go


INVALID_CASES = [
    ("slot below the table", edit(("frame", "slot"), -1), "slot -1 outside"),
    ("slot behind the table", edit(("frame", "slot"), 4), "slot 4 outside"),
    ("previous slot below -1", edit(("frame", "prev_slot"), -2), "previous slot -2 outside"),
    ("previous slot behind the table", edit(("frame", "prev_slot"), 4), "previous slot 4 outside"),
    ("the frame is its own previous keyframe", edit(("frame", "prev_slot"), 1), "its own previous keyframe"),
    ("more keypoints than the stride", edit(("frame", "n_kp"), 33), "33 keypoints in a table of stride 32"),
    ("negative keypoint count", edit(("frame", "n_kp"), -1), "negative size"),
    ("negative slot count", edit(("n_kf",), -1), "negative size"),
    ("negative map point count", edit(("n_mp",), -1), "negative size"),
    ("stride 0", edit(("stride",), 0), "stride 0"),
    ("no frame", edit(("null_frame",), True), "missing array (frame or out)"),
    ("no out", edit(("null_out",), True), "missing array (frame or out)"),
    ("no kf_mp", edit(("array", "kf_mp"), None), "missing array"),
    ("no kp_x", edit(("array", "kp_x"), None), "missing array"),
    ("no kp_y", edit(("array", "kp_y"), None), "missing array"),
    ("no kp_octave", edit(("array", "kp_octave"), None), "missing array"),
    ("no kf_pose", edit(("array", "kf_pose"), None), "missing array"),
    ("no mp_flags", edit(("array", "mp_flags"), None), "missing array (mp_flags or mp_pos)"),
    ("no mp_pos", edit(("array", "mp_pos"), None), "missing array (mp_flags or mp_pos)"),
    ("fx zero", edit(("frame", "cam", 0), 0.0), "bad camera"),
    ("fy negative", edit(("frame", "cam", 1), -1.0), "bad camera"),
    ("fx infinite", edit(("frame", "cam", 0), np.inf), "bad camera"),
    ("cx NaN", edit(("frame", "cam", 2), np.nan), "bad camera"),
    ("cy infinite", edit(("frame", "cam", 3), np.inf), "bad camera"),
    ("no image width", edit(("frame", "cam", 4), 0), "bad camera"),
    ("no image height", edit(("frame", "cam", 5), 0), "bad camera"),
    ("NaN in the measurement", edit(("frame", "edge_meas", 5), np.nan), "edge_meas[5] is not finite"),
    ("infinite information", edit(("frame", "edge_info", 35), np.inf), "edge_info[35] is not finite"),
    ("NaN huber", edit(("frame", "huber_delta"), np.nan), "huber_delta is not finite"),
    ("negative iterations", edit(("frame", "max_iters"), -1), "max_iters -1"),
]


@pytest.mark.parametrize("what, change, message", INVALID_CASES, ids=[c[0] for c in INVALID_CASES])
def test_invalid_calls_are_turned_away(what, change, message):
    c = Call()
    change(c)
    rc, why = c.run()
    assert rc == INVALID and why.startswith("pose tables: ") and message in why, (what, rc, why)


def test_capacity_caps():
    for name, value in (("n_kf", MAX_KF + 1), ("stride", MAX_STRIDE + 1), ("n_mp", MAX_MP)):
        c = Call()
        setattr(c, name, value)
        rc, why = c.run()
        assert rc == CAPACITY and "caps" in why, (name, rc, why)
    c = Call()
    c.n_kf, c.stride, c.n_mp = MAX_KF, MAX_STRIDE, MAX_MP - 1
    c.frame["n_kp"] = MAX_STRIDE
    assert c.run() == (0, "")
