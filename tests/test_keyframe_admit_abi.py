"""CPU checks of the surface of ms_keyframe_admit: the header declares the call, its three structs and its validation twin, the
library exports them, Python binds them with the header's struct layouts, and ms_keyframe_admit_validate, the host-only half that runs in
front of any device call, accepts the valid cases, turns every MS_ERR_INVALID case away with its message and holds every cap -- through the
library, and again in a program of its own compiled with map_checks.cpp alone under ASan and UBSan.  The validation dereferences HOST
arguments only, so host arrays stand in for the device arrays."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mi355slam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-module_amd", "csrc")
INVALID, CAPACITY = mi355slam.MS_ERR_INVALID, mi355slam.MS_ERR_CAPACITY
MAX_KF, MAX_STRIDE, MAX_MP = 65536, 8192, 1 << 24


def header(comments=False):
    text = open(os.path.join(ROOT, "include", "mi355slam.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declaration(name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header())
    assert m, name
    return [" ".join(p.split()).replace("const ", "") for p in m.group(1).split(",")]


def struct_fields(name):
    m = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header())
    assert m, name
    names = []
    for d in m.group(1).split(";"):
        if d.split():
            first, *more = d.split(",")
            names += [first.split()[-1].lstrip("*")] + [x.strip().lstrip("*") for x in more]
    return [re.sub(r"\[.*\]", "", x) for x in names]


def test_library_exports_the_calls_and_python_binds_them():
    for name in ("ms_keyframe_admit", "ms_keyframe_admit_validate"):
        assert hasattr(mi355slam.lib(), name), name
    for name in ("keyframe_admit", "keyframe_admit_device", "keyframe_admit_validate", "keypoints_view", "AdmitFrame"):
        assert callable(getattr(mi355slam, name)), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bkeyframe_admit\.hip\b", mk, flags=re.M) and not re.search(r"^keyframe_admit\.o\s*:.*FLAGS", mk, flags=re.M)
    src = open(os.path.join(CSRC, "keyframe_admit.hip")).read()
    internal = open(os.path.join(CSRC, "ms_internal.h")).read()
    assert '#include "ms_scan.h"' in src and "block_rank<kBlock>" in src and "MS_WS_KEYFRAME_ADMIT" in src and "ms_pinned(" in src and "MS_WS_KEYFRAME_ADMIT" in internal
    # the descent and the bearing are shared device code, not copies
    bow = open(os.path.join(CSRC, "bow.hip")).read()
    assert '#include "bow_descend.h"' in src and '#include "bow_descend.h"' in bow and "struct BowTree" in internal and "struct BowTree" not in bow + src
    calls = lambda text: len(re.findall(r"(?<![\w])bow_descend\(", text))
    assert calls(src) == 1 and calls(bow) == 1 and "__builtin_amdgcn_update_dpp" not in bow + src
    tri = open(os.path.join(CSRC, "triangulate.hip")).read()
    assert "ms_pinhole_bearing(" in src and "ms_pinhole_bearing(" in tri and "sqrt(" not in re.sub(r"//[^\n]*", "", src)
    code = re.sub(r"//[^\n]*", "", src)
    assert set(re.findall(r"\batomic\w*", code)) == {"atomicAdd"} and not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", code)      # integer adds of the verdicts only
    body = code.split('extern "C" int ms_keyframe_admit(')[1]
    assert body.count("hipLaunchKernelGGL(") == 4 and "FOUR launches" in header(True) and "FOUR launches" in src
    assert body.count("hipMemcpyHostToDevice") == 1 and body.count("hipMemcpyDeviceToHost") == 1 and body.count("hipStreamSynchronize") == 1
    assert not re.search(r"\bhipMalloc|\bhipHostMalloc|\bnew\b|std::vector", body)                        # the workspace and the pinned block only


def test_the_header_declares_the_structs_the_binding_uses_and_the_twin_takes_the_arguments_of_the_call():
    assert "DESIGN 9.19" in header(True)
    for name, cls in (("ms_admit_args", mi355slam.AdmitArgsC), ("ms_admit_frame", mi355slam.AdmitFrameC), ("ms_admit_host", mi355slam.AdmitHostC)):
        assert struct_fields(name) == [k for k, _ in cls._fields_], name
    assert C.sizeof(mi355slam.AdmitArgsC) == 8 + 96 + 40 + 8 + 8 + 16 + 8 + 8 + 16 and C.sizeof(mi355slam.AdmitFrameC) == 8 + 11 * 8 and C.sizeof(mi355slam.AdmitHostC) == 64
    assert mi355slam.AdmitArgsC.pose.offset == 8 and mi355slam.AdmitArgsC.cam.offset == 104 and mi355slam.AdmitArgsC.vocab.offset == 152
    call, twin = declaration("ms_keyframe_admit"), declaration("ms_keyframe_admit_validate")
    assert call[0] == "ms_ctx *ctx" and call[1:] == twin[:-2] and twin[-2:] == ["char *why", "size_t why_bytes"]
    assert len(call) == 18 and[p.split("*")[-1].split()[-1] for p in call[1:]] == [
        "view", "frame", "kf_mp", "n_kf", "stride", "n_mp", "kp_x", "kp_y", "kp_octave", "kp_depth", "desc_pool", "n_pool", "kf_pose", "args", "out", "host", "counts"]
    assert "ms_keyframe_admit_check" not in header(True) and re.search(r"/\*[^\n]*_validate[^\n]*22[^\n]*\*/\s*int ms_keyframe_admit_validate", header(True))
    checks = open(os.path.join(CSRC, "map_checks.cpp")).read()
    assert 'extern "C" int ms_keyframe_admit_validate(' in checks
    assert "ms_keyframe_admit_validate(" not in open(os.path.join(CSRC, "keyframe_admit.hip")).read().split('extern "C"')[0]
    # the header says what stands in for what, and what the call leaves out
    text = " ".join(header(True).split())
    for phrase in ("stand-in for frame->getDepth", "addTrackerFeatures", "getPixel", "ms_bow_db_add takes host arrays", "reuse of pool space"):
        assert phrase in text, phrase


class Call:
    """One call of ms_keyframe_admit_validate: a view of capacity 12, 3 slots x 10, a pool of 40, frame arrays of 10, two tracks, a 6 x 4 image."""

    def __init__(self):
        self.n_kf, self.stride, self.n_mp, self.n_pool, self.frame, self.cap_kp, self.capacity = 3, 10, 7, 40, 0, 10, 12
        z = lambda n, dt: np.zeros(n, dt)
        self.view = dict(count=z(2, np.int32), x=z(24, np.float32), y=z(24, np.float32), angle=z(24, np.float32), octave=z(24, np.int32), desc=z(24 * 8 + 4, np.uint32),
                         track_id=z(24, np.int32))
        self.tables = dict(kf_mp=z(30, np.int32), kp_x=z(30, np.float32), kp_y=z(30, np.float32), kp_octave=z(30, np.int32), kp_depth=z(30, np.float32),
                           desc_pool=z(40 * 8 + 4, np.uint32), kf_pose=z(36, np.float64))
        self.out = {k: z(11 * w + 4, dt) for k, dt, w in mi355slam._ADMIT_FRAME}
        self.args = dict(slot=1, desc_base=30, pose=np.arange(12.0), cam=(500.0, 501.0, 320.0, 240.0, 640, 480), levels_up=4, track_ids=np.array([5, 6], np.int32),
                         track_depth=np.array([1, 2], np.float32), depth_image=z(24, np.float32), depth_width=6, depth_height=4, depth_stride=6)
        self.has_view = self.has_out = self.counts = True
        self.shift = {}                                      # name -> bytes added to the array's address

    def ptr(self, d, k):
        a = d.get(k)
        if a is None:
            return None
        base = a.ctypes.data
        return base + (-base) % 16 + self.shift.get(("out." if d is self.out else "") + k, 0)      # 16-byte aligned inside the array's slack, then shifted

    def run(self):
        view = mi355slam.KeypointsView(self.capacity, *[self.ptr(self.view, k) for k in ("count", "x", "y", "angle", "octave", "desc", "track_id")]) if self.has_view else None
        out = mi355slam.AdmitFrameC(self.cap_kp, *[self.ptr(self.out, k) for k, _, _ in mi355slam._ADMIT_FRAME]) if self.has_out else None
        tables = {k: self.ptr(self.tables, k) for k in self.tables}
        return mi355slam.keyframe_admit_validate(view, self.frame, tables, self.n_kf, self.stride, self.n_mp, self.n_pool, self.args, out, None, self.counts)


def changed(**kw):
    c = Call()
    for k, v in kw.items():
        for d in (c.view, c.tables, c.out) if v is None else ():
            if k in d and not hasattr(c, k):
                d[k] = None
                break
        else:
            if k.startswith("args_"):
                c.args[k[5:]] = v
            elif k.startswith("shift_"):
                c.shift[k[6:]] = v
            else:
                setattr(c, k, v)
    return c


def test_valid_calls_and_the_zero_sizes_pass():
    assert Call().run() == (0, "")
    assert changed(args_track_ids=None, args_track_depth=None).run() == (0, "")
    assert changed(args_depth_image=None, args_depth_width=0, args_depth_height=0).run() == (0, "")
    assert changed(args_desc_base=40).run() == (0, "") and changed(args_desc_base=0).run() == (0, "")    # whether n fits is the device's verdict
    assert changed(args_slot=0).run() == (0, "") and changed(args_slot=2).run() == (0, "") and changed(frame=1).run() == (0, "")
    assert changed(n_mp=0).run() == (0, "") and changed(cap_kp=0).run() == (0, "") and changed(capacity=0).run() == (0, "") and changed(n_pool=30).run() == (0, "")
    assert changed(args_track_ids=np.zeros(0, np.int32), args_track_depth=np.zeros(0, np.float32)).run() == (0, "")
    assert changed(args_depth_stride=9).run() == (0, "") and changed(args_levels_up=-1).run() == (0, "")     # levels_up is read with a vocabulary only


NAN, INF = float("nan"), float("inf")
INVALID_CASES = [
    (dict(n_kf=-1), "negative size (-1 slots"), (dict(n_mp=-1), "negative size"), (dict(n_pool=-1), "-1 pool entries"), (dict(stride=0), "stride 0"),
    (dict(has_view=False), "missing array (view, args, out or counts)"), (dict(args=None), "missing array (view, args, out or counts)"),
    (dict(has_out=False), "missing array (view, args, out or counts)"), (dict(counts=False), "missing array (view, args, out or counts)"),
] + [(dict([(k, None)]), "of the view)") for k in ("count", "x", "y", "angle", "octave", "desc", "track_id")] + [
    (dict([(k, None)]), "missing array (kf_mp, the keypoint table, desc_pool or kf_pose)") for k in ("kf_mp", "kp_x", "kp_y", "kp_octave", "kp_depth", "desc_pool", "kf_pose")
] + [(dict([(k, None)]), "missing array (a frame array of out)") for k in ("bearing", "usable", "sorted_x", "sorted_y", "sorted_idx", "node_id", "node_start", "kp_idx")] + [
    (dict(capacity=-1), "negative size (view capacity -1"), (dict(cap_kp=-2), "cap_kp -2"), (dict(args_n_tracks=-1), "-1 tracks"),
    (dict(frame=-1), "frame -1 outside [0, 65536)"), (dict(frame=65536), "frame 65536 outside"),
    (dict(args_slot=-1), "slot -1 outside [0, 3)"), (dict(args_slot=3), "slot 3 outside [0, 3)"),
    (dict(args_desc_base=-1), "desc_base -1 outside [0, 40]"), (dict(args_desc_base=41), "desc_base 41 outside [0, 40]"),
    (dict(shift_desc_pool=8), "16-byte aligned"), (dict(shift_desc=4), "16-byte aligned"),
    (dict(args_pose=[0, 1, 2, NAN, 4, 5, 6, 7, 8, 9, 10, 11]), "pose[3] is not finite"), (dict(args_pose=[0] * 11 + [INF]), "pose[11] is not finite"),
    (dict(args_cam=(0.0, 501.0, 320.0, 240.0, 640, 480)), "bad camera (fx 0"), (dict(args_cam=(500.0, -1.0, 320.0, 240.0, 640, 480)), "bad camera"),
    (dict(args_cam=(500.0, INF, 320.0, 240.0, 640, 480)), "bad camera"), (dict(args_cam=(NAN, 501.0, 320.0, 240.0, 640, 480)), "bad camera"),
    (dict(args_cam=(500.0, 501.0, NAN, 240.0, 640, 480)), "bad camera"), (dict(args_cam=(500.0, 501.0, 320.0, -INF, 640, 480)), "bad camera"),
    (dict(args_track_depth=None), "missing array (track_ids or track_depth)"), (dict(args_track_ids=None, args_n_tracks=2), "missing array (track_ids or track_depth)"),
    (dict(args_track_ids=None, args_track_depth=None, args_n_tracks=2), "missing array (track_ids with 2 tracks)"),
    (dict(args_depth_width=0), "a depth image of 0 x 4"), (dict(args_depth_height=0), "a depth image of 6 x 0"), (dict(args_depth_stride=5), "row stride 5"),
]


@pytest.mark.parametrize("kw, message", INVALID_CASES, ids=["%s: %s" % (",".join(k), m) for k, m in INVALID_CASES])
def test_every_invalid_call_is_turned_away_with_its_message(kw, message):
    rc, why = changed(**kw).run()
    assert rc == INVALID and why.startswith("keyframe admit: ") and message in why, (kw, rc, why)


def test_a_frame_descriptor_array_off_alignment_and_levels_up_with_a_vocabulary():
    rc, why = changed(**{"shift_out.desc": 4}).run()         # the frame's own descriptors
    assert rc == INVALID and "16-byte aligned" in why

    class Vocab:                                             # any non-null handle: the validation never looks inside
        _h = C.c_void_p(64)
    rc, why = changed(args_vocab=Vocab(), args_levels_up=-1).run()
    assert rc == INVALID and "levels_up -1" in why
    assert changed(args_vocab=Vocab(), args_levels_up=0).run() == (0, "")


def test_every_cap_holds_at_its_limit_and_one_beyond():
    for kw, text in ((dict(capacity=MAX_STRIDE + 1), "view capacity 8193"), (dict(cap_kp=MAX_STRIDE + 1), "cap_kp 8193"), (dict(args_n_tracks=MAX_STRIDE + 1), "8193 tracks"),
                     (dict(n_kf=MAX_KF + 1), "65537 slots"), (dict(stride=MAX_STRIDE + 1), "stride 8193"), (dict(n_mp=MAX_MP), "16777216 map points"),
                     (dict(args_depth_stride=1 << 20, args_depth_height=1 << 11), "below 2^31")):
        rc, why = changed(**kw).run()
        assert rc == CAPACITY and text in why and "caps" in why, (text, rc, why)
    for kw in (dict(capacity=MAX_STRIDE), dict(cap_kp=MAX_STRIDE), dict(args_n_tracks=MAX_STRIDE), dict(n_kf=MAX_KF), dict(stride=MAX_STRIDE), dict(n_mp=MAX_MP - 1),
               dict(args_depth_stride=(1 << 20) - 1, args_depth_height=1 << 11)):
        assert changed(**kw).run() == (0, ""), list(kw)


PROGRAM = r"""
#include "mi355slam.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
struct Call {
    int n_kf = 3, stride = 10, n_mp = 7, n_pool = 40, frame = 0;
    alignas(16) uint32_t view_desc[24 * 8] = {0}, pool[40 * 8] = {0}, frame_desc[10 * 8 + 4] = {0};
    std::vector<int32_t> i32 = std::vector<int32_t>(64, 0);
    std::vector<float> f32 = std::vector<float>(64, 0.f);
    std::vector<double> f64 = std::vector<double>(64, 0.0);
    std::vector<uint8_t> u8 = std::vector<uint8_t>(16, 0);
    int32_t ids[2] = {5, 6}, counts[3];
    float depth[2] = {1.f, 2.f};
    ms_keypoints view;
    ms_admit_args args;
    ms_admit_frame out;
    ms_admit_host host;
    char why[128];
    Call() {
        view = ms_keypoints{12, i32.data(), f32.data(), f32.data(), f32.data(), i32.data(), view_desc, i32.data()};
        std::memset(&args, 0, sizeof args);
        args.slot = 1; args.desc_base = 30; args.cam = ms_pinhole{500.0, 501.0, 320.0, 240.0, 640, 480}; args.levels_up = 4;
        args.track_ids = ids; args.track_depth = depth; args.n_tracks = 2;
        args.depth_image = f32.data(); args.depth_width = 6; args.depth_height = 4; args.depth_stride = 6;
        out = ms_admit_frame{10, frame_desc, f32.data(), i32.data(), f64.data(), u8.data(), f32.data(), f32.data(), i32.data(), i32.data(), i32.data(), i32.data()};
        std::memset(&host, 0, sizeof host);
    }
    int run() {
        why[0] = 0;
        return ms_keyframe_admit_validate(&view, frame, i32.data(), n_kf, stride, n_mp, f32.data(), f32.data(), i32.data(), f32.data(), pool, n_pool, f64.data(), &args, &out, &host,
                                          counts, why, sizeof why);
    }
};
static int fails = 0;
static void expect(Call &c, int rc, const char *text) {
    const int got = c.run();
    if (got != rc || !std::strstr(c.why, text)) { std::printf("want %d '%s', got %d '%s'\n", rc, text, got, c.why); ++fails; }
}
int main() {
    { Call c; expect(c, MS_OK, ""); }
    { Call c; c.args.slot = 3; expect(c, MS_ERR_INVALID, "slot 3 outside [0, 3)"); }
    { Call c; c.frame = -1; expect(c, MS_ERR_INVALID, "frame -1 outside"); }
    { Call c; c.args.desc_base = 41; expect(c, MS_ERR_INVALID, "desc_base 41 outside [0, 40]"); }
    { Call c; c.out.desc = c.frame_desc + 1; expect(c, MS_ERR_INVALID, "16-byte aligned"); }
    { Call c; c.view.desc = nullptr; expect(c, MS_ERR_INVALID, "of the view)"); }
    { Call c; c.out.node_start = nullptr; expect(c, MS_ERR_INVALID, "missing array (a frame array of out)"); }
    { Call c; c.args.pose[7] = std::nan(""); expect(c, MS_ERR_INVALID, "pose[7] is not finite"); }
    { Call c; c.args.cam.fy = 0.0; expect(c, MS_ERR_INVALID, "bad camera"); }
    { Call c; c.args.track_depth = nullptr; expect(c, MS_ERR_INVALID, "missing array (track_ids or track_depth)"); }
    { Call c; c.args.depth_stride = 5; expect(c, MS_ERR_INVALID, "row stride 5"); }
    { Call c; c.args.depth_image = nullptr; c.args.depth_stride = 0; expect(c, MS_OK, ""); }
    { Call c; c.stride = 0; expect(c, MS_ERR_INVALID, "stride 0"); }
    { Call c; c.out.cap_kp = MS_COVIS_MAX_STRIDE + 1; expect(c, MS_ERR_CAPACITY, "cap_kp 8193"); }
    { Call c; c.out.cap_kp = MS_COVIS_MAX_STRIDE; expect(c, MS_OK, ""); }
    { Call c; c.n_mp = MS_COVIS_MAX_MP; expect(c, MS_ERR_CAPACITY, "caps"); }
    { Call c; c.args.depth_stride = 1 << 20; c.args.depth_height = 1 << 11; expect(c, MS_ERR_CAPACITY, "below 2^31"); }
    { Call s; char tiny[8]; s.stride = 0;                    // a short buffer is not overrun, a missing one is not written
      if (ms_keyframe_admit_validate(&s.view, 0, s.i32.data(), 3, 0, 7, s.f32.data(), s.f32.data(), s.i32.data(), s.f32.data(), s.pool, 40, s.f64.data(), &s.args, &s.out, nullptr,
                                     s.counts, tiny, sizeof tiny) != MS_ERR_INVALID || std::strlen(tiny) != 7) ++fails;
      if (ms_keyframe_admit_validate(&s.view, 0, s.i32.data(), 3, 0, 7, s.f32.data(), s.f32.data(), s.i32.data(), s.f32.data(), s.pool, 40, s.f64.data(), &s.args, &s.out, nullptr,
                                     s.counts, nullptr, 0) != MS_ERR_INVALID) ++fails; }
    std::printf("keyframe admit validate alone: %d failures\n", fails);
    return fails ? 1 : 0;
}
"""


def test_the_validation_alone_runs_clean_under_sanitizers(tmp_path):
    """A program with its own main and the public header only, compiled together with map_checks.cpp (no HIP, no library, nothing preloaded)."""
    src, exe = tmp_path / "alone.cpp", tmp_path / "alone"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           str(src), os.path.join(CSRC, "map_checks.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and "0 failures" in run.stdout, run.stdout + run.stderr
