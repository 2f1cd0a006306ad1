"""CPU checks of the surface of ms_frame_admit: the header declares the call, its struct and its validation twin, the library
exports them, Python binds them with the header's struct layout, and ms_frame_admit_validate, the host-only half that runs in front of any
device call, accepts the valid cases, turns every MS_ERR_INVALID case away with its message and holds every cap -- through the library, and
again in a program of its own compiled with map_checks.cpp alone under ASan and UBSan.  The validation dereferences HOST arguments only, so
host arrays stand in for the device arrays.  The launch, upload, download and wait counts are read in the entry point's source."""
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
    for name in ("ms_frame_admit", "ms_frame_admit_validate"):
        assert hasattr(mi355slam.lib(), name), name
    for name in ("frame_admit", "frame_admit_device", "frame_admit_validate"):
        assert callable(getattr(mi355slam, name)), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bframe_admit\.hip\b", mk, flags=re.M) and not re.search(r"^frame_admit\.o\s*:.*FLAGS", mk, flags=re.M)
    src = open(os.path.join(CSRC, "frame_admit.hip")).read()
    internal = open(os.path.join(CSRC, "ms_internal.h")).read()
    assert '#include "ms_scan.h"' in src and "block_rank<kBlock>" in src and "MS_WS_FRAME_ADMIT" in src and "ms_pinned(" in src and "MS_WS_FRAME_ADMIT" in internal
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\batomic\w*", code)                                                           # positions are prefix counts, the sums block scans
    assert "__shfl" not in code and "__popcll" not in code and "__ballot" not in code                    # the unit has no scan of its own
    # the depth expression is the shared one, letter for letter
    admit = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "keyframe_admit.hip")).read())
    squeeze = lambda t: "".join(t.split())
    rule = squeeze("""if (depth < 0) { depth = -1.f; if (A.depth_image) { const int ix = __float2int_rn(x), iy = __float2int_rn(y);
                      if (ix >= 0 && ix < A.depth_w && iy >= 0 && iy < A.depth_h) depth = A.depth_image[(size_t)iy * A.depth_stride + ix]; } }""")
    assert rule in squeeze(code) and rule in squeeze(admit)
    body = code.split('extern "C" int ms_frame_admit(')[1]
    assert body.count("hipLaunchKernelGGL(") == 2 and "TWO launches" in header(True) and "TWO launches" in src
    assert body.count("hipMemcpyHostToDevice") == 1 and body.count("hipMemcpyDeviceToHost") == 1 and body.count("hipStreamSynchronize") == 1
    assert body.index("hipStreamSynchronize") > body.rindex("hipLaunchKernelGGL(")                         # the one wait is behind the last launch
    assert not re.search(r"\bhipMalloc|\bhipHostMalloc|\bnew\b|std::vector", body)                        # the workspace and the pinned block only


def test_the_header_declares_the_struct_the_binding_uses_and_the_twin_takes_the_arguments_of_the_call():
    assert "DESIGN 9.22" in header(True)
    A = mi355slam.FrameAdmitArgsC
    assert struct_fields("ms_frame_admit_args") == [k for k, _ in A._fields_]
    assert C.sizeof(A) == 8 + 96 + 8 + 16 + 8 + 16 and A.pose.offset == 8 and A.depth_image.offset == 104 and A.valid_mask.offset == 128 and A.mask_stride.offset == 144
    call, twin = declaration("ms_frame_admit"), declaration("ms_frame_admit_validate")
    assert call[0] == "ms_ctx *ctx" and call[1:] == twin[:-2] and twin[-2:] == ["char *why", "size_t why_bytes"]
    assert len(call) == 21 and [p.split("*")[-1].split()[-1] for p in call[1:]] == [
        "kf_mp", "n_kf", "stride", "n_mp", "kp_x", "kp_y", "kp_octave", "kp_depth", "kf_pose", "x", "y", "id", "depth", "keep", "n_tracks", "args", "kp_track", "kp_feature",
        "cap_kp", "counts"]
    assert "ms_frame_admit_check" not in header(True) and re.search(r"/\*[^\n]*_validate[^\n]*22[^\n]*\*/\s*int ms_frame_admit_validate", header(True))
    checks = open(os.path.join(CSRC, "map_checks.cpp")).read()
    assert 'extern "C" int ms_frame_admit_validate(' in checks
    assert "ms_frame_admit_validate(" not in open(os.path.join(CSRC, "frame_admit.hip")).read().split('extern "C"')[0]
    # the header says what stands in for what, the deviation, and what the call leaves out; ms_keyframe_admit's header points here
    text = " ".join(header(True).split())
    for phrase in ("stand-in for frame->getDepth", "keyframe.cpp:129", "the FEATURE index", "ms_match_tracked refuses such a frame", "Not covered: colours (getPixel), a device-resident kp_track",
                   "come in through ms_frame_admit"):
        assert phrase in text, phrase


class Call:
    """One call of ms_frame_admit_validate: 3 slots x 10, five features, a 6 x 4 image and mask."""

    def __init__(self):
        self.n_kf, self.stride, self.n_mp, self.cap_kp = 3, 10, 7, 5
        z = lambda n, dt: np.zeros(n, dt)
        self.tables = dict(kf_mp=z(30, np.int32), kp_x=z(30, np.float32), kp_y=z(30, np.float32), kp_octave=z(30, np.int32), kp_depth=z(30, np.float32), kf_pose=z(36, np.float64))
        self.features = dict(x=np.arange(5, dtype=np.float32), y=np.arange(5, dtype=np.float32), id=np.array([9, 3, 7, 0, 5], np.int32), depth=z(5, np.float32),
                             keep=np.ones(5, np.uint8))
        self.args = dict(slot=1, pose=np.arange(12.0), depth_image=z(24, np.float32), depth_width=6, depth_height=4, depth_stride=6, valid_mask=z(24, np.uint8), mask_width=6,
                         mask_height=4, mask_stride=6)
        self.kp_track = self.kp_feature = self.counts = True

    def run(self):
        return mi355slam.frame_admit_validate(self.tables, self.n_kf, self.stride, self.n_mp, self.features, self.args, self.cap_kp, self.kp_track, self.kp_feature, self.counts)


def changed(**kw):
    c = Call()
    for k, v in kw.items():
        if k.startswith("args_"):
            c.args[k[5:]] = v
        elif k.startswith("f_"):
            c.features[k[2:]] = v
        elif k in c.tables:
            c.tables[k] = v
        else:
            setattr(c, k, v)
    return c


def test_valid_calls_and_the_zero_sizes_pass():
    assert Call().run() == (0, "")
    assert changed(f_keep=None).run() == (0, "") and changed(kp_track=False).run() == (0, "") and changed(kp_feature=False, kp_track=False).run() == (0, "")
    assert changed(args_depth_image=None, args_depth_width=0, args_depth_height=0).run() == (0, "")
    assert changed(args_valid_mask=None, args_mask_width=0, args_mask_stride=-3).run() == (0, "")          # the sizes are read with a mask only
    assert changed(args_slot=0).run() == (0, "") and changed(args_slot=2).run() == (0, "")
    assert changed(n_mp=0).run() == (0, "") and changed(cap_kp=0).run() == (0, "") and changed(stride=1).run() == (0, "")       # whether n_kp fits is the device's verdict
    assert changed(f_n_tracks=0).run() == (0, "") and changed(f_n_tracks=0, f_x=None, f_y=None, f_id=None, f_depth=None, f_keep=None).run() == (0, "")
    assert changed(args_depth_stride=9, args_mask_stride=8).run() == (0, "")
    assert changed(f_depth=np.array([np.nan, -1, np.inf, 0, 1], np.float32)).run() == (0, "")              # a depth is copied, never judged
    assert changed(f_id=np.array([0, 1, 2, 3, 2**31 - 1], np.int32)).run() == (0, "")


NAN, INF = float("nan"), float("inf")
F32 = lambda *v: np.array(v, np.float32)
INVALID_CASES = [
    (dict(n_kf=-1), "negative size (-1 slots"), (dict(n_mp=-1), "-1 map points"), (dict(f_n_tracks=-1), "-1 features"), (dict(cap_kp=-2), "cap_kp -2"),
    (dict(stride=0), "stride 0"), (dict(stride=-4), "stride -4"),
    (dict(args=None), "missing array (args or counts)"), (dict(counts=False), "missing array (args or counts)"),
] + [(dict([(k, None)]), "missing array (kf_mp, the keypoint table or kf_pose)") for k in ("kf_mp", "kp_x", "kp_y", "kp_octave", "kp_depth", "kf_pose")] + [
    (dict([("f_" + k, None), ("f_n_tracks", 5)]), "missing array (x, y, id or depth with 5 features)") for k in ("x", "y", "id", "depth")
] + [
    (dict(args_slot=-1), "slot -1 outside [0, 3)"), (dict(args_slot=3), "slot 3 outside [0, 3)"), (dict(n_kf=0), "slot 1 outside [0, 0)"),
    (dict(args_pose=[0, 1, 2, NAN, 4, 5, 6, 7, 8, 9, 10, 11]), "pose[3] is not finite"), (dict(args_pose=[0] * 11 + [-INF]), "pose[11] is not finite"),
    (dict(args_depth_width=0), "a depth image of 0 x 4"), (dict(args_depth_height=0), "a depth image of 6 x 0"), (dict(args_depth_stride=5), "a depth image of 6 x 4, row stride 5"),
    (dict(args_mask_width=0), "a valid mask of 0 x 4"), (dict(args_mask_height=-1), "a valid mask of 6 x -1"), (dict(args_mask_stride=5), "a valid mask of 6 x 4, row stride 5"),
    (dict(f_x=F32(0, 1, NAN, 3, 4)), "feature 2 has a coordinate that is not finite"), (dict(f_y=F32(0, 1, 2, 3, INF)), "feature 4 has a coordinate that is not finite"),
    (dict(f_x=F32(-INF, 1, 2, 3, 4)), "feature 0 has a coordinate"),
    (dict(f_id=np.array([9, -1, 7, 0, 5], np.int32)), "feature 1 has the id -1"), (dict(f_id=np.array([9, 3, 7, 0, -2**31], np.int32)), "feature 4 has the id -2147483648"),
    (dict(f_id=np.array([9, 3, 7, 3, 5], np.int32)), "track id 3 is listed twice"), (dict(f_id=np.array([0, 3, 7, 5, 0], np.int32)), "track id 0 is listed twice"),
]


@pytest.mark.parametrize("kw, message", INVALID_CASES, ids=["%s: %s" % (",".join(k), m) for k, m in INVALID_CASES])
def test_every_invalid_call_is_turned_away_with_its_message(kw, message):
    rc, why = changed(**kw).run()
    assert rc == INVALID and why.startswith("frame admit: ") and message in why, (kw, rc, why)


def test_a_dropped_feature_is_validated_like_any_other():
    """keep is the device's to read: a feature that keep drops still has to be finite and to carry an id of its own."""
    keep = np.array([1, 0, 1, 1, 1], np.uint8)
    assert changed(f_keep=keep, f_id=np.array([9, 7, 7, 0, 5], np.int32)).run()[0] == INVALID
    assert changed(f_keep=keep, f_x=F32(0, NAN, 2, 3, 4)).run()[0] == INVALID


def test_every_cap_holds_at_its_limit_and_one_beyond():
    many = lambda n: dict(f_x=np.zeros(n, np.float32), f_y=np.zeros(n, np.float32), f_id=np.arange(n, dtype=np.int32), f_depth=np.zeros(n, np.float32), f_keep=None)
    for kw, text in ((many(MAX_STRIDE + 1), "8193 features"), (dict(cap_kp=MAX_STRIDE + 1), "cap_kp 8193"),
                     (dict(n_kf=MAX_KF + 1), "65537 slots"), (dict(stride=MAX_STRIDE + 1), "stride 8193"), (dict(n_mp=MAX_MP), "16777216 map points"),
                     (dict(args_depth_stride=1 << 20, args_depth_height=1 << 11), "a depth image of 2048 rows of 1048576 elements, caps below 2^31"),
                     (dict(args_mask_stride=1 << 20, args_mask_height=1 << 11), "a valid mask of 2048 rows of 1048576 bytes, caps below 2^31")):
        rc, why = changed(**kw).run()
        assert rc == CAPACITY and text in why and "caps" in why, (text, rc, why)
    for kw in (many(MAX_STRIDE), dict(cap_kp=MAX_STRIDE), dict(n_kf=MAX_KF), dict(stride=MAX_STRIDE), dict(n_mp=MAX_MP - 1),
               dict(args_depth_stride=(1 << 20) - 1, args_depth_height=1 << 11), dict(args_mask_stride=(1 << 20) - 1, args_mask_height=1 << 11)):
        assert changed(**kw).run() == (0, ""), list(kw)


PROGRAM = r"""
#include "mi355slam.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
struct Call {
    int n_kf = 3, stride = 10, n_mp = 7, n_tracks = 5, cap_kp = 5;
    std::vector<int32_t> i32 = std::vector<int32_t>(64, 0);
    std::vector<float> f32 = std::vector<float>(64, 0.f);
    std::vector<double> f64 = std::vector<double>(64, 0.0);
    std::vector<uint8_t> u8 = std::vector<uint8_t>(64, 1);
    std::vector<float> x = {0.f, 1.f, 2.f, 3.f, 4.f}, y = {0.f, 1.f, 2.f, 3.f, 4.f}, depth = {1.f, -1.f, 0.f, 2.f, 3.f};
    std::vector<int32_t> id = {9, 3, 7, 0, 5};
    const uint8_t *keep = nullptr;
    int32_t counts[4];
    ms_frame_admit_args args;
    char why[160];
    Call() {
        std::memset(&args, 0, sizeof args);
        args.slot = 1;
        args.depth_image = f32.data(); args.depth_width = 6; args.depth_height = 4; args.depth_stride = 6;
        args.valid_mask = u8.data(); args.mask_width = 6; args.mask_height = 4; args.mask_stride = 6;
        keep = u8.data();
    }
    int run() {
        why[0] = 0;
        return ms_frame_admit_validate(i32.data(), n_kf, stride, n_mp, f32.data(), f32.data(), i32.data(), f32.data(), f64.data(), x.data(), y.data(), id.data(), depth.data(), keep,
                                       n_tracks, &args, i32.data(), i32.data(), cap_kp, counts, why, sizeof why);
    }
};
static int fails = 0;
static void expect(Call &c, int rc, const char *text) {
    const int got = c.run();
    if (got != rc || !std::strstr(c.why, text)) { std::printf("want %d '%s', got %d '%s'\n", rc, text, got, c.why); ++fails; }
}
int main() {
    { Call c; expect(c, MS_OK, ""); }
    { Call c; c.keep = nullptr; expect(c, MS_OK, ""); }
    { Call c; c.args.slot = 3; expect(c, MS_ERR_INVALID, "slot 3 outside [0, 3)"); }
    { Call c; c.args.slot = -1; expect(c, MS_ERR_INVALID, "slot -1 outside"); }
    { Call c; c.x[2] = std::nanf(""); expect(c, MS_ERR_INVALID, "feature 2 has a coordinate that is not finite"); }
    { Call c; c.y[4] = -std::numeric_limits<float>::infinity(); expect(c, MS_ERR_INVALID, "feature 4 has a coordinate"); }
    { Call c; c.id[1] = -1; expect(c, MS_ERR_INVALID, "feature 1 has the id -1"); }
    { Call c; c.id[3] = 9; expect(c, MS_ERR_INVALID, "track id 9 is listed twice"); }
    { Call c; c.args.pose[7] = std::nan(""); expect(c, MS_ERR_INVALID, "pose[7] is not finite"); }
    { Call c; c.args.depth_stride = 5; expect(c, MS_ERR_INVALID, "a depth image of 6 x 4, row stride 5"); }
    { Call c; c.args.mask_width = 0; expect(c, MS_ERR_INVALID, "a valid mask of 0 x 4"); }
    { Call c; c.args.depth_image = nullptr; c.args.depth_stride = 0; c.args.valid_mask = nullptr; c.args.mask_height = 0; expect(c, MS_OK, ""); }
    { Call c; c.stride = 0; expect(c, MS_ERR_INVALID, "stride 0"); }
    { Call c; c.n_tracks = -1; expect(c, MS_ERR_INVALID, "negative size"); }
    { Call c; c.cap_kp = -1; expect(c, MS_ERR_INVALID, "cap_kp -1"); }
    { Call c; c.n_tracks = 0; c.x.clear(); c.y.clear(); c.id.clear(); c.depth.clear(); expect(c, MS_OK, ""); }
    { Call c; c.cap_kp = MS_COVIS_MAX_STRIDE + 1; expect(c, MS_ERR_CAPACITY, "cap_kp 8193"); }
    { Call c; c.cap_kp = MS_COVIS_MAX_STRIDE; expect(c, MS_OK, ""); }
    { Call c; c.n_mp = MS_COVIS_MAX_MP; expect(c, MS_ERR_CAPACITY, "caps"); }
    { Call c; c.args.mask_stride = 1 << 20; c.args.mask_height = 1 << 11; expect(c, MS_ERR_CAPACITY, "below 2^31"); }
    { Call c; const int n = MS_COVIS_MAX_STRIDE; c.n_tracks = n; c.x.assign(n, 1.f); c.y.assign(n, 2.f); c.depth.assign(n, 0.f); c.id.resize(n); c.keep = nullptr;
      for (int i = 0; i < n; ++i) c.id[i] = n - i;          // the largest list, descending: sorted on a copy
      expect(c, MS_OK, "");
      if (c.id[0] != n) ++fails;                             // the caller's ids are not reordered
      c.id[n - 1] = c.id[0]; expect(c, MS_ERR_INVALID, "is listed twice");
      c.n_tracks = n + 1; expect(c, MS_ERR_CAPACITY, "8193 features"); }
    { Call s; char tiny[8]; s.stride = 0;                    // a short buffer is not overrun, a missing one is not written
      if (ms_frame_admit_validate(s.i32.data(), 3, 0, 7, s.f32.data(), s.f32.data(), s.i32.data(), s.f32.data(), s.f64.data(), s.x.data(), s.y.data(), s.id.data(), s.depth.data(), nullptr,
                                  5, &s.args, nullptr, nullptr, 5, s.counts, tiny, sizeof tiny) != MS_ERR_INVALID || std::strlen(tiny) != 7) ++fails;
      if (ms_frame_admit_validate(s.i32.data(), 3, 0, 7, s.f32.data(), s.f32.data(), s.i32.data(), s.f32.data(), s.f64.data(), s.x.data(), s.y.data(), s.id.data(), s.depth.data(), nullptr,
                                  5, &s.args, nullptr, nullptr, 5, s.counts, nullptr, 0) != MS_ERR_INVALID) ++fails;
      if (ms_frame_admit_validate(s.i32.data(), 3, 10, 7, s.f32.data(), s.f32.data(), s.i32.data(), s.f32.data(), s.f64.data(), s.x.data(), s.y.data(), s.id.data(), s.depth.data(), nullptr,
                                  5, nullptr, nullptr, nullptr, 5, s.counts, nullptr, 0) != MS_ERR_INVALID) ++fails; }
    std::printf("frame admit validate alone: %d failures\n", fails);
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
