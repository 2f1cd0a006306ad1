"""CPU checks of the surface of ms_map_publish: the header declares the call, its struct and its validation twin, the library
exports them, Python binds them with the header's struct layout, and ms_map_publish_validate, the host-only half that runs in front of any
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
PUB = [k for k, _, _ in mi355slam.MAP_PUBLISH_PUB]
EV = [k for k, _, _ in mi355slam.MAP_PUBLISH_EV]


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
    return [d.split()[-1].lstrip("*") for d in m.group(1).split(";") if d.split()]


def test_library_exports_the_calls_and_python_binds_them():
    for name in ("ms_map_publish", "ms_map_publish_validate"):
        assert hasattr(mi355slam.lib(), name), name
    for name in ("map_publish", "map_publish_device", "map_publish_validate"):
        assert callable(getattr(mi355slam, name)), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmap_publish\.hip\b", mk, flags=re.M) and not re.search(r"^map_publish\.o\s*:.*FLAGS", mk, flags=re.M)
    src = open(os.path.join(CSRC, "map_publish.hip")).read()
    internal = open(os.path.join(CSRC, "ms_internal.h")).read()
    assert '#include "ms_scan.h"' in src and "block_rank<kBlock>" in src and "block_offsets<kBlock>" in src and "MS_WS_MAP_PUBLISH" in src and "ms_pinned(" in src
    assert "MS_WS_MAP_PUBLISH" in internal and re.search(r"included by[^\n]*\bmap_publish\b", open(os.path.join(CSRC, "ms_scan.h")).read())
    code = re.sub(r"//[^\n]*", "", src)
    assert set(re.findall(r"\batomic\w*", code)) == {"atomicOr"} and len(re.findall(r"\batomicOr\(", code)) == 2      # the only atomics OR bits into bitmap words
    assert "__shfl" not in code and "__popcll" not in code and "__ballot" not in code and "asm" not in code            # no scan of its own, plain HIP C++
    body = code.split('extern "C" int ms_map_publish(')[1]
    assert body.count("hipLaunchKernelGGL(") == 5 and "FIVE launches" in header(True) and "FIVE launches" in src
    assert body.count("hipMemcpyHostToDevice") == 1 and body.count("hipMemcpyDeviceToHost") == 2 and body.count("hipStreamSynchronize") == 2       # one wait per download
    first_wait = body.index("hipStreamSynchronize")
    assert first_wait > body.rindex("hipLaunchKernelGGL(")                                                # no wait between the launches
    assert body.index("hipMemcpyDeviceToHost") < first_wait < body.rindex("hipMemcpyDeviceToHost") < body.rindex("hipStreamSynchronize")
    assert body.index("MS_ERR_CAPACITY") < body.rindex("hipMemcpyDeviceToHost")                            # a refusal downloads the head alone
    assert not re.search(r"\bhipMalloc|\bhipHostMalloc|\bnew\b|std::vector", body)                        # the workspace and the pinned block only


def test_the_header_declares_the_struct_the_binding_uses_and_the_twin_takes_the_arguments_of_the_call():
    assert "DESIGN 9.23" in header(True)
    A = mi355slam.MapPublishArgsC
    assert struct_fields("ms_map_publish_args") == [k for k, _ in A._fields_] == ["what", "current_slot", "min_record_obs"]
    assert C.sizeof(A) == 12 and A.what.offset == 0 and A.current_slot.offset == 4 and A.min_record_obs.offset == 8
    assert re.search(r"#define MS_PUBLISH_VIEW 1\b", header()) and re.search(r"#define MS_PUBLISH_RECORD 2\b", header())
    assert (mi355slam.MS_PUBLISH_VIEW, mi355slam.MS_PUBLISH_RECORD) == (1, 2)
    call, twin = declaration("ms_map_publish"), declaration("ms_map_publish_validate")
    assert call[0] == "ms_ctx *ctx" and call[1:] == twin[:-2] and twin[-2:] == ["char *why", "size_t why_bytes"]
    assert [p.split("*")[-1].split()[-1] for p in call[1:]] == [
        "mp_pos", "mp_norm", "mp_flags", "mp_live", "n_obs", "mp_color", "n_mp", "kf_mp", "n_kf", "stride", "kf_pose", "local_rows", "n_local", "rec_pos", "rec_state", "args",
        "kf_list", "n_list"] + PUB + ["cap_pub"] + EV + ["cap_ev", "pose_wc", "counts"]
    assert "ms_map_publish_check" not in header(True) and re.search(r"/\*[^\n]*_validate[^\n]*22[^\n]*\*/\s*int ms_map_publish_validate", header(True))
    checks = open(os.path.join(CSRC, "map_checks.cpp")).read()
    assert 'extern "C" int ms_map_publish_validate(' in checks
    assert "ms_map_publish_validate(" not in open(os.path.join(CSRC, "map_publish.hip")).read().split('extern "C"')[0]
    text = " ".join(header(True).replace("\n * ", "\n").split())                    # the comment's line starts taken out
    for phrase in ("MapPointStatus::BAD cannot be seen in a map", "map_point.cpp:154", "one unit in the last place", "one copy more than ms_frame_finish",
                   "the caps are the size of the map and the answer usually is not", "-0.0f equals 0.0f and a NaN always differs", "The reference never reuses an id"):
        assert phrase in text, phrase


class Call:
    """One call of ms_map_publish_validate: 7 rows, 3 slots x 10, four local rows, two listed slots."""

    def __init__(self):
        self.n_mp, self.n_kf, self.stride, self.n_local, self.cap_pub, self.cap_ev, self.n_list = 7, 3, 10, 4, 7, 7, None
        z = lambda n, dt: np.zeros(n, dt)
        self.tables = dict(mp_pos=z(21, np.float64), mp_norm=z(21, np.float32), mp_flags=z(7, np.uint8), mp_live=z(7, np.uint8), n_obs=z(7, np.int32), mp_color=z(21, np.uint8),
                           kf_mp=z(30, np.int32), kf_pose=z(36, np.float64), local_rows=z(4, np.int32), rec_pos=z(21, np.float32), rec_state=z(7, np.uint8))
        self.args = dict(what=3, current_slot=2, min_record_obs=4)
        self.kf_list = [2, 0]
        self.missing = ()

    def run(self):
        return mi355slam.map_publish_validate(self.tables, self.n_mp, self.n_kf, self.stride, self.n_local, self.args, self.kf_list, self.cap_pub, self.cap_ev, self.n_list,
                                              self.missing)


def changed(**kw):
    c = Call()
    for k, v in kw.items():
        if k.startswith("args_"):
            c.args[k[5:]] = v
        elif k in c.tables:
            c.tables[k] = v
        else:
            setattr(c, k, v)
    return c


def test_valid_calls_and_the_zero_sizes_pass():
    assert Call().run() == (0, "")
    assert changed(args_what=1).run() == (0, "") and changed(args_what=2).run() == (0, "")
    assert changed(args_what=1, n_obs=None, rec_pos=None, rec_state=None, missing=EV).run() == (0, "")      # VIEW alone needs nothing of the record
    assert changed(args_what=2, missing=PUB).run() == (0, "")                                               # RECORD alone needs nothing of the view
    assert changed(mp_color=None).run() == (0, "")
    assert changed(local_rows=None, n_local=0).run() == (0, "") and changed(args_current_slot=-1).run() == (0, "") and changed(args_current_slot=0).run() == (0, "")
    assert changed(kf_list=[], missing=("pose_wc",)).run() == (0, "") and changed(kf_list=None, missing=("pose_wc",)).run() == (0, "")
    assert changed(cap_pub=0, cap_ev=0, missing=PUB + EV).run() == (0, "")                                  # whether the streams fit is the device's verdict
    assert changed(args_min_record_obs=0).run() == (0, "") and changed(stride=1).run() == (0, "")
    none = dict(mp_pos=None, mp_norm=None, mp_flags=None, mp_live=None, n_obs=None, rec_pos=None, rec_state=None, mp_color=None)
    assert changed(n_mp=0, **none).run() == (0, "")
    assert changed(n_mp=0, n_kf=0, kf_mp=None, kf_pose=None, kf_list=[], args_current_slot=-1, missing=("pose_wc",), **none).run() == (0, "")
    assert changed(kf_list=[0, 1, 2]).run() == (0, "")


INVALID_CASES = [
    (dict(n_mp=-1), "negative size (-1 map points"), (dict(n_kf=-1), "-1 slots"), (dict(n_local=-1), "-1 local rows"), (dict(n_list=-1), "-1 listed slots"),
    (dict(cap_pub=-2), "cap_pub -2"), (dict(cap_ev=-3), "cap_ev -3"), (dict(stride=0), "stride 0"), (dict(stride=-4), "stride -4"),
    (dict(args=None), "missing array (args or counts)"), (dict(missing=("counts",)), "missing array (args or counts)"),
    (dict(args_what=0), "what 0 outside 1 .. 3"), (dict(args_what=4), "what 4 outside 1 .. 3"), (dict(args_what=-1), "what -1 outside"),
    (dict(args_min_record_obs=-1), "min_record_obs -1"),
] + [(dict([(k, None)]), "missing array (mp_pos, mp_norm, mp_flags or mp_live)") for k in ("mp_pos", "mp_norm", "mp_flags", "mp_live")] + [
    (dict([(k, None)]), "missing array (kf_mp or kf_pose)") for k in ("kf_mp", "kf_pose")] + [
    (dict(local_rows=None), "missing array (local_rows with 4 entries)"),
    (dict(kf_list=None, n_list=2), "missing array (kf_list or pose_wc with 2 listed slots)"), (dict(missing=("pose_wc",)), "missing array (kf_list or pose_wc with 2 listed slots)"),
] + [(dict([(k, None)]), "missing array (n_obs, rec_pos or rec_state with MS_PUBLISH_RECORD)") for k in ("n_obs", "rec_pos", "rec_state")] + [
    (dict(missing=(k,)), "missing array (a pub_ array with cap_pub 7)") for k in PUB] + [
    (dict(missing=(k,)), "missing array (an ev_ array with cap_ev 7)") for k in EV] + [
    (dict(args_current_slot=-2), "current slot -2 outside [-1, 3)"), (dict(args_current_slot=3), "current slot 3 outside [-1, 3)"),
    (dict(n_kf=0, kf_list=[], missing=("pose_wc",)), "current slot 2 outside [-1, 0)"),
    (dict(kf_list=[0, 3]), "listed slot 3 outside [0, 3)"), (dict(kf_list=[-1]), "listed slot -1 outside [0, 3)"), (dict(kf_list=[1, 2, 1]), "listed slot 1 is listed twice"),
]


@pytest.mark.parametrize("kw, message", INVALID_CASES, ids=["%s: %s" % (",".join(k), m) for k, m in INVALID_CASES])
def test_every_invalid_call_is_turned_away_with_its_message(kw, message):
    rc, why = changed(**kw).run()
    assert rc == INVALID and why.startswith("map publish: ") and message in why, (kw, rc, why)


def test_every_cap_holds_at_its_limit_and_one_beyond():
    for kw, text in ((dict(n_kf=MAX_KF + 1), "65537 slots"), (dict(stride=MAX_STRIDE + 1), "stride 8193"), (dict(n_mp=MAX_MP), "16777216 map points"),
                     (dict(n_local=MAX_MP), "16777216 local rows"), (dict(n_kf=MAX_KF, kf_list=np.zeros(MAX_KF + 1, np.int32)), "65537 listed slots")):
        rc, why = changed(**kw).run()
        assert rc == CAPACITY and text in why and "caps" in why, (text, rc, why)
    for kw in (dict(n_kf=MAX_KF), dict(stride=MAX_STRIDE), dict(n_mp=MAX_MP - 1), dict(n_local=MAX_MP - 1), dict(n_kf=MAX_KF, kf_list=np.arange(MAX_KF, dtype=np.int32)),
               dict(cap_pub=2**31 - 1, cap_ev=2**31 - 1)):                                                # a capacity beyond the map is only a bound
        assert changed(**kw).run() == (0, ""), list(kw)


PROGRAM = r"""
#include "mi355slam.h"
#include <cstdio>
#include <cstring>
#include <vector>
struct Call {
    int n_mp = 7, n_kf = 3, stride = 10, n_local = 4, n_list = 2, cap_pub = 7, cap_ev = 7;
    std::vector<int32_t> i32 = std::vector<int32_t>(64, 0);
    std::vector<float> f32 = std::vector<float>(64, 0.f);
    std::vector<double> f64 = std::vector<double>(64, 0.0);
    std::vector<uint8_t> u8 = std::vector<uint8_t>(64, 1);
    std::vector<int32_t> list = {2, 0};
    const int32_t *n_obs, *local_rows, *pub_row, *ev_row;
    const uint8_t *mp_color, *rec_state, *ev_kind;
    const float *rec_pos, *pose_wc;
    int32_t counts[8];
    ms_map_publish_args args;
    char why[200];
    Call() {
        args.what = MS_PUBLISH_VIEW | MS_PUBLISH_RECORD; args.current_slot = 2; args.min_record_obs = 4;
        n_obs = local_rows = pub_row = ev_row = i32.data(); mp_color = rec_state = ev_kind = u8.data(); rec_pos = pose_wc = f32.data();
    }
    int run(char *w, size_t bytes, const ms_map_publish_args *a) {
        return ms_map_publish_validate(f64.data(), f32.data(), u8.data(), u8.data(), n_obs, mp_color, n_mp, i32.data(), n_kf, stride, f64.data(), local_rows, n_local, rec_pos,
                                       rec_state, a, list.data(), n_list, pub_row, f32.data(), f32.data(), f32.data(), u8.data(), u8.data(), cap_pub, ev_row, ev_kind, f32.data(),
                                       f32.data(), cap_ev, pose_wc, counts, w, bytes);
    }
    int run() { why[0] = 0; return run(why, sizeof why, &args); }
};
static int fails = 0;
static void expect(Call &c, int rc, const char *text) {
    const int got = c.run();
    if (got != rc || !std::strstr(c.why, text)) { std::printf("want %d '%s', got %d '%s'\n", rc, text, got, c.why); ++fails; }
}
int main() {
    { Call c; expect(c, MS_OK, ""); }
    { Call c; c.args.what = MS_PUBLISH_VIEW; c.n_obs = nullptr; c.rec_pos = nullptr; c.rec_state = nullptr; c.ev_row = nullptr; c.ev_kind = nullptr; expect(c, MS_OK, ""); }
    { Call c; c.args.what = MS_PUBLISH_RECORD; c.pub_row = nullptr; c.mp_color = nullptr; expect(c, MS_OK, ""); }
    { Call c; c.args.what = 0; expect(c, MS_ERR_INVALID, "what 0 outside 1 .. 3"); }
    { Call c; c.args.what = 4; expect(c, MS_ERR_INVALID, "what 4 outside"); }
    { Call c; c.args.current_slot = 3; expect(c, MS_ERR_INVALID, "current slot 3 outside [-1, 3)"); }
    { Call c; c.args.current_slot = -2; expect(c, MS_ERR_INVALID, "current slot -2 outside"); }
    { Call c; c.args.current_slot = -1; expect(c, MS_OK, ""); }
    { Call c; c.args.min_record_obs = -1; expect(c, MS_ERR_INVALID, "min_record_obs -1"); }
    { Call c; c.list = {0, 3}; expect(c, MS_ERR_INVALID, "listed slot 3 outside [0, 3)"); }
    { Call c; c.list = {1, 1}; expect(c, MS_ERR_INVALID, "listed slot 1 is listed twice"); }
    { Call c; c.stride = 0; expect(c, MS_ERR_INVALID, "stride 0"); }
    { Call c; c.n_local = -1; expect(c, MS_ERR_INVALID, "negative size"); }
    { Call c; c.cap_ev = -1; expect(c, MS_ERR_INVALID, "cap_ev -1"); }
    { Call c; c.n_obs = nullptr; expect(c, MS_ERR_INVALID, "n_obs, rec_pos or rec_state with MS_PUBLISH_RECORD"); }
    { Call c; c.rec_state = nullptr; expect(c, MS_ERR_INVALID, "n_obs, rec_pos or rec_state"); }
    { Call c; c.pub_row = nullptr; expect(c, MS_ERR_INVALID, "a pub_ array with cap_pub 7"); }
    { Call c; c.ev_kind = nullptr; expect(c, MS_ERR_INVALID, "an ev_ array with cap_ev 7"); }
    { Call c; c.ev_kind = nullptr; c.cap_ev = 0; expect(c, MS_OK, ""); }
    { Call c; c.local_rows = nullptr; expect(c, MS_ERR_INVALID, "local_rows with 4 entries"); }
    { Call c; c.local_rows = nullptr; c.n_local = 0; expect(c, MS_OK, ""); }
    { Call c; c.pose_wc = nullptr; expect(c, MS_ERR_INVALID, "kf_list or pose_wc with 2 listed slots"); }
    { Call c; c.pose_wc = nullptr; c.n_list = 0; expect(c, MS_OK, ""); }
    { Call c; c.n_mp = 0; c.n_list = 0; expect(c, MS_OK, ""); }
    { Call c; c.n_mp = MS_COVIS_MAX_MP; expect(c, MS_ERR_CAPACITY, "caps"); }
    { Call c; c.n_local = MS_COVIS_MAX_MP; expect(c, MS_ERR_CAPACITY, "16777216 local rows"); }
    { Call c; c.stride = MS_COVIS_MAX_STRIDE + 1; expect(c, MS_ERR_CAPACITY, "stride 8193"); }
    { Call c; const int n = MS_COVIS_MAX_KF; c.n_kf = n; c.n_list = n; c.list.resize(n);
      for (int i = 0; i < n; ++i) c.list[i] = n - 1 - i;     // the largest list, descending: sorted on a copy
      expect(c, MS_OK, "");
      if (c.list[0] != n - 1) ++fails;                       // the caller's list is not reordered
      c.list[n - 1] = c.list[0]; expect(c, MS_ERR_INVALID, "is listed twice");
      c.list.push_back(0); c.n_list = n + 1; expect(c, MS_ERR_CAPACITY, "65537 listed slots"); }
    { Call s; char tiny[8]; s.stride = 0;                    // a short buffer is not overrun, a missing one is not written, missing args are no crash
      if (s.run(tiny, sizeof tiny, &s.args) != MS_ERR_INVALID || std::strlen(tiny) != 7) ++fails;
      if (s.run(nullptr, 0, &s.args) != MS_ERR_INVALID) ++fails;
      s.stride = 10;
      if (s.run(nullptr, 0, nullptr) != MS_ERR_INVALID) ++fails; }
    std::printf("map publish validate alone: %d failures\n", fails);
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
