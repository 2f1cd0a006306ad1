"""CPU checks of the surface of ms_frame_finish: the header declares the call and its validation twin, the library exports them,
Python binds them with the header's struct layout, and ms_frame_finish_validate, the host-only half that runs in front of any device call,
accepts the valid cases, turns every MS_ERR_INVALID case away with its message and holds every cap -- through the library, and again in a
program of its own compiled with map_checks.cpp alone under ASan and UBSan.  The validation dereferences HOST arguments only, so host arrays
stand in for the device tables."""
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
MAX_KF, MAX_STRIDE, MAX_MP, MAX_QUERIES = 65536, 8192, 1 << 24, 4096


def header(comments=False):
    text = open(os.path.join(ROOT, "include", "mi355slam.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declaration(name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header())
    assert m, name
    return [" ".join(p.split()).replace("const ", "") for p in m.group(1).split(",")]


def test_library_exports_the_calls_and_python_binds_them():
    for name in ("ms_frame_finish", "ms_frame_finish_validate"):
        assert hasattr(mi355slam.lib(), name), name
    for name in ("frame_finish", "frame_finish_device"):
        assert callable(getattr(mi355slam.KeyframeTable, name)), name
    assert callable(mi355slam.frame_finish_validate)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bframe_finish\.hip\b", mk, flags=re.M) and not re.search(r"^frame_finish\.o\s*:.*FLAGS", mk, flags=re.M)
    src = open(os.path.join(CSRC, "frame_finish.hip")).read()
    assert '#include "ms_scan.h"' in src and "block_rank<kBlock>" in src and "block_offsets<kBlock>" in src and "MS_WS_FRAME_FINISH" in src and "ms_pinned(" in src
    assert "MS_WS_FRAME_FINISH" in open(os.path.join(CSRC, "ms_internal.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert set(re.findall(r"\batomic\w*", code)) == {"atomicMin", "atomicAdd"} and not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", code)      # integer atomics only
    body = code.split('extern "C" int ms_frame_finish(')[1]
    assert body.count("hipLaunchKernelGGL(") == 6 and body.count("hipMemcpyHostToDevice") == 1 and body.count("hipMemcpyDeviceToHost") == 1
    assert body.count("hipStreamSynchronize") == 1           # one wait, behind the download


def test_the_header_declares_the_struct_the_binding_uses_and_the_twin_takes_the_arguments_of_the_call():
    assert "DESIGN 9.18" in header(True)
    m = re.search(r"typedef struct \{([^}]*)\} ms_frame_finish_args;", header())
    assert m and [d.split()[-1] for d in m.group(1).split(";") if d.split()] == [k for k, _ in mi355slam.FrameFinishArgsC._fields_]
    assert C.sizeof(mi355slam.FrameFinishArgsC) == 8
    call, twin = declaration("ms_frame_finish"), declaration("ms_frame_finish_validate")
    assert call[0] == "ms_ctx *ctx" and call[1:] == twin[:-2] and twin[-2:] == ["char *why", "size_t why_bytes"]
    assert len(call) == 21 and [p.split("*")[-1].split()[-1] for p in call[1:]] == [
        "kf_mp", "n_kf", "stride", "mp_flags", "mp_live", "mp_pos", "mp_track", "n_obs", "n_mp", "kf_id", "remove_slots", "n_remove", "args", "cloud_row", "cloud_kp",
        "cloud_track", "cloud_pos", "removed_rows", "cap_removed", "counts"]
    # the set of ms_*_check twins stays as tests/test_map_checks_corpus.py records it; the line above the twin says why it is named otherwise
    assert "ms_frame_finish_check" not in header(True) and re.search(r"/\*[^\n]*_validate[^\n]*22[^\n]*\*/\s*int ms_frame_finish_validate", header(True))
    checks = open(os.path.join(CSRC, "map_checks.cpp")).read()
    assert 'extern "C" int ms_frame_finish_validate(' in checks and "ms_frame_finish_validate(" not in open(os.path.join(CSRC, "frame_finish.hip")).read().split('extern "C"')[0]


class Call:
    """One call of ms_frame_finish_validate: 5 slots x 8 on 10 map points; slot 2 is empty; slots 4 and 1 are removed; the cloud is slot 4's, 6 keypoints."""

    def __init__(self):
        self.n_kf, self.stride, self.n_mp, self.cloud_slot, self.n_kp, self.cap_removed, self.args = 5, 8, 10, 4, 6, 16, True
        z = lambda n, dt: np.zeros(n, dt)
        self.arrays = dict(kf_mp=np.full(40, -1, np.int32), mp_flags=z(10, np.uint8), mp_live=z(10, np.uint8), mp_pos=z(30, np.float64), mp_track=z(10, np.int32),
                           n_obs=z(10, np.int32), kf_id=np.array([7, 3, -1, 9, 12], np.int32), remove_slots=np.array([4, 1], np.int32), cloud_row=z(6, np.int32),
                           cloud_kp=z(6, np.int32), cloud_track=z(6, np.int32), cloud_pos=z(18, np.float64), removed_rows=z(16, np.int32), counts=z(3, np.int32))

    def run(self):
        rem = self.arrays["remove_slots"]
        n_remove = self.n_remove if "n_remove" in self.__dict__ else (0 if rem is None else len(rem))
        return mi355slam.frame_finish_validate(self.arrays, self.n_kf, self.stride, self.n_mp, n_remove, self.cloud_slot, self.n_kp, self.cap_removed, self.args)


def changed(**kw):
    c = Call()
    for k, v in kw.items():
        if k in c.arrays:
            c.arrays[k] = v
        else:
            setattr(c, k, v)
    return c


def i32(*v):
    return np.array(v, np.int32)


def test_valid_calls_and_the_zero_sizes_pass():
    assert Call().run() == (0, "")
    for k in ("mp_track", "n_obs", "cloud_row", "cloud_kp", "cloud_track", "cloud_pos"):                 # each may be NULL
        assert changed(**{k: None}).run() == (0, ""), k
    assert changed(remove_slots=i32(), mp_live=None).run() == (0, "")                                   # nothing removed: no live bytes needed
    assert changed(remove_slots=None, n_remove=0, removed_rows=None, cap_removed=0).run() == (0, "")
    assert changed(cloud_slot=-1).run() == (0, "") and changed(cloud_slot=-1, remove_slots=i32()).run() == (0, "")
    assert changed(n_kp=0).run() == (0, "") and changed(n_kp=8).run() == (0, "")
    assert changed(n_mp=0, mp_flags=None, mp_pos=None).run() == (0, "")
    assert changed(n_kf=0, kf_mp=None, kf_id=None, remove_slots=i32(), cloud_slot=-1).run() == (0, "")
    assert changed(cap_removed=0, removed_rows=None).run() == (0, "")                                   # the call then reports what it needs


INVALID_CASES = [
    (dict(n_kf=-1), "negative size"), (dict(n_mp=-1), "negative size"), (dict(n_remove=-1), "negative size (-1 removed slots"), (dict(cap_removed=-1), "capacity -1"),
    (dict(stride=0), "stride 0"), (dict(args=False), "missing array (args or counts)"), (dict(counts=None), "missing array (args or counts)"),
    (dict(kf_mp=None), "missing array (kf_mp or kf_id)"), (dict(kf_id=None), "missing array (kf_mp or kf_id)"),
    (dict(mp_flags=None), "missing array (mp_flags or mp_pos)"), (dict(mp_pos=None), "missing array (mp_flags or mp_pos)"),
    (dict(remove_slots=None, n_remove=2), "missing array (remove_slots)"), (dict(removed_rows=None), "missing array (removed_rows)"),
    (dict(mp_live=None), "mp_live == NULL with 2 removed slots"),
    (dict(kf_id=i32(7, 3, -1, 9, 7)), "kf_id 7 is listed twice"),
    (dict(cloud_slot=-2), "cloud slot -2 outside [-1, 5)"), (dict(cloud_slot=5), "cloud slot 5 outside [-1, 5)"), (dict(cloud_slot=2), "cloud slot 2 is empty (kf_id -1)"),
    (dict(n_kp=-1), "-1 keypoints in a table of stride 8"), (dict(n_kp=9), "9 keypoints in a table of stride 8"), (dict(n_kp=9, cloud_slot=-1), "9 keypoints"),
    (dict(remove_slots=i32(4, 5)), "removed slot 5 outside [0, 5)"), (dict(remove_slots=i32(-1, 1)), "removed slot -1 outside [0, 5)"),
    (dict(remove_slots=i32(4, 1, 4)), "removed slot 4 is listed twice"), (dict(remove_slots=i32(4, 2)), "removed slot 2 is empty (kf_id -1)"),
]


@pytest.mark.parametrize("kw, message", INVALID_CASES, ids=[m for _, m in INVALID_CASES])
def test_every_invalid_call_is_turned_away_with_its_message(kw, message):
    rc, why = changed(**kw).run()
    assert rc == INVALID and why.startswith("frame finish: ") and message in why, (kw, rc, why)


def test_every_cap_holds_at_its_limit_and_one_beyond():
    ids = lambda n: np.arange(n, dtype=np.int32)
    for kw, text in ((dict(n_kf=MAX_KF + 1, kf_id=ids(MAX_KF + 1)), "65537 slots"), (dict(stride=MAX_STRIDE + 1), "stride 8193"), (dict(n_mp=MAX_MP), "16777216 map points"),
                     (dict(n_kf=MAX_QUERIES + 1, kf_id=ids(MAX_QUERIES + 1), remove_slots=ids(MAX_QUERIES + 1)), "4097 removed slots")):
        rc, why = changed(**kw).run()
        assert rc == CAPACITY and text in why and "caps" in why, (text, rc, why)
    for kw in (dict(n_kf=MAX_KF, kf_id=ids(MAX_KF)), dict(stride=MAX_STRIDE, n_kp=MAX_STRIDE), dict(n_mp=MAX_MP - 1),
               dict(n_kf=MAX_QUERIES + 1, kf_id=ids(MAX_QUERIES + 1), remove_slots=ids(MAX_QUERIES))):
        assert changed(**kw).run() == (0, ""), list(kw)


PROGRAM = r"""
#include "mi355slam.h"
#include <cstdio>
#include <cstring>
#include <vector>
struct Call {
    int n_kf = 5, stride = 8, n_mp = 10, n_remove = 2, cap = 16;
    std::vector<int32_t> kf_mp = std::vector<int32_t>(40, -1), kf_id = {7, 3, -1, 9, 12}, remove = {4, 1}, out = std::vector<int32_t>(16, 0);
    std::vector<uint8_t> bytes = std::vector<uint8_t>(10, 0);
    std::vector<double> pos = std::vector<double>(30, 0.0);
    ms_frame_finish_args args = {4, 6};
    bool has_live = true;
    char why[96];
    int run() {
        why[0] = 0;
        return ms_frame_finish_validate(kf_mp.data(), n_kf, stride, bytes.data(), has_live ? bytes.data() : nullptr, pos.data(), nullptr, nullptr, n_mp, kf_id.data(), remove.data(), n_remove, &args, nullptr,
                                        nullptr, nullptr, nullptr, out.data(), cap, out.data(), why, sizeof why);
    }
};
static int fails = 0;
static void expect(Call c, int rc, const char *text) {
    const int got = c.run();
    if (got != rc || !std::strstr(c.why, text)) { std::printf("want %d '%s', got %d '%s'\n", rc, text, got, c.why); ++fails; }
}
int main() {
    Call c;
    expect(c, MS_OK, "");
    c.remove = {4, 4}; expect(c, MS_ERR_INVALID, "removed slot 4 is listed twice");
    c.remove = {4, 2}; expect(c, MS_ERR_INVALID, "removed slot 2 is empty");
    c.remove = {4, 5}; expect(c, MS_ERR_INVALID, "removed slot 5 outside [0, 5)");
    c = Call(); c.kf_id[4] = 3; expect(c, MS_ERR_INVALID, "kf_id 3 is listed twice");
    c = Call(); c.args.cloud_slot = 2; expect(c, MS_ERR_INVALID, "cloud slot 2 is empty");
    c = Call(); c.args.cloud_slot = 5; expect(c, MS_ERR_INVALID, "cloud slot 5 outside [-1, 5)");
    c = Call(); c.args.n_kp = 9; expect(c, MS_ERR_INVALID, "9 keypoints in a table of stride 8");
    c = Call(); c.has_live = false; expect(c, MS_ERR_INVALID, "mp_live == NULL with 2 removed slots");
    c = Call(); c.has_live = false; c.n_remove = 0; expect(c, MS_OK, "");
    c = Call(); c.stride = 0; expect(c, MS_ERR_INVALID, "stride 0");
    c = Call(); c.n_mp = MS_COVIS_MAX_MP; expect(c, MS_ERR_CAPACITY, "caps");
    c = Call(); c.n_kf = MS_COVIS_MAX_QUERIES + 1; c.kf_id.resize(c.n_kf); c.remove.resize(c.n_kf);
    for (int k = 0; k < c.n_kf; ++k) c.kf_id[k] = c.remove[k] = k;
    c.n_remove = c.n_kf; expect(c, MS_ERR_CAPACITY, "4097 removed slots");
    c.n_remove = MS_COVIS_MAX_QUERIES; expect(c, MS_OK, "");
    { Call s; char tiny[8]; s.stride = 0;                    // a short buffer is not overrun, a missing one is not written
      if (ms_frame_finish_validate(s.kf_mp.data(), 5, 0, s.bytes.data(), s.bytes.data(), s.pos.data(), nullptr, nullptr, 10, s.kf_id.data(), s.remove.data(), 2, &s.args, nullptr, nullptr,
                                   nullptr, nullptr, s.out.data(), 16, s.out.data(), tiny, sizeof tiny) != MS_ERR_INVALID || std::strlen(tiny) != 7) ++fails;
      if (ms_frame_finish_validate(s.kf_mp.data(), 5, 0, s.bytes.data(), s.bytes.data(), s.pos.data(), nullptr, nullptr, 10, s.kf_id.data(), s.remove.data(), 2, &s.args, nullptr, nullptr,
                                   nullptr, nullptr, s.out.data(), 16, s.out.data(), nullptr, 0) != MS_ERR_INVALID) ++fails; }
    std::printf("frame finish validate alone: %d failures\n", fails);
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
