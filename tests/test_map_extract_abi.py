"""CPU checks of the surface of ms_map_extract: the header declares the call, its two structs and its validation twin, the library
exports them, Python binds them with the header's struct layouts, and ms_map_extract_validate, the host-only half that runs in front of any
device call, accepts the valid cases, turns every MS_ERR_INVALID case away with its message and holds every cap -- through the library, and
again in a program of its own compiled with map_checks.cpp alone under ASan and UBSan.  The validation dereferences HOST arguments only, so
host arrays stand in for the device tables."""
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
MAX_KF, MAX_STRIDE, MAX_MP, MAX_TRACKS = 65536, 8192, 1 << 24, 1 << 24


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
    return [f.strip().lstrip("*") for d in m.group(1).split(";") if d.split() for f in d.split(None, 2 if d.split()[0] == "const" else 1)[-1].split(",")]


def test_library_exports_the_calls_and_python_binds_them():
    for name in ("ms_map_extract", "ms_map_extract_validate"):
        assert hasattr(mi355slam.lib(), name), name
    for name in ("map_extract", "map_extract_device"):
        assert callable(getattr(mi355slam.KeyframeTable, name)), name
    assert callable(mi355slam.map_extract_validate)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmap_extract\.hip\b", mk, flags=re.M) and not re.search(r"^map_extract\.o\s*:", mk, flags=re.M)      # no per-object flags
    src = open(os.path.join(CSRC, "map_extract.hip")).read()
    assert '#include "ms_scan.h"' in src and "block_rank<kBlock>" in src and "block_offsets<kBlock>" in src and "MS_WS_MAP_EXTRACT" in src and "ms_pinned(" in src
    assert "MS_WS_MAP_EXTRACT" in open(os.path.join(CSRC, "ms_internal.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "__shfl" not in code and "__ballot" in code       # no scan of its own: the ranks and offsets are ms_scan.h's
    assert set(re.findall(r"\batomic\w*", code)) == {"atomicAdd"} and not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", code)      # integer adds only
    body = code.split('extern "C" int ms_map_extract(')[1]
    # the call count DESIGN 9.21 states: nine launches, one upload, one download, one wait behind it; nothing between the launches
    assert body.count("hipLaunchKernelGGL(") == 9 and body.count("hipMemcpyHostToDevice") == 1 and body.count("hipMemcpyDeviceToHost") == 1
    assert body.count("hipStreamSynchronize") == 1 and body.index("hipStreamSynchronize") > body.rindex("hipLaunchKernelGGL(")
    assert "NINE launches" in header(True) and "NINE launches" in src


def test_the_header_declares_the_structs_the_binding_uses_and_the_twin_takes_the_arguments_of_the_call():
    assert "DESIGN 9.21" in header(True)
    for name, cls in (("ms_map_extract_src", mi355slam.MapExtractSrcC), ("ms_map_extract_dst", mi355slam.MapExtractDstC)):
        assert struct_fields(name) == [k for k, _ in cls._fields_], name
    assert C.sizeof(mi355slam.MapExtractSrcC) == 16 * 8 + 6 * 4 and C.sizeof(mi355slam.MapExtractDstC) == 19 * 8 + 3 * 4 + 4
    call, twin = declaration("ms_map_extract"), declaration("ms_map_extract_validate")
    assert call[0] == "ms_ctx *ctx" and call[1:] == twin[:-2] and twin[-2:] == ["char *why", "size_t why_bytes"]
    assert [p.split("*")[-1].split()[-1] for p in call[1:]] == ["src", "dst", "kf_id", "active", "n_active", "desc_base", "n_kp", "dst_desc_base", "counts"]
    # the set of ms_*_check twins stays as tests/test_map_checks_corpus.py records it; the line above the twin says why it is named otherwise
    assert "ms_map_extract_check" not in header(True) and re.search(r"/\*[^\n]*_validate[^\n]*22[^\n]*\*/\s*int ms_map_extract_validate", header(True))
    checks = open(os.path.join(CSRC, "map_checks.cpp")).read()
    unit = open(os.path.join(CSRC, "map_extract.hip")).read()
    assert 'extern "C" int ms_map_extract_validate(' in checks and 'int ms_map_extract_validate(' not in unit and unit.count("ms_map_extract_validate(") == 1      # called once, defined elsewhere


SIZES = dict(n_kf=5, stride=8, n_mp=10, track_base=100, n_track=6, pool_size=40, n_kf_dst=4, n_mp_dst=10, pool_size_dst=24)


class Call:
    """One call of ms_map_extract_validate: 5 slots x 8 on 10 map points, slot 2 is empty, slots 4, 1, 3 are active (slot 3 without descriptors);
    every optional array is there."""

    def __init__(self):
        self.sizes = dict(SIZES)
        z = dict(SIZES, n_kf=5)
        arr = lambda k, dst: np.zeros(max(int(np.prod(mi355slam.map_extract_shape(k, z, dst))), 4), mi355slam.MAP_EXTRACT_FIELDS[k][0])
        self.src = {k: arr(k, False) for k in mi355slam.MAP_EXTRACT_SRC}
        self.dst = {k: arr(k, True) for k in mi355slam.MAP_EXTRACT_DST}
        self.kf_id, self.active = np.array([7, 3, -1, 9, 12], np.int32), np.array([4, 1, 3], np.int32)
        self.desc_base, self.n_kp = np.array([0, 8, 16, -1, 32], np.int32), np.array([8, 8, 5], np.int32)
        self.n_active, self.dst_desc_base, self.counts = None, True, True

    def run(self):
        return mi355slam.map_extract_validate(self.src, self.dst, self.sizes, self.kf_id, self.active, self.n_active, self.desc_base, self.n_kp, self.dst_desc_base, self.counts)


def changed(src=None, dst=None, same=(), **kw):
    """A Call with src / dst arrays replaced (None: taken away), dst arrays made the source's (same), sizes or members changed."""
    c = Call()
    c.src.update(src or {})
    c.dst.update(dst or {})
    for k in same:
        c.dst[k] = c.src[k]
    for k, v in kw.items():
        if k in c.sizes:
            c.sizes[k] = v
        else:
            setattr(c, k, v)
    return c


def i32(*v):
    return np.array(v, np.int32)


def none(*names):
    return {k: None for k in names}


KP = ("kp_x", "kp_y", "kp_octave", "kp_depth")


def test_valid_calls_and_the_zero_sizes_pass():
    assert Call().run() == (0, "")
    assert changed(src=none("mp_live")).run() == (0, "")                                                 # every row live
    assert changed(dst=none("n_obs", "row_src", "row_dst")).run() == (0, "")                              # each may be NULL
    for names in (("track_row",), ("track_row", "mp_track"), KP, ("kf_pose",)):
        assert changed(src=none(*names), dst=none(*names)).run() == (0, ""), names
    assert changed(src=none("desc_pool"), dst=none("desc_pool"), desc_base=None, n_kp=None).run() == (0, "")
    assert changed(active=i32(), n_kf_dst=0, dst=none("kf_mp")).run() == (0, "")                          # no active slots, no destination slots
    assert changed(active=None, n_active=0, dst_desc_base=False).run() == (0, "")
    assert changed(active=i32(3, 1, 4), n_kp=i32(5, 8, 8)).run() == (0, "")                               # any order
    assert changed(n_mp=0, src=none("mp_flags", "mp_pos", "mp_norm", "mp_min_dist", "mp_max_dist", "mp_desc")).run() == (0, "")
    assert changed(n_mp_dst=0, dst=none("mp_flags", "mp_live", "mp_pos", "mp_norm", "mp_min_dist", "mp_max_dist", "mp_desc")).run() == (0, "")      # the call then reports what it needs
    assert changed(pool_size_dst=16).run() == (0, "")                                                    # exactly the two slices


INVALID_CASES = [
    (dict(src=False), "missing array (src, dst or counts)"), (dict(dst=False), "missing array (src, dst or counts)"), (dict(counts=False), "missing array (src, dst or counts)"),
    (dict(n_active=-1), "negative size (-1 active slots"), (dict(n_track=-1), "negative size"), (dict(pool_size=-1), "negative size"), (dict(n_kf_dst=-1), "negative size"),
    (dict(n_mp_dst=-1), "negative size"), (dict(pool_size_dst=-1), "negative size"), (dict(n_kf=-1), "negative size"), (dict(n_mp=-1), "negative size"),
    (dict(stride=0), "stride 0"), (dict(src=none("kf_mp")), "missing array (kf_mp or kf_id)"), (dict(kf_id=None), "missing array (kf_mp or kf_id)"),
    (dict(kf_id=i32(7, 3, -1, 9, 7)), "kf_id 7 is listed twice"),
    (dict(src=none("mp_desc")), "missing array (a source map-point array)"), (dict(src=none("mp_pos")), "missing array (a source map-point array)"),
    (dict(dst=none("mp_live")), "missing array (a destination map-point array)"), (dict(dst=none("mp_norm")), "missing array (a destination map-point array)"),
    (dict(dst=none("kf_mp")), "missing array (the destination's kf_mp)"),
    (dict(active=None, n_active=3), "missing array (active or dst_desc_base)"), (dict(dst_desc_base=False), "missing array (active or dst_desc_base)"),
    (dict(src=none("mp_track"), dst=none("mp_track")), "track_row without mp_track"),
    (dict(src=none("kp_y")), "3 of the four keypoint arrays of the source"), (dict(dst=none("kp_x", "kp_depth")), "2 of the four keypoint arrays of the destination"),
    (dict(src=none(*KP)), "the keypoint arrays are given for the destination only"), (dict(dst=none(*KP)), "the keypoint arrays are given for the source only"),
    (dict(dst=none("mp_track")), "mp_track is given for the source only"), (dict(src=none("kf_pose")), "kf_pose is given for the destination only"),
    (dict(dst=none("track_row")), "track_row is given for the source only"), (dict(src=none("desc_pool")), "desc_pool is given for the destination only"),
    (dict(same=("kf_mp",)), "the destination's kf_mp is the source's"), (dict(same=("mp_pos",)), "the destination's mp_pos is the source's"),
    (dict(same=("track_row",)), "the destination's track_row is the source's"), (dict(same=("desc_pool",)), "the destination's desc_pool is the source's"),
    (dict(n_kf_dst=2), "3 active slots for a destination of 2 slots"),
    (dict(active=i32(4, 5, 3)), "active slot 5 outside [0, 5)"), (dict(active=i32(-1, 1, 3)), "active slot -1 outside [0, 5)"),
    (dict(active=i32(4, 1, 4)), "active slot 4 is listed twice"), (dict(active=i32(4, 2, 3)), "active slot 2 is empty (kf_id -1)"),
    (dict(desc_base=None), "missing array (desc_base or n_kp with a pool)"), (dict(n_kp=None), "missing array (desc_base or n_kp with a pool)"),
    (dict(n_kp=i32(8, 9, 5)), "active slot 1: 9 keypoints in a table of stride 8"), (dict(n_kp=i32(8, 8, -1)), "active slot 3: -1 keypoints"),
    (dict(pool_size=39), "active slot 4: descriptors [32, 32 + 8) outside the pool of 39"), (dict(pool_size_dst=15), "16 descriptors for a destination pool of 15"),
]


@pytest.mark.parametrize("kw, message", INVALID_CASES, ids=["%02d %s" % (i, m) for i, (_, m) in enumerate(INVALID_CASES)])
def test_every_invalid_call_is_turned_away_with_its_message(kw, message):
    kw = dict(kw)
    no_src, no_dst = kw.get("src") is False, kw.get("dst") is False
    c = changed(**{k: v for k, v in kw.items() if v is not False or k not in ("src", "dst")})
    if no_src:
        c.src = None
    if no_dst:
        c.dst = None
    rc, why = c.run()
    assert rc == INVALID and why.startswith("map extract: ") and message in why, (kw, rc, why)


def test_misaligned_descriptor_arrays_are_turned_away():
    for side, k in (("src", "mp_desc"), ("dst", "mp_desc"), ("src", "desc_pool"), ("dst", "desc_pool")):
        c = Call()
        a = getattr(c, side)[k]
        big = np.zeros(a.size + 8, np.uint32)
        off = next(o for o in range(1, 5) if (big.ctypes.data + 4 * o) % 16)
        getattr(c, side)[k] = big[off:off + a.size]
        rc, why = c.run()
        assert rc == INVALID and "descriptor arrays must be 16-byte aligned" in why, (side, k, why)


def test_every_cap_holds_at_its_limit_and_one_beyond():
    ids = lambda n: np.arange(n, dtype=np.int32)
    for kw, text in ((dict(n_kf=MAX_KF + 1, kf_id=ids(MAX_KF + 1)), "65537 slots"), (dict(stride=MAX_STRIDE + 1), "stride 8193"), (dict(n_mp=MAX_MP), "16777216 map points"),
                     (dict(n_kf_dst=MAX_KF + 1), "destination: 65537 slots"), (dict(n_mp_dst=MAX_MP), "destination: 4 slots / stride 8 / 16777216 map points"),
                     (dict(n_track=MAX_TRACKS + 1), "a track window of 16777217, cap 16777216")):
        rc, why = changed(**kw).run()
        assert rc == CAPACITY and text in why and "cap" in why, (text, rc, why)
    big = np.full(MAX_KF, -1, np.int32)
    big[:5] = [0, 8, 16, -1, 32]
    for kw in (dict(n_kf=MAX_KF, kf_id=ids(MAX_KF), desc_base=big), dict(stride=MAX_STRIDE), dict(n_mp=MAX_MP - 1), dict(n_kf_dst=MAX_KF), dict(n_mp_dst=MAX_MP - 1),
               dict(n_track=MAX_TRACKS)):
        assert changed(**kw).run() == (0, ""), list(kw)


PROGRAM = r"""
#include "mi355slam.h"
#include <cstdio>
#include <cstring>
#include <vector>
struct Call {
    std::vector<double> mem = std::vector<double>(64, 0.0), mem2 = std::vector<double>(64, 0.0);      // 16-byte aligned stand-ins for the device arrays of either side
    std::vector<int32_t> kf_id = {7, 3, -1, 9, 12}, active = {4, 1, 3}, desc_base = {0, 8, 16, -1, 32}, n_kp = {8, 8, 5}, out = std::vector<int32_t>(8, 0);
    ms_map_extract_src S;
    ms_map_extract_dst D;
    int n_active = 3;
    char why[128];
    template <class T> static T *as(std::vector<double> &v) { return reinterpret_cast<T *>(v.data()); }
    Call() {
        S = {as<int32_t>(mem), as<uint8_t>(mem), as<uint8_t>(mem), mem.data(), as<float>(mem), as<float>(mem), as<float>(mem), as<uint32_t>(mem), as<int32_t>(mem),
             as<float>(mem), as<float>(mem), as<int32_t>(mem), as<float>(mem), mem.data(), as<int32_t>(mem), as<uint32_t>(mem), 5, 8, 10, 100, 6, 40};
        D = {as<int32_t>(mem2), as<uint8_t>(mem2), as<uint8_t>(mem2), mem2.data(), as<float>(mem2), as<float>(mem2), as<float>(mem2), as<uint32_t>(mem2), as<int32_t>(mem2),
             as<float>(mem2), as<float>(mem2), as<int32_t>(mem2), as<float>(mem2), mem2.data(), as<int32_t>(mem2), as<uint32_t>(mem2), nullptr, nullptr, nullptr, 4, 10, 24};
    }
    int run() {
        why[0] = 0;
        return ms_map_extract_validate(&S, &D, kf_id.data(), active.data(), n_active, desc_base.data(), n_kp.data(), out.data(), out.data(), why, sizeof why);
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
    c.active = {4, 4, 3}; expect(c, MS_ERR_INVALID, "active slot 4 is listed twice");
    c.active = {4, 2, 3}; expect(c, MS_ERR_INVALID, "active slot 2 is empty");
    c.active = {4, 5, 3}; expect(c, MS_ERR_INVALID, "active slot 5 outside [0, 5)");
    c = Call(); c.kf_id[4] = 3; expect(c, MS_ERR_INVALID, "kf_id 3 is listed twice");
    c = Call(); c.D.n_kf = 2; expect(c, MS_ERR_INVALID, "3 active slots for a destination of 2 slots");
    c = Call(); c.n_kp[1] = 9; expect(c, MS_ERR_INVALID, "9 keypoints in a table of stride 8");
    c = Call(); c.S.pool_size = 39; expect(c, MS_ERR_INVALID, "outside the pool of 39");
    c = Call(); c.D.pool_size = 15; expect(c, MS_ERR_INVALID, "16 descriptors for a destination pool of 15");
    c = Call(); c.S.mp_track = nullptr; c.D.mp_track = nullptr; expect(c, MS_ERR_INVALID, "track_row without mp_track");
    c = Call(); c.S.kp_y = nullptr; expect(c, MS_ERR_INVALID, "3 of the four keypoint arrays of the source");
    c = Call(); c.D.kf_pose = nullptr; expect(c, MS_ERR_INVALID, "kf_pose is given for the source only");
    c = Call(); c.D.mp_pos = c.mem.data(); expect(c, MS_ERR_INVALID, "the destination's mp_pos is the source's");
    c = Call(); c.S.desc_pool = reinterpret_cast<const uint32_t *>(c.mem.data()) + 1; expect(c, MS_ERR_INVALID, "16-byte aligned");
    c = Call(); c.S.stride = 0; expect(c, MS_ERR_INVALID, "stride 0");
    c = Call(); c.S.mp_live = nullptr; expect(c, MS_OK, "");
    c = Call(); c.n_active = 0; expect(c, MS_OK, "");
    c = Call(); c.S.n_mp = MS_COVIS_MAX_MP; expect(c, MS_ERR_CAPACITY, "caps");
    c = Call(); c.D.n_mp = MS_COVIS_MAX_MP; expect(c, MS_ERR_CAPACITY, "destination");
    c = Call(); c.S.n_track = MS_TRACKED_MAX_WINDOW + 1; expect(c, MS_ERR_CAPACITY, "a track window of");
    c = Call(); c.S.n_kf = MS_COVIS_MAX_KF; c.kf_id.resize(c.S.n_kf); c.desc_base.assign(c.S.n_kf, -1); c.active.resize(c.S.n_kf); c.n_kp.assign(c.S.n_kf, 8);
    for (int k = 0; k < c.S.n_kf; ++k) c.kf_id[k] = c.active[k] = k;
    c.out.resize(c.S.n_kf); c.n_active = c.S.n_kf; c.D.n_kf = c.S.n_kf; expect(c, MS_OK, "");      // the full copy of the largest table
    c.S.n_kf += 1; c.kf_id.push_back(70000); expect(c, MS_ERR_CAPACITY, "65537 slots");
    { Call s; char tiny[8]; s.S.stride = 0;                  // a short buffer is not overrun, a missing one is not written
      if (ms_map_extract_validate(&s.S, &s.D, s.kf_id.data(), s.active.data(), 3, s.desc_base.data(), s.n_kp.data(), s.out.data(), s.out.data(), tiny, sizeof tiny) != MS_ERR_INVALID ||
          std::strlen(tiny) != 7) ++fails;
      if (ms_map_extract_validate(&s.S, &s.D, s.kf_id.data(), s.active.data(), 3, s.desc_base.data(), s.n_kp.data(), s.out.data(), s.out.data(), nullptr, 0) != MS_ERR_INVALID) ++fails;
      if (ms_map_extract_validate(nullptr, &s.D, s.kf_id.data(), s.active.data(), 3, s.desc_base.data(), s.n_kp.data(), s.out.data(), s.out.data(), nullptr, 0) != MS_ERR_INVALID) ++fails; }
    std::printf("map extract validate alone: %d failures\n", fails);
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
