"""CPU checks of the surface of the loop closer's pieces on the map tables: the header declares the calls, the library exports them,
Python binds them, and the host-only halves that run in front of any device call -- ms_loop_usable_mask_check, ms_loop_pairs_check and
ms_loop_sim3_lists_check -- turn every MS_ERR_INVALID case away with its message, hold every cap and accept the zero sizes.  The checks
dereference HOST arguments only, so host arrays stand in for the device tables."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import mi355slam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ms_loop_usable_mask", "ms_loop_pairs", "ms_loop_sim3_lists")
INVALID, CAPACITY = mi355slam.MS_ERR_INVALID, mi355slam.MS_ERR_CAPACITY
MAX_KF, MAX_STRIDE, MAX_MP, MAX_QUERIES, MAX_CAND, MAX_LEVELS = 65536, 8192, 1 << 24, 4096, 4096, 32
PAIR_OUT = ("pair_start", "kp1", "kp2", "row1", "row2", "pts1", "pts2", "thr1", "thr2", "cur_pose", "cand_pose", "n_pairs")
SIM3_OUT = ("pts1", "pts2", "obs1", "obs2", "info1", "info2", "row1", "row2")


def test_library_exports_the_calls_and_python_binds_them():
    for name in CALLS:
        assert hasattr(mi355slam.lib(), name) and hasattr(mi355slam.lib(), name + "_check"), name
    for name in ("loop_usable_mask", "loop_pairs", "loop_sim3_lists"):
        assert callable(getattr(mi355slam.KeyframeTable, name)), name
    assert {"mp_flags", "mp_live", "slots", "n_kp", "require_triangulated", "usable", "tri_row"} <= set(mi355slam.LoopMaskArgs.FIELDS)
    assert {"mp_pos", "kf_pose", "kp_octave", "cur", "cand_slot", "n_kp_cand", "matched", "level_sigma_sq", "cap_pairs"} <= set(mi355slam.LoopPairsArgs.FIELDS)
    assert {"kp_x", "kp_y", "cams", "kp1", "kp2", "match_start"} <= set(mi355slam.LoopSim3ListsArgs.FIELDS)
    assert [k for k, _, _ in mi355slam.LOOP_PAIRS_OUT] == list(PAIR_OUT[1:9]) and [k for k, _, _ in mi355slam.LOOP_SIM3_OUT] == list(SIM3_OUT)
    try:
        mi355slam.LoopPairsArgs(no_such_field=1)
    except TypeError as e:
        assert "no_such_field" in str(e)
    else:
        raise AssertionError("an unknown field passed")
    mk = open(os.path.join(ROOT, "slam-module_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bloop_chain\.hip\b", mk, flags=re.M)
    assert not re.search(r"^loop_chain\.o\s*:.*FLAGS", mk, flags=re.M)                           # the default -ffp-contract=off
    src = open(os.path.join(ROOT, "slam-module_amd", "csrc", "loop_chain.hip")).read()
    assert '#include "ms_scan.h"' in src and "block_rank<kBlock>" in src and "block_offsets<kBlock>" in src and "MS_WS_LOOP_CHAIN" in src and "ms_pinned(" in src
    internal = open(os.path.join(ROOT, "slam-module_amd", "csrc", "ms_internal.h")).read()
    checks = open(os.path.join(ROOT, "slam-module_amd", "csrc", "map_checks.cpp")).read()
    assert '#include "ms_internal.h"' in src and '#include "ms_check.h"' in internal and '#include "ms_check.h"' in checks     # the validation is one host-only unit
    for name in CALLS:
        assert 'extern "C" int %s_check(' % name not in src and 'extern "C" int %s_check(' % name in checks, name
    assert "MS_WS_LOOP_CHAIN" in open(os.path.join(ROOT, "slam-module_amd", "csrc", "ms_internal.h")).read()


def test_the_check_twins_take_the_arguments_of_the_calls():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355slam.h")).read(), flags=re.S)
    assert "DESIGN 9.16" in open(os.path.join(ROOT, "include", "mi355slam.h")).read()

    def declaration(name):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        return [" ".join(p.split()).replace("const ", "") for p in m.group(1).split(",")]

    for name in CALLS:
        call, check = declaration(name), declaration(name + "_check")
        assert call[0] == "ms_ctx *ctx" and call[1:] == check[:-2] and check[-2:] == ["char *why", "size_t why_bytes"], name


def test_caps_match_the_header(tmp_path):
    src, exe = tmp_path / "caps.c", tmp_path / "caps"
    src.write_text('#include <stdio.h>\n#include "mi355slam.h"\nint main(void) { printf("%d %d %d %d %d %d\\n", MS_COVIS_MAX_KF, MS_COVIS_MAX_STRIDE, MS_COVIS_MAX_MP, '
                   "MS_COVIS_MAX_QUERIES, MS_LOOP_MAX_CANDIDATES, MS_TRI_MAX_LEVELS); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == [MAX_KF, MAX_STRIDE, MAX_MP, MAX_QUERIES, MAX_CAND, MAX_LEVELS]


def test_the_check_header_compiles_alone_and_clean_under_sanitizers(tmp_path):
    """map_checks.cpp is plain C++: a program with its own main links the three checks and runs under ASan and UBSan."""
    src, exe = tmp_path / "alone.cpp", tmp_path / "alone"
    src.write_text('#include "mi355slam.h"\n#include <cstring>\nint main() {\n'
                   "  char why[64]; int32_t kf_mp[8] = {0}, slots[2] = {1, 0}, n_kp[2] = {4, 0}, req[2] = {1, 0}, row[4]; uint8_t flags[3] = {0}, mask[4];\n"
                   "  uint8_t *usable[2] = {mask, nullptr}; int32_t *tri[2] = {row, nullptr};\n"
                   "  if (ms_loop_usable_mask_check(kf_mp, 2, 4, flags, nullptr, 3, slots, n_kp, req, usable, tri, 2, why, sizeof why)) return 1;\n"
                   "  slots[1] = 2;\n"
                   "  if (ms_loop_usable_mask_check(kf_mp, 2, 4, flags, nullptr, 3, slots, n_kp, req, usable, tri, 2, why, sizeof why) != MS_ERR_INVALID) return 2;\n"
                   '  return std::strncmp(why, "loop mask: slot 2", 17) ? 3 : 0;\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "include"), str(src), os.path.join(ROOT, "slam-module_amd", "csrc", "map_checks.cpp"), "-o", str(exe)])
    subprocess.check_call([str(exe)])


class Call:
    """One call of each check: 5 slots x 8, 10 map points, 3 levels; the current keyframe in slot 1 with 6 keypoints; candidates in slots 3, 0
    and 4 with 8, 0 and 5 keypoints; match lists of 2, 0 and 3 entries."""

    def __init__(self):
        self.n_kf, self.stride, self.n_mp, self.n_levels, self.cur, self.n_kp_cur, self.cap_pairs = 5, 8, 10, 3, 1, 6, 18
        a = lambda n, dt: np.zeros(max(n, 1), dt)
        self.arrays = dict(kf_mp=np.full(40, -1, np.int32), mp_flags=a(10, np.uint8), mp_live=a(10, np.uint8), mp_pos=a(30, np.float64), kf_pose=a(60, np.float64),
                           kp_x=a(40, np.float32), kp_y=a(40, np.float32), kp_octave=a(40, np.int32),
                           slots=np.array([1, 3, 0], np.int32), n_kp=np.array([6, 8, 0], np.int32), require_triangulated=np.array([0, 1, 1], np.int32),
                           cand_slot=np.array([3, 0, 4], np.int32), n_kp_cand=np.array([8, 0, 5], np.int32), level_sigma_sq=np.array([1, 1.44, 2.0736], np.float32),
                           kp1=np.array([0, 5, 1, 2, 3], np.int32), kp2=np.array([7, 0, 4, 0, 1], np.int32), match_start=np.array([0, 2, 2, 5], np.int32),
                           cams=np.array([[500.0, 510.0, 320.0, 240.0]] * 5))
        self.arrays.update({"p_" + k: a(64, np.float64) for k in PAIR_OUT})
        self.arrays.update({"s_" + k: a(64, np.float64) for k in SIM3_OUT})
        self.masks = [a(8, np.uint8) for _ in range(3)]
        self.rows = [a(8, np.int32) for _ in range(3)]
        self.matched = [a(8, np.int32) for _ in range(3)]
        self.no_tri_row = False

    def ptr(self, name):
        v = self.arrays.get(name)
        return C.c_void_p(0) if v is None else C.c_void_p(v.ctypes.data)

    def ptrs(self, arrays, n):
        if arrays is None:
            return None
        return (C.c_void_p * max(n, 1))(*[None if m is None else m.ctypes.data for m in arrays[:max(n, 0)]])

    def cam_structs(self):
        if self.arrays["cams"] is None:
            return None
        k = np.zeros(max(self.n_kf, 1), dtype=[("fx", "f8"), ("fy", "f8"), ("cx", "f8"), ("cy", "f8"), ("w", "i4"), ("h", "i4")])
        k[:] = (500.0, 510.0, 320.0, 240.0, 640, 480)
        for s, c in enumerate(self.arrays["cams"][:len(k)]):
            k[s] = (c[0], c[1], c[2], c[3], 640, 480)
        self.cam_block = k                                   # ms_pinhole per slot; slots beyond the five of the call get the default camera
        return C.c_void_p(k.ctypes.data)

    def mask(self, why_bytes=512):
        p, why = self.ptr, C.create_string_buffer(512)
        n = self.n_slots if "n_slots" in self.__dict__ else 3
        rc = mi355slam.lib().ms_loop_usable_mask_check(p("kf_mp"), self.n_kf, self.stride, p("mp_flags"), p("mp_live"), self.n_mp, p("slots"), p("n_kp"),
                                                       p("require_triangulated"), self.ptrs(self.masks, n), None if self.no_tri_row else self.ptrs(self.rows, n), n,
                                                       why if why_bytes else None, C.c_size_t(why_bytes))
        return rc, why.value.decode()

    def n_cand(self):
        return self.n_cand_ if "n_cand_" in self.__dict__ else 3 if self.arrays["cand_slot"] is None else len(self.arrays["cand_slot"])

    def pairs(self):
        p, why = self.ptr, C.create_string_buffer(512)
        n = self.n_cand()
        rc = mi355slam.lib().ms_loop_pairs_check(p("kf_mp"), self.n_kf, self.stride, p("mp_live"), p("mp_pos"), self.n_mp, p("kf_pose"), p("kp_octave"), self.cur,
                                                 self.n_kp_cur, p("cand_slot"), p("n_kp_cand"), self.ptrs(self.matched, n), n, p("level_sigma_sq"), self.n_levels,
                                                 self.cap_pairs, *[p("p_" + k) for k in PAIR_OUT], why, C.c_size_t(512))
        return rc, why.value.decode()

    def sim3(self):
        p, why = self.ptr, C.create_string_buffer(512)
        n = self.n_cand()
        rc = mi355slam.lib().ms_loop_sim3_lists_check(p("kf_mp"), self.n_kf, self.stride, p("mp_live"), p("mp_pos"), self.n_mp, p("kf_pose"), p("kp_x"), p("kp_y"),
                                                      p("kp_octave"), self.cur, self.n_kp_cur, p("cand_slot"), p("n_kp_cand"), n, self.cam_structs(), p("level_sigma_sq"),
                                                      self.n_levels, p("kp1"), p("kp2"), p("match_start"), *[p("s_" + k) for k in SIM3_OUT], why, C.c_size_t(512))
        return rc, why.value.decode()


def changed(**kw):
    c = Call()
    for k, v in kw.items():
        if k in c.arrays:
            c.arrays[k] = v
        elif k in ("n_slots", "n_cand_"):
            setattr(c, k, v)
        else:
            assert hasattr(c, k), k
            setattr(c, k, v)
    return c


def i32(*v):
    return np.array(v, np.int32)


def f32(*v):
    return np.array(v, np.float32)


def test_valid_calls_and_the_zero_sizes_pass():
    assert Call().mask() == (0, "") and Call().pairs() == (0, "") and Call().sim3() == (0, "")
    assert changed(no_tri_row=True).mask() == (0, "") and changed(rows=[None, None, None]).mask() == (0, "")
    assert changed(mp_live=None).mask() == (0, "") and changed(mp_live=None).pairs() == (0, "") and changed(mp_live=None).sim3() == (0, "")
    assert changed(mp_flags=None, no_tri_row=True, require_triangulated=i32(0, 0, 0)).mask() == (0, "")        # nothing asks for the flags
    assert changed(n_slots=0, slots=None, n_kp=None, require_triangulated=None, masks=None, rows=None).mask() == (0, "")
    assert changed(masks=[np.zeros(8, np.uint8), np.zeros(8, np.uint8), None]).mask() == (0, "")               # a slot without keypoints needs no mask
    assert changed(n_mp=0, mp_pos=None).pairs() == (0, "") and changed(n_mp=0, mp_pos=None).sim3() == (0, "")
    assert changed(n_cand_=0, cand_slot=None, n_kp_cand=None, matched=None, p_cand_pose=None).pairs() == (0, "")
    assert changed(n_kp_cur=0, matched=[None, None, None]).pairs() == (0, "")
    assert changed(cap_pairs=0, **{"p_" + k: None for k in PAIR_OUT[1:9]}).pairs() == (0, "")
    assert changed(n_cand_=0, cand_slot=None, n_kp_cand=None, match_start=i32(0), kp1=None, kp2=None, **{"s_" + k: None for k in SIM3_OUT}).sim3() == (0, "")
    assert changed(match_start=i32(0, 0, 0, 0), kp1=None, kp2=None, **{"s_" + k: None for k in SIM3_OUT}).sim3() == (0, "")
    assert changed(n_kp_cur=8).pairs() == (0, "") and changed(n_kp_cand=i32(8, 8, 8)).sim3() == (0, "")        # keypoint counts at the stride


def test_every_invalid_mask_call_is_turned_away_with_its_message():
    cases = [(dict(n_kf=-1), "negative size"), (dict(n_mp=-1), "negative size"), (dict(n_slots=-1), "negative size"), (dict(stride=0), "stride 0"),
             (dict(kf_mp=None), "missing array"), (dict(slots=None), "missing array"), (dict(n_kp=None), "missing array"), (dict(require_triangulated=None), "missing array"),
             (dict(masks=None), "missing array"), (dict(masks=[np.zeros(8, np.uint8), None, None]), "missing array (usable of slot 3)"),
             (dict(slots=i32(1, 5, 0)), "slot 5 outside [0, 5)"), (dict(slots=i32(-1, 3, 0)), "slot -1 outside [0, 5)"),
             (dict(n_kp=i32(6, 9, 0)), "9 keypoints in a table of stride 8"), (dict(n_kp=i32(-1, 8, 0)), "-1 keypoints"),
             (dict(mp_flags=None), "mp_flags == NULL"), (dict(mp_flags=None, no_tri_row=True), "slot 3 requires TRIANGULATED"),
             (dict(mp_flags=None, require_triangulated=i32(0, 0, 0)), "slot 1 requires TRIANGULATED or asks for tri_row")]
    for kw, text in cases:
        rc, why = changed(**kw).mask()
        assert rc == INVALID and text in why and why.startswith("loop mask: "), (kw, rc, why)
    assert changed(stride=0).mask(why_bytes=0)[0] == INVALID                                                   # no buffer for the message


def both(c):
    return (("pairs", c.pairs()), ("sim3", c.sim3()))


def test_every_invalid_call_of_the_two_list_builders_is_turned_away_with_its_message():
    shared = [(dict(n_kf=-1), "negative size"), (dict(n_mp=-1), "negative size"), (dict(n_cand_=-1), "negative size"), (dict(stride=0), "stride 0"),
              (dict(kf_mp=None), "missing array"), (dict(kf_pose=None), "missing array"), (dict(kp_octave=None), "missing array"), (dict(mp_pos=None), "missing array"),
              (dict(cur=5), "slot 5 outside [0, 5)"), (dict(cur=-1), "slot -1 outside [0, 5)"), (dict(n_kp_cur=9), "9 keypoints in a table of stride 8"),
              (dict(n_kp_cur=-1), "-1 keypoints"), (dict(cand_slot=None), "missing array (cand_slot or n_kp_cand)"), (dict(n_kp_cand=None), "missing array (cand_slot or n_kp_cand)"),
              (dict(cand_slot=i32(3, 5, 4)), "slot 5 outside [0, 5)"), (dict(cand_slot=i32(3, -2, 4)), "slot -2 outside"),
              (dict(cand_slot=i32(3, 1, 4)), "the current keyframe's slot 1 is among the candidates"), (dict(cand_slot=i32(3, 0, 3)), "candidate slot 3 is listed twice"),
              (dict(n_kp_cand=i32(8, 9, 5)), "9 keypoints in a table of stride 8"), (dict(n_kp_cand=i32(8, -1, 5)), "-1 keypoints"),
              (dict(n_levels=0), "0 levels outside [1, 32]"), (dict(n_levels=MAX_LEVELS + 1), "33 levels outside [1, 32]"), (dict(level_sigma_sq=None), "missing array (level_sigma_sq)"),
              (dict(level_sigma_sq=f32(1, 0, 2)), "level_sigma_sq[1] = 0"), (dict(level_sigma_sq=f32(1, 2, -1)), "level_sigma_sq[2] = -1"),
              (dict(level_sigma_sq=f32(np.nan, 1, 2)), "level_sigma_sq[0] = nan"), (dict(level_sigma_sq=f32(1, np.inf, 2)), "level_sigma_sq[1] = inf")]
    for kw, text in shared:
        for which, (rc, why) in both(changed(**kw)):
            assert rc == INVALID and text in why and why.startswith("loop pairs: " if which == "pairs" else "loop sim3 lists: "), (which, kw, rc, why)
    pairs = [(dict(cap_pairs=-1), "negative size (capacity -1)"), (dict(matched=None), "missing array (matched)"),
             (dict(matched=[np.zeros(8, np.int32), None, np.zeros(8, np.int32)]), "missing array (matched of candidate slot 0)")]
    pairs += [(dict(**{"p_" + k: None}), "missing array (pair_start, n_pairs, cur_pose or cand_pose)") for k in ("pair_start", "n_pairs", "cur_pose", "cand_pose")]
    pairs += [(dict(**{"p_" + k: None}), "missing array (kp1, kp2, row1, row2, pts1, pts2, thr1 or thr2)") for k in PAIR_OUT[1:9]]
    for kw, text in pairs:
        rc, why = changed(**kw).pairs()
        assert rc == INVALID and text in why and why.startswith("loop pairs: "), (kw, rc, why)
    cams = lambda slot, col, v: np.array([[v if (s, c) == (slot, col) else x for c, x in enumerate((500.0, 510.0, 320.0, 240.0))] for s in range(5)])
    sim3 = [(dict(kp_x=None), "missing array"), (dict(kp_y=None), "missing array"), (dict(cams=None), "missing array"), (dict(match_start=None), "missing array (match_start)"),
            (dict(match_start=i32(1, 2, 2, 5)), "match_start[0] = 1"), (dict(match_start=i32(0, 2, 1, 5)), "match_start descends at candidate 1 (1 after 2)"),
            (dict(kp1=None), "missing array (kp1, kp2"), (dict(kp2=None), "missing array (kp1, kp2"),
            (dict(cams=cams(1, 0, 0.0)), "the camera of slot 1 has fx 0"), (dict(cams=cams(3, 1, -2.0)), "the camera of slot 3 has fx 500, fy -2"),
            (dict(cams=cams(4, 0, np.inf)), "the camera of slot 4 has fx inf"), (dict(cams=cams(0, 1, np.nan)), "the camera of slot 0 has fx 500, fy nan"),
            (dict(cams=cams(0, 2, np.nan)), "the camera of slot 0 has cx nan")]
    sim3 += [(dict(**{"s_" + k: None}), "missing array (kp1, kp2, pts1") for k in SIM3_OUT]
    for kw, text in sim3:
        rc, why = changed(**kw).sim3()
        assert rc == INVALID and text in why and why.startswith("loop sim3 lists: "), (kw, rc, why)
    assert changed(cams=cams(2, 0, -1.0)).sim3() == (0, "")                                                    # slot 2 is neither the current keyframe nor a candidate


def test_every_cap_holds_at_its_limit_and_one_beyond():
    big = [(dict(n_kf=MAX_KF + 1), "65537 slots"), (dict(stride=MAX_STRIDE + 1), "stride 8193"), (dict(n_mp=MAX_MP), "16777216 map points")]
    for kw, text in big:
        for rc, why in (changed(**kw).mask(), changed(**kw).pairs(), changed(**kw).sim3()):
            assert rc == CAPACITY and text in why, (kw, rc, why)
    for kw in (dict(n_kf=MAX_KF), dict(stride=MAX_STRIDE), dict(n_mp=MAX_MP - 1)):
        assert changed(**kw).mask() == (0, "") and changed(**kw).pairs() == (0, "") and changed(**kw).sim3() == (0, "")
    n = MAX_QUERIES + 1
    many = dict(n_kf=n, kf_mp=np.full(8 * n, -1, np.int32), slots=np.arange(n, dtype=np.int32), n_kp=np.zeros(n, np.int32), require_triangulated=np.zeros(n, np.int32),
                masks=[None] * n, rows=[None] * n, n_slots=n)
    rc, why = changed(**many).mask()
    assert rc == CAPACITY and "4097 listed" in why
    assert changed(**dict(many, n_slots=MAX_QUERIES)).mask() == (0, "")
    n = MAX_CAND + 1
    many = dict(n_kf=n + 1, cur=n, cand_slot=np.arange(n, dtype=np.int32), n_kp_cand=np.zeros(n, np.int32), matched=[np.zeros(8, np.int32)] * n,
                match_start=np.zeros(n + 1, np.int32), p_pair_start=np.zeros(n + 1, np.float64), p_cand_pose=np.zeros(12 * n))
    for rc, why in (changed(**many).pairs(), changed(**many).sim3()):
        assert rc == CAPACITY and "4097 listed" in why and "4096" in why, (rc, why)
    assert changed(**dict(many, n_cand_=MAX_CAND)).pairs() == (0, "") and changed(**dict(many, n_cand_=MAX_CAND)).sim3() == (0, "")
    rc, why = changed(match_start=i32(0, 9, 9, 9), kp1=np.zeros(9, np.int32), kp2=np.zeros(9, np.int32)).sim3()                # a list longer than the stride
    assert rc == CAPACITY and "9 matches for candidate slot 3, more than the stride of 8" in why
    assert changed(match_start=i32(0, 8, 8, 8), kp1=np.zeros(8, np.int32), kp2=np.zeros(8, np.int32)).sim3() == (0, "")
