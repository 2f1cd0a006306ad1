"""CPU checks of the surface of the culling step (ms_observation_count, ms_map_cull, ms_map_cull_check): the header declares them, the
library exports them, the Python bindings are there, the host mirror's DeviceMapPointLive / observationCounts / cullMap compile and link
(tests/map_cull_smoke.cpp), and every MS_ERR_INVALID case is turned away by the host-only half of ms_map_cull, which runs in front of any
device call."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "map_cull_smoke")
NAMES = ("ms_observation_count", "ms_map_cull", "ms_map_cull_check")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "map_cull_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_header_declares_the_culling_calls():
    hdr = open(os.path.join(ROOT, "include", "mi355slam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert re.search(r"}\s*ms_cull_settings\s*;", code)


def test_library_exports_the_culling_calls_and_python_binds_them():
    import mi355slam
    import map_cull_ref
    for name in NAMES:
        assert hasattr(mi355slam.lib(), name), name
    for method in ("observation_count", "cull", "cull_device"):
        assert callable(getattr(mi355slam.KeyframeTable, method)), method
    # the C layout of ms_cull_settings: int32, int32, double, int32, (4 bytes), double, int32, (4 bytes)
    S = mi355slam.CullSettingsC
    assert C.sizeof(S) == 40
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 16, 24, 32]
    assert [f for f, _ in S._fields_] == ["current_slot", "cull_points", "min_age", "min_obs_for_ba", "max_critical_ratio", "ratio_float32"]
    assert sorted(map_cull_ref.settings(0)) == sorted(f for f, _ in S._fields_)
    assert (map_cull_ref.EMPTY, map_cull_ref.AGED, map_cull_ref.ORPHANED) == (1, 2, 3)


def test_makefile_builds_the_new_source():
    mk = open(os.path.join(ROOT, "slam-module_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmap_cull\.hip\b", mk, flags=re.M)


def test_mirror_links_and_every_invalid_case_is_rejected_without_a_device():
    out = subprocess.check_output([build_smoke(), "--no-gpu"], text=True)
    assert "link ok 1" in out
    m = re.search(r"no-gpu ok (\d+) cull cases", out)
    assert m, out
    assert int(m.group(1)) >= 12
