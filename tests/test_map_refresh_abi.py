"""CPU checks of the surface of the map-point table's writers (ms_map_refresh, ms_loop_correct): the header declares them, the library exports
them, the Python bindings are there, the host mirror's DeviceKeyframePoses / DeviceMapPoints::refresh / correctLoop compile and link
(tests/map_refresh_smoke.cpp), and every MS_ERR_INVALID case is turned away by the host-only halves of the two calls, which run in front of
any device call."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "map_refresh_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "map_refresh_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_header_declares_the_writers():
    hdr = open(os.path.join(ROOT, "include", "mi355slam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("ms_map_refresh", "ms_map_refresh_check", "ms_loop_correct", "ms_loop_correct_check"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name


def test_library_exports_the_writers_and_python_binds_them():
    import mi355slam
    import map_refresh_ref
    for name in ("ms_map_refresh", "ms_map_refresh_check", "ms_loop_correct", "ms_loop_correct_check"):
        assert hasattr(mi355slam.lib(), name), name
    assert callable(mi355slam.map_refresh) and callable(mi355slam.loop_correct) and callable(mi355slam.KeyframePoseTable)
    assert np.array_equal(map_refresh_ref.scale_factors(8, 1.2), mi355slam.scale_factors(8, 1.2))
    assert map_refresh_ref.MEDOID_MAX_OBS == 256


def test_makefile_builds_the_new_source():
    mk = open(os.path.join(ROOT, "slam-module_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmap_refresh\.hip\b", mk, flags=re.M)


def test_mirror_links_and_every_invalid_case_is_rejected_without_a_device():
    out = subprocess.check_output([build_smoke(), "--no-gpu"], text=True)
    assert "link ok 1" in out
    m = re.search(r"no-gpu ok (\d+) refresh cases (\d+) loop cases", out)
    assert m, out
    assert int(m.group(1)) >= 20 and int(m.group(2)) >= 12
