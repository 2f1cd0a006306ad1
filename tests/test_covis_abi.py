"""CPU checks of the surface of the map-graph queries (ms_covisibility, ms_map_point_union): the header declares them, the library exports
them, the Python bindings are there, the host mirror's DeviceKeyframeMapPoints / getNeighbors / computeAdjacentKeyframes / localMapPoints
compile and link (tests/covis_smoke.cpp), and every MS_ERR_INVALID case is turned away by the host-only halves of the two calls, which run
in front of any device call."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "covis_smoke")
NAMES = ("ms_covisibility", "ms_covisibility_check", "ms_map_point_union", "ms_map_point_union_check")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "covis_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_header_declares_the_queries():
    hdr = open(os.path.join(ROOT, "include", "mi355slam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    for struct in ("ms_covis_query", "ms_union_problem"):
        assert re.search(r"}\s*%s\s*;" % struct, code), struct


def test_library_exports_the_queries_and_python_binds_them():
    import mi355slam
    import covis_ref
    for name in NAMES:
        assert hasattr(mi355slam.lib(), name), name
    for method in ("update", "covisibility", "map_point_union"):
        assert callable(getattr(mi355slam.KeyframeTable, method)), method
    assert C.sizeof(mi355slam.CovisQueryC) == 20 and C.sizeof(mi355slam.UnionProblemC) == 16      # the C layout of the two host structs
    assert covis_ref.NONE == -1


def test_makefile_builds_the_new_source():
    mk = open(os.path.join(ROOT, "slam-module_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bcovis\.hip\b", mk, flags=re.M)


def test_mirror_links_and_every_invalid_case_is_rejected_without_a_device():
    out = subprocess.check_output([build_smoke(), "--no-gpu"], text=True)
    assert "link ok 1" in out
    m = re.search(r"no-gpu ok (\d+) covis cases (\d+) union cases", out)
    assert m, out
    assert int(m.group(1)) >= 8 and int(m.group(2)) >= 8
