"""CPU checks of the surface of the map-point gates (ms_project_gate): the header declares them, the library exports them, the Python struct
has the header's layout (read from the compiled smoke program), and the table-based overloads of the host mirror
(mi355slam/keyframe_matcher.hpp) compile and link (tests/project_gate_smoke.cpp)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "project_gate_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "project_gate_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_header_declares_the_gate_entry_point():
    hdr = open(os.path.join(ROOT, "include", "mi355slam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+ms_project_gate\s*\(", code)
    assert re.search(r"}\s*ms_gate_view;", code)
    for name, value in (("MS_GATE_SEARCH", 0), ("MS_GATE_FUSE", 1), ("MS_GATE_SIM3", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), code), name


def test_library_exports_the_gate_entry_point():
    import mi355slam
    assert hasattr(mi355slam.lib(), "ms_project_gate")
    assert callable(mi355slam.project_gate) and callable(mi355slam.search_by_projection)
    assert (mi355slam.GATE_SEARCH, mi355slam.GATE_FUSE, mi355slam.GATE_SIM3) == (0, 1, 2)


def test_python_struct_and_mirror_match_the_header_layout():
    import mi355slam
    out = subprocess.check_output([build_smoke(), "--no-gpu"], text=True)
    assert "link ok 1" in out and "no-gpu ok 3 modes" in out
    m = re.search(r"ms_gate_view size (\d+) (.*)", out)
    assert m, out
    words = m.group(2).split()
    header = dict(zip(words[0::2], map(int, words[1::2])))
    G = mi355slam.GateViewC
    assert C.sizeof(G) == int(m.group(1))
    assert {name: getattr(G, name).offset for name, _ in G._fields_} == header
    assert [name for name, _ in G._fields_] == ["R_cw", "t_cw", "cam", "threshold", "view_cos_limit", "mode", "first", "count"]
