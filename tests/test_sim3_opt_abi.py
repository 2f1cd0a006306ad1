"""CPU checks of the Sim3 refinement's surface (ms_sim3_optimize): the header declares it, the library exports it, the ctypes structs have the
header's layout, and the host mirror (mi355slam/optimize_transform.hpp) compiles and links against it (tests/sim3_opt_smoke.cpp), its Sim3
value type agreeing with a plain restatement."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "sim3_opt_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "sim3_opt_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_header_declares_the_sim3_entry_point():
    hdr = open(os.path.join(ROOT, "include", "mi355slam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bms_sim3_optimize\s*\(", code)
    for name in ("ms_sim3_opt_problem", "ms_sim3_opt_result"):
        assert re.search(r"}\s*%s;" % name, code), name
    for name in ("MS_SIM3_OPT_MAX_MATCHES", "MS_SIM3_OPT_MAX_PROBLEMS"):
        assert "#define " + name in code


def test_library_exports_the_sim3_entry_point():
    import mi355slam
    assert hasattr(mi355slam.lib(), "ms_sim3_optimize")
    assert callable(mi355slam.sim3_optimize)


def test_python_structs_match_the_header_layout():
    import ctypes as C
    import mi355slam
    P, R = mi355slam.Sim3OptProblemC, mi355slam.Sim3OptResultC
    assert P.pts1.offset == 8 and P.huber_delta.offset == 8 + 6 * 8 and P.fix_scale.offset == 64 and P.R12.offset == 72
    assert C.sizeof(P) == 72 + 13 * 8
    assert R.chi2_init.offset == 13 * 8 and R.iters.offset == 16 * 8 and C.sizeof(R) == 16 * 8 + 16


def test_packing_checks_the_array_lengths():
    import numpy as np
    import pytest
    import mi355slam
    import sim3_opt_ref as ref
    prob = ref.make_scene(np.random.default_rng(0), 12)
    P, keep = mi355slam.sim3_opt_pack([prob, ref.empty_problem()])
    assert P[0].n_matches == 12 and P[0].max_iters == 20 and P[0].scale12 == prob["scale12"] and list(P[0].R12) == list(prob["R12"].ravel())
    assert P[1].n_matches == 0 and not P[1].pts1
    with pytest.raises(ValueError):
        mi355slam.sim3_opt_pack([dict(prob, obs2=prob["obs2"][:5])])


def test_mirror_links_and_its_sim3_type_agrees_with_a_plain_restatement():
    out = subprocess.check_output([build_smoke(), "--no-gpu"], text=True)
    assert "link ok 1" in out and "value type ok 1" in out
