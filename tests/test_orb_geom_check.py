"""The host side of ms_orb_create (slam-module_amd/csrc/orb_geom.h) on the CPU: tests/orb_geom_check.cpp derives the pyramid geometry, the resize
and describe tables and the device block's layout for the configurations of tests/golden/orb_geom_cases.txt -- the usual frame sizes, one level,
twelve levels, a minimum keypoint distance, tracks, level quotas that add up to more than max_kpts, a scale factor above 2, and the nine
configurations ms_orb_create turns away -- compares every field with the record, and checks the invariants the kernels rely on (disjoint planes
and candidate lists, exact tile division, a block whose arrays are disjoint, 256-aligned and no smaller than the allocations they replace)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-module_amd", "csrc")
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "orb_geom_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *extra, "-I", CSRC, os.path.join(ROOT, "tests", "orb_geom_check.cpp"),
                           os.path.join(CSRC, "geometry.cpp"), "-o", exe])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "orb_geom_cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "orb geom ok" in out.stdout


def test_geometry_tables_and_block_layout():
    _build_and_run(EXE, [])


def test_geometry_tables_and_block_layout_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_one_device_block_in_the_source():
    """The extractor owns two device allocations, its block and the valid mask, and the per-array helper is gone."""
    with open(os.path.join(CSRC, "orb.hip")) as f:
        src = f.read()
    assert len(re.findall(r"\bhipMalloc\(", src)) == 2
    assert "dev_calloc" not in src
