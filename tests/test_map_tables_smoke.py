"""MapTables::require, the one consistency check of the host mirror's map-table entry points (slam-module_amd/host/mi355slam/map_tables.hpp):
the mirror compiles and links against the C ABI and, on the GPU, every entry point turns away each call that has exactly one thing wrong
with std::invalid_argument naming the function, before anything is written to the tables, and takes the consistent tables
(tests/map_tables_smoke.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "map_tables_smoke")
# the std::invalid_argument conditions the entry points had before they took the view (listed per function at the top of the program)
CONDITIONS = 99


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "map_tables_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_compiles_and_links():
    build_smoke()
    out = subprocess.check_output([EXE, "--no-gpu"], text=True)
    assert "link ok 1" in out, out


@pytest.mark.gpu
def test_every_entry_point_turns_away_each_inconsistency_and_takes_the_consistent_tables():
    build_smoke()
    out = subprocess.check_output([EXE, "--gpu"], text=True)
    m = re.search(r"rejections ok (\d+) cases", out)
    assert m and int(m.group(1)) == CONDITIONS, out
    assert "passing calls ok 16 functions" in out, out
