"""k_fast's tile cover (slam-module_amd/csrc/fast_tiles.h) on the CPU: tests/fast_tile_cover_check.cpp sweeps level sizes and checks that
every position that can be a corner lies in exactly one tile's output rectangle, that tiles start on dword columns and are never empty,
and that the cover never needs more workgroups than the plain 248 x 30 grid.  The per-frame totals of the two benchmark pyramids are held
against the counts the cover was designed for."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "fast_tile_cover_check")


def test_cover_is_exact_and_small():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fast_tile_cover_check.cpp"), "-o", EXE])
    out = subprocess.run([EXE], stdout=subprocess.PIPE, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "cover ok" in out.stdout
    totals = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^total (\d+x\d+) (\d+) (\d+)$", out.stdout, re.M)}
    assert totals["1280x720"][1] == 452 and totals["640x480"][1] == 175          # the plain grid, as counted before
    assert totals["1280x720"][0] <= 406
    assert totals["640x480"][0] <= 149
