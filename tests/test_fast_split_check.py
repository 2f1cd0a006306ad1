"""The split of k_fast's tile table by pyramid level (slam-module_amd/csrc/orb_geom.h) on the CPU: tests/fast_split_check.cpp derives the geometry
of five configurations -- the two benchmark pyramids, a small one with scale 1.5, one level, twelve levels -- and checks that the level-0 count
cuts the table exactly between level 0 and the higher levels, that the two parts add up to the whole, and that the automatic rule for the two
part-launches agrees with a direct count of each part's workgroups for 1, 16, 17, 32 and 256 frames."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-module_amd", "csrc")
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "fast_split_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", *extra, "-I", CSRC, os.path.join(ROOT, "tests", "fast_split_check.cpp"),
                           os.path.join(CSRC, "geometry.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "split ok" in out.stdout
    return {m.group(1): tuple(int(m.group(i)) for i in (2, 3, 4)) for m in re.finditer(r"^split (\d+x\d+) (\d+) (\d+) (\d+)$", out.stdout, re.M)}


def test_level0_count_cuts_the_table_and_the_rule_counts_workgroups():
    got = _build_and_run(EXE, [])
    assert len(got) == 5
    assert got["1280x720"] == (126, 275, 17)            # 16 x 126 = 2016 workgroups stay one launch, 17 x 126 = 2142 split
    assert got["100x100"][1:] == (0, 0)                 # one level: nothing to run beside, at any batch


def test_level0_count_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
