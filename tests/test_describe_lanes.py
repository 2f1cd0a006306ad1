"""k_describe's lane maps (slam-module_amd/csrc/describe_lanes.h) on the CPU: tests/describe_lanes_check.cpp checks for all 64 lanes that the
window fetch covers each of the 45 x 12 window dwords exactly once, that the orientation copy reads exactly window rows 7 .. 37, dwords 2 .. 9
and fills each patch dword once, that the moments' dword arithmetic gives orb_extractor's m10 / m01 (every pixel alone, all-255, 200 random
windows), and that the blur's tap index selects the entry the operand select used to produce."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "describe_lanes_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", *extra, "-I", os.path.join(ROOT, "slam-module_amd", "csrc"),
                           os.path.join(ROOT, "tests", "describe_lanes_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "lanes ok" in out.stdout


def test_lane_maps_are_exact():
    _build_and_run(EXE, [])


def test_lane_maps_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
