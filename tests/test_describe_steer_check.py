"""k_describe's steering arithmetic (slam-module_amd/csrc/describe_steer.h) on the CPU: tests/describe_steer_check.cpp compares the one-division,
one-polynomial arc tangent and the select-then-evaluate cosine with the two-branch and four-branch forms they replace, bit for bit, on every
integer pair of moments in [-300, 300]^2, 10^7 random pairs over the moments' full range, the axes, the diagonals and (0, 0), and the cosine and
sine of every angle these produce."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "describe_steer_check")


def test_steering_is_bit_exact():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "slam-module_amd", "csrc"),
                           os.path.join(ROOT, "tests", "describe_steer_check.cpp"), "-o", EXE])
    out = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "steer ok" in out.stdout
