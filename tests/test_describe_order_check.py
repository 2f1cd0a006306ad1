"""Which workgroup of k_describe takes which keypoint, on the CPU (slam-module_amd/csrc/describe_strips.h: remap; describe_order.h: key).
tests/describe_order_check.cpp walks the plan set of describe_strips_check plus hand-made plans with regions of 1 .. 40 blocks: remap is a
bijection of every region onto itself, the blocks with the same index modulo 8 get one contiguous rising run, regions of fewer than 8 and of
8 k + 1 .. 8 k + 7 blocks occur; the visit-order key is a strict total order on (x, y, index), checked on hand-made levels with equal keys."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "describe_order_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *extra, "-I", os.path.join(ROOT, "slam-module_amd", "csrc"),
                           os.path.join(ROOT, "tests", "describe_order_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "order ok" in out.stdout


def test_remap_is_a_bijection_and_the_key_a_total_order():
    _build_and_run(EXE, [])


def test_remap_and_key_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
