"""k_hamming_mfma's 32-bit keys (slam-module_amd/csrc/hamming_fp4.h) on the CPU: tests/hamming_key_check.cpp checks the float arithmetic that leaves
the key in the accumulator register (dot = -256, 0, +256, every register and lane half), its bit pattern, the ageing by 32 per tile over the 256
tiles a set may have, the recovery of row and distance, the empty sentinel, and the three-instruction update of (best, second) by two keys against
a sort on all quadruples of small keys."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "hamming_key_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "slam-module_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hamming_key_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "keys ok" in out.stdout


def test_keys_are_exact():
    _build_and_run(EXE, [])


def test_keys_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
