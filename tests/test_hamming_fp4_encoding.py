"""k_hamming_mfma's FP4 operand encoding (slam-module_amd/csrc/hamming_fp4.h) on the CPU: tests/hamming_fp4_check.cpp decodes the E2M1 nibbles
on the host and checks, for every bit position alone, all-zero / all-one descriptors and 1000 random pairs, that query bit i and target bit i
land in the same (k-step, lane half, dword, nibble) slot and that popcount(q) + the decoded product sum is the Hamming distance."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "hamming_fp4_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", *extra, "-I", os.path.join(ROOT, "slam-module_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hamming_fp4_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "encoding ok" in out.stdout


def test_encoding_is_exact():
    _build_and_run(EXE, [])


def test_encoding_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
