"""The block layout helper of the map-side entry points (slam-module_amd/csrc/ms_layout.h) on the CPU: tests/ms_layout_check.cpp checks the
helper's contract (offsets are multiples of 256 and never decrease, an empty array takes nothing, a copied layout goes on independently,
the typed accessor is base + offset, fill / put write exactly their elements between guard bytes) and that it reproduces, offset for offset
and total for total, the hand-chained layouts ms_triangulate and ms_project_gate used before it, for three shapes each."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "ms_layout_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", *extra, "-I", os.path.join(ROOT, "slam-module_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ms_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "layout ok" in out.stdout


def test_layout_contract_and_old_chains():
    _build_and_run(EXE, [])


def test_layout_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
