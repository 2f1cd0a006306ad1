"""Ownership of device memory in the host mirror (mi355slam::DeviceArray in slam-module_amd/host/mi355slam/common.hpp and every owner built on
it) on the CPU: tests/device_array_check.cpp defines the handful of ABI functions the headers reach over malloc and memcpy, with a set of live
blocks, a call log and a counter that makes the k-th allocation fail, and checks DeviceArray alone, every owner's call log without a failure,
every owner with each allocation failing in turn (a std::runtime_error, nothing stays live, the grow-only owners stay usable) and
updateDescriptors when its kernel call fails.  Every assertion is exact.

The expected call logs in the program are those of the headers before DeviceArray existed, printed by the same program built against them:

    git worktree add /tmp/before <the commit before DeviceArray>
    g++ -std=c++17 -DDEVICE_ARRAY_CHECK_RECORD -I /tmp/before/slam-module_amd/host tests/device_array_check.cpp -o /tmp/record && /tmp/record

Against those headers the logs print, the failing-allocation checks then report the blocks that leak, and the program stops in the regrow
check, where DeviceObservationLists claims a capacity it has no buffers for."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "device_array_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *extra, "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "device_array_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "device arrays ok: 11 owners" in out.stdout


def test_owners_free_what_they_allocate():
    _build_and_run(EXE, [])


def test_owners_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer (leaks included) and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
