"""CPU checks of the keyframe database's surface (ms_bow_db): the header declares it, the library exports it, and the host
mirror's BowIndex::add / remove / getBowSimilar compile and link against it (tests/bow_db_smoke.cpp)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "bow_db_smoke")
SYMBOLS = ["ms_bow_db_create", "ms_bow_db_destroy", "ms_bow_db_add", "ms_bow_db_remove", "ms_bow_db_size", "ms_bow_db_query", "ms_bow_db_query_ids"]


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "bow_db_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_header_declares_the_bow_db_entry_points():
    hdr = open(os.path.join(ROOT, "include", "mi355slam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "typedef struct ms_bow_db ms_bow_db;" in code
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name


def test_library_exports_the_bow_db_entry_points():
    import mi355slam
    L = mi355slam.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), "libmi355slam.so does not export %s" % name


def test_python_binding_has_the_database():
    import mi355slam
    for m in ("add", "remove", "query", "query_ids", "close", "size"):
        assert hasattr(mi355slam.BowDatabase, m)


def test_bow_db_mirror_compiles_and_links():
    out = subprocess.check_output([build_smoke(), "--no-gpu"], text=True)
    assert "link ok 1 1 1" in out
