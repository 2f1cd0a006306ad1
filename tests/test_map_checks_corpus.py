"""The 22 host-only ms_*_check twins of the map entry points (csrc/map_checks.cpp) against a recorded corpus: tests/map_checks_corpus.cpp prints
one line per call -- function, case, return code, message -- and the output must equal tests/golden/map_checks_corpus.txt byte for byte.  The
golden file is this project's own recorded output, taken from the commit before the checks moved into one unit:
    g++ -std=c++17 -Wall -Werror -I include tests/map_checks_corpus.cpp -o corpus -L slam-module_amd/lib -lmi355slam -Wl,-rpath,$PWD/slam-module_amd/lib
    ./corpus > tests/golden/map_checks_corpus.txt
The program runs twice: linked against the library, and compiled together with map_checks.cpp alone (no library, no Python) under ASan and UBSan."""
import os
import re
import subprocess

import mi355slam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "tests", "map_checks_corpus.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "map_checks_corpus.txt")
OK, INVALID = "0", str(mi355slam.MS_ERR_INVALID)


def golden():
    with open(GOLDEN, "rb") as f:
        return f.read()


def declared_checks():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355slam.h")).read(), flags=re.S)
    return [n for n in re.findall(r"\bint\s+(ms_\w+_check)\s*\(", hdr) if n != "ms_angle_check"]       # in the header's order


def test_the_golden_file_covers_every_check_twin_with_an_accepted_and_a_rejected_call():
    names = declared_checks()
    assert len(names) == len(set(names)) == 22, names
    codes = {}
    for line in golden().decode().splitlines():
        fn, case, rc, why = line.split("\t")
        codes.setdefault(fn, set()).add(rc)
        assert (rc == OK) == (why == ""), line               # a message exactly where a call is turned away
    assert sorted(codes) == sorted(names)                    # no twin without a line, no line for anything else
    for fn in names:
        assert OK in codes[fn] and INVALID in codes[fn], (fn, codes[fn])


def test_the_library_gives_the_recorded_codes_and_messages(tmp_path):
    mi355slam.lib()
    exe, libdir = tmp_path / "corpus", os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), PROGRAM, "-o", str(exe), "-L", libdir, "-lmi355slam",
                           "-Wl,-rpath," + libdir])
    assert subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True).stdout == golden()


def test_the_checks_alone_give_them_under_sanitizers(tmp_path):
    """map_checks.cpp and the program, nothing else: no HIP, no library.  A sanitizer finding ends the run with a non-zero status."""
    exe = tmp_path / "corpus_san"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           PROGRAM, os.path.join(ROOT, "slam-module_amd", "csrc", "map_checks.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()
    assert run.stdout == golden()


def test_the_validation_is_one_plain_unit():
    csrc = os.path.join(ROOT, "slam-module_amd", "csrc")
    unit = open(os.path.join(csrc, "map_checks.cpp")).read()
    code = re.sub(r"//[^\n]*", "", unit + open(os.path.join(csrc, "ms_check.h")).read())
    assert "hip" not in code.lower() and "ms_ctx" not in code
    assert re.findall(r'extern "C" int (ms_\w+_check)\(', unit) == declared_checks()                # all of them, in the header's order
    for name in os.listdir(csrc):
        if name.endswith(".hip"):
            assert not re.search(r'extern "C" int ms_\w+_check\(', open(os.path.join(csrc, name)).read()), name
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmap_checks\.cpp\b", mk, flags=re.M) and not re.search(r"^map_checks\.o\s*:", mk, flags=re.M)
