"""CPU checks of the surface of the device BowVector: the header declares ms_bow_vector, its validation twin, ms_bow_db_add_words,
ms_bow_db_entry and ms_keyframe_admit_words, the library exports them, Python binds them, and ms_bow_vector_validate, the host-only half
that runs in front of any device call, accepts the valid cases, turns every bad call away with its message and holds both caps -- through the
library, and again in a program of its own compiled with map_checks.cpp alone under ASan and UBSan.  The validation dereferences no array,
so host arrays stand in for the device arrays."""
import os
import re
import subprocess

import numpy as np
import pytest

import mi355slam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-module_amd", "csrc")
INVALID, CAPACITY = mi355slam.MS_ERR_INVALID, mi355slam.MS_ERR_CAPACITY
MAX_STRIDE = 8192


def header(comments=False):
    text = open(os.path.join(ROOT, "include", "mi355slam.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declaration(name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header())
    assert m, name
    return [" ".join(p.split()).replace("const ", "") for p in m.group(1).split(",")]


def test_the_library_exports_the_calls_and_python_binds_them():
    for name in ("ms_bow_vector", "ms_bow_vector_validate", "ms_bow_db_add_words", "ms_bow_db_entry", "ms_keyframe_admit_words"):
        assert hasattr(mi355slam.lib(), name), name
    for name in ("bow_vector", "bow_vector_device", "bow_vector_validate", "keyframe_admit_words", "keyframe_admit_words_device"):
        assert callable(getattr(mi355slam, name)), name
    for name in ("add_words", "add_words_device", "entry", "entry_device"):
        assert callable(getattr(mi355slam.BowDatabase, name)), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bbow_vector\.hip\b", mk, flags=re.M) and not re.search(r"^bow_vector\.o\s*:.*FLAGS", mk, flags=re.M)      # no contraction: the unit keeps -ffp-contract=off
    src = open(os.path.join(CSRC, "bow_vector.hip")).read()
    internal = open(os.path.join(CSRC, "ms_internal.h")).read()
    assert '#include "ms_scan.h"' in src and "block_rank<kThreads>" in src and "MS_WS_BOW_VECTOR" in src and "MS_WS_BOW_VECTOR" in internal and "ms_pinned(" in src
    code = re.sub(r"//[^\n]*", "", src)
    # the only atomic is the integer add of the verdict counter; nothing floating-point is added atomically or through shuffles
    assert set(re.findall(r"\batomic\w*", code)) == {"atomicAdd"} and code.count("atomicAdd(") == 1 and "atomicAdd(&s_bad, bad)" in code
    assert not re.search(r"__shfl\w*\(\s*(v|norm|val)\b", code) and "fma(" not in code
    # ONE launch whatever n is, one download, one wait, no upload, nothing allocated outside the workspace
    body = code.split('extern "C" int ms_bow_vector(')[1]
    assert code.count("hipLaunchKernelGGL(") == 1 and body.count("ms_bow_vector_enqueue(") == 1 and "ONE launch" in header(True) and "ONE launch" in src
    assert body.count("hipMemcpyDeviceToHost") == 1 and body.count("hipStreamSynchronize") == 1 and "hipMemcpyHostToDevice" not in code
    assert not re.search(r"\bhipMalloc|\bhipHostMalloc|\bnew\b|std::vector", code)
    # the database's add runs the same kernel and commits after the head has come down
    db = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "bowdb.hip")).read())
    add = db.split("int ms_bow_db_add_words(")[1].split("\nint ms_bow_db_entry(")[0]
    assert add.count("ms_bow_vector_enqueue(") == 1 and "reserve_entries(" in add and "reserve_pool(" in add and "seg_cells(n)" in add and "seg_cells(len)" in add
    assert add.index("find_slot(") < add.index("hipSetDevice") < add.index("reserve_pool(") < add.index("ms_bow_vector_enqueue(") < add.index("sync_stream(") < add.index("hash_insert(")
    assert add.index("n_bad > 0") < add.index("upload(") and "hipMemcpyHostToDevice" not in add
    adm = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "keyframe_admit.hip")).read())
    assert 'extern "C" int ms_keyframe_admit_words(' in adm and adm.index("c->admit_n = -1;") < adm.index("ms_keyframe_admit_validate(view")


def test_the_header_declares_the_calls_and_the_twin_takes_the_arguments_of_the_call():
    assert "DESIGN 9.20" in header(True)
    call, twin = declaration("ms_bow_vector"), declaration("ms_bow_vector_validate")
    assert call[0] == "ms_ctx *ctx" and call[1:] == twin[:-2] and twin[-2:] == ["char *why", "size_t why_bytes"]
    assert [p.split("*")[-1].split()[-1] for p in call[1:]] == ["word", "weight", "n", "vocab_words", "cap", "words", "values", "counts"]
    assert declaration("ms_keyframe_admit_words") == ["ms_ctx *ctx", "int32_t **word", "double **weight", "int32_t *n"]
    assert declaration("ms_bow_db_add_words") == ["ms_bow_db *db", "int32_t map_id", "int32_t kf_id", "int32_t *word_dev", "double *weight_dev", "int n", "int32_t *n_words"]
    assert declaration("ms_bow_db_entry") == ["ms_bow_db *db", "int32_t map_id", "int32_t kf_id", "int cap", "int32_t *words_host", "double *values_host", "int *n"]
    assert "ms_bow_vector_check" not in header(True) and re.search(r"/\*[^\n]*_validate[^\n]*22[^\n]*\*/\s*int ms_bow_vector_validate", header(True))
    checks = open(os.path.join(CSRC, "map_checks.cpp")).read()
    assert 'extern "C" int ms_bow_vector_validate(' in checks
    text = " ".join(header(True).replace("\n *", " ").split())               # comment lines joined
    for phrase in ("valid until the next ms_keyframe_admit on that context", "tests/bow_vector_ref.py", "no floating-point atomic and no tree reduction",
                   "Every verdict is taken before any output byte is written", "ms_keyframe_admit_words, DESIGN 9.20"):
        assert phrase in text, phrase


class Call:
    """One call of ms_bow_vector_validate: 100 keypoints, a vocabulary of 1000 words, outputs of 100."""

    def __init__(self):
        self.n, self.vocab_words, self.cap, self.counts = 100, 1000, 100, True
        self.arr = dict(word=np.zeros(104, np.int32), weight=np.zeros(104, np.float64), words=np.zeros(104, np.int32), values=np.zeros(104, np.float64))
        self.shift = {}

    def ptr(self, k):
        a = self.arr[k]
        return None if a is None else a.ctypes.data + self.shift.get(k, 0)

    def run(self):
        return mi355slam.bow_vector_validate(self.ptr("word"), self.ptr("weight"), self.n, self.vocab_words, self.cap, self.ptr("words"), self.ptr("values"), self.counts)


def changed(**kw):
    c = Call()
    for k, v in kw.items():
        if k in c.arr:
            c.arr[k] = v
        elif k.startswith("shift_"):
            c.shift[k[6:]] = v
        else:
            setattr(c, k, v)
    return c


def test_valid_calls_and_the_zero_sizes_pass():
    assert Call().run() == (0, "")
    assert changed(n=0, word=None, weight=None).run() == (0, "") and changed(cap=0, words=None, values=None).run() == (0, "")
    assert changed(n=0, cap=0, word=None, weight=None, words=None, values=None).run() == (0, "")
    assert changed(vocab_words=1).run() == (0, "") and changed(cap=1).run() == (0, "") and changed(vocab_words=2**31 - 1).run() == (0, "")
    assert changed(shift_word=4, shift_words=4).run() == (0, "") and changed(shift_weight=8, shift_values=16).run() == (0, "")


INVALID_CASES = [
    (dict(n=-1), "negative size (-1 keypoints, cap 100)"), (dict(cap=-1), "negative size (100 keypoints, cap -1)"),
    (dict(vocab_words=0), "a vocabulary of 0 words"), (dict(vocab_words=-5), "a vocabulary of -5 words"),
    (dict(counts=False), "missing array (counts)"),
    (dict(word=None), "missing array (word or weight with 100 keypoints)"), (dict(weight=None), "missing array (word or weight with 100 keypoints)"),
    (dict(words=None), "missing array (words or values with cap 100)"), (dict(values=None), "missing array (words or values with cap 100)"),
    (dict(shift_values=4), "must be 8-byte aligned"), (dict(shift_weight=4), "must be 8-byte aligned"), (dict(shift_values=1), "must be 8-byte aligned"),
]


@pytest.mark.parametrize("kw, message", INVALID_CASES, ids=["%s: %s" % (",".join(k), m) for k, m in INVALID_CASES])
def test_every_invalid_call_is_turned_away_with_its_message(kw, message):
    rc, why = changed(**kw).run()
    assert rc == INVALID and why.startswith("bow vector: ") and message in why, (kw, rc, why)


def test_both_caps_hold_at_their_limit_and_one_beyond():
    for kw, text in ((dict(n=MAX_STRIDE + 1), "8193 keypoints / cap 100"), (dict(cap=MAX_STRIDE + 1), "100 keypoints / cap 8193")):
        rc, why = changed(**kw).run()
        assert rc == CAPACITY and text in why and "caps 8192 each" in why, (text, rc, why)
    assert changed(n=MAX_STRIDE).run() == (0, "") and changed(cap=MAX_STRIDE).run() == (0, "")


PROGRAM = r"""
#include "mi355slam.h"
#include <cstdio>
#include <cstring>
#include <vector>
struct Call {
    int n = 100, vocab_words = 1000, cap = 100;
    std::vector<int32_t> word = std::vector<int32_t>(104, 0), words = std::vector<int32_t>(104, 0);
    std::vector<double> weight = std::vector<double>(104, 0.0), values = std::vector<double>(104, 0.0);
    const int32_t *p_word = word.data(), *p_words = words.data();
    const double *p_weight = weight.data(), *p_values = values.data();
    int32_t counts[2];
    const int32_t *p_counts = counts;
    char why[128];
    int run() {
        why[0] = 0;
        return ms_bow_vector_validate(p_word, p_weight, n, vocab_words, cap, p_words, p_values, p_counts, why, sizeof why);
    }
};
static int fails = 0;
static void expect(Call &c, int rc, const char *text) {
    const int got = c.run();
    if (got != rc || !std::strstr(c.why, text)) { std::printf("want %d '%s', got %d '%s'\n", rc, text, got, c.why); ++fails; }
}
static const double *off(const double *p, int bytes) { return reinterpret_cast<const double *>(reinterpret_cast<const char *>(p) + bytes); }
int main() {
    { Call c; expect(c, MS_OK, ""); }
    { Call c; c.n = 0; c.p_word = nullptr; c.p_weight = nullptr; expect(c, MS_OK, ""); }
    { Call c; c.cap = 0; c.p_words = nullptr; c.p_values = nullptr; expect(c, MS_OK, ""); }
    { Call c; c.n = -1; expect(c, MS_ERR_INVALID, "negative size (-1 keypoints, cap 100)"); }
    { Call c; c.cap = -1; expect(c, MS_ERR_INVALID, "negative size (100 keypoints, cap -1)"); }
    { Call c; c.vocab_words = 0; expect(c, MS_ERR_INVALID, "a vocabulary of 0 words"); }
    { Call c; c.p_counts = nullptr; expect(c, MS_ERR_INVALID, "missing array (counts)"); }
    { Call c; c.p_word = nullptr; expect(c, MS_ERR_INVALID, "missing array (word or weight with 100 keypoints)"); }
    { Call c; c.p_weight = nullptr; expect(c, MS_ERR_INVALID, "missing array (word or weight with 100 keypoints)"); }
    { Call c; c.p_words = nullptr; expect(c, MS_ERR_INVALID, "missing array (words or values with cap 100)"); }
    { Call c; c.p_values = nullptr; expect(c, MS_ERR_INVALID, "missing array (words or values with cap 100)"); }
    { Call c; c.p_values = off(c.p_values, 4); expect(c, MS_ERR_INVALID, "must be 8-byte aligned"); }
    { Call c; c.p_weight = off(c.p_weight, 4); expect(c, MS_ERR_INVALID, "must be 8-byte aligned"); }
    { Call c; c.n = MS_COVIS_MAX_STRIDE + 1; expect(c, MS_ERR_CAPACITY, "8193 keypoints / cap 100, caps 8192 each"); }
    { Call c; c.cap = MS_COVIS_MAX_STRIDE + 1; expect(c, MS_ERR_CAPACITY, "100 keypoints / cap 8193, caps 8192 each"); }
    { Call c; c.n = MS_COVIS_MAX_STRIDE; c.cap = MS_COVIS_MAX_STRIDE; expect(c, MS_OK, ""); }
    { Call s; char tiny[8];                                  // a short buffer is not overrun, a missing one is not written
      if (ms_bow_vector_validate(s.p_word, s.p_weight, -1, 1000, 100, s.p_words, s.p_values, s.counts, tiny, sizeof tiny) != MS_ERR_INVALID || std::strlen(tiny) != 7) ++fails;
      if (ms_bow_vector_validate(s.p_word, s.p_weight, -1, 1000, 100, s.p_words, s.p_values, s.counts, nullptr, 0) != MS_ERR_INVALID) ++fails; }
    std::printf("bow vector validate alone: %d failures\n", fails);
    return fails ? 1 : 0;
}
"""


def test_the_validation_alone_runs_clean_under_sanitizers(tmp_path):
    """A program with its own main and the public header only, compiled together with map_checks.cpp (no HIP, no library, nothing preloaded)."""
    src, exe = tmp_path / "alone.cpp", tmp_path / "alone"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           str(src), os.path.join(CSRC, "map_checks.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and "0 failures" in run.stdout, run.stdout + run.stderr
