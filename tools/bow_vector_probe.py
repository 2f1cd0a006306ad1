"""Times the keyframe's BowVector on the device against the path it replaces.

  shape   2 000 keypoints in a device keypoint view of the extractor's layout, a vocabulary of k = 10, L = 5 (111 111 nodes, 100 000 words),
          tables of 8 slots x 2 048.
  new     ms_keyframe_admit with NULL for the host word / weight (every other host output wanted), ms_keyframe_admit_words, then
          ms_bow_db_add_words: the vector is assembled and packed into the database's pool on the device.
  old     ms_keyframe_admit with the host word / weight, the host assembly (the dict walk of BowIndex::assembleVector in Python; the C++
          mirror fills a std::map), then ms_bow_db_add and a wait for its upload.
  pieces  add_words alone and (host assembly + ms_bow_db_add + wait) alone on an admitted keyframe, and the host assembly alone, so that a
          reader can put another host's assembly time in its place.
  sizes   ms_bow_vector and ms_bow_db_add_words at n = 8 192 with all words distinct and with every keypoint on one word (the serial sum).

Host clock around the synchronous calls, three warm-ups, the best and the mean of --reps calls; the entry of the timed call is removed
outside the timed span.  The entries of both databases are compared for equal bits.  Prints one JSON line.
python tools/bow_vector_probe.py [--reps 20] [--n 2000]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-module_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import bow_vector_ref                 # noqa: E402
import keyframe_admit_ref as R        # noqa: E402
import mi355slam                      # noqa: E402
from keyframe_admit_probe import CAM6, clock, make_vocab      # noqa: E402

N_KF, STRIDE, SLOT, CUR = 8, 2048, 5, 1000


def assemble(word, weight):
    """BowIndex::assembleVector: v[word] += weight in feature order for weight > 0, then the L1 norm over the sorted words."""
    v = {}
    for w, wt in zip(word.tolist(), weight.tolist()):
        if wt > 0:
            v[w] = v.get(w, 0.0) + wt
    keys = sorted(v)
    norm = 0.0
    for k in keys:
        norm += abs(v[k])
    return np.array(keys, np.int32), np.array([v[k] / norm if norm > 0 else v[k] for k in keys], np.float64)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def probe(ctx, n, reps):
    arrays = make_vocab(10, 5)
    vocab = mi355slam.BowVocabulary(ctx, arrays["parent"], arrays["desc"], arrays["weight"], arrays["word"], 5)
    n_words = int(arrays["word"].max()) + 1
    frame = R.synth_frame(n, 5)
    leaves = np.flatnonzero(arrays["word"] >= 0)
    rng = np.random.default_rng(6)
    noise = lambda: rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    frame["desc"] = arrays["desc"][rng.choice(leaves[:n // 3], n)] ^ (noise() & noise() & noise() & noise())      # about three keypoints per word
    cap = n + 64
    vb = dict(count=ctx.upload(np.array([n], np.int32)))
    for k, dt, w in (("x", np.float32, 1), ("y", np.float32, 1), ("angle", np.float32, 1), ("octave", np.int32, 1), ("desc", np.uint32, 8), ("track_id", np.int32, 1)):
        a = np.zeros((cap, w), dt)
        a[:n] = np.asarray(frame[k], dt).reshape(n, w)
        vb[k] = ctx.upload(a)
    view = mi355slam.keypoints_view(cap, vb["count"], vb["x"], vb["y"], vb["angle"], vb["octave"], vb["desc"], vb["track_id"])
    t = R.empty_tables(N_KF, STRIDE, N_KF * STRIDE, 1)
    tab = {k: ctx.upload(t[k]) for k in R.TABLES}
    out_frame = mi355slam.AdmitFrame(ctx, STRIDE)
    args = dict(slot=SLOT, desc_base=SLOT * STRIDE, pose=np.arange(12, dtype=np.float64), cam=CAM6, levels_up=4, vocab=vocab)
    dbs = dict(new=mi355slam.BowDatabase(ctx, n_words), old=mi355slam.BowDatabase(ctx, n_words))
    without_words = [k for k, _, _ in mi355slam._ADMIT_HOST if k not in ("word", "weight")]

    def admit(host):
        rc, res = mi355slam.keyframe_admit_device(ctx, view, 0, tab, N_KF, STRIDE, 50, N_KF * STRIDE, args, out_frame, host)
        ctx.check(rc, "ms_keyframe_admit")
        return res

    def add_words():
        dw, dwt, m = mi355slam.keyframe_admit_words(ctx)
        rc, length = dbs["new"].add_words_device(CUR, 1, dw, dwt, m)
        ctx.check(rc, "ms_bow_db_add_words")
        return length

    def host_add(res):
        words, values = assemble(res["word"], res["weight"])
        dbs["old"].add(CUR, 1, words, values)
        ctx.sync()
        return len(words)

    def new_path():
        admit(without_words)
        return add_words()

    def old_path():
        return host_add(admit(True))

    def sized(word, weight):
        """ms_bow_vector and add_words on a descent that lies on the device"""
        dw, dwt = ctx.upload(word), ctx.upload(weight)
        ow, ov = ctx.alloc(4 * len(word)), ctx.alloc(8 * len(word))
        want = bow_vector_ref.bow_vector(word, weight, n_words)

        def vector():
            rc, length, bad = mi355slam.bow_vector_device(ctx, dw, dwt, len(word), n_words, len(word), ow, ov)
            ctx.check(rc, "ms_bow_vector")
            return length

        def add():
            rc, length = dbs["new"].add_words_device(CUR, 2, dw, dwt, len(word))
            ctx.check(rc, "ms_bow_db_add_words")
            return length

        r = dict(n=len(word))
        r["bow_vector"], length = clock(vector, reps, lambda: None)
        r["add_words"], _ = clock(add, reps, lambda: dbs["new"].remove(CUR, 2))
        got = dbs["new"].entry(CUR, 2)
        r.update(n_words=length, equal_bits=bool(length == want[2] and same(got[0], want[0]) and same(got[1], want[1]) and
                                                 same(ow.download(np.int32, (length,)), want[0]) and same(ov.download(np.float64, (length,)), want[1])))
        dbs["new"].remove(CUR, 2)
        for b in (dw, dwt, ow, ov):
            b.free()
        return r

    try:
        out = dict(n=n, vocabulary_nodes=int(len(arrays["parent"])), vocabulary_words=n_words)
        drop_new, drop_old = (lambda: dbs["new"].remove(CUR, 1)), (lambda: dbs["old"].remove(CUR, 1))
        out["new_path"], length = clock(new_path, reps, drop_new)
        out["old_path"], old_length = clock(old_path, reps, drop_old)
        a, b = dbs["new"].entry(CUR, 1), dbs["old"].entry(CUR, 1)
        out.update(n_words=length, equal_bits=bool(length == old_length and same(a[0], b[0]) and same(a[1], b[1])))
        # the pieces, on the keyframe as admitted last (with its host words)
        res = admit(True)
        out["admit_without_host_words"], _ = clock(lambda: admit(without_words), reps, lambda: None)
        out["admit_with_host_words"], _ = clock(lambda: admit(True), reps, lambda: None)
        out["add_words_alone"], _ = clock(add_words, reps, drop_new)
        out["host_assembly_add_wait_alone"], _ = clock(lambda: host_add(res), reps, drop_old)
        out["host_assembly_alone_python"], _ = clock(lambda: assemble(res["word"], res["weight"]), reps, lambda: None)
        drop_new(); drop_old()
        rng = np.random.default_rng(9)
        weight = np.exp2(rng.uniform(-6.0, 3.0, 8192))
        out["n8192_all_distinct"] = sized(rng.permutation(n_words)[:8192].astype(np.int32), weight)
        out["n8192_one_word"] = sized(np.full(8192, 4242, np.int32), weight)
        return out
    finally:
        for d in dbs.values():
            d.close()
        for b in list(vb.values()) + list(tab.values()):
            b.free()
        out_frame.free()
        vocab.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=2000)
    a = ap.parse_args()
    ctx = mi355slam.Context(0)
    try:
        print(json.dumps(dict(probe="bow_vector", reps=a.reps, result=probe(ctx, a.n, a.reps))))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
