"""Measures the device loop-closure RANSAC (ms_loop_ransac): for batches of 1, 11 and 64 problems x 100, 300 and 1000 iterations x 50, 300
and 2000 matches, the host-call latency of one ms_loop_ransac (packing, upload, three kernels, download, synchronisation; the C call with
its arguments built beforehand, as a C++ caller has them) and of the Python wrapper mi355slam.loop_ransac around it.
loopClosureRansacIterations is set by the parent project and its default is not in
the reference tree, hence the sweep.  For comparison it times the numpy restatement (tests/loop_ransac_ref.py -- NOT the reference's
Eigen code) on the headline batch of 11 x 300 x 500 and on smaller ones.

    python tools/loop_ransac_probe.py [--calls 20] [--out FILE]

Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (use --calls 5 there)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-module_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import mi355slam  # noqa: E402
import loop_ransac_ref as ref  # noqa: E402


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(ts.min()), 4), "max_ms": round(float(ts.max()), 4), "n": len(ts)}


def batch(rng, n_prob, n_iter, n_match):
    probs = []
    for i in range(n_prob):
        p = ref.make_scene(rng, n_match, noise_px=0.5, outliers=0.3, n_iter=n_iter, min_inliers=10)
        p["samples"] = ref.draw(rng, n_match, n_iter)
        probs.append(p)
    return probs


def raw_call(ctx, probs):
    """A closure that makes exactly the ms_loop_ransac call of mi355slam.loop_ransac, with every argument prepared once."""
    M = mi355slam
    keep = []
    structs = []
    for p in probs:
        a = [np.ascontiguousarray(p["pts1"], np.float64), np.ascontiguousarray(p["pts2"], np.float64), np.ascontiguousarray(p["thr1"], np.float32),
             np.ascontiguousarray(p["thr2"], np.float32), np.ascontiguousarray(p["samples"], np.int32)]
        keep.append(a)
        structs.append(M.LoopRansacProblemC(len(a[0]), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, M.Pinhole(*p["cam1"]),
                                            M.Pinhole(*p["cam2"]), int(p["n_iter"]), a[4].ctypes.data, int(p["dof"]), int(p["fix_scale"]), int(p["min_inliers"])))
    n = len(probs)
    P = (M.LoopRansacProblemC * n)(*structs)
    R = (M.LoopRansacResultC * n)()
    masks = [np.zeros(len(k[0]), np.uint8) for k in keep] + [np.zeros(len(k[0]), np.uint8) for k in keep]
    um = (C.c_void_p * n)(*[m.ctypes.data for m in masks[:n]])
    bm = (C.c_void_p * n)(*[m.ctypes.data for m in masks[n:]])
    fn, h = M.lib().ms_loop_ransac, ctx._h

    def call():
        rc = fn(h, P, n, R, um, bm, None)
        if rc != 0:
            ctx.check(rc, "ms_loop_ransac")
    call.keep = (keep, masks)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--problems", default="1,11,64")
    ap.add_argument("--iters", default="100,300,1000")
    ap.add_argument("--matches", default="50,300,2000")
    ap.add_argument("--numpy", default="1x300x500,11x300x500,1x1000x2000", help="batches (PxIxM) the numpy restatement is timed on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = mi355slam.Context(0)
    rng = np.random.default_rng(0)
    rows = []
    configs = [(int(p), int(i), int(m)) for p in a.problems.split(",") for i in a.iters.split(",") for m in a.matches.split(",")]
    configs.append((11, 300, 500))
    for P, I, M in configs:
        probs = batch(rng, P, I, M)
        call = raw_call(ctx, probs)
        call()                                                              # warm-up: the workspace grows here
        host, py = [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            call()
            host.append(time.perf_counter() - t0)
        for _ in range(a.calls):
            t0 = time.perf_counter()
            mi355slam.loop_ransac(ctx, probs)
            py.append(time.perf_counter() - t0)
        row = {"problems": P, "iters": I, "matches": M, "host_call": stats(host), "python_wrapper": stats(py)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    for spec in filter(None, a.numpy.split(",")):
        P, I, M = (int(x) for x in spec.split("x"))
        probs = batch(rng, P, I, M)
        t0 = time.perf_counter()
        for p in probs:
            ref.ransac_solve(p, p["samples"])
        row = {"numpy_restatement": {"problems": P, "iters": I, "matches": M, "seconds": round(time.perf_counter() - t0, 4)}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
