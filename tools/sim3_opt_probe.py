"""Measures the device Sim3 refinement (ms_sim3_optimize): for batches of 1, 11 and 64 problems x 50, 300 and 2000 matches, 20 iterations, the
host-call latency of one ms_sim3_optimize (packing into the pinned planes, upload, one kernel, download, synchronisation; the C call with its
arguments built beforehand, as a C++ caller has them) and of the Python wrapper mi355slam.sim3_optimize around it.  For comparison it times the
numpy restatement (tests/sim3_opt_ref.py -- numpy, NOT g2o) on the same batches, on this machine's host.

    python tools/sim3_opt_probe.py [--calls 20] [--out FILE]

The kernel's time alone comes from a separate run under `rocprofv3 --kernel-trace --stats`."""
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
import sim3_opt_ref as ref  # noqa: E402


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(ts.min()), 4), "max_ms": round(float(ts.max()), 4), "n": len(ts)}


def raw_call(ctx, probs):
    """A closure that makes exactly the ms_sim3_optimize call of mi355slam.sim3_optimize, with every argument prepared once."""
    n = len(probs)
    P, keep = mi355slam.sim3_opt_pack(probs)
    R = (mi355slam.Sim3OptResultC * n)()
    fn, h = mi355slam.lib().ms_sim3_optimize, ctx._h

    def call():
        rc = fn(h, P, n, R, None)
        if rc != 0:
            ctx.check(rc, "ms_sim3_optimize")
    call.keep = (keep, P)
    call.results = R
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--problems", default="1,11,64")
    ap.add_argument("--matches", default="50,300,2000")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--numpy", default="1x300,11x300,11x2000", help="batches (PxM) the numpy restatement is timed on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = mi355slam.Context(0)
    rng = np.random.default_rng(0)
    rows = []
    for P in (int(x) for x in a.problems.split(",")):
        for M in (int(x) for x in a.matches.split(",")):
            probs = [ref.make_scene(rng, M, fix_scale=bool(i % 2), max_iters=a.iters) for i in range(P)]
            call = raw_call(ctx, probs)
            call()                                                          # warm-up: the workspace grows here
            host, py = [], []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                call()
                host.append(time.perf_counter() - t0)
            for _ in range(a.calls):
                t0 = time.perf_counter()
                mi355slam.sim3_optimize(ctx, probs)
                py.append(time.perf_counter() - t0)
            sweeps = [1 + r.trials_total for r in call.results]
            row = {"problems": P, "matches": M, "iters": a.iters, "host_call": stats(host), "python_wrapper": stats(py),
                   "sweeps_per_problem": {"median": float(np.median(sweeps)), "max": int(max(sweeps))}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    for spec in filter(None, a.numpy.split(",")):
        P, M = (int(x) for x in spec.split("x"))
        probs = [ref.make_scene(rng, M, fix_scale=bool(i % 2), max_iters=a.iters) for i in range(P)]
        t0 = time.perf_counter()
        for p in probs:
            ref.optimize(p)
        row = {"numpy_restatement": {"problems": P, "matches": M, "iters": a.iters, "seconds": round(time.perf_counter() - t0, 4)}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
