"""Measures the device keyframe database (ms_bow_db): host-to-host latency of one query and one query_ids, query_ids throughput in
batches of 256, and the host cost of add / remove, on synthetic databases of 1k, 10k and 50k entries of 300-1000 words over 10^6 words.

    python tools/bow_db_probe.py [--sizes 1000,10000,50000] [--calls 200] [--out FILE]

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (use --calls 20 there); the scan's bytes are the
live words' 12 B each (word + value), printed here as live_words per size."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-module_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import mi355slam  # noqa: E402
import bow_db_ref as R  # noqa: E402


def stats(ts):
    ts = np.asarray(ts) * 1e6
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(float(ts.min()), 1), "max_us": round(float(ts.max()), 1), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,50000")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = mi355slam.Context(0)
    results = []
    for n in [int(x) for x in a.sizes.split(",")]:
        s = R.Synth(n, n_places=max(20, n // 50))
        vecs = [s.keyframe(keep=0.8, extra=60) for _ in range(n + a.calls + 16)]
        db = mi355slam.BowDatabase(ctx, 1_000_000, capacity=n + 64)
        t_add = []
        for i in range(n):
            t0 = time.perf_counter(); db.add(0, i, *vecs[i]); t_add.append(time.perf_counter() - t0)
        ctx.sync()
        live_words = int(sum(len(v[0]) for v in vecs[:n]))
        q = vecs[n]
        for _ in range(10): db.query(*q, exclude=(0, -1)); db.query_ids([(0, 1)])
        t_q, t_qi, n_res = [], [], []
        for c in range(a.calls):
            qw, qv = vecs[n + 1 + c]
            t0 = time.perf_counter(); r = db.query(qw, qv, exclude=(1000, c)); t_q.append(time.perf_counter() - t0)
            n_res.append(len(r[0]))
            t0 = time.perf_counter(); db.query_ids([(0, (7 * c) % n)]); t_qi.append(time.perf_counter() - t0)
        ids = [(0, int(i)) for i in np.random.default_rng(1).integers(0, n, 256)]
        db.query_ids(ids)
        reps = max(3, a.calls // 40)
        t0 = time.perf_counter()
        for _ in range(reps): db.query_ids(ids)
        t_batch = (time.perf_counter() - t0) / reps
        # a sliding step's removal and re-add (the mapper's cull + add)
        t_rm, t_add2 = [], []
        for c in range(min(a.calls, n)):
            t0 = time.perf_counter(); db.remove(0, c); t_rm.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); db.add(0, c, *vecs[c]); t_add2.append(time.perf_counter() - t0)
        ctx.sync()
        res = {"entries": n, "live_words": live_words, "scan_bytes": 12 * live_words, "query": stats(t_q), "query_ids_1": stats(t_qi),
               "results_per_query_median": float(np.median(n_res)), "query_ids_256_batch_ms": round(t_batch * 1e3, 2),
               "query_ids_256_per_query_us": round(t_batch / 256 * 1e6, 1), "add": stats(t_add[-a.calls:]), "remove": stats(t_rm), "re_add": stats(t_add2)}
        print(json.dumps(res), flush=True)
        results.append(res)
        db.close()
    if a.out:
        with open(a.out, "w") as f: json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
