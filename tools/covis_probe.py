"""Times the two map-graph queries on the device against the reference's loops on one host core, for three shapes over one map of 1000
keyframe slots x 2000 entries and 200 000 map-point rows:

  keyframe   computeAdjacentKeyframes (mapper_helpers.cpp:160-176): 11 getNeighbors queries in one ms_covisibility call
  whole_map  publishMapForViewer (:862-872): getNeighbors of all 1000 keyframes in one call
  loop       localMapPoints of correctLoop (loop_closer.cpp:418-433): one union of 1000 slots with owners, ms_map_point_union

  device     the synchronous calls with their outputs left on the device, timed with the host clock
  baseline   tests/covis_smoke.cpp --baseline: the std::map / std::set restatement of the reference's loops on one core (best of three)

Both paths run on the same map (the baseline writes it to a temporary file) and the probe compares a checksum of every result.
Prints one JSON line.  python tools/covis_probe.py [--reps 20]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-module_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import mi355slam                      # noqa: E402
import test_covis_abi                 # noqa: E402

N_KF, STRIDE, N_MP, MIN_COVIS = 1000, 2000, 200000, 5


def baseline(exe, n_q, n_union, dump=None):
    out = subprocess.check_output([exe, "--baseline", str(N_KF), str(STRIDE), str(N_MP), str(n_q), str(n_union)] + ([dump] if dump else []), text=True)
    m = re.search(r"neighbours_ms (\S+) neighbours_sum (\d+) union_ms (\S+) union_sum (\d+)", out)
    return float(m.group(1)), int(m.group(2)), float(m.group(3)), int(m.group(4))


def chain_queries(n_q):
    slots = [q * N_KF // n_q for q in range(n_q)]
    return [(k, k - 1, k + 1 if k + 1 < N_KF else -1, MIN_COVIS, 0) for k in slots]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    exe = test_covis_abi.build_smoke()
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "kf_mp.i32")
        key_ms, key_sum, union_ms, union_sum = baseline(exe, 11, N_KF, dump)
        kf_mp = np.fromfile(dump, np.int32).reshape(N_KF, STRIDE)
    map_ms, map_sum, _, _ = baseline(exe, N_KF, 0)
    ctx = mi355slam.Context(0)
    table = mi355slam.KeyframeTable(ctx, kf_mp)
    d_count, d_nb = ctx.alloc(4 * N_KF * N_KF), ctx.alloc(4 * N_KF * N_KF)
    d_rows, d_owner = ctx.alloc(4 * N_MP), ctx.alloc(4 * N_MP)
    q = lambda a: [round(1e3 * float(np.percentile(a, p)), 3) for p in (10, 50, 90)]
    result = {}
    for name, n_q, base_ms, base_sum in (("keyframe", 11, key_ms, key_sum), ("whole_map", N_KF, map_ms, map_sum)):
        queries, times = chain_queries(n_q), []
        for rep in range(args.reps + 2):                      # two warm-up rounds
            t0 = time.perf_counter()
            n_nb = table.covisibility_device(queries, N_MP, None, d_count, d_nb)
            if rep >= 2:
                times.append(time.perf_counter() - t0)
        packed = d_nb.download(np.int32, (n_q, N_KF))
        got = sum(int(packed[i, :n_nb[i]].sum()) + int(n_nb[i]) for i in range(n_q))
        result[name] = dict(queries=n_q, device_ms_p10_p50_p90=q(times), baseline_ms=base_ms, neighbours=int(n_nb.sum()), outputs_equal=got == base_sum)
    kfs, times = np.arange(N_KF, dtype=np.int32), []
    for rep in range(args.reps + 2):
        t0 = time.perf_counter()
        n_rows = table.map_point_union_device(kfs, [(0, N_KF, -1, 0)], N_MP, None, d_rows, d_owner)
        if rep >= 2:
            times.append(time.perf_counter() - t0)
    n = int(n_rows[0])
    rows, owner = d_rows.download(np.int32, (N_MP,))[:n].astype(np.int64), d_owner.download(np.int32, (N_MP,))[:n].astype(np.int64)
    result["loop"] = dict(slots=N_KF, device_ms_p10_p50_p90=q(times), baseline_ms=union_ms, rows=n, outputs_equal=int((rows * 31 + owner).sum()) == union_sum)
    print(json.dumps(dict(probe="covis", reps=args.reps, slots=N_KF, stride=STRIDE, map_points=N_MP, min_covis=MIN_COVIS, **result)))
    ctx.close()


if __name__ == "__main__":
    main()
