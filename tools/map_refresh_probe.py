"""Times the two writers of the device map-point table against what a caller had before them, for two shapes:

  keyframe  mapper_helpers.cpp:1062-1077: 2000 rows, 8 observations on average (1-15), 400 keyframes
  loop      loop_closer.cpp:398-506: 1000 corrected keyframes, 200 000 moved points, each refreshed from 8 observations on average

  device    ms_map_refresh (keyframe) / ms_loop_correct + ms_map_refresh (loop), synchronous calls timed with the host clock; the lists are
            built before the timed region, as a mapper that keeps them next to its observation maps would have them
  baseline  tests/map_refresh_smoke.cpp --baseline: the same arithmetic on one core of the host, then DeviceMapPoints::update of the rows
            one by one (keyframe shape) or of the whole table in one call (both shapes)

Prints one JSON line.  python tools/map_refresh_probe.py [--reps 20]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-module_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import map_refresh_ref as R           # noqa: E402
import mi355slam                      # noqa: E402
import test_map_refresh_abi           # noqa: E402


def make(rng, n_kf, n_rows, mean_obs, n_corr):
    n_mp, n_pool = n_rows + n_rows // 4, 4 * n_rows
    kf_pose = np.stack([R.random_pose(rng) for _ in range(n_kf)])
    table = dict(pos=rng.uniform(-8, 8, (n_mp, 3)), norm=np.zeros((n_mp, 3), np.float32), min_dist=np.zeros(n_mp, np.float32), max_dist=np.zeros(n_mp, np.float32),
                 desc=np.zeros((n_mp, 8), np.uint32))
    pool = rng.integers(0, 2 ** 32, (n_pool, 8), dtype=np.uint64).astype(np.uint32)
    lengths = rng.integers(1, 2 * mean_obs, n_rows)
    start = np.zeros(n_rows + 1, np.int32); start[1:] = np.cumsum(lengths)
    n_obs = int(start[-1])
    rows = rng.permutation(n_mp)[:n_rows].astype(np.int32)
    refresh = dict(rows=rows, obs_start=start, obs_kf=rng.integers(0, n_kf, n_obs).astype(np.int32), obs_desc=rng.integers(0, n_pool, n_obs).astype(np.int32),
                   first_octave=rng.integers(0, 8, n_rows).astype(np.int32))
    loop = None
    if n_corr:
        rigid = np.zeros(n_corr, np.uint8); rigid[:n_corr // 4] = 1
        loop = dict(kf_slot=rng.permutation(n_kf)[:n_corr].astype(np.int32), kf_rigid=rigid, kf_lambda=rng.uniform(0, 1, n_corr), mp_row=rows,
                    mp_ref=rng.integers(0, n_corr, n_rows).astype(np.int32))
    return kf_pose, table, pool, refresh, loop, n_obs


def baseline(n_kf, n_rows, mean_obs):
    out = subprocess.check_output([test_map_refresh_abi.build_smoke(), "--baseline", str(n_kf), str(n_rows), str(mean_obs)], text=True)
    m = re.search(r"arithmetic_ms (\S+) update_rows_ms (\S+) update_table_ms (\S+)", out)
    return dict(arithmetic_ms=float(m.group(1)), update_rows_ms=float(m.group(2)), update_table_ms=float(m.group(3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ctx = mi355slam.Context(0)
    rng = np.random.default_rng(3)
    sf = mi355slam.scale_factors(8, 1.2)
    q = lambda a: [round(1e3 * float(np.percentile(a, p)), 3) for p in (10, 50, 90)]
    result = {}
    for name, n_kf, n_rows, n_corr in (("keyframe", 400, 2000, 0), ("loop", 1000, 200000, 1000)):
        kf_pose, t, pool, refresh, loop, n_obs = make(rng, n_kf, n_rows, 8, n_corr)
        table = mi355slam.MapPointTable(ctx, t["pos"], t["norm"], t["min_dist"], t["max_dist"], t["desc"])
        poses, dpool = mi355slam.KeyframePoseTable(ctx, kf_pose), ctx.upload(pool)
        t_loop, t_refresh, t_geom = [], [], []
        for rep in range(args.reps + 2):                      # two warm-up rounds
            t0 = time.perf_counter()
            if loop:
                mi355slam.loop_correct(ctx, table, poses, R.loop_transforms()["usual"], loop)
            t1 = time.perf_counter()
            mi355slam.map_refresh(ctx, table, poses, refresh, sf, dpool)
            t2 = time.perf_counter()
            mi355slam.map_refresh(ctx, table, poses, refresh, sf, None)
            t3 = time.perf_counter()
            if rep >= 2:
                t_loop.append(t1 - t0); t_refresh.append(t2 - t1); t_geom.append(t3 - t2)
        result[name] = dict(rows=n_rows, observations=n_obs, refresh_ms_p10_p50_p90=q(t_refresh), refresh_without_descriptors_ms_p10_p50_p90=q(t_geom),
                            baseline=baseline(n_corr, n_rows, 8))
        if loop:
            result[name]["loop_correct_ms_p10_p50_p90"] = q(t_loop)
    print(json.dumps(dict(probe="map_refresh", reps=args.reps, **result)))
    ctx.close()


if __name__ == "__main__":
    main()
