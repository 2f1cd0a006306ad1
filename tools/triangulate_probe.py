"""Times ms_triangulate on the device against its restatement on one host core, for three shapes of the corridor scene of
tests/triangulate_ref.py (70 keyframes, MS_TRI_TME, no depths):

  new_points    1 000 points x 8 observations      createNewMapPoints (mapper_helpers.cpp:308)
  local         20 000 points x 8 observations     the non-BA'd points after local BA (:1083-1090)
  loop          100 000 points x 8 observations    the re-triangulation of LoopCloser::correctLoop (loop_closer.cpp:508-523)

  device     MapPointTable.triangulate: the synchronous call, upload and result download included, timed with the host clock; the table
             is reset between repetitions outside the timed region
  baseline   tests/triangulate_ref.py (triangulate), the float64 numpy restatement, once, on one core.  It is an interpreted
             point-by-point loop: the figure says what the specification costs to evaluate, not what a tuned host routine would.

The outputs are compared as the GPU test compares them: status, reason and n_pass equal, failed rows bit-equal, positions within
GPU_POSITION_TOLERANCE.  Prints one JSON line.  python tools/triangulate_probe.py [--reps 20] [--shapes new_points,local,loop]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-module_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import mi355slam                      # noqa: E402
import triangulate_ref as R           # noqa: E402

SHAPES = dict(new_points=1000, local=20000, loop=100000)
KINDS = ("clean",) * 7 + ("noisy", "outlier", "far")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="new_points,local,loop")
    args = ap.parse_args()
    ctx = mi355slam.Context(0)
    S = R.settings()
    q = lambda a: [round(1e3 * float(np.percentile(a, p)), 3) for p in (10, 50, 90)]
    result = {}
    for name in args.shapes.split(","):
        n = SHAPES[name]
        sc = R.make_scene(seed=7 + n, n_points=n, obs_counts=(8,), kinds=KINDS, n_mp=n)
        prob = R.sub_problem(sc["prob"], range(n), with_depth=False)
        table = mi355slam.MapPointTable(ctx, sc["mp_pos"], np.zeros((n, 3), np.float32), np.ones(n, np.float32), np.ones(n, np.float32), np.zeros((n, 8), np.uint32))
        poses = mi355slam.KeyframePoseTable(ctx, sc["poses"])
        flags = ctx.upload(sc["mp_flags"])
        times = []
        for rep in range(args.reps + 2):                      # two warm-up rounds
            table.update(0, n, pos=sc["mp_pos"])
            t0 = time.perf_counter()
            status, reason, n_pass = table.triangulate(poses, sc["cams"], sc["focal"], prob, S, R.TME, flags=flags)
            if rep >= 2:
                times.append(time.perf_counter() - t0)
        pos, got_flags = table.pos.download(np.float64, (n, 3)), flags.download(np.uint8, (n,))
        t0 = time.perf_counter()
        w_pos, w_flags, w_status, w_reason, w_pass = R.triangulate(sc["mp_pos"], sc["mp_flags"], sc["poses"], sc["cams"], sc["focal"], prob, S, R.TME)
        base_ms = 1e3 * (time.perf_counter() - t0)
        failed = np.ones(n, bool)
        failed[prob["rows"][w_status != 0]] = False
        equal = (np.array_equal(status, w_status) and np.array_equal(reason, w_reason) and np.array_equal(n_pass, w_pass) and np.array_equal(got_flags, w_flags)
                 and np.array_equal(pos[failed].view(np.uint64), w_pos[failed].view(np.uint64)))
        diff = R.relative_difference(pos[~failed], w_pos[~failed])
        result[name] = dict(points=n, observations=int(prob["obs_start"][-1]), device_ms_p10_p50_p90=q(times), baseline_ms=round(base_ms, 1),
                            triangulated=int((w_status != 0).sum()), outputs_equal=bool(equal and diff <= R.GPU_POSITION_TOLERANCE), position_rel_diff=diff)
        for b in (table.pos, table.norm, table.min_dist, table.max_dist, table.desc, poses.pose, flags):
            b.free()
    print(json.dumps(dict(probe="triangulate", reps=args.reps, keyframes=R.N_KF, mode="TME", **result)))
    ctx.close()


if __name__ == "__main__":
    main()
