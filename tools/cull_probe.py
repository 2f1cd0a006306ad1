"""Times the observation counts and the culling step on the device against the reference's loops on one host core, on the shape of DESIGN
9.6: one map of 1000 keyframe slots x 2000 entries, 200 000 map-point rows, 20 candidate keyframes.

  count     ms_observation_count: n_obs, first_slot and last_slot of every row
  cull      ms_map_cull: cullMapPoints + cullKeyframes (mapper_helpers.cpp:1095-1096), tables updated in place

  device    the synchronous calls with tables and outputs on the device, timed with the host clock: they include the upload of the slot order
            (and of kf_t and the candidates) and, for cull, the download of cand_removed and the two counts.  The tables are restored between
            repetitions outside the timed span.  Nothing here is a kernel trace.
  baseline  tests/map_cull_smoke.cpp --baseline: the std::map restatement of the reference on one core (best of three): building
            MapPoint::observations of every row from the keyframes (what the host keeps today to answer both questions), and the two passes

Both paths run on the same map (the baseline writes it to a temporary file) and the probe compares a checksum of every result.
Prints one JSON line.  python tools/cull_probe.py [--reps 20]"""
import argparse
import ctypes as C
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
import test_map_cull_abi              # noqa: E402

N_KF, STRIDE, N_MP, N_CAND = 1000, 2000, 200000, 20
SETTINGS = dict(current_slot=N_KF - 1, cull_points=1, min_age=12.0, min_obs_for_ba=2, max_critical_ratio=0.3, ratio_float32=0)      # smoke_settings()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    exe = test_map_cull_abi.build_smoke()
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "map.bin")
        out = subprocess.check_output([exe, "--baseline", str(N_KF), str(STRIDE), str(N_MP), str(N_CAND), dump], text=True)
        raw = np.fromfile(dump, np.uint8)
    m = re.search(r"count_ms (\S+) count_sum (\d+) cull_ms (\S+) rows_sum (\d+) keyframes_sum (\d+)", out)
    count_ms, count_sum, cull_ms, rows_sum, kfs_sum = float(m.group(1)), int(m.group(2)), float(m.group(3)), int(m.group(4)), int(m.group(5))
    at = 0

    def take(dtype, n):
        nonlocal at
        a = raw[at:at + n * np.dtype(dtype).itemsize].view(dtype).copy()
        at += a.nbytes
        return a
    kf_mp = take(np.int32, N_KF * STRIDE).reshape(N_KF, STRIDE)
    flags, live, kf_id, kf_t, cand = take(np.uint8, N_MP), take(np.uint8, N_MP), take(np.int32, N_KF), take(np.float64, N_KF), take(np.int32, N_CAND)
    assert at == len(raw)
    ctx = mi355slam.Context(0)
    table = mi355slam.KeyframeTable(ctx, kf_mp)
    d_flags, d_live = ctx.upload(flags), ctx.upload(live)
    d_n, d_first, d_last, d_rows, d_why = (ctx.alloc(4 * N_MP) for _ in range(5))
    q = lambda a: [round(1e3 * float(np.percentile(a, p)), 3) for p in (10, 50, 90)]
    upload = lambda buf, a: ctx.check(mi355slam.lib().ms_dev_upload(ctx._h, C.c_void_p(buf.ptr), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes)), "ms_dev_upload")
    times = []
    for rep in range(args.reps + 2):                          # two warm-up rounds
        t0 = time.perf_counter()
        ctx.check(mi355slam.lib().ms_observation_count(ctx._h, C.c_void_p(table.kf_mp.ptr), N_KF, STRIDE, N_MP, C.c_void_p(kf_id.ctypes.data), C.c_void_p(d_n.ptr),
                                                       C.c_void_p(d_first.ptr), C.c_void_p(d_last.ptr)), "ms_observation_count")
        if rep >= 2:
            times.append(time.perf_counter() - t0)
    n_obs, first = d_n.download(np.int32, (N_MP,)).astype(np.int64), d_first.download(np.int32, (N_MP,)).astype(np.int64)
    result = dict(count=dict(device_ms_p10_p50_p90=q(times), baseline_ms=count_ms, observations=int(n_obs.sum()),
                             outputs_equal=int((n_obs * 7 + first + 1).sum()) == count_sum))
    times = []
    for rep in range(args.reps + 2):
        upload(table.kf_mp, kf_mp); upload(d_flags, flags); upload(d_live, live)
        ctx.sync()
        t0 = time.perf_counter()
        removed, n_rows, n_kfs = table.cull_device(d_flags, d_live, N_MP, kf_id, kf_t, cand, None, SETTINGS, d_n, d_rows, d_why)
        if rep >= 2:
            times.append(time.perf_counter() - t0)
    rows, why = d_rows.download(np.int32, (N_MP,))[:n_rows].astype(np.int64), d_why.download(np.uint8, (N_MP,))[:n_rows].astype(np.int64)
    got_kfs = int((cand[removed != 0].astype(np.int64) + 1).sum())
    result["cull"] = dict(candidates=N_CAND, device_ms_p10_p50_p90=q(times), baseline_ms=cull_ms, removed_rows=int(n_rows), removed_keyframes=int(n_kfs),
                          outputs_equal=int((rows * 31 + why).sum()) == rows_sum and got_kfs == kfs_sum)
    print(json.dumps(dict(probe="cull", reps=args.reps, slots=N_KF, stride=STRIDE, map_points=N_MP, **result)))
    ctx.close()


if __name__ == "__main__":
    main()
