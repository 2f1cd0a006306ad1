"""Times the map-point update of a keyframe with the observation lists built on the device against the host path it replaces, on the map of
tools/cull_probe.py (1000 keyframe slots x 2000 entries, 200 000 map-point rows), for two selections:

  slot      the usable map points of the newest keyframe (mapper_helpers.cpp:1062-1092; MS_OBS_FROM_SLOT, MS_OBS_REFRESH)
  whole     every observed row of the map (a whole-map pass of correctLoop; MS_OBS_FROM_ROWS over all rows, drop_empty)

  device    ms_observation_lists + ms_map_refresh_lists (descriptors, promote_min_obs = 3) + ms_triangulate_lists (TME), the three synchronous
            calls timed with the host clock one by one and together: they include the upload of the slot order, the descriptor bases, the
            cameras and the level tables, the download of the counts, of the longest descriptor list and of the per-row results.  No list
            crosses the bus.  Positions and flags are restored between repetitions outside the timed span.  Nothing here is a kernel trace.
  baseline  tests/obs_lists_smoke.cpp --baseline on one core (best of three): building std::map<KfId, KpId> observations of every map point
            from the keyframes (`build`, what the host keeps today) and walking them into the CSR lists of the selection (`walk`); plus the
            existing host-list calls ms_map_refresh + ms_triangulate on those lists, timed here the same way (they upload the lists).

Both paths run on the same map; the probe compares a checksum of the lists (device against the std::map restatement) and the tables after the
device path against the tables after the host-list path, byte for byte.  Prints one JSON line.  python tools/obs_lists_probe.py [--reps 10]"""
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
import obs_lists_ref as R             # noqa: E402
import test_map_cull_abi              # noqa: E402
import test_obs_lists_smoke           # noqa: E402

N_KF, STRIDE, N_MP, N_CAND, N_LEVELS = 1000, 2000, 200000, 20, 8
SLOT = N_KF - 1


def checksum(rows, kf, kp):
    """Csr::sum of tests/obs_lists_smoke.cpp: order-sensitive, wrapping in 64 bits."""
    with np.errstate(over="ignore"):
        a = (np.arange(1, len(rows) + 1, dtype=np.uint64) * (rows.astype(np.uint64) + np.uint64(1))).sum(dtype=np.uint64)
        b = (np.arange(1, len(kf) + 1, dtype=np.uint64) * (kf.astype(np.uint64) * np.uint64(8192) + kp.astype(np.uint64) + np.uint64(1))).sum(dtype=np.uint64)
        return int(a + b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "map.bin")
        subprocess.check_output([test_map_cull_abi.build_smoke(), "--baseline", str(N_KF), str(STRIDE), str(N_MP), str(N_CAND), dump], text=True)
        raw = np.fromfile(dump, np.uint8)
        out = subprocess.check_output([test_obs_lists_smoke.build_smoke(), "--baseline", dump, str(N_KF), str(STRIDE), str(N_MP), str(SLOT)], text=True)
    base = {k: float(v) if "ms" in k else int(v) for k, v in re.findall(r"(\w+) ([\d.]+)", out)}
    kf_mp = raw[:4 * N_KF * STRIDE].view(np.int32).reshape(N_KF, STRIDE).copy()
    flags = raw[4 * N_KF * STRIDE:][:N_MP].copy()
    kf_id = raw[4 * N_KF * STRIDE + 2 * N_MP:][:4 * N_KF].view(np.int32).copy()

    # geometry for the map: keyframe k looks down +z from (0.3 k, 0, 0) (the chain of the cull map); a row lies in front of the middle of
    # the run of keyframes that observe it, and its keypoints are its projections with a little noise
    rng = np.random.default_rng(17)
    start, slots, js = R.transpose(kf_mp, N_MP, kf_id)
    n_obs_all = np.diff(start)
    mid = np.zeros(N_MP)
    seen = n_obs_all > 0
    mid[seen] = np.add.reduceat(slots.astype(np.float64), start[:-1][seen]) / n_obs_all[seen]
    pos = np.stack([0.3 * mid + rng.uniform(-1, 1, N_MP), rng.uniform(-1.5, 1.5, N_MP), rng.uniform(5, 12, N_MP)], axis=1)
    poses = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64), (N_KF, 1))
    poses[:, 3] = -0.3 * np.arange(N_KF)
    cams = np.tile(np.array([500.0, 500.0, 320.0, 240.0, 640, 480]), (N_KF, 1))
    focal = np.full(N_KF, 500, np.int32)
    ok = (kf_mp >= 0) & (kf_mp < N_MP)
    X = pos[np.where(ok, kf_mp, 0)]
    kp = dict(x=(500.0 * (X[..., 0] - 0.3 * np.arange(N_KF)[:, None]) / X[..., 2] + 320.0 + rng.normal(0, 0.3, kf_mp.shape)).astype(np.float32),
              y=(500.0 * X[..., 1] / X[..., 2] + 240.0 + rng.normal(0, 0.3, kf_mp.shape)).astype(np.float32),
              octave=rng.integers(0, N_LEVELS, kf_mp.shape).astype(np.int32), depth=np.full(kf_mp.shape, -1.0, np.float32))
    del X
    desc_base = (np.arange(N_KF) * STRIDE).astype(np.int32)
    pool_host = rng.integers(0, 2 ** 32, (N_KF * STRIDE, 8), dtype=np.uint64).astype(np.uint32)
    sf, sigma = mi355slam.scale_factors(N_LEVELS, 1.2), mi355slam.level_sigma_sq(N_LEVELS, 1.2)
    S = dict(level_sigma_sq=sigma, min_angle_two_obs=1.0, min_angle_multiple_obs=3.0, rel_reprojection_threshold=0.004, dense_stereo_depth=False)

    ctx = mi355slam.Context(0)
    table, kpt = mi355slam.KeyframeTable(ctx, kf_mp), mi355slam.KeypointTable(ctx, **kp)
    mpt = mi355slam.MapPointTable(ctx, pos, np.zeros((N_MP, 3), np.float32), np.ones(N_MP, np.float32), np.ones(N_MP, np.float32), np.zeros((N_MP, 8), np.uint32))
    posed = mi355slam.KeyframePoseTable(ctx, poses)
    pool, d_flags = ctx.upload(pool_host), ctx.upload(flags)
    d_all = ctx.upload(np.arange(N_MP, dtype=np.int32))
    upload = lambda buf, a: ctx.check(mi355slam.lib().ms_dev_upload(ctx._h, C.c_void_p(buf.ptr), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes)), "ms_dev_upload")
    q = lambda a: [round(1e3 * float(np.percentile(a, p)), 3) for p in (10, 50, 90)]

    def restore():
        upload(mpt.pos, pos); upload(d_flags, flags)
        ctx.sync()

    def state():
        return b"".join(b.download(np.uint8, (n,)).tobytes() for b, n in ((mpt.pos, 24 * N_MP), (mpt.norm, 12 * N_MP), (mpt.min_dist, 4 * N_MP), (mpt.max_dist, 4 * N_MP),
                                                                         (mpt.desc, 32 * N_MP), (d_flags, N_MP)))

    result = {}
    selections = (("slot", dict(source=R.FROM_SLOT, filter=R.REFRESH, drop_empty=1, slot=SLOT), R.select(R.FROM_SLOT, R.REFRESH, 1, SLOT)),
                  ("whole", dict(source=R.FROM_ROWS, filter=R.ALL, drop_empty=1, rows_in=d_all, n_in=N_MP), R.select(R.FROM_ROWS, R.ALL, 1, rows_in=np.arange(N_MP))))
    for name, sel, ref_sel in selections:
        want = R.observation_lists(kf_mp, N_MP, kf_id, flags, kp, desc_base, ref_sel, N_LEVELS, (start, slots, js))
        lists = mi355slam.ObservationLists(ctx, want["n_rows"], want["n_obs"])
        t_lists, t_refresh, t_tri, t_all = [], [], [], []
        for rep in range(args.reps + 2):                      # two warm-up rounds
            restore()
            t0 = time.perf_counter()
            rc, n_rows, n_obs = table.observation_lists_device(lists, kf_id, N_MP, sel, kpt, desc_base, d_flags, N_LEVELS)
            ctx.check(rc, "ms_observation_lists")
            t1 = time.perf_counter()
            mpt.refresh_lists(posed, lists, n_rows, n_obs, sf, pool, 3, d_flags, want_medoid=False)
            t2 = time.perf_counter()
            mpt.triangulate_lists(posed, cams, focal, lists, n_rows, n_obs, S, mi355slam.TRI_TME, flags=d_flags)
            t3 = time.perf_counter()
            if rep >= 2:
                t_lists.append(t1 - t0); t_refresh.append(t2 - t1); t_tri.append(t3 - t2); t_all.append(t3 - t0)
        got = lists.download(n_rows, n_obs, ("rows", "obs_kf", "obs_kp"))
        device_state = state()
        # the host-list path on the same lists (from the restatement): the calls the std::map walk feeds today
        prob = {k: want[k] for k in ("rows", "obs_start", "obs_kf", "obs_desc", "first_octave", "was_triangulated", "obs_x", "obs_y", "obs_octave", "obs_depth")}
        h_refresh, h_tri = [], []
        for rep in range(3):
            restore()
            t0 = time.perf_counter()
            mi355slam.map_refresh(ctx, mpt, posed, prob, sf, pool)
            t1 = time.perf_counter()
            promoted = flags.copy()                           # the promotion of :1072-1076 on the host, outside the timed spans
            promoted[want["rows"]] = np.where(want["n_obs_row"] >= 3, 3, 2)
            upload(d_flags, promoted)
            ctx.sync()
            t2 = time.perf_counter()
            mpt.triangulate(posed, cams, focal, dict(prob, was_triangulated=np.ones(len(want["rows"]), np.uint8)), S, mi355slam.TRI_TME, flags=d_flags)
            t3 = time.perf_counter()
            h_refresh.append(t1 - t0); h_tri.append(t3 - t2)
        result[name] = dict(rows=int(n_rows), observations=int(n_obs), device_lists_ms_p10_p50_p90=q(t_lists), device_refresh_ms_p10_p50_p90=q(t_refresh),
                            device_triangulate_ms_p10_p50_p90=q(t_tri), device_total_ms_p10_p50_p90=q(t_all), baseline_build_ms=base["build_ms"],
                            baseline_walk_ms=base[name + "_walk_ms"], host_list_refresh_ms=round(1e3 * min(h_refresh), 3), host_list_triangulate_ms=round(1e3 * min(h_tri), 3),
                            lists_equal=(n_rows, n_obs) == (base[name + "_rows"], base[name + "_obs"]) and
                            checksum(got["rows"], got["obs_kf"], got["obs_kp"]) == base[name + "_sum"],
                            tables_equal=device_state == state())
        lists.free()
    print(json.dumps(dict(probe="obs_lists", reps=args.reps, slots=N_KF, stride=STRIDE, map_points=N_MP, **result)))
    ctx.close()


if __name__ == "__main__":
    main()
