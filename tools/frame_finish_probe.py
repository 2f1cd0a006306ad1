"""Times ms_frame_finish, the end of every frame on the device map tables, against the path it replaces.

  shapes  per_frame  58 slots x 1 024 on 2 000 rows, the bench's per-frame shape: 57 keyframes of 350 map points each and a frame of 500
                     keypoints, 380 of them bound (300 to rows the keyframes see, 80 to rows of its own)
          large      1 000 slots x 2 048 on 200 000 rows: 999 keyframes of 1 500 map points and a frame of 2 000 keypoints
  device  ms_frame_finish: the cloud alone (n_remove = 0), the removal alone (cloud_slot = -1), and both in one call -- synchronous calls
          through the Python binding, timed with the host clock.
  before  what an application had to do without it: for the cloud, the downloads of the slot's kf_mp row, the flags, the live bytes, the
          tracks and the positions and a numpy gather on the host; for the removal, ms_map_cull with the frame as its single candidate
          (cull_points = 0, min_obs_for_ba = 0, a huge finite ratio).

Three warm-up calls, the tables restored outside the timed span, the best and the mean of --reps calls.  The outputs of both paths are
compared for equal bits (ms_map_cull reports its removed rows in row order: the sets are compared).  Prints one JSON line.
python tools/frame_finish_probe.py [--reps 20]"""
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
import frame_finish_ref as R          # noqa: E402
import mi355slam                      # noqa: E402

SHAPES = dict(per_frame=dict(n_kf=58, stride=1024, n_mp=2000, per_kf=350, n_kp=500, shared=300, own=80),
              large=dict(n_kf=1000, stride=2048, n_mp=200000, per_kf=1500, n_kp=2000, shared=1200, own=400))


def make_scene(n_kf, stride, n_mp, per_kf, n_kp, shared, own, seed=7):
    """The frame sits in the last slot; the last `own` rows are seen by it alone."""
    rng = np.random.default_rng(seed)
    kf_mp = np.full((n_kf, stride), -1, np.int32)
    for s in range(n_kf - 1):
        kf_mp[s, :per_kf] = rng.choice(n_mp - own, per_kf, replace=False)
    entries = np.full(n_kp, -1, np.int64)
    at = rng.permutation(n_kp)
    entries[at[:shared]] = rng.choice(n_mp - own, shared, replace=False)
    entries[at[shared:shared + own]] = n_mp - own + np.arange(own)
    kf_mp[-1, :n_kp] = entries
    t = dict(kf_mp=kf_mp, kf_id=np.arange(n_kf, dtype=np.int32) + 3, mp_flags=(rng.random(n_mp) < 0.7).astype(np.uint8) * 3, mp_live=np.ones(n_mp, np.uint8),
             mp_pos=rng.standard_normal((n_mp, 3)), mp_track=rng.permutation(n_mp).astype(np.int32), n_obs=np.zeros(n_mp, np.int32))
    return t


def clock(fn, reps, before):
    best, total, out = float("inf"), 0.0, None
    for i in range(3 + reps):
        before()
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        if i >= 3:
            best, total = min(best, dt), total + dt
    return dict(best_ms=round(best * 1e3, 4), mean_ms=round(total / reps * 1e3, 4)), out


def put(ctx, buf, arr):
    arr = np.ascontiguousarray(arr)
    ctx.check(mi355slam.lib().ms_dev_upload(ctx._h, C.c_void_p(buf.ptr), mi355slam._vp(arr), C.c_size_t(arr.nbytes)), "ms_dev_upload")


def probe(ctx, name, shape, reps):
    t = make_scene(**shape)
    n_kf, stride, n_mp, n_kp, frame = shape["n_kf"], shape["stride"], shape["n_mp"], shape["n_kp"], shape["n_kf"] - 1
    kt = mi355slam.KeyframeTable(ctx, t["kf_mp"])
    flags, live, tracks, n_obs = ctx.upload(t["mp_flags"]), ctx.upload(t["mp_live"]), ctx.upload(t["mp_track"]), ctx.upload(t["n_obs"])
    table = mi355slam.MapPointTable(ctx, t["mp_pos"], np.zeros((n_mp, 3), np.float32), np.zeros(n_mp, np.float32), np.zeros(n_mp, np.float32), np.zeros((n_mp, 8), np.uint32))
    d_rows = ctx.alloc(4 * n_mp)

    def restore():
        put(ctx, kt.kf_mp, t["kf_mp"]); put(ctx, flags, t["mp_flags"]); put(ctx, live, t["mp_live"]); put(ctx, n_obs, t["n_obs"])
        ctx.sync()

    finish = lambda remove, slot: kt.frame_finish(flags, live, table, tracks, n_obs, t["kf_id"], remove, slot, n_kp)

    def host_cloud():
        row = kt.download_slot(frame)[:n_kp]
        f, l, pos = flags.download(np.uint8, (n_mp,)), live.download(np.uint8, (n_mp,)), table.pos.download(np.float64, (n_mp, 3))
        trk = tracks.download(np.int32, (n_mp,))
        ok = (row >= 0) & (row < n_mp)
        r = np.where(ok, row, 0)
        kept = ok & (l[r] != 0) & ((f[r] & 1) != 0)
        rows = row[kept]
        return dict(cloud_row=rows, cloud_kp=np.nonzero(kept)[0].astype(np.int32), cloud_track=trk[rows], cloud_pos=pos[rows])

    settings = dict(current_slot=0, cull_points=0, min_age=0.0, min_obs_for_ba=0, max_critical_ratio=1e300, ratio_float32=0)
    kf_t = np.arange(n_kf, dtype=np.float64)
    cull = lambda: kt.cull_device(flags, live, n_mp, t["kf_id"], kf_t, [frame], None, settings, n_obs, d_rows, None)
    state = lambda: (kt.download(), flags.download(np.uint8, (n_mp,)), live.download(np.uint8, (n_mp,)))
    try:
        want = R.finish(t, [frame], frame, n_kp)
        out = dict(shape=name, n_kf=n_kf, stride=stride, n_mp=n_mp, n_kp=n_kp, cloud=int(want["counts"][0]), removed_rows=int(want["counts"][1]), erased=int(want["counts"][2]))
        out["finish_cloud"], got_cloud = clock(lambda: finish([], frame), reps, restore)
        out["host_cloud"], host = clock(host_cloud, reps, restore)
        out["finish_remove"], got_remove = clock(lambda: finish([frame], -1), reps, restore)
        after_finish = state()
        out["cull_remove"], culled = clock(cull, reps, restore)
        after_cull = state()
        cull_rows = d_rows.download(np.int32, (culled[1],)) if culled[1] else np.zeros(0, np.int32)
        out["finish_both"], got = clock(lambda: finish([frame], frame), reps, restore)
        same = lambda a, b: a.dtype == b.dtype and a.tobytes() == b.tobytes()
        cloud_keys = ("cloud_row", "cloud_kp", "cloud_track", "cloud_pos")
        out["equal_bits"] = bool(all(same(got_cloud[k], host[k]) and same(got[k], want[k]) and same(got_cloud[k], want[k]) for k in cloud_keys)
                                 and all(same(a, b) for a, b in zip(after_finish, after_cull)) and same(got_remove["removed_rows"], want["removed_rows"])
                                 and same(got["removed_rows"], want["removed_rows"]) and sorted(cull_rows.tolist()) == sorted(want["removed_rows"].tolist())
                                 and culled[0].tolist() == [1] and all(same(a, want[k]) for a, k in zip(state(), ("kf_mp", "mp_flags", "mp_live"))))
        return out
    finally:
        for b in (kt.kf_mp, flags, live, tracks, n_obs, d_rows, table.pos, table.norm, table.min_dist, table.max_dist, table.desc):
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ctx = mi355slam.Context(0)
    try:
        print(json.dumps(dict(probe="frame_finish", reps=args.reps, shapes=[probe(ctx, name, shape, args.reps) for name, shape in SHAPES.items()])))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
