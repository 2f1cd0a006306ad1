"""Times ms_frame_admit, the arrival of a frame of tracker features on the device map tables, against the path it replaces.

  shapes  per_frame  58 slots x 1 024, the bench's per-frame shape, and a frame of 500 tracker features
          large      1 000 slots x 2 048 and a frame of 2 000 tracker features
          each `plain` (no keep, no mask, no depth image) and `rasters` (keep drops 3 %, a 640 x 480 valid mask drops a border and a blob,
          a 640 x 480 depth image fills the 40 % of the depths the tracker does not have)
  device  ms_frame_admit through the Python binding (frame_admit_device): one upload block, two launches, one download.
  before  the same frame without it: the host compaction and depth fill in numpy, then the uploads of the cleared kf_mp row, the four
          keypoint rows and the pose (KeyframeTable.update, KeypointTable.update, KeyframePoseTable.update: six synchronous uploads).

The host clock around each synchronous path; three warm-up calls, then the best and the mean of --reps calls, the two paths alternating; the
slot is put back outside the timed span.  Both paths must leave the same table bytes and the same kp_track: the probe ends without a result
otherwise.  Prints one JSON line.
python tools/frame_admit_probe.py [--reps 20]"""
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
import frame_admit_ref as R           # noqa: E402
import mi355slam                      # noqa: E402

F = np.float32
W, H = 640, 480
SHAPES = dict(per_frame=dict(n_kf=58, stride=1024, n=500), large=dict(n_kf=1000, stride=2048, n=2000))
POSE = np.arange(12, dtype=np.float64) * 0.125 - 0.5


def make_frame(n, rasters, seed=7):
    rng = np.random.default_rng(seed)
    feat = dict(x=rng.uniform(-2, W + 1, n).astype(F), y=rng.uniform(-2, H + 1, n).astype(F), id=(rng.permutation(4 * n)[:n] + 5000).astype(np.int32),
                depth=rng.uniform(0.5, 12, n).astype(F), keep=None)
    feat["depth"][rng.random(n) < 0.4] = -1
    if not rasters:
        return feat, None, None
    feat["keep"] = (rng.random(n) > 0.03).astype(np.uint8)
    mask = np.zeros((H, W), np.uint8)
    mask[8:H - 8, 8:W - 8] = 1
    mask[200:260, 300:380] = 0
    return feat, rng.uniform(0.3, 15, (H, W)).astype(F), mask


def put(ctx, buf, offset, arr):
    arr = np.ascontiguousarray(arr)
    ctx.check(mi355slam.lib().ms_dev_upload(ctx._h, C.c_void_p(buf.ptr + offset), mi355slam._vp(arr), C.c_size_t(arr.nbytes)), "ms_dev_upload")


def probe(ctx, name, shape, rasters, reps):
    n_kf, stride, n = shape["n_kf"], shape["stride"], shape["n"]
    slot, n_mp = n_kf - 1, 2000
    feat, image, mask = make_frame(n, rasters)
    t = R.empty_tables(n_kf, stride, seed=3)
    i = np.arange(400, dtype=np.int32)
    t["kf_mp"][slot, :400] = np.where(i % 3 == 0, -1, n_mp + i)     # what an earlier frame in the slot left: cleared entries and entries beyond the map
    kt = mi355slam.KeyframeTable(ctx, t["kf_mp"])
    kp = mi355slam.KeypointTable(ctx, t["kp_x"], t["kp_y"], t["kp_octave"], t["kp_depth"])
    poses = mi355slam.KeyframePoseTable(ctx, t["kf_pose"])
    tables = dict(kf_mp=kt.kf_mp, kp_x=kp.x, kp_y=kp.y, kp_octave=kp.octave, kp_depth=kp.depth, kf_pose=poses.pose)
    d_image, d_mask = (ctx.upload(image), ctx.upload(mask)) if rasters else (None, None)
    args = dict(slot=slot, pose=POSE)
    if rasters:
        args.update(depth_image=d_image, depth_width=W, depth_height=H, valid_mask=d_mask, mask_width=W, mask_height=H)

    def restore():
        put(ctx, kt.kf_mp, 4 * stride * slot, t["kf_mp"][slot])
        for k in ("x", "y", "octave", "depth"):
            put(ctx, getattr(kp, k), 4 * stride * slot, t["kp_" + k][slot])
        put(ctx, poses.pose, 96 * slot, t["kf_pose"][slot])
        ctx.sync()

    def device():
        rc, res = mi355slam.frame_admit_device(ctx, tables, n_kf, stride, n_mp, feat, args)
        ctx.check(rc, "ms_frame_admit")
        return res["kp_track"]

    rows = {k: t["kp_" + k][slot] for k in ("x", "y", "octave", "depth")}

    def before():
        kept, _, _ = R.kept_mask(feat, mask)                 # the host walk: compaction and depth fill
        idx = np.flatnonzero(kept)
        m = len(idx)
        depth, _ = R.depth_of(feat["x"][idx], feat["y"][idx], feat["depth"][idx], image)
        row = {k: v.copy() for k, v in rows.items()}
        row["x"][:m], row["y"][:m], row["octave"][:m], row["depth"][:m] = feat["x"][idx], feat["y"][idx], 0, depth
        kt.update(slot, [])                                  # the cleared row
        kp.update(slot, **row)                               # four keypoint rows
        poses.update(slot, 1, POSE)
        return feat["id"][idx]

    def state():
        shape2 = (n_kf, stride)
        return [kt.download(), kp.x.download(F, shape2), kp.y.download(F, shape2), kp.octave.download(np.int32, shape2), kp.depth.download(F, shape2), poses.download()]

    try:
        times = dict(device=[], before=[])
        states, tracks = {}, {}
        for i in range(3 + reps):
            for path, fn in (("device", device), ("before", before)):
                restore()
                t0 = time.perf_counter()
                out = fn()
                dt = time.perf_counter() - t0
                if i >= 3:
                    times[path].append(dt)
                if i == 0 or i == 2 + reps:
                    states[path, i], tracks[path, i] = state(), out
        same = lambda a, b: a.dtype == b.dtype and a.tobytes() == b.tobytes()
        rc, want_t, want = R.frame_admit(t, n_mp, feat, slot, POSE, image, mask)
        want_state = [want_t[k] for k in R.TABLES]
        equal = rc == 0 and all(all(same(a, b) for a, b in zip(s, want_state)) for s in states.values()) and all(same(np.asarray(v, np.int32), want["kp_track"]) for v in tracks.values())
        if not equal:
            raise SystemExit("frame_admit_probe: the two paths do not leave the same bytes on %s (rasters %s): no result" % (name, rasters))
        stat = lambda v: dict(best_ms=round(min(v) * 1e3, 4), mean_ms=round(sum(v) / len(v) * 1e3, 4))
        return dict(shape=name, rasters=bool(rasters), n_kf=n_kf, stride=stride, n_tracks=n, n_kp=int(want["counts"][0]), dropped_by_keep=int(want["counts"][1]),
                    dropped_by_mask=int(want["counts"][2]), depths_from_image=int(want["counts"][3]), frame_admit=stat(times["device"]), before=stat(times["before"]),
                    equal_bits=True)
    finally:
        for b in [kt.kf_mp, poses.pose] + ([d_image, d_mask] if rasters else []):
            b.free()
        kp.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ctx = mi355slam.Context(0)
    try:
        runs = [probe(ctx, name, shape, rasters, a.reps) for name, shape in SHAPES.items() for rasters in (False, True)]
        print(json.dumps(dict(probe="frame_admit", reps=a.reps, shapes=runs)))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
