"""Times ms_map_publish, the viewer map and the point-cloud record on the device map tables, against the parent's path for the
same result.

  shapes  per_frame  58 slots x 1 024 with 2 000 rows, the bench's per-frame map shape
          large      1 000 slots x 2 048 with 200 000 rows
  cases   view             MS_PUBLISH_VIEW alone, with a local list of about 2 000 rows (all rows on per_frame) and every slot's poseWC
          record_same      MS_PUBLISH_RECORD on a record that is current: no event
          record_window    MS_PUBLISH_RECORD after a local window of about 2 000 rows moved (all recorded rows on per_frame)
  device  ms_map_publish through the Python binding (map_publish_device): five launches, two downloads.
  before  the table downloads through the DevBufs of MapPointTable / KeyframeTable / KeyframePoseTable (mp_pos, mp_norm, mp_flags, mp_live,
          n_obs or mp_color, the current slot's row, the poses, the local list), the numpy restatement (tests/map_publish_ref.py) on a host
          copy of the record state, which that path keeps on the host.

The host clock around each synchronous path; three warm-up calls, then the best and the mean of --reps calls, the two paths alternating; the
record state is put back outside the timed span.  Both paths must give the same bytes: the probe ends without a result otherwise.  Prints one
JSON line.
python tools/map_publish_probe.py [--reps 20]"""
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
import map_publish_ref as R           # noqa: E402
import mi355slam                      # noqa: E402

F = np.float32
SHAPES = dict(per_frame=dict(n_kf=58, stride=1024, n_mp=2000), large=dict(n_kf=1000, stride=2048, n_mp=200000))
WINDOW = 2000


def make_map(n_kf, stride, n_mp, seed=5):
    rng = np.random.default_rng(seed)
    t = dict(mp_pos=rng.normal(size=(n_mp, 3)) * 20, mp_norm=rng.normal(size=(n_mp, 3)).astype(F), mp_flags=rng.choice(np.array([0, 2, 3], np.uint8), n_mp, p=(0.1, 0.2, 0.7)),
             mp_live=(rng.random(n_mp) < 0.9).astype(np.uint8), n_obs=rng.integers(1, 9, n_mp).astype(np.int32), mp_color=rng.integers(0, 256, (n_mp, 3)).astype(np.uint8),
             kf_mp=np.where(rng.random((n_kf, stride)) < 0.4, rng.integers(0, n_mp, (n_kf, stride)), -1).astype(np.int32), kf_pose=rng.normal(size=(n_kf, 12)))
    return t


def probe(ctx, name, shape, reps):
    n_kf, stride, n_mp = shape["n_kf"], shape["stride"], shape["n_mp"]
    t = make_map(n_kf, stride, n_mp)
    window = np.sort(np.random.default_rng(6).choice(n_mp, min(WINDOW, n_mp), replace=False)).astype(np.int32)
    current, kf_list = n_kf - 1, np.arange(n_kf, dtype=np.int32)
    table = mi355slam.MapPointTable(ctx, t["mp_pos"], t["mp_norm"], np.zeros(n_mp, F), np.zeros(n_mp, F), np.zeros((n_mp, 8), np.uint32))
    kt = mi355slam.KeyframeTable(ctx, t["kf_mp"])
    poses = mi355slam.KeyframePoseTable(ctx, t["kf_pose"])
    bufs = dict(mp_flags=ctx.upload(t["mp_flags"]), mp_live=ctx.upload(t["mp_live"]), n_obs=ctx.upload(t["n_obs"]), mp_color=ctx.upload(t["mp_color"]),
                local_rows=ctx.upload(window), rec_pos=ctx.alloc(12 * n_mp), rec_state=ctx.alloc(n_mp))
    tables = dict(mp_pos=table.pos, mp_norm=table.norm, kf_mp=kt.kf_mp, kf_pose=poses.pose, **bufs)
    # the record as a first call leaves it, and the map after the window moved
    _, _, rec_pos, rec_state = R.map_publish(t, *R.empty_record(n_mp), R.RECORD)
    moved = t["mp_pos"].copy()
    moved[window] += 0.125

    def put(buf, arr):
        arr = np.ascontiguousarray(arr)
        ctx.check(mi355slam.lib().ms_dev_upload(ctx._h, mi355slam._vp(buf), mi355slam._vp(arr), C.c_size_t(arr.nbytes)), "ms_dev_upload")

    host_rec = {}

    def restore():
        put(bufs["rec_pos"], rec_pos); put(bufs["rec_state"], rec_state)
        host_rec["pos"], host_rec["state"] = rec_pos, rec_state
        ctx.sync()

    def device(what):
        rc, res = mi355slam.map_publish_device(ctx, tables, n_mp, n_kf, stride, len(window) if what & R.VIEW else 0, dict(what=what, current_slot=current if what & R.VIEW else -1),
                                               kf_list if what & R.VIEW else ())
        ctx.check(rc, "ms_map_publish")
        return res

    def before(what):
        d = dict(mp_pos=table.pos.download(np.float64, (n_mp, 3)), mp_norm=table.norm.download(F, (n_mp, 3)), mp_flags=bufs["mp_flags"].download(np.uint8, (n_mp,)),
                 mp_live=bufs["mp_live"].download(np.uint8, (n_mp,)))
        if what & R.VIEW:
            # the current slot's row alone, as row 0 of a table of one slot
            d.update(mp_color=bufs["mp_color"].download(np.uint8, (n_mp, 3)), kf_pose=poses.download(), n_obs=None,
                     kf_mp=mi355slam._download_i32_at(kt.kf_mp, 4 * stride * current, stride).reshape(1, stride))
            rc, out, _, _ = R.map_publish(d, None, None, what, 0, 4, bufs["local_rows"].download(np.int32, (len(window),)), kf_list)
        else:
            d.update(n_obs=bufs["n_obs"].download(np.int32, (n_mp,)), mp_color=None, kf_mp=np.zeros((0, stride), np.int32), kf_pose=np.zeros((0, 12)))
            rc, out, host_rec["pos"], host_rec["state"] = R.map_publish(d, host_rec["pos"], host_rec["state"], what)
        assert rc == 0
        return out

    same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    cases = (("view", R.VIEW, t["mp_pos"]), ("record_same", R.RECORD, t["mp_pos"]), ("record_window", R.RECORD, moved))
    result = dict(shape=name, n_kf=n_kf, stride=stride, n_mp=n_mp, window=len(window))
    try:
        for case, what, mp_pos in cases:
            table.update(0, n_mp, pos=mp_pos)
            times = dict(device=[], before=[])
            for i in range(3 + reps):
                outs = {}
                for path, fn in (("device", device), ("before", before)):
                    restore()
                    t0 = time.perf_counter()
                    outs[path] = fn(what)
                    dt = time.perf_counter() - t0
                    if i >= 3:
                        times[path].append(dt)
                    if path == "device":
                        outs["rec"] = (bufs["rec_pos"].download(F, (n_mp, 3)), bufs["rec_state"].download(np.uint8, (n_mp,)))
                a, b = outs["device"], outs["before"]
                equal = all(same(a[k], np.ascontiguousarray(b[k])) for k in a) and (what == R.VIEW or (same(outs["rec"][0], host_rec["pos"]) and same(outs["rec"][1], host_rec["state"])))
                if not equal:
                    raise SystemExit("map_publish_probe: the two paths do not give the same bytes on %s / %s: no result" % (name, case))
            stat = lambda v: dict(best_ms=round(min(v) * 1e3, 4), mean_ms=round(sum(v) / len(v) * 1e3, 4))
            n_pub, n_ev = int(a["counts"][0]), int(a["counts"][1])
            result[case] = dict(n_pub=n_pub, n_ev=n_ev, bytes_down=32 + (64 * n_kf if what & R.VIEW else 0) + 42 * n_pub + 29 * n_ev,
                                bytes_down_before=int(n_mp * (24 + 12 + 1 + 1) + (n_mp * 3 + 4 * stride + 96 * n_kf + 4 * len(window) if what & R.VIEW else 4 * n_mp)),
                                map_publish=stat(times["device"]), before=stat(times["before"]), equal_bits=True)
        return result
    finally:
        for b in list(bufs.values()) + [kt.kf_mp, poses.pose, table.pos, table.norm, table.min_dist, table.max_dist, table.desc]:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ctx = mi355slam.Context(0)
    try:
        print(json.dumps(dict(probe="map_publish", reps=a.reps, shapes=[probe(ctx, name, shape, a.reps) for name, shape in SHAPES.items()])))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
