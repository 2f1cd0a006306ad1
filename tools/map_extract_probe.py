"""Times ms_map_extract, the partial map copy for the front end on the device map tables, against the path an application had
without it, and the end of a frame (ms_frame_finish) on the whole map against the same call on the extraction.

  shapes  window  58 slots x 1 024 on 2 000 rows: 57 keyframes of 350 map points each and a frame of 500 keypoints, 380 of them bound
          large   1 000 slots x 2 048 on 200 000 rows: 999 keyframes of 1 500 map points and a frame of 2 000 keypoints (9.18's second shape)
          In both the active set is the frame's slot and the 20 keyframes before it, 21 slots; no descriptor pool.
  device  ms_map_extract into a destination of 21 slots and n_rows + 16 rows: a synchronous call through the Python binding, host clock.
  before  download the active slots' rows of kf_mp, of the keypoint arrays and of the poses (one block each: the slots are adjacent, which
          favours this path), every row table and the track window; the numpy restatement (tests/map_extract_ref.py: bincount, nonzero,
          fancy indexing) on the host; upload a second set of tables.
  finish  ms_frame_finish for the frame (cloud and removal in one call) on the source tables and on the extraction, the tables restored
          outside the timed span.

Three warm-up calls, the best and the mean of --reps calls.  The outputs of both paths are asserted to be equal bit for bit (every destination
array of the call against the host path's, and the clouds of the two ms_frame_finish calls): a difference ends the probe before it prints.
Prints one JSON line.
python tools/map_extract_probe.py [--reps 20]"""
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
import map_extract_ref as R           # noqa: E402
import mi355slam                      # noqa: E402

SHAPES = dict(window=dict(n_kf=58, stride=1024, n_mp=2000, per_kf=350, n_kp=500, shared=300, own=80),
              large=dict(n_kf=1000, stride=2048, n_mp=200000, per_kf=1500, n_kp=2000, shared=1200, own=400))
N_ACTIVE, BASE = 21, 1000
PER_SLOT = ("kf_mp", "kf_pose") + R.KP_FIELDS


def make_scene(n_kf, stride, n_mp, per_kf, n_kp, shared, own, seed=7):
    """tools/frame_finish_probe.py's scene with every table of the map: the frame sits in the last slot; the last `own` rows are seen by it alone."""
    rng = np.random.default_rng(seed)
    kf_mp = np.full((n_kf, stride), -1, np.int32)
    for s in range(n_kf - 1):
        kf_mp[s, :per_kf] = rng.choice(n_mp - own, per_kf, replace=False)
    entries = np.full(n_kp, -1, np.int64)
    at = rng.permutation(n_kp)
    entries[at[:shared]] = rng.choice(n_mp - own, shared, replace=False)
    entries[at[shared:shared + own]] = n_mp - own + np.arange(own)
    kf_mp[-1, :n_kp] = entries
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    track = rng.permutation(n_mp).astype(np.int32)
    track_row = np.zeros(n_mp, np.int32)
    track_row[track] = np.arange(n_mp, dtype=np.int32)
    return dict(kf_mp=kf_mp, kf_id=np.arange(n_kf, dtype=np.int32) + 3, mp_flags=(rng.random(n_mp) < 0.7).astype(np.uint8) * 3, mp_live=np.ones(n_mp, np.uint8),
                mp_pos=rng.standard_normal((n_mp, 3)), mp_norm=f32(n_mp, 3), mp_min_dist=f32(n_mp), mp_max_dist=f32(n_mp), mp_desc=rng.integers(0, 2 ** 32, (n_mp, 8), dtype=np.uint32),
                mp_track=(track + BASE).astype(np.int32), kp_x=f32(n_kf, stride), kp_y=f32(n_kf, stride), kp_octave=rng.integers(0, 8, (n_kf, stride)).astype(np.int32), kp_depth=f32(n_kf, stride),
                kf_pose=rng.standard_normal((n_kf, 12)), track_row=track_row, track_base=BASE, desc_pool=None, desc_base=np.full(n_kf, -1, np.int32), n_kp=np.zeros(n_kf, np.int32))


def clock(fn, reps, before=None):
    best, total, out = float("inf"), 0.0, None
    for i in range(3 + reps):
        if before:
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


def get(ctx, buf, dtype, shape, first_byte=0):
    out = np.empty(shape, dtype)
    ctx.check(mi355slam.lib().ms_dev_download(ctx._h, mi355slam._vp(out), C.c_void_p(buf.ptr + first_byte), C.c_size_t(out.nbytes)), "ms_dev_download")
    return out


def point_table(ctx, bufs, n):
    table = mi355slam.MapPointTable.__new__(mi355slam.MapPointTable)
    table.ctx, table.n = ctx, n
    table.pos, table.norm, table.min_dist, table.max_dist, table.desc = (bufs[k] for k in ("mp_pos", "mp_norm", "mp_min_dist", "mp_max_dist", "mp_desc"))
    return table


def probe(ctx, name, shape, reps):
    t = make_scene(**shape)
    n_kf, stride, n_mp, n_kp, frame = shape["n_kf"], shape["stride"], shape["n_mp"], shape["n_kp"], shape["n_kf"] - 1
    active = list(range(n_kf - N_ACTIVE, n_kf))
    n_rows = int(R.extract(t, active, R.sizes(t, N_ACTIVE, n_mp))["counts"][0])
    z = R.sizes(t, N_ACTIVE, n_rows + 16)
    names = R.dst_names(t)
    shapes = {k: R.dst_shape(k, z) for k in names}
    src = {k: ctx.upload(t[k]) for k in mi355slam.MAP_EXTRACT_SRC if t.get(k) is not None}
    zeros = {k: np.zeros(shapes[k], R.DTYPES[k]) for k in names}
    dst, second = ({k: ctx.upload(zeros[k]) for k in names} for _ in range(2))
    kt = mi355slam.KeyframeTable.__new__(mi355slam.KeyframeTable)
    kt.ctx, kt.kf_mp, kt.n_kf, kt.stride = ctx, src["kf_mp"], n_kf, stride
    kd = mi355slam.KeyframeTable.__new__(mi355slam.KeyframeTable)
    kd.ctx, kd.kf_mp, kd.n_kf, kd.stride = ctx, dst["kf_mp"], N_ACTIVE, stride
    rest = {k: v for k, v in src.items() if k != "kf_mp"}

    def call():
        rc, out = kt.map_extract_device(rest, dst, z, t["kf_id"], active)
        ctx.check(rc, "ms_map_extract")
        return out

    def host_path():
        first = active[0]
        td = dict(t)                                         # the host arrays of the scene stand for nothing below: every table comes down
        for k in mi355slam.MAP_EXTRACT_SRC:
            if k not in src:
                continue
            a = np.asarray(t[k])
            if k in PER_SLOT:
                row = a[0].nbytes
                td[k] = get(ctx, src[k], a.dtype, (N_ACTIVE,) + a.shape[1:], first * row)
            else:
                td[k] = get(ctx, src[k], a.dtype, a.shape)
        td["kf_id"] = t["kf_id"][active]
        td["desc_base"], td["n_kp"] = t["desc_base"][active], t["n_kp"][active]
        out = R.extract(td, list(range(N_ACTIVE)), dict(z, n_kf=N_ACTIVE), zeros)
        for k in names:
            put(ctx, second[k], out[k])
        ctx.sync()
        return out

    finish_src = lambda: kt.frame_finish(src["mp_flags"], src["mp_live"], point_table(ctx, src, n_mp), src["mp_track"], n_obs_src, t["kf_id"], [frame], frame, n_kp)
    finish_dst = lambda: kd.frame_finish(dst["mp_flags"], dst["mp_live"], point_table(ctx, dst, z["n_mp_dst"]), dst["mp_track"], dst["n_obs"], t["kf_id"][active], [N_ACTIVE - 1],
                                         N_ACTIVE - 1, n_kp)
    n_obs_src = ctx.upload(np.zeros(n_mp, np.int32))

    def restore_src():
        put(ctx, src["kf_mp"], t["kf_mp"]); put(ctx, src["mp_flags"], t["mp_flags"]); put(ctx, src["mp_live"], t["mp_live"])
        ctx.sync()

    try:
        out = dict(shape=name, n_kf=n_kf, stride=stride, n_mp=n_mp, n_active=N_ACTIVE, rows=n_rows)
        out["extract"], got = clock(call, reps)
        out["host_path"], host = clock(host_path, reps)
        state = {k: get(ctx, dst[k], R.DTYPES[k], shapes[k]) for k in names}
        again = {k: get(ctx, second[k], R.DTYPES[k], shapes[k]) for k in names}
        same = lambda a, b: a.dtype == b.dtype and a.tobytes() == b.tobytes()
        out["counts"] = [int(v) for v in got["counts"]]
        out["equal_bits"] = bool(all(same(state[k], host[k]) and same(again[k], host[k]) for k in names) and got["counts"].tolist() == host["counts"].tolist())
        differing = [k for k in names if not (same(state[k], host[k]) and same(again[k], host[k]))]
        assert out["equal_bits"], "%s: the host path and ms_map_extract leave different bytes (%s; counts %s / %s)" % (name, differing, got["counts"].tolist(), host["counts"].tolist())
        out["finish_on_source"], a = clock(finish_src, reps, restore_src)
        restore_src()                                        # the last timed call took the frame out of the source
        out["finish_on_extraction"], b = clock(finish_dst, reps, lambda: (call(), ctx.sync()))
        out["finish_equal_bits"] = bool(all(same(a[k], b[k]) for k in ("cloud_kp", "cloud_track", "cloud_pos")) and same(a["cloud_row"], state["row_src"][b["cloud_row"]])
                                        and a["counts"][[0, 2]].tolist() == b["counts"][[0, 2]].tolist())      # the removed rows differ: a row only inactive keyframes share with the frame goes on the extraction alone
        assert out["finish_equal_bits"], "%s: ms_frame_finish gives another cloud on the extraction than on the source" % name
        return out
    finally:
        for b_ in list(src.values()) + list(dst.values()) + list(second.values()) + [n_obs_src]:
            b_.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ctx = mi355slam.Context(0)
    try:
        print(json.dumps(dict(probe="map_extract", reps=args.reps, shapes=[probe(ctx, name, shape, args.reps) for name, shape in SHAPES.items()])))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
