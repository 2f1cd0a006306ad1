"""Times deduplicateMapPoints as a device-resident chain against the path the application ran before it, on the geometry scene
of tests/map_fuse_ref.py at two sizes (440 rows, 4 adjacent keyframes of ~70 keypoints; 3 000 rows, 8 adjacent keyframes of ~400):

  device  KeyframeTable.deduplicate: per batch one read of the current slot's row, ms_project_gate over all remaining adjacent views,
          ms_projection_topk per view, ONE ms_map_fuse on the lists where they lie, the download of the erased rows; then
          ms_map_point_union and one more batch for direction 2.  Synchronous calls through the Python binding, timed with the host clock.
          No candidate list and no table crosses the bus.
  host    a Python STAND-IN for the application's walk, not the reference build and not C++: per adjacent keyframe the gate and the scoring
          on the device (the same two calls, one view at a time, because the list is read live), the download of kept_entry / top_idx /
          top_dist, then replaceDuplication over dicts of observations (map_fuse_ref.fuse_sequential), and at the end the re-upload of
          every kf_mp row a replace touched plus mp_live, mp_flags, n_obs, mp_track and track_row.  A std::map walk in C++ would be much
          faster than the dict walk; the column says what the downloads, the uploads and a per-view gate cost around a walk on the host.

Both paths start from the same restored tables (outside the timed span) and alternate; the probe compares every table and the erased
lists after the two paths for equal bits.  Prints one JSON line.  python tools/map_fuse_probe.py [--reps 20]"""
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
import map_fuse_ref as R              # noqa: E402
import mi355slam                      # noqa: E402
from mi355slam import _vp, lib        # noqa: E402

SIZES = (("rows_440", {}), ("rows_3000", dict(seed=4, n_pairs=1500, n_kf=12, stride=640, n_kp=600, n_adjacent=8)))
NAMES = ("mp_flags", "mp_live", "n_obs", "mp_track", "track_row")


def put(ctx, buf, a):
    a = np.ascontiguousarray(a)
    ctx.check(lib().ms_dev_upload(ctx._h, _vp(buf), _vp(a), C.c_size_t(a.nbytes)), "ms_dev_upload")


def host_path(ctx, kt, bufs, table, kfs, S):
    """replaceDuplication per keyframe on the host, fed by the device's gate and scoring of that one view; the touched tables go back up."""
    T = R.copy_tables(S["T"])
    n_mp = len(T["mp_live"])
    erased_rows, erased_into = [], []

    def one(slot, rows):
        nonlocal T
        view = dict(S["views_of"][slot], threshold=S["margin"], mode=mi355slam.GATE_FUSE, indices=rows)
        kept, ti, td, _, _, dev = mi355slam._gate_then_topk(ctx, kfs[slot], table, view, S["sf"], S["scale_factor"], None)
        for b in dev.values():
            b.free()
        cand = np.full(len(rows), -1, np.int32)
        ok = (ti[:, 0] >= 0) & (td[:, 0] <= 50)
        cand[kept[ok]] = ti[ok, 0]
        out = R.fuse_sequential(T, rows, [(slot, 0, len(rows))], cand, -1)
        erased_rows.extend(out["erased_rows"].tolist()); erased_into.extend(out["erased_into"].tolist())
        T = {k: out.get(k, T.get(k)) for k in R.TABLE_KEYS + ("track_base",)}

    for slot in S["adjacent"]:
        row = T["kf_mp"][S["current"]]
        one(slot, row[(row >= 0) & (row < n_mp)].astype(np.int32))
    adj = T["kf_mp"][S["adjacent"]]
    one(S["current"], np.unique(adj[(adj >= 0) & (adj < n_mp)]).astype(np.int32))
    for s in np.flatnonzero((T["kf_mp"] != S["T"]["kf_mp"]).any(axis=1)):
        kt.update(int(s), T["kf_mp"][s])
    for name in NAMES:
        put(ctx, bufs[name], T[name])
    return T, erased_rows, erased_into


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ctx = mi355slam.Context(0)
    q = lambda a: [round(1e3 * float(np.percentile(a, p)), 3) for p in (10, 50, 90)]
    result = {}
    for name, size in SIZES:
        S = R.make_geometry_scene(**size)
        t = S["table"]
        n_mp = len(S["T"]["mp_live"])
        table = mi355slam.MapPointTable(ctx, t["pos"], t["norm"], t["min_dist"], t["max_dist"], t["desc"])
        kfs = {s: mi355slam.ProjectionKeyframe(ctx, k["x"], k["y"], k["desc"], k["octave"]) for s, k in S["kfs"].items()}
        kt = mi355slam.KeyframeTable(ctx, S["T"]["kf_mp"])
        bufs, n_track = kt._fuse_tables(S["T"], n_mp)

        def restore():
            put(ctx, kt.kf_mp, S["T"]["kf_mp"])
            for k in NAMES:
                put(ctx, bufs[k], S["T"][k])
            ctx.sync()

        t_dev, t_host = [], []
        for rep in range(args.reps + 2):                     # two warm-up rounds
            restore()
            t0 = time.perf_counter()
            got = kt.deduplicate(table, kfs, S["views_of"], S["T"], S["current"], S["adjacent"], S["margin"], S["sf"], S["scale_factor"], device_tables=(bufs, n_track))
            t1 = time.perf_counter()
            after_device = kt._fuse_download(bufs, S["T"], n_mp, n_track)
            restore()
            t2 = time.perf_counter()
            want, rows, into = host_path(ctx, kt, bufs, table, kfs, S)
            ctx.sync()
            t3 = time.perf_counter()
            after_host = kt._fuse_download(bufs, S["T"], n_mp, n_track)
            if rep >= 2:
                t_dev.append(t1 - t0); t_host.append(t3 - t2)
        keep = [0, 2, 3, 4, 5, 6, 7]
        result[name] = dict(rows=n_mp, slots=int(S["T"]["kf_mp"].shape[0]), stride=int(S["T"]["kf_mp"].shape[1]), adjacent=len(S["adjacent"]),
                            current_rows=int((S["T"]["kf_mp"][S["current"]] >= 0).sum()), counts_per_outcome=[int(v) for v in got["counts"]],
                            replaces=len(got["erased_rows"]), regates=int(got["regates"]), kf_mp_bytes=int(S["T"]["kf_mp"].nbytes),
                            device_ms_p10_p50_p90=q(t_dev), host_stand_in_ms_p10_p50_p90=q(t_host),
                            tables_equal=R.same(after_device, after_host, R.TABLE_KEYS) == [] and R.same(after_host, want, R.TABLE_KEYS) == [],
                            erased_equal=bool(got["erased_rows"].tolist() == rows and got["erased_into"].tolist() == into))
        for b in bufs.values():
            b.free()
        kt.kf_mp.free()
    print(json.dumps(dict(probe="map_fuse", reps=args.reps, **result)))
    ctx.close()


if __name__ == "__main__":
    main()
