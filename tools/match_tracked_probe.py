"""Times matchTrackedFeatures on the device map tables against the path the application ran before it, on the scene of
tests/match_tracked_ref.py at 600 keypoints (12 keyframes, stride 640, 2 000 rows) and at 2 000 (stride 2 048, 8 000 rows, three times as many
keypoints of every kind):

  device  KeyframeTable.match_tracked: ms_match_tracked -> ms_observation_lists -> ms_triangulate_lists (FIRST_LAST) -> ms_match_tracked_finish
          -> ms_observation_lists -> ms_map_refresh_lists, synchronous calls through the Python binding, timed together with the host clock.
          They include the upload of the frame record, kp_track and new_rows, the per-call tables of the list and triangulation calls and
          the download of outcomes, created rows, counts and statuses.  No list and no table row crosses the bus.
  host    a numpy STAND-IN for the application's walk, not the reference build and not C++: keyPointToTrackId / trackIdToMapPoint resolved
          with array lookups, isInFrustum and checkReprojectionError evaluated on the host for all keypoints at once (project_gate_ref,
          the arithmetic of triangulate_ref), then kfTable.update of the frame's row and the new points' rows, observation lists built on
          the host (obs_lists_ref) and uploaded to the host-list calls ms_triangulate (FIRST_LAST) and ms_map_refresh, the descriptor of the
          UNSURE points uploaded row by row.  A std::map walk in C++ would spend its time differently; the column says what the calls and
          uploads of that path cost with the walk done by vectorised numpy.

Both paths start from the same restored tables (outside the timed span); the probe compares the outcomes and every table after the two
paths for equal bits.  Prints one JSON line.  python tools/match_tracked_probe.py [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-module_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import match_tracked_ref as R         # noqa: E402
import mi355slam                      # noqa: E402
import obs_lists_ref as OL            # noqa: E402
import project_gate_ref as PG         # noqa: E402
import test_gpu_match_tracked as T    # noqa: E402
import triangulate_ref as TR          # noqa: E402

SIZES = ((600, {}), (2000, dict(n_kp=2000, stride=2048, n_mp=8000, n_track=6000, filled=6000, scale=3)))
LIST_KEYS = ("rows", "obs_start", "obs_kf", "obs_desc", "first_octave", "was_triangulated", "obs_x", "obs_y", "obs_octave", "obs_depth")


def host_walk(sc, frame):
    """Outcomes and rows of :76-141 for all keypoints at once (no created rows yet)."""
    slot, t, n_mp = frame["slot"], frame["kp_track"], len(sc["mp_live"])
    has = t >= 0
    r = np.where(has, sc["track_row"][np.where(has, t - sc["track_base"], 0)], -1)
    inside = (r >= 0) & (r < n_mp)
    rr = np.where(inside, r, 0)
    present = has & inside & (sc["mp_live"][rr] != 0) & (sc["mp_track"][rr] == t)
    tri = present & ((sc["mp_flags"][rr] & 1) != 0)
    outcome = np.zeros(len(t), np.uint8)
    outcome[present & ~tri] = R.TRACKED
    outcome[has & ~present] = R.CREATED if sc["desc_base"][slot] >= 0 else R.NO_DESCRIPTORS
    j = np.flatnonzero(tri)
    P = sc["poses"][slot].reshape(3, 4)
    view = dict(R=P[:, :3], t=P[:, 3], cam=tuple(sc["cams"][slot]), threshold=0.0, view_cos_limit=sc["view_cos_limit"], mode=PG.SEARCH, indices=rr[j].astype(np.int32))
    g = PG.gate_view(sc["table"], view, sc["sf"], 1.2)
    du, dv = g["x"] - sc["kp"]["x"][slot, j], g["y"] - sc["kp"]["y"][slot, j]
    sq = du * du + dv * dv
    ls = sc["S"]["level_sigma_sq"]
    base = np.float64(np.float32(int(sc["focal"][slot])) * np.float32(sc["S"]["rel_reprojection_threshold"]))
    sigma2 = (ls[sc["kp"]["octave"][slot, j]] / ls[len(ls) // 2]).astype(np.float64) * base * base
    ok = sq.astype(np.float64) <= TR.CHI2_INV2D * sigma2
    outcome[j] = np.where(g["status"] != PG.KEPT, R.FRUSTUM, np.where(ok, R.CHECKED, R.REPROJECTION))
    return outcome, rr


def host_path(ctx, d, sc, frame, new_rows):
    """The path before ms_match_tracked, on the device tables of `d`.  Returns the outcomes."""
    slot, t, n_mp = frame["slot"], frame["kp_track"], len(sc["mp_live"])
    outcome, rr = host_walk(sc, frame)
    created_kp = np.flatnonzero(outcome == R.CREATED)
    created_rows = new_rows[:len(created_kp)]
    tracked, checked = rr[outcome == R.TRACKED].astype(np.int32), rr[outcome == R.CHECKED].astype(np.int32)
    row = np.full(sc["kf_mp"].shape[1], -1, np.int32)
    bound = (outcome == R.TRACKED) | (outcome == R.CHECKED)
    row[:len(t)][bound] = rr[bound]
    row[created_kp] = created_rows
    flags, live, mp_track, track_row = (sc[k].copy() for k in ("mp_flags", "mp_live", "mp_track", "track_row"))
    flags[created_rows], live[created_rows], mp_track[created_rows] = 0, 1, t[created_kp]
    track_row[t[created_kp] - sc["track_base"]] = created_rows
    d.kf.update(slot, row)                                   # kfTable.update, and the new points' rows
    for buf, a in ((d.flags, flags), (d.live, live), (d.tracks.mp_track, mp_track), (d.tracks.track_row, track_row)):
        T.put(ctx, buf, a)
    for r, v in zip(created_rows, created_kp):
        d.table.update(int(r), 1, desc=sc["pool"][sc["desc_base"][slot] + v])
    kf_mp = sc["kf_mp"].copy()
    kf_mp[slot] = row
    lists = OL.observation_lists(kf_mp, n_mp, sc["kf_id"], flags, sc["kp"], sc["desc_base"], OL.select(OL.FROM_ROWS, rows_in=tracked), 8)
    status = d.table.triangulate(d.poses, sc["cams"], sc["focal"], {k: lists[k] for k in LIST_KEYS}, sc["S"], mi355slam.TRI_FIRST_LAST, flags=d.flags)[0]
    for i in np.flatnonzero(status == TR.UNSURE):            # :811 for two observations
        od = lists["obs_desc"][lists["obs_start"][i]:lists["obs_start"][i + 1]]
        have = od[od != -1]
        if len(have):
            d.table.update(int(tracked[i]), 1, desc=sc["pool"][have[0]])
    refresh_rows = np.concatenate([tracked[status == TR.TRIANGULATED], checked]).astype(np.int32)
    lists = OL.observation_lists(kf_mp, n_mp, sc["kf_id"], flags, sc["kp"], sc["desc_base"], OL.select(OL.FROM_ROWS, drop_empty=1, rows_in=refresh_rows), 8)
    if lists["n_rows"]:
        mi355slam.map_refresh(ctx, d.table, d.poses, {k: lists[k] for k in LIST_KEYS}, sc["sf"], d.pool)
    return outcome


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ctx = mi355slam.Context(0)
    q = lambda a: [round(1e3 * float(np.percentile(a, p)), 3) for p in (10, 50, 90)]
    result = {}
    for n_kp, size in SIZES:
        sc, frame, new_rows = R.make_scene(**size)
        d = T.Device(ctx, sc)
        t_dev, t_host = [], []
        for rep in range(args.reps + 2):                     # two warm-up rounds
            d.restore(sc); ctx.sync()
            t0 = time.perf_counter()
            res = d.kf.match_tracked(*d.args(sc), d.frame(sc, frame), new_rows, sc["S"], sc["sf"], sc["view_cos_limit"])
            t1 = time.perf_counter()
            after_device = d.state()
            d.restore(sc); ctx.sync()
            t2 = time.perf_counter()
            outcome = host_path(ctx, d, sc, frame, new_rows)
            ctx.sync()
            t3 = time.perf_counter()
            if rep >= 2:
                t_dev.append(t1 - t0); t_host.append(t3 - t2)
        counts = [int(v) for v in res["counts"]]
        result["kp_%d" % n_kp] = dict(keypoints=n_kp, tracked=int((frame["kp_track"] >= 0).sum()), counts=counts, refresh_rows=len(res["refresh_rows"]),
                                      device_ms_p10_p50_p90=q(t_dev), host_stand_in_ms_p10_p50_p90=q(t_host),
                                      outcomes_equal=bool(np.array_equal(outcome, res["outcome"])), tables_equal=bool(R.same_state(after_device, d.state())))
        d.free()
    print(json.dumps(dict(probe="match_tracked", reps=args.reps, **result)))
    ctx.close()


if __name__ == "__main__":
    main()
