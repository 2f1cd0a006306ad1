"""Times the gather and the apply step of the local BA window on the device map tables on the bench's 50-keyframe window
(tests/ba_synth.make_problem_fast: 50 keyframes, 2 000 map points seen by runs of 10 keyframes, 20 000 projection edges), laid out as map
tables of 58 slots (stride 1 024; 8 more keyframes that are not local observe 300 of the points) and 2 000 rows.

  device  ms_map_point_union -> ms_observation_lists (the lists the window is gathered from), ms_ba_window_lists, ms_ba_window_apply
          (MS_BA_APPLY_LOCAL, about 2 % of the edges above the threshold): synchronous calls through the Python binding, timed with the
          host clock, each on its own.
  host    the same two steps the way bundle_adjuster.cpp:214-290 / :376-390 take them: a walk over dictionaries of keyframes and map points
          with `observations` ordered by KfId (tests/ba_window_ref.literal_gather / literal_apply: Python, ONE core, a STAND-IN for the
          application's std::map walk, not the reference build and not C++), then the uploads that path ends in: the keyframe-table rows
          of the slots that lost an observation, the flags, the observation counts, the positions of the window's rows and the local poses.

Both paths start from the same restored tables (outside the timed span); the probe compares the gathered arrays and every table after the
two paths for equal bits.  Prints one JSON line.  python tools/ba_window_probe.py [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-module_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ba_synth                       # noqa: E402
import ba_window_ref as R             # noqa: E402
import mi355slam                      # noqa: E402
import obs_lists_ref as OL            # noqa: E402
import test_gpu_ba_window as T        # noqa: E402

N_LOCAL, N_OTHER, STRIDE, N_MP = 50, 8, 1024, 2000


def make_scene(seed=42):
    w = ba_synth.make_problem_fast(n_pose=N_LOCAL, n_point=N_MP, run=10, seed=seed)
    rng = np.random.default_rng(seed)
    n_kf = N_LOCAL + N_OTHER
    cam = np.array([500.0, 500.0, 320.0, 240.0, 640, 480])
    kf_mp = np.full((n_kf, STRIDE), -1, np.int32)
    kp = dict(x=np.zeros((n_kf, STRIDE), np.float32), y=np.zeros((n_kf, STRIDE), np.float32), octave=np.zeros((n_kf, STRIDE), np.int32),
              depth=np.full((n_kf, STRIDE), -1, np.float32))
    slot_of_pose = rng.permutation(n_kf)[:N_LOCAL]           # vertex i of the bench window lives in slot slot_of_pose[i]
    fill = np.zeros(n_kf, np.int64)
    sigma = R.sigma_levels()
    for o in range(len(w["obs_pose"])):
        s = slot_of_pose[w["obs_pose"][o]]
        j = fill[s]; fill[s] += 1
        kf_mp[s, j] = w["obs_point"][o]
        kp["x"][s, j], kp["y"][s, j] = w["obs_uv"][o] * cam[:2] + cam[2:4]
        kp["octave"][s, j] = int(np.argmin(np.abs(500.0 ** 2 / sigma.astype(np.float64) - w["obs_info"][o])))
    others = np.setdiff1d(np.arange(n_kf), slot_of_pose)
    for s in others:
        rows = rng.permutation(N_MP)[:300]
        kf_mp[s, :300] = rows
        kp["x"][s, :300], kp["y"][s, :300] = rng.random(300) * 640, rng.random(300) * 480
    kf_id = np.zeros(n_kf, np.int32)
    kf_id[slot_of_pose] = 10 + 2 * np.arange(N_LOCAL)        # the window's vertices in ascending KfId, as the bench's odometry chain has them
    kf_id[others] = 1 + np.arange(N_OTHER)
    poses = np.zeros((n_kf, 12))
    poses[:] = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).reshape(12)
    for i, s in enumerate(slot_of_pose):
        poses[s] = np.concatenate([ba_synth._R_from_quat(w["pose"][i, :4]), w["pose"][i, 4:, None]], 1).reshape(12)
    cams = np.tile(cam, (n_kf, 1))
    sc = dict(n_kf=n_kf, stride=STRIDE, n_mp=N_MP, kf_id=kf_id, kf_mp=kf_mp, kp=kp, cams=cams, focal=np.full(n_kf, 500, np.int32), poses=poses, mp_pos=w["point"].copy(),
              mp_flags=np.full(N_MP, 3, np.uint8), sigma=sigma)
    start, _, _ = OL.transpose(kf_mp, N_MP, kf_id)
    sc["n_obs"] = np.diff(start).astype(np.int32)
    local = slot_of_pose[::-1].astype(np.int32)              # descending KfId
    return sc, local


def clock(fn, reps, before=None):
    best, total = float("inf"), 0.0
    for _ in range(reps):
        if before:
            before()
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best, total = min(best, dt), total + dt
    return out, 1e3 * total / reps, 1e3 * best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    sc, local = make_scene()
    ctx = mi355slam.Context(0)
    d = T.Device(ctx, sc)
    rng = np.random.default_rng(1)
    # ---- device
    def lists_call():
        d.lists.clear()
        return d.observation_lists(local)
    for _ in range(3):
        lists_call()
    (lists, n_rows, n_obs), lists_ms, lists_best = clock(lists_call, args.reps)
    edges = mi355slam.BaWindowEdges(ctx, n_obs)
    out = dict(pose=np.zeros((N_LOCAL, 7)), point=np.zeros((n_rows, 3)), obs_point=np.zeros(n_obs, np.int32), obs_pose=np.zeros(n_obs, np.int32), obs_uv=np.zeros((n_obs, 2)),
               obs_info=np.zeros(n_obs))
    gather_call = lambda: d.kf.ba_window_lists_device(d.table, d.poses, lists, n_rows, n_obs, local, 0, sc["cams"], sc["focal"], sc["sigma"], edges, out)
    for _ in range(3):
        gather_call()
    (rc, n_edge, n_current), gather_ms, gather_best = clock(gather_call, args.reps)
    ctx.check(rc, "ms_ba_window_lists")
    want = R.gather(sc, local, 0)
    same = all(T.same_bits(out[k].reshape(-1)[:want[k].size], want[k].reshape(-1)) for k, _, _ in T.HOST_OUT) and (n_edge, n_current) == (want["n_edge"], want["n_current"])
    chi2 = np.where(rng.random(n_edge) < 0.02, 9.0, 1.0)
    pose, point = want["pose"] + rng.normal(0, 1e-4, want["pose"].shape), want["point"] + rng.normal(0, 1e-3, want["point"].shape)
    window = dict(lists=lists, edges=edges, n_rows=n_rows, n_edge=n_edge, local_slot=local, current_index=0)
    apply_call = lambda: d.kf.ba_window_apply(d.table, d.poses, d.flags, d.n_obs, window, pose, point, chi2, R.LOCAL)
    for _ in range(3):
        d.restore(); apply_call()
    (rc, erased, _), apply_ms, apply_best = clock(apply_call, args.reps, before=d.restore)
    ctx.check(rc, "ms_ba_window_apply")
    after_device = d.state()
    # ---- host stand-in
    reps_host = max(args.reps // 10, 2)
    lit, host_gather_ms, host_gather_best = clock(lambda: R.literal_gather(sc, local, 0), reps_host)
    same = same and all(T.same_bits(np.ascontiguousarray(lit[k], dt).reshape(-1), want[k].reshape(-1)) for k, dt, _ in T.HOST_OUT)
    window_host = dict(want)

    def host_apply():
        st, erased_host, _ = R.literal_apply(R.state_of(sc), window_host, pose, point, chi2, R.LOCAL)
        for s in np.unique(want["edge_slot"][erased_host]):
            d.kf.update(int(s), st["kf_mp"][s])
        T.put(ctx, d.flags, st["mp_flags"]); T.put(ctx, d.n_obs, st["n_obs"])
        rows = want["rows"]
        d.table.update(int(rows[0]), int(rows[-1] - rows[0] + 1), pos=st["mp_pos"][rows[0]:rows[-1] + 1])
        for s in local:
            d.poses.update(int(s), 1, st["poses"][s])
        return erased_host
    erased_host, host_apply_ms, host_apply_best = clock(host_apply, reps_host, before=d.restore)
    after_host = d.state()
    same = same and all(T.same_bits(after_device[k], after_host[k]) for k in T.TABLES) and T.same_bits(erased, erased_host)
    print(json.dumps(dict(window=dict(local_keyframes=N_LOCAL, slots=sc["n_kf"], rows=n_rows, listed_observations=n_obs, edges=n_edge, erased=int(len(erased))),
                          device_ms=dict(union_and_lists=round(lists_ms, 3), gather=round(gather_ms, 3), apply=round(apply_ms, 3),
                                         best=dict(union_and_lists=round(lists_best, 3), gather=round(gather_best, 3), apply=round(apply_best, 3))),
                          host_stand_in_ms=dict(gather_walk=round(host_gather_ms, 1), apply_walk_and_uploads=round(host_apply_ms, 1),
                                                best=dict(gather_walk=round(host_gather_best, 1), apply_walk_and_uploads=round(host_apply_best, 1))),
                          reps=args.reps, equal_bits=bool(same))))
    edges.free(); d.free(); ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
