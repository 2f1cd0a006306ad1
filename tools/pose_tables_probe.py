"""poseBundleAdjust per frame on the device map tables (ms_pose_tables_solve) against the path an application on the tables had
before it: download the frame's kf_mp row, the flags (and live marks) and the positions, gather the problem on the host, ms_ba_solve_host.
Both paths run on the same tables in the same session, in alternating blocks; every call starts from the same table pose (put back outside
the timed region).  Two shapes: the bench's pose-only shape (481 bound points of 2000 keypoints) and a 50-point frame, on a 200 000-row map.
Prints the median and the 10th / 90th percentile of each path per shape, and checks that both paths return the same pose bit for bit.

    python tools/pose_tables_probe.py [--calls 300] [--warmup 30]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("slam-module_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import mi355slam                                             # noqa: E402
import pose_tables_ref as R                                  # noqa: E402
from mi355slam import BaResultC, _ba_struct, _vp, lib       # noqa: E402

N_MP, N_KP, STRIDE, MAX_ITERS = 200000, 2000, 2048, 10


def big_scene(n_kept, seed):
    """A frame of N_KP keypoints with n_kept TRIANGULATED points, its rows spread over a map of N_MP rows."""
    sc, frame = R.make_scene(R.mixed(N_KP, n_kept, seed), stride=STRIDE, seed=seed)
    rng = np.random.default_rng(seed)
    small = sc["n_mp"]
    to_big = np.sort(rng.choice(N_MP, small, replace=False))
    pos = np.stack([rng.uniform(-3, 3, N_MP), rng.uniform(-2, 2, N_MP), rng.uniform(4, 10, N_MP)], 1)
    flags, live = np.full(N_MP, 3, np.uint8), np.ones(N_MP, np.uint8)
    pos[to_big], flags[to_big], live[to_big] = sc["mp_pos"], sc["mp_flags"], sc["mp_live"]
    kf_mp = sc["kf_mp"].astype(np.int64)
    valid = (kf_mp >= 0) & (kf_mp < small)
    kf_mp[kf_mp == small] = N_MP
    kf_mp[valid] = to_big[kf_mp[valid]]
    big = dict(sc, n_mp=N_MP, mp_pos=pos, mp_flags=flags, mp_live=live, kf_mp=kf_mp.astype(np.int32))
    return big, dict(frame, max_iters=MAX_ITERS)


class Tables:
    def __init__(self, ctx, sc):
        self.ctx, self.sc = ctx, sc
        n = sc["n_mp"]
        self.table = mi355slam.MapPointTable(ctx, sc["mp_pos"], np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 8), np.uint32))
        self.kf = mi355slam.KeyframeTable(ctx, sc["kf_mp"])
        self.kp = mi355slam.KeypointTable(ctx, **sc["kp"])
        self.flags, self.live = ctx.upload(sc["mp_flags"]), ctx.upload(sc["mp_live"])
        self.poses = mi355slam.KeyframePoseTable(ctx, sc["poses"])
        self.pose0 = np.ascontiguousarray(sc["poses"], np.float64)
        # the host copies an application keeps of what does not change per frame: the frame's keypoints
        self.kp_host = {k: sc["kp"][k][R.FRAME].copy() for k in ("x", "y", "octave")}

    def reset_pose(self):
        self.ctx.check(lib().ms_dev_upload(self.ctx._h, C.c_void_p(self.poses.pose.ptr), _vp(self.pose0), C.c_size_t(self.pose0.nbytes)), "ms_dev_upload")


def parent_path(ctx, t, frame):
    """Download the row, the flags and the positions; gather on the host; ms_ba_solve_host.  Returns the solved pose 0."""
    sc, s, n_kp = t.sc, frame["slot"], frame["n_kp"]
    n = sc["n_mp"]
    row = np.empty(n_kp, np.int32)
    ctx.check(lib().ms_dev_download(ctx._h, _vp(row), C.c_void_p(t.kf.kf_mp.ptr + 4 * s * t.kf.stride), C.c_size_t(row.nbytes)), "ms_dev_download")
    flags, live = t.flags.download(np.uint8, (n,)), t.live.download(np.uint8, (n,))
    pos = t.table.pos.download(np.float64, (n, 3))
    poses = t.poses.download()
    host = dict(n_mp=n, kf_mp={s: row}, mp_flags=flags, mp_live=live, mp_pos=pos, poses=poses, sigma=sc["sigma"],
                kp={k: {s: v} for k, v in t.kp_host.items()})
    g = gather_host(host, frame)
    if g["n"] < frame["min_visible"]:
        return None
    st, keep = _ba_struct(R.problem(frame, g), frame["max_iters"])
    pose, res = np.zeros((2, 7)), BaResultC()
    ctx.check(lib().ms_ba_solve_host(ctx._h, C.byref(st), _vp(pose), None, None, C.byref(res)), "ms_ba_solve_host")
    return pose[0]


def gather_host(sc, frame):
    """pose_tables_ref.gather on the downloaded row (the same expressions, without the scene's other slots)."""
    s, n_kp = frame["slot"], frame["n_kp"]
    r = sc["kf_mp"][s].astype(np.int64)
    keep = (r >= 0) & (r < sc["n_mp"])
    keep[keep] = (sc["mp_live"][r[keep]] != 0) & ((sc["mp_flags"][r[keep]] & 1) != 0)
    kept = np.nonzero(keep)[0]
    rows = r[kept]
    fx, fy, cx, cy = (float(v) for v in frame["cam"][:4])
    x, y = sc["kp"]["x"][s][:n_kp][kept].astype(np.float64), sc["kp"]["y"][s][:n_kp][kept].astype(np.float64)
    focal = float(int(frame["focal"]))
    info = focal * focal / np.asarray(sc["sigma"], np.float32).astype(np.float64)[sc["kp"]["octave"][s][:n_kp][kept]]
    n = len(kept)
    pose = np.array([R.pose_of_matrix(sc["poses"][s]), R.pose_of_matrix(sc["poses"][frame["prev_slot"]])]).reshape(2, 7)
    return dict(pose=pose, point=sc["mp_pos"][rows].reshape(-1, 3), obs_point=np.arange(n, dtype=np.int32), obs_pose=np.zeros(n, np.int32),
                obs_uv=np.stack([(x - cx) / fx, (y - cy) / fy], 1), obs_info=info, n=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--only-new", action="store_true", help="the new call alone (for a kernel trace)")
    a = ap.parse_args()
    ctx = mi355slam.Context(0)
    adj = mi355slam.PoseAdjuster(ctx, 1024, R.W.sigma_levels())
    block = 25
    for label, n_kept in (("481 of 2000 keypoints", 481), ("50 of 2000 keypoints", 50)):
        sc, frame = big_scene(n_kept, seed=17 + n_kept)
        t = Tables(ctx, sc)
        F = mi355slam.pose_tables_frame(frame)
        O = mi355slam.PoseTablesOutC()

        def new_path():
            ctx.check(lib().ms_pose_tables_solve(adj._h, _vp(t.kf.kf_mp), t.kf.n_kf, t.kf.stride, _vp(t.flags), _vp(t.live), _vp(t.table.pos), t.table.n, _vp(t.kp.x), _vp(t.kp.y),
                                                 _vp(t.kp.octave), _vp(t.poses.pose), C.byref(F), C.byref(O), None), "ms_pose_tables_solve")
            return np.array(list(O.pose))

        paths = [("tables", new_path)] if a.only_new else [("tables", new_path), ("parent", lambda: parent_path(ctx, t, frame))]
        times = {k: [] for k, _ in paths}
        poses = {}
        done = 0
        while done < a.warmup + a.calls:
            for name, fn in paths:                           # alternating blocks: both paths see the same machine state
                for _ in range(block):
                    t.reset_pose()
                    ctx.sync()
                    t0 = time.perf_counter()
                    poses[name] = fn()
                    dt = time.perf_counter() - t0
                    if done >= a.warmup:
                        times[name].append(dt * 1e3)
            done += block
        assert O.ran == 1 and O.n_triangulated == n_kept, (O.ran, O.n_triangulated)
        if not a.only_new:
            assert poses["tables"].tobytes() == poses["parent"].tobytes(), "the two paths disagree"
        for name, _ in paths:
            v = np.sort(np.array(times[name]))
            print("%-22s %-7s median %.3f ms  p10 %.3f  p90 %.3f  (%d calls, %d iterations, %d trials)" %
                  (label, name, np.median(v), v[len(v) // 10], v[len(v) * 9 // 10], len(v), O.result.iterations, O.result.trials))
    adj.close()
    ctx.close()


if __name__ == "__main__":
    main()
