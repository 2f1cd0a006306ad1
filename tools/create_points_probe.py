"""Times createNewMapPoints on the device map tables against the path INTEGRATION.md documented before it: one new keyframe
against 20 adjacent keyframes, 2 000 keypoints each (21 slots, stride 2 048, 8 000 rows), 60 true points per adjacent pair at depths on
both sides of the two-observation angle, 200 keypoints of the new keyframe bound beforehand.

  device  per adjacent: ms_match_triangulation -> ms_create_points_lists -> ms_triangulate_lists -> ms_create_points_bind, synchronous
          calls through the Python binding, timed with the host clock, each of the four calls also on its own.  Uploaded per adjacent: E, the
          free rows, the per-slot camera table of the triangulator; downloaded: the counts, the per-match status and the packed lists.
  host    per adjacent: ms_match_triangulation, the download of `matched`, the observation lists built with numpy (a STAND-IN for the
          application's loop over the matches, not the reference build and not C++), ms_triangulate with host lists, kfTable.update of both
          keyframes' rows, the upload of mp_live and of both `usable` masks, and the descriptors of the created rows uploaded as one range
          of the table.

Both paths start from the same restored tables (outside the timed span); the probe compares every table and mask after the two paths for
equal bits.  Prints one JSON line.  python tools/create_points_probe.py [--reps 10]"""
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
import create_points_ref as R         # noqa: E402
import map_refresh_ref as MR          # noqa: E402
import mi355slam                      # noqa: E402
import test_gpu_create_points as T    # noqa: E402
import triangulate_ref as TR          # noqa: E402

N_KF, STRIDE, N_MP, N_KP, CURRENT, PER_PAIR, BOUND = 21, 2048, 8000, 2000, 10, 60, 200
F = np.float32


def make_scene(seed=3):
    rng = np.random.default_rng(seed)
    poses, cams, focal = TR.make_keyframes(rng, N_KF, special=False)
    kf_id = (2 * rng.permutation(N_KF) + 1).astype(np.int32)
    kp = dict(x=(rng.random((N_KF, STRIDE)) * 640).astype(F), y=(rng.random((N_KF, STRIDE)) * 480).astype(F),
              octave=rng.integers(0, 8, (N_KF, STRIDE)).astype(np.int32), depth=np.full((N_KF, STRIDE), -1.0, F))
    angle = (rng.random((N_KF, STRIDE)) * 360).astype(F)
    node = rng.integers(0, 64, (N_KF, STRIDE)).astype(np.int32)
    desc_base = (rng.permutation(N_KF) * STRIDE).astype(np.int32)
    pool = rng.integers(0, 2 ** 32, (N_KF * STRIDE, 8), dtype=np.uint64).astype(np.uint32)
    kf_mp = np.full((N_KF, STRIDE), -1, np.int32)
    table = dict(pos=rng.uniform(-50, 50, (N_MP, 3)), norm=rng.normal(0, 1, (N_MP, 3)).astype(F), min_dist=rng.uniform(0.5, 1, N_MP).astype(F),
                 max_dist=rng.uniform(20, 30, N_MP).astype(F), desc=rng.integers(0, 2 ** 32, (N_MP, 8), dtype=np.uint64).astype(np.uint32))
    mp_flags, mp_live = np.zeros(N_MP, np.uint8), np.zeros(N_MP, np.uint8)
    mp_live[:4000] = 1; mp_flags[:4000] = 3
    order = {s: iter(rng.permutation(N_KP).tolist()) for s in range(N_KF)}
    for j in range(BOUND):
        kf_mp[CURRENT, next(order[CURRENT])] = j
    Pc = poses[CURRENT].reshape(3, 4)
    point = 0
    for adj in range(N_KF):
        for _ in range(0 if adj == CURRENT else PER_PAIR):
            zc = rng.uniform(2.0, 8.0) * abs(adj - CURRENT) ** 0.5
            X = Pc[:, :3].T @ (np.array([rng.uniform(-0.2, 0.2) * zc, rng.uniform(-0.15, 0.15) * zc, zc]) - Pc[:, 3])
            d0, a0, octave = rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32), rng.random() * 360, int(rng.integers(0, 8))
            for s in (CURRENT, adj):
                j = next(order[s])
                u, v, _ = TR.project(poses, cams, s, X)
                kp["x"][s, j], kp["y"][s, j], kp["octave"][s, j] = u + rng.normal(0, 0.02), v + rng.normal(0, 0.02), octave
                angle[s, j], node[s, j] = a0 + rng.normal(0, 0.5), point % 64
                pool[desc_base[s] + j] = d0
                pool[desc_base[s] + j, 0] ^= np.uint32(1 << int(rng.integers(0, 32)))
            point += 1
    free_rows = np.arange(4000, N_MP, dtype=np.int32)
    return dict(kf_mp=kf_mp, kf_id=kf_id, n_kp=np.full(N_KF, N_KP, np.int32), poses=poses, cams=cams, focal=focal, kp=kp, angle=angle, node=node, desc_base=desc_base, pool=pool,
                table=table, mp_flags=mp_flags, mp_live=mp_live, n_obs=np.zeros(N_MP, np.int32), mp_track=np.full(N_MP, -1, np.int32), S=TR.settings(),
                sf=MR.scale_factors(), thr_deg=2.0), free_rows


class Chain:
    """The buffers both paths share and the matcher call."""

    def __init__(self, ctx, d, sc):
        self.ctx, self.d, self.sc = ctx, d, sc
        self.sf = ctx.upload(sc["sf"])
        self.d_E, self.d_matched, self.d_count = ctx.alloc(72), ctx.alloc(4 * N_KP), ctx.alloc(16)
        self.bufs = {k: ctx.alloc(4 * N_KP) for k in ("match_kp1", "match_kp2", "created_rows", "created_kp1", "created_kp2")}
        self.lists = mi355slam.ObservationLists(ctx, 256, 512)

    def match(self, adj):
        ctx, d, sc = self.ctx, self.d, self.sc
        P = sc["poses"].reshape(-1, 3, 4)
        E = mi355slam.create_E21(P[adj][:, :3], P[adj][:, 3], P[CURRENT][:, :3], P[CURRENT][:, 3])
        T.put(ctx, self.d_E, E)
        A1, A2 = (mi355slam.MatchFrame * 1)(d.frames[CURRENT].struct), (mi355slam.MatchFrame * 1)(d.frames[adj].struct)
        ptrs = (C.c_void_p * 1)(self.d_matched.ptr)
        ctx.check(mi355slam.lib().ms_match_triangulation(ctx._h, A1, A2, 1, mi355slam._vp(self.d_E), mi355slam._vp(self.sf), C.c_float(sc["thr_deg"]), 1, ptrs,
                                                         mi355slam._vp(self.d_count)), "ms_match_triangulation")


def device_path(ch, adjacent, free_rows, split):
    d, sc, b = ch.d, ch.sc, ch.bufs
    free = free_rows.tolist()
    created = 0
    for adj in adjacent:
        t0 = time.perf_counter()
        ch.match(adj)
        t1 = time.perf_counter()
        rc, n = d.kf.create_points_lists_device(ch.lists, d.live, d.table.n, sc["kf_id"], d.kp, sc["desc_base"], CURRENT, adj, ch.d_matched, N_KP, N_KP, free, 8, b["match_kp1"],
                                                b["match_kp2"])
        ch.ctx.check(rc, "ms_create_points_lists")
        t2 = time.perf_counter()
        d.table.triangulate_lists(d.poses, sc["cams"], sc["focal"], ch.lists, n, 2 * n, sc["S"], mi355slam.TRI_TME, flags=d.flags)
        t3 = time.perf_counter()
        rc, n_created = d.kf.create_points_bind_device(d.table, d.flags, d.live, d.pool, CURRENT, adj, ch.lists, b["match_kp1"], b["match_kp2"], n, N_KP, N_KP,
                                                       d.frames[CURRENT].bufs["usable"], d.frames[adj].bufs["usable"], d.n_obs, d.mp_track, b)
        ch.ctx.check(rc, "ms_create_points_bind")
        rows = b["created_rows"].download(np.int32, (n_created,)) if n_created else np.zeros(0, np.int32)
        taken = set(rows.tolist())
        free = [r for r in free if r not in taken]
        t4 = time.perf_counter()
        split += np.array([t1 - t0, t2 - t1, t3 - t2, t4 - t3])
        created += n_created
    return created


def host_path(ch, adjacent, free_rows, host):
    """The documented path before ms_create_points_*; `host` = the application's copies of kf_mp, mp_live, the descriptors, n_obs and mp_track."""
    d, sc, ctx = ch.d, ch.sc, ch.ctx
    free = free_rows.tolist()
    kp = sc["kp"]
    created = 0
    for adj in adjacent:
        ch.match(adj)
        matched = ch.d_matched.download(np.int32, (N_KP,))                                               # the download of `matched`
        kp1 = np.flatnonzero(matched >= 0).astype(np.int32)
        kp2 = matched[kp1]
        n = len(kp1)
        rows = np.array(free[:n], np.int32)
        first_cur = sc["kf_id"][CURRENT] < sc["kf_id"][adj]
        slots = np.tile(np.array([CURRENT, adj] if first_cur else [adj, CURRENT], np.int32), n)
        js = np.stack([kp1, kp2] if first_cur else [kp2, kp1], axis=1).reshape(-1)
        prob = dict(rows=rows, was_triangulated=np.zeros(n, np.uint8), obs_start=2 * np.arange(n + 1, dtype=np.int32), obs_kf=slots, obs_x=kp["x"][slots, js],
                    obs_y=kp["y"][slots, js], obs_octave=kp["octave"][slots, js], obs_depth=kp["depth"][slots, js])
        status = d.table.triangulate(d.poses, sc["cams"], sc["focal"], prob, sc["S"], mi355slam.TRI_TME, flags=d.flags)[0]
        ok = status != TR.NOT_TRIANGULATED
        r = rows[ok]
        host["kf_mp"][CURRENT, kp1[ok]] = r
        host["kf_mp"][adj, kp2[ok]] = r
        host["mp_live"][r], host["n_obs"][r], host["mp_track"][r] = 1, 2, -1
        first = np.flatnonzero(ok) * 2                       # the descriptor of the first observation
        host["desc"][r] = sc["pool"][sc["desc_base"][slots[first]] + js[first]]
        d.kf.update(CURRENT, host["kf_mp"][CURRENT]); d.kf.update(adj, host["kf_mp"][adj])             # kfTable.update, twice
        T.put(ctx, d.live, host["mp_live"]); T.put(ctx, d.n_obs, host["n_obs"]); T.put(ctx, d.mp_track, host["mp_track"])
        for s in (CURRENT, adj):                             # the masks of both frames
            T.put(ctx, d.frames[s].bufs["usable"], (host["kf_mp"][s, :N_KP] < 0).astype(np.uint8))
        if len(r):
            lo, hi = int(r.min()), int(r.max()) + 1
            d.table.update(lo, hi - lo, desc=host["desc"][lo:hi])
        taken = set(r.tolist())
        free = [x for x in free if x not in taken]
        created += len(r)
    return created


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    ctx = mi355slam.Context(0)
    sc, free_rows = make_scene()
    d = T.Device(ctx, sc)
    ch = Chain(ctx, d, sc)
    adjacent = [s for s in range(N_KF) if s != CURRENT]
    q = lambda a: [round(1e3 * float(np.percentile(a, p)), 3) for p in (10, 50, 90)]
    t_dev, t_host, split = [], [], np.zeros(4)
    for rep in range(args.reps + 2):                         # two warm-up rounds
        d.restore(); ctx.sync()
        part = np.zeros(4)
        t0 = time.perf_counter()
        created = device_path(ch, adjacent, free_rows, part)
        ctx.sync()
        t1 = time.perf_counter()
        after_device, masks_device = d.state(), d.masks()
        d.restore(); ctx.sync()
        host = dict(kf_mp=sc["kf_mp"].copy(), mp_live=sc["mp_live"].copy(), n_obs=sc["n_obs"].copy(), mp_track=sc["mp_track"].copy(), desc=sc["table"]["desc"].copy())
        t2 = time.perf_counter()
        created_host = host_path(ch, adjacent, free_rows, host)
        ctx.sync()
        t3 = time.perf_counter()
        if rep >= 2:
            t_dev.append(t1 - t0); t_host.append(t3 - t2); split += part
    per_adjacent = [round(1e3 * float(v) / (args.reps * len(adjacent)), 4) for v in split]
    print(json.dumps(dict(probe="create_points", reps=args.reps, adjacents=len(adjacent), keypoints=N_KP, created=created, created_host_path=created_host,
                          device_ms_p10_p50_p90=q(t_dev), host_list_ms_p10_p50_p90=q(t_host),
                          per_adjacent_ms=dict(zip(("match_triangulation", "create_points_lists", "triangulate_lists", "create_points_bind"), per_adjacent)),
                          tables_equal=bool(R.same_state(after_device, d.state())), masks_equal=bool(R.same_masks(masks_device, d.masks())))))
    ctx.close()


if __name__ == "__main__":
    main()
