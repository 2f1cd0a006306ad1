"""Times the projection-guided matchers' front half two ways, for 1 view x 2000 map points and 20 views x 2000:

  device  ms_project_gate (all views, one call) + ms_projection_topk per view on the packed slices where they lie
  host    the path before ms_project_gate: the gate loop on the host, then per view the surviving queries packed into one block and
          uploaded with one copy into a reused device buffer (as mi355slam::detail::score_candidates does), then ms_projection_topk.
          The host loop here is tests/project_gate_ref.gate_view, the VECTORISED NUMPY restatement, not the application's C++ loop.

Every device buffer of either path is allocated before the timed region.  Both end in a device synchronise and are timed with the host
clock, alternating, after a warm-up of every shape; the lists they produce are compared first.  Prints one JSON line.
python tools/project_gate_probe.py [--reps 100]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-module_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import mi355slam                      # noqa: E402
import project_gate_ref as R          # noqa: E402
from mi355slam import _vp, lib        # noqa: E402


def topk(ctx, kf, qx, qy, qr, qlo, qhi, qd, nq, outs):
    ctx.check(lib().ms_projection_topk(ctx._h, _vp(kf.d_sx), _vp(kf.d_sy), _vp(kf.d_si), kf.n, _vp(kf.d_desc), _vp(kf.d_oct), None, qx, qy, qr, qlo, qhi, qd, nq,
                                       *outs, None), "ms_projection_topk")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    args = ap.parse_args()
    ctx = mi355slam.Context(0)
    rng = np.random.default_rng(1)
    result = {}
    for n_views in (1, 20):
        sc = R.make_views(rng, [2000] * n_views, [R.FUSE] * n_views, n_mp=4000)
        sc["sf"] = mi355slam.scale_factors(8, 1.2); R.regate(sc)
        t = sc["table"]
        table = mi355slam.MapPointTable(ctx, t["pos"], t["norm"], t["min_dist"], t["max_dist"], t["desc"])
        kfs = [mi355slam.ProjectionKeyframe(ctx, rng.uniform(0, 640, 2000), rng.uniform(0, 480, 2000), rng.integers(0, 2 ** 32, (2000, 8), dtype=np.uint64).astype(np.uint32),
                                            rng.integers(0, 8, 2000)) for _ in range(n_views)]
        ne = 2000 * n_views
        outs = [ctx.alloc(16 * ne + 16), ctx.alloc(8 * ne + 16), ctx.alloc(16 * ne + 16), ctx.alloc(4 * ne + 16)]
        off = lambda b, byts: _vp(b.ptr + byts)
        slices = lambda f: [off(outs[0], 16 * f), off(outs[1], 8 * f), off(outs[2], 16 * f), off(outs[3], 4 * f)]

        gate_out = mi355slam.gate_buffers(ctx, ne, per_entry=False)
        sec = 4 * 2000                                          # one view's host-built block: x | y | radius | min octave | max octave | descriptors
        qblock = [ctx.alloc(5 * sec + 32 * 2000 + 16) for _ in range(n_views)]
        stage = np.zeros(5 * 2000 + 8 * 2000, np.uint32)

        def device():
            out, n_kept, V = mi355slam.project_gate_device(ctx, table, sc["views"], sc["sf"], 1.2, per_entry=False, out=gate_out)
            for v, kf in enumerate(kfs):
                f = V[v].first
                topk(ctx, kf, off(out["q_x"], 4 * f), off(out["q_y"], 4 * f), off(out["q_radius"], 4 * f), off(out["q_min_octave"], 4 * f), off(out["q_max_octave"], 4 * f),
                     off(out["q_desc"], 32 * f), int(n_kept[v]), slices(f))
            ctx.sync()
            return n_kept, [V[v].first for v in range(n_views)]

        def host():
            kept, firsts = [], []
            for v, kf in enumerate(kfs):
                g = R.gate_view(t, sc["views"][v], sc["sf"], 1.2)
                k = g["kept"]
                n = len(k)
                stage[0:n] = g["x"][k].view(np.uint32); stage[2000:2000 + n] = g["y"][k].view(np.uint32); stage[4000:4000 + n] = g["radius"][k].view(np.uint32)
                stage[6000:6000 + n] = g["q_min_octave"].view(np.uint32); stage[8000:8000 + n] = g["q_max_octave"].view(np.uint32)
                stage[10000:10000 + 8 * n] = t["desc"][np.asarray(sc["views"][v]["indices"])[k]].reshape(-1)
                q = qblock[v]
                ctx.check(lib().ms_dev_upload(ctx._h, _vp(q), _vp(stage), ctypes.c_size_t(stage.nbytes)), "ms_dev_upload")
                topk(ctx, kf, off(q, 0), off(q, sec), off(q, 2 * sec), off(q, 3 * sec), off(q, 4 * sec), off(q, 5 * sec), n, slices(2000 * v))
                kept.append(n); firsts.append(2000 * v)
            ctx.sync()
            return np.array(kept), firsts

        def lists(n_kept, firsts):
            ti, td = outs[0].download(np.int32, (ne, 4)), outs[1].download(np.uint16, (ne, 4))
            return [(ti[f:f + k].copy(), td[f:f + k].copy()) for f, k in zip(firsts, n_kept)]

        nk_d, f_d = device(); ld = lists(nk_d, f_d)
        nk_h, f_h = host(); lh = lists(nk_h, f_h)
        near = sum(int(r["near_level"].sum()) for r in sc["ref"])
        same = np.array_equal(nk_d, nk_h) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(ld, lh))
        for _ in range(5):
            device(); host()
        td_, th_ = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); device(); t1 = time.perf_counter(); host(); t2 = time.perf_counter()
            td_.append(t1 - t0); th_.append(t2 - t1)
        q = lambda a: [round(1e3 * float(np.percentile(a, p)), 3) for p in (10, 50, 90)]
        result["views_%d" % n_views] = dict(entries=ne, kept=int(nk_d.sum()), near_level=near, lists_equal=bool(same), device_ms_p10_p50_p90=q(td_), host_ms_p10_p50_p90=q(th_))
    print(json.dumps(dict(probe="project_gate", reps=args.reps, **result)))
    ctx.close()


if __name__ == "__main__":
    main()
