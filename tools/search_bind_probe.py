"""Times matchLocalMapPoints' searchByProjection as a device-resident chain against the path the application ran before it, on
two scenes of tests/search_bind_ref.py: `matcher` (make_matcher_scene: 300 map points under a SEARCH view, 500 keypoints, real geometry, no
rescan) and `clustered` (340 clusters, 2 720 kept queries, 2 699 keypoints, ~900 rescans; its queries are given, so no gate runs in either path).

  device  ms_bound_mask -> [ms_project_gate] -> ms_projection_topk -> ms_search_bind, everything staying where the kernels left it; what
          comes down is the gate's n_kept and the result block.  Synchronous calls through the Python binding, timed with the host clock.
  host    a Python STAND-IN for the parent path, not the reference build and not C++: the bound mask goes up, [gate] and scoring run on the
          device (the same calls), kept_entry and the top-4 lists (and, for a rescan, the query arrays) come down, the greedy walk is replayed
          in Python (search_bind_ref.tables over the downloaded lists), then the current keyframe's row of kf_mp and n_obs go up.  A C++
          replay would be much faster than the Python loop; the column says what the transfers and the host walk cost around the same kernels.

Both paths start from the same restored tables (outside the timed span) and alternate; the probe compares kf_mp and n_obs after the two
paths for equal bits.  Prints one JSON line.  python tools/search_bind_probe.py [--reps 20]"""
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
import search_bind_ref as R           # noqa: E402
import mi355slam                      # noqa: E402
from mi355slam import _vp, lib        # noqa: E402

QUERIES = (("kept_entry", np.int32, 1), ("q_x", np.float32, 1), ("q_y", np.float32, 1), ("q_radius", np.float32, 1), ("q_min_octave", np.int32, 1),
           ("q_max_octave", np.int32, 1), ("q_desc", np.uint32, 8))
LISTS = (("top_idx", np.int32, 4), ("top_dist", np.uint16, 4), ("top_octave", np.int32, 4), ("n_scored", np.int32, 1))


def put(ctx, buf, a):
    a = np.ascontiguousarray(a)
    ctx.check(lib().ms_dev_upload(ctx._h, _vp(buf), _vp(a), C.c_size_t(a.nbytes)), "ms_dev_upload")


class Chain:
    """One scene on the device: the tables, the keyframe, the query buffers (written by the gate, or uploaded once) and the list buffers."""

    def __init__(self, ctx, S, gate=None):
        self.ctx, self.S, self.gate = ctx, S, gate
        k = S["kf"]
        self.kf = mi355slam.ProjectionKeyframe(ctx, k["x"], k["y"], k["desc"], k["octave"])
        self.kt = mi355slam.KeyframeTable(ctx, S["kf_mp"])
        self.live, self.n_obs = ctx.upload(S["mp_live"]), ctx.upload(S["n_obs"])
        ne = S["count"]
        self.skip = ctx.alloc(S["n_kp"] + 16)
        self.q = mi355slam.gate_buffers(ctx, ne, per_entry=False)
        self.l = {name: ctx.alloc(np.dtype(dt).itemsize * w * ne + 16) for name, dt, w in LISTS}
        if gate is None:
            for name, _, _ in QUERIES:
                put(ctx, self.q[name], S[name])
        else:
            sc = gate
            t = sc["table"]
            self.table = mi355slam.MapPointTable(ctx, t["pos"], t["norm"], t["min_dist"], t["max_dist"], t["desc"])

    def restore(self):
        put(self.ctx, self.kt.kf_mp, self.S["kf_mp"]); put(self.ctx, self.n_obs, self.S["n_obs"])
        self.ctx.sync()

    def tables(self):
        return self.kt.download(), self.n_obs.download(np.int32, (self.S["n_mp"],))

    def gate_and_score(self):
        ctx, S, kf, q, l = self.ctx, self.S, self.kf, self.q, self.l
        nq = S["n_kept"]
        if self.gate is not None:
            sc = self.gate
            _, n_kept, _ = mi355slam.project_gate_device(ctx, self.table, [sc["views"][0]], sc["sf"], sc["scale_factor"], per_entry=False, out=q)
            nq = int(n_kept[0])
        ctx.check(lib().ms_projection_topk(ctx._h, _vp(kf.d_sx), _vp(kf.d_sy), _vp(kf.d_si), kf.n, _vp(kf.d_desc), _vp(kf.d_oct), _vp(self.skip), _vp(q["q_x"]), _vp(q["q_y"]),
                                           _vp(q["q_radius"]), _vp(q["q_min_octave"]), _vp(q["q_max_octave"]), _vp(q["q_desc"]), nq, _vp(l["top_idx"]), _vp(l["top_dist"]),
                                           _vp(l["top_octave"]), _vp(l["n_scored"]), None), "ms_projection_topk")
        return nq

    def device_path(self):
        S, q, l = self.S, self.q, self.l
        self.kt.bound_mask(S["slot"], S["n_kp"], S["n_mp"], self.skip)
        nq = self.gate_and_score()
        return self.kt.search_bind(mi355slam.SearchBindArgs(mp_live=self.live, n_obs=self.n_obs, n_mp=S["n_mp"], skip=self.skip, kf=self.kf, mp_index=S["mp_index"],
                                                            first=S["first"], count=S["count"], n_kept=nq, slot=S["slot"], **{n: q[n] for n, _, _ in QUERIES},
                                                            **{n: l[n] for n, _, _ in LISTS}))

    def host_path(self):
        S, q, l = self.S, self.q, self.l
        skip = R.bound_mask(S["kf_mp"], S["slot"], S["n_kp"], S["n_mp"])          # the host owns Keyframe::mapPoints on this path
        put(self.ctx, self.skip, skip)
        nq = self.gate_and_score()
        down = lambda b, dt, w: b.download(dt, (nq, w) if w > 1 else (nq,))
        lists = {name: down(l[name], dt, w) for name, dt, w in LISTS}
        host = dict(S, n_kept=nq, kept_entry=down(q["kept_entry"], np.int32, 1))
        if ((lists["top_idx"] >= 0).sum(axis=1) == 4).any() and (lists["n_scored"] > 4).any():      # a list may run out: the query arrays come down for the rescans
            host.update({name: down(q[name], dt, w) for name, dt, w in QUERIES[1:]})
        w = R.tables(host, lists, skip)
        self.kt.update(S["slot"], w["kf_mp"][S["slot"]])
        put(self.ctx, self.n_obs, w["n_obs"])
        self.ctx.sync()
        return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ctx = mi355slam.Context(0)
    pct = lambda a: [round(1e3 * float(np.percentile(a, p)), 3) for p in (10, 50, 90)]
    sc, _, SM = R.matcher_scene()
    result = {}
    for name, S, gate in (("matcher", SM, sc), ("clustered", R.clustered_scene(340, 11, stride=2816), None)):
        ch = Chain(ctx, S, gate)
        t_dev, t_host = [], []
        for rep in range(args.reps + 2):                     # two warm-up rounds
            ch.restore()
            t0 = time.perf_counter()
            got = ch.device_path()
            t1 = time.perf_counter()
            after_device = ch.tables()
            ch.restore()
            t2 = time.perf_counter()
            want = ch.host_path()
            t3 = time.perf_counter()
            after_host = ch.tables()
            if rep >= 2:
                t_dev.append(t1 - t0); t_host.append(t3 - t2)
        equal = all(np.array_equal(a, b) for a, b in zip(after_device, after_host)) and np.array_equal(after_host[0], want["kf_mp"]) and \
            np.array_equal(after_host[1], want["n_obs"]) and got.n_matched == want["n_matched"] and np.array_equal(got.counts, want["counts"])
        result[name] = dict(entries=int(S["count"]), kept=int(S["n_kept"]), keypoints=int(S["n_kp"]), stride=int(S["stride"]), rows=int(S["n_mp"]), matched=got.n_matched,
                            counts_per_outcome=[int(v) for v in got.counts[:5]], rescans=int(got.counts[5]), device_ms_p10_p50_p90=pct(t_dev),
                            host_stand_in_ms_p10_p50_p90=pct(t_host), tables_equal=bool(equal))
    print(json.dumps(dict(probe="search_bind", reps=args.reps, **result)))
    ctx.close()


if __name__ == "__main__":
    main()
