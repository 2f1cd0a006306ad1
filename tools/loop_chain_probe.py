"""Times the loop closer's three table calls for one new keyframe with 11 candidates x 2000 keypoints on a map of 200 000 rows
(40 slots, stride 2048, 8 levels): ms_loop_usable_mask (12 slots, masks and tri_row), ms_loop_pairs (11 candidates) and ms_loop_sim3_lists
(every other pair of each candidate), and the three back to back.

  device  the calls through the Python binding, synchronous, each timed twice: with the context's events around it (ms_timer: what the
          stream saw) and with the host clock around the binding (what the caller waits, ctypes marshalling included).
  host    what the table path would need without them: the 12 slots' rows of kf_mp and kp_octave, mp_live, mp_pos, the poses and the 11
          matched arrays come down (timed, ms_dev_download), then tests/loop_chain_ref.py's tables form (numpy on one core) builds the same
          arrays.  It is a STAND-IN for the std::map walk of loop_closer.cpp:203-213 / loop_ransac.cpp:17-41 / optimize_transform.cpp:101-142,
          not the reference build; the probe checks that both give the same bits.  tools/loop_chain_stdmap.cpp is that walk itself over
          std::map<MpId, MapPoint> / std::map<KfId, Keyframe> built from the same tables, compiled with g++ -O2 and
          run on one core on the probe's own scene (written to a file): the masks, the pairs and the Sim3 arrays of the 11 candidates.
  mirror  tests/loop_chain_smoke.cpp --time at this size: tryLoopClosureOnTables (15 candidates, 11 past the cheap tests, 2000 keypoints,
          200 000 rows) and the candidate-by-candidate walk over std::map observations it is compared with, host clock, median.

Warm-up, then the median of --reps runs.  Prints one JSON line.  python tools/loop_chain_probe.py [--reps 30]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-module_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import loop_chain_ref as R            # noqa: E402
import mi355slam                      # noqa: E402


def big_scene(n_kf=40, stride=2048, n_mp=200000, n_kp=2000, n_cand=11, n_levels=8, seed=9):
    rng = np.random.default_rng(seed)
    t = dict(kf_mp=np.full((n_kf, stride), -1, np.int32), mp_flags=rng.choice(np.array([0, 2, 3, 3], np.uint8), n_mp), mp_live=(rng.random(n_mp) < 0.97).astype(np.uint8),
             mp_pos=rng.uniform(-20, 20, (n_mp, 3)), kf_pose=np.zeros((n_kf, 12)), kp_x=rng.uniform(0, 640, (n_kf, stride)).astype(np.float32),
             kp_y=rng.uniform(0, 480, (n_kf, stride)).astype(np.float32), kp_octave=rng.integers(0, n_levels, (n_kf, stride)).astype(np.int32),
             cams=np.tile(np.array([500.0, 500.0, 320.0, 240.0, 640, 480]), (n_kf, 1)), n_kp=np.full(n_kf, n_kp, np.int32))
    for s in range(n_kf):
        t["kf_pose"][s] = np.concatenate([R._rotation(rng), rng.uniform(-2, 2, (3, 1))], axis=1).reshape(12)
        bound = rng.random(n_kp) < 0.8
        t["kf_mp"][s, :n_kp][bound] = rng.choice(n_mp, int(bound.sum()), replace=False)
    cand = rng.choice(np.arange(1, n_kf), n_cand, replace=False).astype(np.int32)
    matched = []
    for _ in cand:
        m = rng.permutation(n_kp).astype(np.int32)
        m[rng.random(n_kp) < 0.4] = -1
        matched.append(m)
    S = dict(n_kf=n_kf, stride=stride, n_mp=n_mp, n_levels=n_levels, level_sigma_sq=R.level_sigma_sq(n_levels), cur=0, n_kp_cur=n_kp, cand_slot=cand,
             n_kp_cand=np.full(n_cand, n_kp, np.int32), matched=matched)
    return S, t


def timed(ctx, fn, reps, warm=5):
    ev, wall = [], []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        ctx.timer_start()
        fn()
        ms = ctx.timer_stop_ms()
        t1 = time.perf_counter()
        if i >= warm:
            ev.append(ms); wall.append(1e3 * (t1 - t0))
    return round(statistics.median(ev), 4), round(statistics.median(wall), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    S, t = big_scene()
    ctx = mi355slam.Context(0)
    kt = mi355slam.KeyframeTable(ctx, t["kf_mp"])
    d = {k: ctx.upload(t[k]) for k in ("mp_flags", "mp_live", "mp_pos", "kf_pose", "kp_x", "kp_y", "kp_octave")}
    dm = [ctx.upload(m) for m in S["matched"]]
    n_kp, cand = S["n_kp_cur"], S["cand_slot"]
    slots = np.concatenate([[S["cur"]], cand]).astype(np.int32)
    masks, rows = [ctx.alloc(n_kp) for _ in slots], [ctx.alloc(4 * n_kp) for _ in slots]
    want = R.pairs_tables(S, t)
    cap = want["n_pairs"]
    out_p = {k: np.zeros((cap, w) if w > 1 else cap, dt) for k, dt, w in mi355slam.LOOP_PAIRS_OUT}
    out_p.update(pair_start=np.zeros(len(cand) + 1, np.int32), cur_pose=np.zeros(12), cand_pose=np.zeros((len(cand), 12)))
    sel = np.concatenate([np.arange(a0, b0, 2) for a0, b0 in zip(want["pair_start"], want["pair_start"][1:])])
    kp1, kp2 = want["kp1"][sel], want["kp2"][sel]
    start = np.concatenate([[0], np.cumsum([len(range(a0, b0, 2)) for a0, b0 in zip(want["pair_start"], want["pair_start"][1:])])]).astype(np.int32)
    out_s = {k: np.zeros((len(kp1), w) if w > 1 else len(kp1), dt) for k, dt, w in mi355slam.LOOP_SIM3_OUT}
    A_mask = mi355slam.LoopMaskArgs(mp_flags=d["mp_flags"], mp_live=d["mp_live"], n_mp=S["n_mp"], slots=slots, n_kp=[n_kp] * len(slots),
                                    require_triangulated=[0] + [1] * len(cand), usable=masks, tri_row=rows)
    A_pairs = mi355slam.LoopPairsArgs(mp_live=d["mp_live"], mp_pos=d["mp_pos"], n_mp=S["n_mp"], kf_pose=d["kf_pose"], kp_octave=d["kp_octave"], cur=S["cur"], n_kp_cur=n_kp,
                                      cand_slot=cand, n_kp_cand=S["n_kp_cand"], matched=dm, level_sigma_sq=S["level_sigma_sq"], cap_pairs=cap, out=out_p)
    A_sim3 = mi355slam.LoopSim3ListsArgs(mp_live=d["mp_live"], mp_pos=d["mp_pos"], n_mp=S["n_mp"], kf_pose=d["kf_pose"], kp_x=d["kp_x"], kp_y=d["kp_y"], kp_octave=d["kp_octave"],
                                         cur=S["cur"], n_kp_cur=n_kp, cand_slot=cand, n_kp_cand=S["n_kp_cand"], cams=t["cams"], level_sigma_sq=S["level_sigma_sq"], kp1=kp1,
                                         kp2=kp2, match_start=start, out=out_s)

    def f_mask():
        kt.loop_usable_mask(A_mask)

    def f_pairs():
        assert kt.loop_pairs(A_pairs)[0] == 0

    def f_sim3():
        kt.loop_sim3_lists(A_sim3)

    def f_all():
        f_mask(); f_pairs(); f_sim3()

    res = dict(scene="11 candidates x 2000 keypoints, 200000 rows, 40 slots x 2048", n_pairs=int(cap), n_listed=int(len(kp1)), reps=a.reps)
    for name, fn in (("usable_mask", f_mask), ("pairs", f_pairs), ("sim3_lists", f_sim3), ("three_calls", f_all)):
        res[name + "_event_ms"], res[name + "_wall_ms"] = timed(ctx, fn, a.reps)
    res["launches"] = dict(usable_mask=1, pairs=3, sim3_lists=1)
    res["copies"] = dict(usable_mask="1 up", pairs="1 up, 1 clear, 1 down", sim3_lists="1 up, 1 clear, 1 down")
    ws = R.sim3_lists_tables(S, t, kp1, kp2, start)
    same = all(np.array_equal(out_p[k][:cap].view(np.uint8), want[k].view(np.uint8)) for k in R.PAIR_ARRAYS) and np.array_equal(out_p["pair_start"], want["pair_start"])
    same = same and all(np.array_equal(out_s[k].view(np.uint8), ws[k].view(np.uint8)) for k in R.SIM3_ARRAYS)
    res["same_bits_as_host"] = bool(same)

    # the host path: the downloads it needs, then the numpy tables form on one core
    def downloads():
        for s in slots:
            mi355slam._download_i32_at(kt.kf_mp, 4 * S["stride"] * int(s), S["stride"])
            mi355slam._download_i32_at(d["kp_octave"], 4 * S["stride"] * int(s), S["stride"])
        d["mp_live"].download(np.uint8, (S["n_mp"],)); d["mp_pos"].download(np.float64, (S["n_mp"], 3)); d["kf_pose"].download(np.float64, (S["n_kf"], 12))
        for m in dm:
            m.download(np.int32, (n_kp,))

    wall = []
    for i in range(3 + a.reps):
        t0 = time.perf_counter()
        downloads()
        wall.append(1e3 * (time.perf_counter() - t0))
    res["host_downloads_ms"] = round(statistics.median(wall[3:]), 4)
    wall = []
    for i in range(2 + min(a.reps, 10)):
        t0 = time.perf_counter()
        for s, nk, req in zip(slots, [n_kp] * len(slots), [0] + [1] * len(cand)):
            R.usable_mask_tables(t, s, nk, req)
        R.pairs_tables(S, t)
        R.sim3_lists_tables(S, t, kp1, kp2, start)
        wall.append(1e3 * (time.perf_counter() - t0))
    res["host_numpy_one_core_ms"] = round(statistics.median(wall[2:]), 4)
    with tempfile.TemporaryDirectory() as tmp:
        # the std::map walk on one core, on the scene the device calls got
        scene = os.path.join(tmp, "scene.bin")
        with open(scene, "wb") as f:
            f.write(np.array([S["n_kf"], n_kp, S["n_mp"], len(cand), S["n_levels"], S["cur"]], np.int32).tobytes())
            for k in ("kf_mp", "kp_octave", "kp_x", "kp_y"):
                f.write(np.ascontiguousarray(t[k][:, :n_kp]).tobytes())
            for k in ("kf_pose", "mp_pos", "mp_live", "mp_flags"):
                f.write(np.ascontiguousarray(t[k]).tobytes())
            f.write(cand.astype(np.int32).tobytes()); f.write(np.stack(S["matched"]).astype(np.int32).tobytes()); f.write(S["level_sigma_sq"].astype(np.float32).tobytes())
        exe = os.path.join(tmp, "loop_chain_stdmap")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "loop_chain_stdmap.cpp"), "-o", exe])
        walk = json.loads(subprocess.check_output(["taskset", "-c", "0", exe, str(min(a.reps, 15)), scene], text=True))
        res["host_std_map_one_core_ms"], res["host_std_map_pairs"] = walk["std_map_one_core_ms"], walk["n_pairs"]
        assert walk["n_pairs"] == cap and walk["n_listed"] == len(kp1), walk
        # the whole mirror (tryLoopClosureOnTables) and the candidate-by-candidate walk it replaces, tests/loop_chain_smoke.cpp's scene at this size:
        # 15 candidates, 11 of them past the cheap tests, 2000 keypoints each, 200 000 rows
        lib_dir = os.path.join(ROOT, "slam-module_amd", "lib")
        smoke = os.path.join(tmp, "loop_chain_smoke")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "slam-module_amd", "host"), os.path.join(ROOT, "tests", "loop_chain_smoke.cpp"), "-o", smoke,
                               "-L", lib_dir, "-lmi355slam", "-Wl,-rpath," + lib_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
        ctx.close()                                          # the binary opens the device itself
        timing = json.loads(subprocess.check_output([smoke, "--time", str(n_kp - 20), str(S["n_mp"])], text=True).strip().splitlines()[-1])
    res["mirror_ms"], res["mirror_walk_ms"] = timing["mirror_ms"], timing["walk_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
