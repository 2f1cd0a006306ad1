"""Differential fuzz of the bundle adjuster against the CPU oracle: N random windows (2..70 keyframes, ragged visibility, fixed poses and
points, outliers, loop-closure edges, pose-only cases, stage-1 shaped batches with one free keyframe, poseBundleAdjust-shaped batches with one free keyframe and
every point fixed), solved alone / in a batch / on teams, some with forced rejections (the test hook, passed to the oracle too); residuals within 1e-7 (north_star:
1e-5; observed 2e-10 over 8000 windows), LM trajectory equal, chi2 per observation at test_gpu_ba._check's bar, fixed poses and points unmoved.  Every batch is
classified by the host's routing rule (k_ba_pose_only / k_ba_one_pose / k_ba_lm) and the summary line counts the routes.
With a third argument `domain` every drawn window is also put through a random subset of the transforms of tests/ba_scenes.py (another world frame, flipped
quaternion signs, full and non-symmetric information matrices, other Huber deltas, large SE3 errors, other units, points close to a camera), drawn from a
stream of its own; without it the windows and the random stream are what they always were.
usage: python tools/ba_fuzz.py [N] [seed] [domain]"""
import os, sys
R = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("slam-module_amd", "oracle", "tests", "tools"): sys.path.insert(0, os.path.join(R, p))
import numpy as np, mi355slam, mso, ba_synth
from ba_route import route                                      # the host's routing rule (tools/ba_route.py: one copy, shared with tests/ba_scenes.py)
N = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
DOMAIN = len(sys.argv) > 3 and sys.argv[3] == "domain"
if DOMAIN: import ba_scenes
drng = np.random.default_rng([int(sys.argv[2]) if len(sys.argv) > 2 else 3, 77])          # the domain transforms' own stream
ctx = mi355slam.Context(0)


def domain_transforms(p):
    """A random subset of ba_scenes' transforms (each with probability 0.4) on a drawn window.  degenerate() is left to the scene tests: it fixes keyframes
    0 and 1, which could leave a one-free-keyframe window without a free keyframe."""
    ne = len(p["edge_i"])
    pick = lambda: drng.random() < 0.4
    cnt = np.bincount(p["obs_point"], minlength=len(p["point"]))
    if pick() and (cnt >= 2).sum() >= 4: p = ba_scenes.near_points(p, drng, n_near=2)
    if pick() and ne: p = ba_scenes.edge_errors(p, [float(drng.choice(ba_scenes.SMALL_ANGLES + ba_scenes.LARGE_ANGLES))], drng, edges=[int(drng.integers(0, ne))])
    if pick() and ne: p = ba_scenes.dense_edge_info(p, drng, nonsymmetric=(int(drng.integers(0, ne)),) if drng.random() < 0.5 else ())
    if pick(): p = ba_scenes.rescale(p, float(drng.choice([1e3, 1e-3])))
    if pick(): p = ba_scenes.move_world(p, ba_scenes.random_rigid(drng, float(drng.uniform(1.0, 3.1)), float(drng.uniform(1.0, 8.0))))
    if pick(): p = ba_scenes.flip_quaternion_signs(p, drng.random(len(p["pose"])) < 0.5, drng.random(ne) < 0.5)
    if pick(): p = ba_scenes.huber(p, float(drng.choice([0.0, -1.0, 0.5, 1e6])))
    return p


def random_problem(one_pose=False):
    n_pose = int(rng.integers(2, 71)); n_point = int(rng.integers(5, 900)); run = int(rng.integers(2, min(n_pose, 14) + 1))
    p = ba_synth.make_problem(n_pose, n_point, run, seed=int(rng.integers(0, 1 << 30)), outlier_frac=float(rng.choice([0, 0, 0.05, 0.15])),
                              fix_first=bool(rng.integers(0, 2)))
    op, ol, uv, info = list(p["obs_pose"]), list(p["obs_point"]), list(p["obs_uv"]), list(p["obs_info"])
    seen = set(zip(op, ol))
    for _ in range(int(rng.integers(0, 3 * n_point // 4 + 1))):            # scattered extra observations: ragged visibility, wider envelope
        l, i = int(rng.integers(0, n_point)), int(rng.integers(0, n_pose))
        q = ba_synth._R_from_quat(p["gt_pose"][i, :4]) @ p["gt_point"][l] + p["gt_pose"][i, 4:]
        if q[2] < 0.5 or (i, l) in seen: continue
        seen.add((i, l)); op.append(i); ol.append(l); uv.append(q[:2] / q[2] + rng.normal(0, 1 / 500, 2)); info.append(500.0 ** 2 / float(rng.choice([1.0, 1.44, 2.07])))
    p["obs_pose"], p["obs_point"] = np.array(op, np.int32), np.array(ol, np.int32)
    p["obs_uv"], p["obs_info"] = np.array(uv), np.array(info)
    p["pose_fixed"] = p["pose_fixed"].copy()
    for i in rng.choice(n_pose, size=int(rng.integers(0, max(n_pose // 4, 1))), replace=False): p["pose_fixed"][i] = 1
    if p["pose_fixed"].all(): p["pose_fixed"][int(rng.integers(0, n_pose))] = 0
    if one_pose:                                                                              # stage 1 of localBundleAdjust: ONE free keyframe (any position), the points free or partly fixed
        p["pose_fixed"][:] = 1; p["pose_fixed"][int(rng.integers(0, n_pose))] = 0
    kind = int(rng.integers(1 if one_pose else 0, 6))
    if kind == 0: p["point_fixed"] = np.ones(n_point, np.uint8)                               # pose-only
    elif kind == 1: p["point_fixed"] = (rng.random(n_point) < 0.3).astype(np.uint8)
    if n_pose > 6 and rng.random() < 0.4:                                                     # a loop-closure edge between far keyframes
        a, b = 1, n_pose - 2
        M = ba_synth._compose(p["gt_pose"][b], ba_synth._inverse(p["gt_pose"][a]))
        p["edge_i"] = np.append(p["edge_i"], a).astype(np.int32); p["edge_j"] = np.append(p["edge_j"], b).astype(np.int32)
        p["edge_meas"] = np.vstack([p["edge_meas"], M[None]]); p["edge_info"] = np.vstack([p["edge_info"], (np.eye(6) * 400.0).reshape(1, 36)])
    return p


def pose_only_problem():
    """poseBundleAdjust-shaped: one free keyframe, every other keyframe and every point fixed; 0..8 SE3 edges at the free keyframe (either side), the chain's
    edges between fixed keyframes; the free keyframe's observations on both sides of what k_ba_pose_only keeps in registers (192 x 8), optionally the fixed
    keyframes' too."""
    n_pose = int(rng.integers(2, 9)); run = n_pose if rng.random() < 0.5 else int(rng.integers(1, n_pose + 1))
    n_point = int(rng.integers(1700, 3500)) if run == n_pose and rng.random() < 0.5 else int(rng.integers(5, 1500))
    w = ba_synth.make_problem(n_pose, n_point, run, seed=int(rng.integers(0, 1 << 30)), outlier_frac=float(rng.choice([0, 0, 0.05, 0.15])))
    cur = int(rng.choice(np.unique(w["obs_pose"])))                                          # (a keyframe that sees something: its 6 x 6 system is not empty)
    p = dict(w)
    p["pose_fixed"] = np.ones(n_pose, np.uint8); p["pose_fixed"][cur] = 0
    p["point_fixed"] = np.ones(n_point, np.uint8)
    if rng.random() < 0.5: p["point"] = w["gt_point"].copy()
    if rng.random() < 0.5:                                                                    # only the free keyframe's observations, as poseBundleAdjust builds it
        sel = w["obs_pose"] == cur
        for k in ("obs_pose", "obs_point", "obs_uv", "obs_info"): p[k] = w[k][sel]
    touch = (w["edge_i"] == cur) | (w["edge_j"] == cur)
    ei, ej, em, ew = list(w["edge_i"][~touch]), list(w["edge_j"][~touch]), list(w["edge_meas"][~touch]), list(w["edge_info"][~touch])
    for _ in range(int(rng.integers(0, 9))):                                                  # edges at the free keyframe (a pair may repeat)
        o = int(rng.integers(0, n_pose - 1)); o += o >= cur
        a, b = (cur, o) if rng.random() < 0.5 else (o, cur)
        ei.append(a); ej.append(b); em.append(ba_synth._compose(w["gt_pose"][b], ba_synth._inverse(w["gt_pose"][a]))); ew.append(w["edge_info"][0])
    p["edge_i"], p["edge_j"] = np.array(ei, np.int32), np.array(ej, np.int32)
    p["edge_meas"], p["edge_info"] = np.array(em, np.float64).reshape(-1, 7), np.array(ew, np.float64).reshape(-1, 36)
    return p


bad = done = 0
worst = 0.0
routes = dict(pose_only=0, one_pose=0, general=0)
while done < N:
    shape = rng.random()
    if shape < 0.2:                                                      # the whole batch in the shape k_ba_pose_only takes
        probs = [pose_only_problem() for _ in range(int(rng.integers(1, 5)))]
        team = int(rng.choice([0, 1]))
    else:
        one_pose = shape < 0.4                                           # the whole batch in the shape k_ba_one_pose takes (teams, lanes per point and rounds by the sizes drawn)
        probs = [random_problem(one_pose) for _ in range(int(rng.integers(1, 5)))]
        team = int(rng.choice([0, 1, 2, 5, 16]))
    iters = int(rng.integers(1, 9)); n_rej = int(rng.choice([0, 0, 0, 0, 0, 0, 3, 7, 10]))
    if DOMAIN: probs = [domain_transforms(p) for p in probs]
    routes[route(probs, team)] += 1
    want = [mso.ba_solve(p, iters, False, force_reject=n_rej) for p in probs]
    ba = mi355slam.BundleAdjuster(ctx, probs, max_iters=iters); ba.set_team(team); ba.debug_force_reject(n_rej); ba.solve()
    for p, w, i in zip(probs, want, range(len(probs))):
        g = ba.download(i)
        rg, rw = ba_synth.residuals_fast(p, g["pose"], g["point"]), ba_synth.residuals_fast(p, w["pose"], w["point"])
        worst = max(worst, float(np.abs(rg - rw).max()))
        ok = np.abs(rg - rw).max() < 1e-7 and abs(g["stats"]["chi2_final"] - w["stats"]["chi2_final"]) <= 1e-7 * abs(w["stats"]["chi2_final"]) + 1e-8
        ok = ok and np.allclose(g["chi2"], w["chi2"], rtol=1e-4, atol=1e-6)                  # (the bar of test_gpu_ba._check)
        pf = p["pose_fixed"] != 0
        ok = ok and np.array_equal(g["pose"][pf], p["pose"][pf])
        if p.get("point_fixed") is not None:
            lf = p["point_fixed"] != 0
            ok = ok and np.array_equal(g["point"][lf], p["point"][lf])
        # the LM trajectory (iterations, trials, stop reason) must be the oracle's, except once the solve has converged and the gain ratio is
        # rounding noise (then a trial or an iteration more or less is taken at the same minimum): the same robust chi2 to 1e-10 relative.  (Round 4: the bar for
        # that case used to be 1e-8 on the residuals; one window in 6000 -- 27 keyframes on a team of 16, 15 trials against 14 -- ended 1.17e-8 away with chi2 equal
        # to 4e-15: the extra trial at the minimum moves the estimate along the valley's floor.  The residual bar of every case stays 1e-7, north_star's is 1e-5.)
        same_path = (g["stats"]["iters"], g["stats"]["trials"], g["stats"]["stop"]) == (w["stats"]["iters"], w["stats"]["trials"], w["stats"]["stop"])
        ok = ok and (same_path or abs(g["stats"]["chi2_final"] - w["stats"]["chi2_final"]) <= 1e-10 * abs(w["stats"]["chi2_final"]))
        done += 1
        if not ok:
            bad += 1
            print("MISMATCH", dict(poses=len(p["pose"]), points=len(p["point"]), obs=len(p["obs_pose"]), iters=iters, team=team, fixed=int(p["pose_fixed"].sum()),
                                   route=route(probs, team), forced=n_rej,
                                   dres=float(np.abs(rg - rw).max()), stats=(g["stats"]["iters"], g["stats"]["trials"], w["stats"]["iters"], w["stats"]["trials"]),
                                   chi2=(g["stats"]["chi2_final"], w["stats"]["chi2_final"])), flush=True)
    ba.close()
print("ba fuzz: %d windows, %d mismatches; largest residual difference to the oracle %.2e (the fuzz fails above 1e-7; north_star's tolerance is 1e-5); "
      "routes: pose_only=%d one_pose=%d general=%d (batches)" % (done, bad, worst, routes["pose_only"], routes["one_pose"], routes["general"]))
sys.exit(1 if bad else 0)
