"""GPU parity of the LM trial loops of the two one-free-pose solvers against the CPU oracle: k_ba_pose_only (poseBundleAdjust, every frame) and k_ba_one_pose
(stage 1 of localBundleAdjust, every keyframe).  Each keeps its own copy of g2o's trial loop -- accept / reject, the lambda / nu schedule, the state restore after a
rejected trial, the qmax == 10 Terminate, the chi2 per observation -- so each is driven through the shared test hook (ms_ba_debug_force_reject: the first n trials
count as rejected) and compared with oracle.ba_solve(..., force_reject=n) step for step, and with the general kernel (MS_BA_NO_POSE_KERNEL /
MS_BA_NO_ONE_POSE_KERNEL) on the same handles.  Also: the routing edges (8 / 9 SE3 edges at the free pose, many edges between fixed poses), the hook on
recycled handles, and MS_ERR_NUMERIC."""
import ctypes as C

import numpy as np
import pytest

import ba_synth
from test_gpu_ba import _check, _pose_ba_problem, _stage1

pytestmark = pytest.mark.gpu

FORCED = ((10, 6), (12, 6), (7, 5))        # (rejections forced, max_iters): Terminate in the first iteration; the same with two spare; seven, then accepted steps


def _no_edges(p):
    q = dict(p)
    for k in ("edge_i", "edge_j", "edge_meas", "edge_info"): q[k] = p[k][:0]
    return q


def _check_forced(p, got, want, n_rej):
    """The oracle's trajectory under n forced rejections; ten or more end the solve in the first iteration with the input state restored bit for bit, and
    chi2_per_obs evaluated at that state (the header's contract), not g2o's stale last trial."""
    _check(p, got, want)
    s = got["stats"]
    if n_rej >= 10:
        assert (s["iters"], s["trials"], s["stop"]) == (1, 10, 1)
        assert np.array_equal(got["pose"], p["pose"]) and np.array_equal(got["point"], p["point"])
        assert np.allclose(got["chi2"], want["chi2"], rtol=1e-9, atol=1e-12)       # the state is the input's: only the projection's rounding may differ
    else:
        assert s["stop"] == 0 and s["trials"] == s["iters"] + n_rej and s["chi2_final"] < s["chi2_init"]
    fixed = p["pose_fixed"].astype(bool)
    assert np.array_equal(got["pose"][fixed], p["pose"][fixed])
    if p.get("point_fixed") is not None:
        pf = p["point_fixed"].astype(bool)
        assert np.array_equal(got["point"][pf], p["point"][pf])


def _stale_differs(oracle, p, iters):
    """fresh (at the returned state) and stale (g2o's edge->chi2() of the last rejected trial) must be told apart by the bar of _check_forced on this problem."""
    fresh = oracle.ba_solve(p, iters, False, force_reject=10)["chi2"]
    stale = oracle.ba_solve(p, iters, False, g2o_stale_chi2=True, force_reject=10)["chi2"]
    return not np.allclose(stale, fresh, rtol=1e-9, atol=1e-12)


def _pose_only_set():
    edge = _pose_ba_problem(11)                                                       # the odometry edge to the fixed previous keyframe
    big = ba_synth.pose_only_from_window(ba_synth.make_problem(6, 4000, 6, seed=33), 3, use_gt_points=True)
    assert len(big["obs_pose"]) > 192 * 8                                             # beyond the registers: the overflow re-evaluation runs
    return [edge, _no_edges(edge), big, _pose_ba_problem(13, 6, 60, 4, 3)]


def test_forced_rejections_on_the_pose_only_kernel(oracle, ctx, monkeypatch):
    """k_ba_pose_only keeps the pose in registers and double-buffers the chi2 per observation (c2 / c2t): the restore and the buffer swap under 10, 12 and 7
    forced rejections -- single problems (packed results, and beyond the registers) and a batch -- against the oracle and against the general kernel."""
    import mi355slam
    probs = _pose_only_set()
    assert _stale_differs(oracle, probs[0], 6) and _stale_differs(oracle, probs[2], 6)
    for n_rej, iters in FORCED:
        wants = [oracle.ba_solve(p, iters, False, force_reject=n_rej) for p in probs]
        handles = [([i], mi355slam.BundleAdjuster(ctx, [probs[i]], max_iters=iters)) for i in range(3)]
        handles.append(([0, 1, 3], mi355slam.BundleAdjuster(ctx, [probs[0], probs[1], probs[3]], max_iters=iters)))
        for idx, ba in handles:
            ba.debug_force_reject(n_rej); ba.solve()
            fast = [ba.download(k) for k in range(len(idx))]
            monkeypatch.setenv("MS_BA_NO_POSE_KERNEL", "1")
            ba.solve()
            slow = [ba.download(k) for k in range(len(idx))]
            monkeypatch.delenv("MS_BA_NO_POSE_KERNEL")
            for k, i in enumerate(idx):
                _check_forced(probs[i], fast[k], wants[i], n_rej)
                _check_forced(probs[i], slow[k], wants[i], n_rej)
                assert np.abs(fast[k]["pose"] - slow[k]["pose"]).max() < 1e-8 and np.array_equal(fast[k]["point"], slow[k]["point"])
            assert ba.team_fallbacks() == 0
            ba.close()


def _one_pose_set():
    base = ba_synth.make_problem(12, 400, 6, seed=7)
    some_fixed = _stage1(ba_synth.make_problem(9, 250, 5, seed=12), 4)
    some_fixed["point_fixed"] = (np.arange(250) % 3 == 0).astype(np.uint8)
    return [_stage1(base, 11), _stage1(base, 0), _stage1(base, 5), some_fixed]


def test_forced_rejections_on_the_one_pose_kernel(oracle, ctx, monkeypatch):
    """k_ba_one_pose writes a trial into separate buffers (trial_pose, trial[] / Xt) and copies them back only on acceptance: 10, 12 and 7 forced rejections
    on teams of 1, 2 and 8 workgroups with 1, 4 and 8 lanes per point, the current keyframe last / first / in the middle, some points fixed; a batch and a
    single window; against the oracle and the general kernel."""
    import mi355slam
    probs = _one_pose_set()
    assert _stale_differs(oracle, probs[2], 6)
    for n_rej, iters in FORCED:
        wants = [oracle.ba_solve(p, iters, False, force_reject=n_rej) for p in probs]
        ba = mi355slam.BundleAdjuster(ctx, probs, max_iters=iters)
        ba.debug_force_reject(n_rej)
        monkeypatch.setenv("MS_BA_NO_ONE_POSE_KERNEL", "1")
        ba.solve()
        slow = [ba.download(i) for i in range(len(probs))]
        monkeypatch.delenv("MS_BA_NO_ONE_POSE_KERNEL")
        for i, p in enumerate(probs):
            _check_forced(p, slow[i], wants[i], n_rej)
        for team, lanes in ((1, 1), (1, 8), (2, 4), (8, 8), (8, 1)):
            monkeypatch.setenv("MS_BA_ONE_POSE_LANES", str(lanes))
            ba.set_team(team); ba.solve()
            for i, p in enumerate(probs):
                got = ba.download(i)
                _check_forced(p, got, wants[i], n_rej)
                assert np.abs(got["pose"] - slow[i]["pose"]).max() < 1e-8 and np.abs(got["point"] - slow[i]["point"]).max() < 1e-8
            assert ba.team_fallbacks() == 0
        monkeypatch.delenv("MS_BA_ONE_POSE_LANES")
        ba.close()
        one = mi355slam.BundleAdjuster(ctx, [probs[2]], max_iters=iters)              # a single window: its descriptors ride in its own arena
        one.debug_force_reject(n_rej)
        for team in (1, 4):
            one.set_team(team); one.solve()
            _check_forced(probs[2], one.download(0), wants[2], n_rej)
        assert one.team_fallbacks() == 0
        one.close()


def _routed_problem(n_touch, n_fixed_fixed, seed):
    """poseBundleAdjust-shaped (keyframe 6 of 12 free, every point fixed at its true position) with the whole window's observations (those of the fixed keyframes
    are a constant), n_touch SE3 edges at the free keyframe and n_fixed_fixed between fixed keyframes; the edges' measurements are the true relative poses with
    a little noise, the free keyframe is on either side."""
    w = ba_synth.make_problem(12, 500, 6, seed=seed)
    rng = np.random.default_rng(seed)
    cur = 6
    p = dict(w)
    p["pose_fixed"] = np.ones(12, np.uint8); p["pose_fixed"][cur] = 0
    p["point"] = w["gt_point"].copy(); p["point_fixed"] = np.ones(500, np.uint8)
    gt = w["gt_pose"]
    others = [k for k in range(12) if k != cur]
    pairs = [(cur, cur - 1), (cur + 1, cur)]                                           # the chain's own
    pairs += [(cur, k) if j % 2 else (k, cur) for j, k in enumerate(rng.permutation(others)[:n_touch - 2])]
    pairs += [(k, k - 1) for k in range(1, 12) if cur not in (k, k - 1)]
    while len(pairs) - n_touch < n_fixed_fixed:
        a, b = rng.choice(others, 2, replace=False)
        pairs.append((int(a), int(b)))
    pairs = pairs[:n_touch + n_fixed_fixed]
    W = w["edge_info"][0].reshape(6, 6)
    meas, info = [], []
    for j, (a, b) in enumerate(pairs):
        n = np.concatenate([rng.normal(0, 0.001, 3), rng.normal(0, 0.002, 3)])
        meas.append(ba_synth._compose(ba_synth._pose(ba_synth._rotvec(n[:3]), n[3:]), ba_synth._compose(gt[b], ba_synth._inverse(gt[a]))))
        info.append(W if j % 3 else np.eye(6) * 400.0)
    p["edge_i"] = np.array([a for a, _ in pairs], np.int32); p["edge_j"] = np.array([b for _, b in pairs], np.int32)
    p["edge_meas"] = np.array(meas).reshape(-1, 7); p["edge_info"] = np.array(info).reshape(-1, 36)
    touching = int(((p["edge_i"] == cur) | (p["edge_j"] == cur)).sum())
    assert touching == n_touch and len(pairs) - touching == n_fixed_fixed
    return p


def test_pose_only_routing_edges(oracle, ctx, monkeypatch):
    """At most PO_MAXE = 8 SE3 edges at the free pose take k_ba_pose_only (9 go to the general kernel); edges between fixed poses are folded into a constant, any
    number of them.  Each against the oracle, chi2_init to 1e-10 relative (a constant term counted twice or not at all shows there), and the two kernels
    against each other."""
    import mi355slam
    probs = [_routed_problem(8, 9, 51), _routed_problem(9, 9, 52), _routed_problem(2, 24, 53), _routed_problem(8, 30, 54)]
    for iters in (3, 10):
        wants = [oracle.ba_solve(p, iters, False) for p in probs]
        for i, p in enumerate(probs):
            ba = mi355slam.BundleAdjuster(ctx, [p], max_iters=iters); ba.solve()
            got = ba.download(0)
            _check(p, got, wants[i], strict_trajectory=iters == 3)                     # (10 iterations reach rounding, where rho = 0/0 decides)
            monkeypatch.setenv("MS_BA_NO_POSE_KERNEL", "1")
            ba.solve(); slow = ba.download(0)
            monkeypatch.delenv("MS_BA_NO_POSE_KERNEL")
            _check(p, slow, wants[i], strict_trajectory=iters == 3)
            assert np.abs(got["pose"] - slow["pose"]).max() < 1e-8
            assert np.array_equal(got["pose"][p["pose_fixed"] == 1], p["pose"][p["pose_fixed"] == 1]) and np.array_equal(got["point"], p["point"])
            ba.close()
    batch = mi355slam.BundleAdjuster(ctx, [probs[0], probs[2], probs[3]], max_iters=3); batch.solve()
    wants = [oracle.ba_solve(p, 3, False) for p in (probs[0], probs[2], probs[3])]
    for k, p in enumerate((probs[0], probs[2], probs[3])):
        _check(p, batch.download(k), wants[k])
    batch.close()


def test_forced_reject_hook_does_not_outlive_its_handle(oracle, ctx):
    """The hook belongs to a handle: a handle object recycled from the context's pool starts without it, and debug_force_reject(0) switches it off on a live one."""
    import mi355slam
    for p in (_pose_ba_problem(11), _one_pose_set()[0]):
        want, forced = oracle.ba_solve(p, 3, False), oracle.ba_solve(p, 3, False, force_reject=10)
        ba = mi355slam.BundleAdjuster(ctx, [p], max_iters=3)
        ba.debug_force_reject(10); ba.solve()
        _check_forced(p, ba.download(0), forced, 10)
        ba.close()
        again = mi355slam.BundleAdjuster(ctx, [p], max_iters=3)                        # the same size: the object closed above, from the pool
        again.solve()
        _check(p, again.download(0), want)
        again.debug_force_reject(10); again.solve()
        _check_forced(p, again.download(0), forced, 10)
        again.debug_force_reject(0); again.solve()
        _check(p, again.download(0), want)
        with pytest.raises(mi355slam.MsError):
            again.debug_force_reject(256)
        again.close()


def test_numeric_error_on_the_specialised_kernels(ctx):
    """A NaN measurement in a pose-only and in a one-pose problem: ms_ba_download returns MS_ERR_NUMERIC and leaves the caller's arrays alone; the same for the
    pose-only problem through ms_ba_solve_host (the path of the poseBundleAdjust mirror)."""
    import mi355slam
    po = _pose_ba_problem(13, 6, 60, 4, 3)
    op = _stage1(ba_synth.make_problem(4, 30, 3, seed=5), 3)
    for p in (po, op):
        p["obs_uv"] = p["obs_uv"].copy(); p["obs_uv"][int(np.flatnonzero(p["obs_pose"] == int(np.flatnonzero(p["pose_fixed"] == 0)[0]))[0]), 0] = np.nan
    for p in (po, op):
        ba = mi355slam.BundleAdjuster(ctx, [p], max_iters=3)
        ba.solve()
        pose, point, chi2 = np.full(p["pose"].shape, 7.5), np.full(p["point"].shape, -2.5), np.full(len(p["obs_pose"]), 3.25)
        rc = mi355slam.lib().ms_ba_download(ba._h, 0, pose.ctypes.data_as(C.c_void_p), point.ctypes.data_as(C.c_void_p), chi2.ctypes.data_as(C.c_void_p), None)
        assert rc == -5                                                                # MS_ERR_NUMERIC
        assert (pose == 7.5).all() and (point == -2.5).all() and (chi2 == 3.25).all()
        ba.close()
    s, keep = mi355slam._ba_struct(po, 3)
    pose, point, chi2 = np.full(po["pose"].shape, 7.5), np.full(po["point"].shape, -2.5), np.full(len(po["obs_pose"]), 3.25)
    res = mi355slam.BaResultC()
    rc = mi355slam.lib().ms_ba_solve_host(ctx._h, C.byref(s), pose.ctypes.data_as(C.c_void_p), point.ctypes.data_as(C.c_void_p), chi2.ctypes.data_as(C.c_void_p), C.byref(res))
    assert rc == -5
    assert (pose == 7.5).all() and (point == -2.5).all() and (chi2 == 3.25).all()
    del keep
