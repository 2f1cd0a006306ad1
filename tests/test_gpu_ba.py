"""GPU parity: bundle adjustment through the C ABI vs the CPU oracle.

Bar (north_star): final per-observation reprojection residuals within 1e-5 (normalised image units); here also the
LM trajectory (iterations, trials, lambda) must agree, and the final robust chi2 to 1e-8 relative."""
import numpy as np
import pytest

import ba_synth

pytestmark = pytest.mark.gpu
RES_TOL = 1e-5


def _check(prob, got, want, tol=RES_TOL, strict_trajectory=True):
    rg = ba_synth.residuals(prob, got["pose"], got["point"]); rw = ba_synth.residuals(prob, want["pose"], want["point"])
    assert rg.size == 0 or np.abs(rg - rw).max() < tol, np.abs(rg - rw).max()     # (a pose graph has no observations)
    if strict_trajectory:      # not meaningful once LM has converged to rounding (rho = 0/0 decides accept vs reject)
        assert got["stats"]["iters"] == want["stats"]["iters"] and got["stats"]["trials"] == want["stats"]["trials"]
        assert got["stats"]["stop"] == want["stats"]["stop"]
        assert abs(got["stats"]["lam"] - want["stats"]["lam"]) <= 1e-6 * abs(want["stats"]["lam"])
    assert abs(got["stats"]["chi2_final"] - want["stats"]["chi2_final"]) <= 1e-8 * abs(want["stats"]["chi2_final"]) + 1e-9
    assert abs(got["stats"]["chi2_init"] - want["stats"]["chi2_init"]) <= 1e-10 * abs(want["stats"]["chi2_init"])
    assert np.allclose(got["chi2"], want["chi2"], rtol=1e-4, atol=1e-6)   # chi2 = info * |r|^2 amplifies residual differences by up to 2*info*|r|


def test_small_problems_match_oracle(oracle, ctx):
    import mi355slam
    probs = [ba_synth.make_problem(8, 60, 5, seed=1), ba_synth.make_problem(3, 20, 3, seed=2, fix_first=True),
             ba_synth.make_problem(20, 300, 7, seed=3), ba_synth.make_problem(17, 111, 17, seed=4, outlier_frac=0.1)]
    ba = mi355slam.BundleAdjuster(ctx, probs, max_iters=10)
    ba.solve()
    for i, p in enumerate(probs):
        _check(p, ba.download(i), oracle.ba_solve(p, 10, False))


def test_rejected_lm_steps_follow_the_oracle(oracle, ctx):
    """Start far from the optimum: several damped solves are REJECTED (rho < 0: state restored, lambda *= nu, nu *= 2 -- the pop() path of the
    kernel), so trials > iterations.  The whole trajectory (iterations, trials, final lambda, final state) must be the oracle's, with one
    workgroup per problem and with teams (the restore sits between team barriers there)."""
    import mi355slam
    probs = []
    for seed, (npose, npt, run, sig) in enumerate([(6, 80, 5, 0.6), (6, 80, 5, 1.5), (20, 400, 6, 1.0), (12, 300, 8, 0.8)]):
        p = ba_synth.make_problem(npose, npt, run, seed=seed + 2)
        p["point"] = p["point"] + np.random.default_rng(seed).normal(0, sig, p["point"].shape)
        probs.append(p)
    wants = [oracle.ba_solve(p, 12, False) for p in probs]
    assert all(w["stats"]["trials"] > w["stats"]["iters"] for w in wants)       # every one of them rejects at least one step
    assert all(w["stats"]["chi2_final"] < 0.01 * w["stats"]["chi2_init"] for w in wants)
    for team in (1, 4):
        ba = mi355slam.BundleAdjuster(ctx, probs, max_iters=12)
        ba.set_team(team); ba.solve()
        for i, p in enumerate(probs):
            _check(p, ba.download(i), wants[i])
        assert ba.team_fallbacks() == 0
        ba.close()


def test_ten_rejected_trials_terminate_like_the_oracle(oracle, ctx):
    """g2o's Terminate: ten damped trials rejected in ONE iteration (OptimizationAlgorithmLevenberg, _maxTrialsAfterFailure = 10) end the solve with the state
    restored ten times and lambda grown by 2 * 4 * ... * 1024 = 2^55.  Rejections cannot be provoked ten times in a row by data alone without the outcome hanging
    on rounding, so the solver and the oracle share a test hook (the first n trials count as rejected): the control flow after the decision -- pop(), the lambda /
    nu schedule, qmax, the stop flag, the team barriers around the restore -- is the real one.  One workgroup per problem and teams; also a run of seven
    rejections followed by an accepted step (the solve goes on with the grown lambda), and the chi2_per_obs contract next to g2o's stale edge->chi2()."""
    import mi355slam
    probs = [ba_synth.make_problem(8, 150, 5, seed=3), ba_synth.make_problem(20, 400, 6, seed=9, outlier_frac=0.05)]
    for n_rej, iters in ((10, 6), (12, 6), (7, 5)):
        wants = [oracle.ba_solve(p, iters, False, force_reject=n_rej) for p in probs]
        if n_rej >= 10:
            assert all(w["stats"]["iters"] == 1 and w["stats"]["trials"] == 10 and w["stats"]["stop"] == 1 for w in wants)
            assert all(np.array_equal(w["pose"], p["pose"]) and np.array_equal(w["point"], p["point"]) for w, p in zip(wants, probs))      # restored, not "nearly"
        else:
            assert all(w["stats"]["stop"] == 0 and w["stats"]["trials"] == w["stats"]["iters"] + n_rej and w["stats"]["chi2_final"] < w["stats"]["chi2_init"] for w in wants)
        for team in (1, 4):
            ba = mi355slam.BundleAdjuster(ctx, probs, max_iters=iters)
            ba.set_team(team); ba.debug_force_reject(n_rej); ba.solve()
            for i, p in enumerate(probs):
                got = ba.download(i)
                _check(p, got, wants[i])
                if n_rej >= 10:
                    assert np.array_equal(got["pose"], p["pose"]) and np.array_equal(got["point"], p["point"])
            assert ba.team_fallbacks() == 0
            ba.close()
    # chi2_per_obs is evaluated at the state that is returned; g2o's edge->chi2() after a solve that ends on rejected trials is the last REJECTED trial's (oracle flag):
    # after ten rejections the two differ by a step damped 2^55 times -- measurably (the oracle has both), but far inside what the outlier rule chi2 > 5.991 can see
    fresh, stale = oracle.ba_solve(probs[0], 6, False, force_reject=10), oracle.ba_solve(probs[0], 6, False, g2o_stale_chi2=True, force_reject=10)
    d = np.abs(fresh["chi2"] - stale["chi2"]).max()
    assert 0 < d < 1e-5 and np.array_equal(fresh["chi2"] > 5.991, stale["chi2"] > 5.991)


def test_c4_local_ba_matches_oracle(oracle, ctx):
    """BASELINE config C4: 50 keyframes x 2000 points x 20000 observations, 10 LM iterations, seed 42."""
    import mi355slam
    p = ba_synth.make_problem()
    assert len(p["obs_pose"]) == 20000
    ba = mi355slam.BundleAdjuster(ctx, [p], max_iters=10)
    ba.solve()
    got = ba.download(0); want = oracle.ba_solve(p, 10, False)
    _check(p, got, want)
    r = ba_synth.residuals(p, got["pose"], got["point"])
    assert np.sqrt((r ** 2).mean()) < 1.2 / 500                   # converged to the noise floor
    # repeatable solve from the same initial state
    ba.solve()
    again = ba.download(0)
    assert np.abs(ba_synth.residuals(p, again["pose"], again["point"]) - r).max() < 1e-9


def test_reference_two_stage_schedule(oracle, ctx):
    """bundle_adjuster.cpp:245-373: stage 1 frees only the current keyframe (+ all points), stage 2 frees every pose and adds
    the soft orientation prior Omega = diag((100 r)^2 I3, 0) against the stage-1 pose; iterations = int(1 + sqrt(50)) = 8."""
    import mi355slam
    p = ba_synth.make_problem(12, 400, 6, seed=7)
    iters = int(1 + np.sqrt(50.0))
    cur = 11
    s1 = dict(p); s1["pose_fixed"] = np.ones(12, np.uint8); s1["pose_fixed"][cur] = 0
    ba = mi355slam.BundleAdjuster(ctx, [s1], max_iters=iters); ba.solve(); g1 = ba.download(0)
    w1 = oracle.ba_solve(s1, iters, False)
    _check(s1, g1, w1)
    def stage2(res):
        s2 = dict(p); s2["pose"] = np.vstack([res["pose"], res["pose"][cur:cur + 1]]); s2["point"] = res["point"]
        s2["pose_fixed"] = np.concatenate([np.zeros(12, np.uint8), [1]]).astype(np.uint8)
        W = np.zeros((6, 6)); W[:3, :3] = np.eye(3) * (100 * 100.0) ** 2
        s2["edge_i"] = np.concatenate([p["edge_i"], [12]]).astype(np.int32); s2["edge_j"] = np.concatenate([p["edge_j"], [cur]]).astype(np.int32)
        s2["edge_meas"] = np.vstack([p["edge_meas"], [[0, 0, 0, 1, 0, 0, 0]]]); s2["edge_info"] = np.vstack([p["edge_info"], W.reshape(1, 36)])
        return s2
    s2g, s2w = stage2(g1), stage2(w1)
    ba2 = mi355slam.BundleAdjuster(ctx, [s2g], max_iters=iters); ba2.solve(); g2 = ba2.download(0)
    w2 = oracle.ba_solve(s2w, iters, False)
    _check(s2w, g2, w2)
    # the prior held the current keyframe's orientation (softly)
    dq = np.abs(np.abs(g2["pose"][cur, :4] @ g1["pose"][cur, :4]) - 1)
    assert dq < 1e-6
    # the same schedule chained on the device (ms_ba_copy_state): the stage-2 handle is built from the INITIAL window (its values are
    # placeholders), takes stage 1's state and the fixed copy of the current keyframe's pose on the device, and ends where the
    # download / re-create route ended
    s2c = stage2(dict(pose=p["pose"], point=p["point"]))
    ba3 = mi355slam.BundleAdjuster(ctx, [s2c], max_iters=iters)
    ba.solve(); ba3.copy_state_from(ba, [cur]); ba3.solve()
    g3 = ba3.download(0)
    _check(s2w, g3, w2)
    assert np.abs(g3["pose"] - g2["pose"]).max() < 1e-9 and np.abs(g3["point"] - g2["point"]).max() < 1e-9
    g1b = ba.download(0)                                              # stage 1 as it ran this time (its atomic sums differ in the last bits from run to run)
    assert np.array_equal(g3["pose"][12], g1b["pose"][cur])           # the fixed extra vertex is that run's stage-1 pose, bit for bit
    # a stage 1 whose team barriers gave up is repeated by its download; the chain is then redone from the repeated solve (the recipe of the
    # host mirror localBundleAdjust): same end state
    ba.set_team(4); ba.debug_fail_team_barriers(True)
    ba.solve(); ba3.copy_state_from(ba, [cur]); ba3.solve()
    ba.debug_fail_team_barriers(False)
    ba.download(0)
    assert ba.team_fallbacks() == 1
    ba3.copy_state_from(ba, [cur]); ba3.solve()
    g4 = ba3.download(0)
    _check(s2w, g4, w2)
    with pytest.raises(mi355slam.MsError):
        ba3.copy_state_from(ba, None)                                   # one pose more than the source and nothing to fill it from
    with pytest.raises(mi355slam.MsError):
        ba.copy_state_from(ba3, None)                                   # fewer poses than the source


def test_pose_only_and_fixed_points(oracle, ctx):
    """poseBundleAdjust (bundle_adjuster.cpp:396-491): every point fixed, one pose free."""
    import mi355slam
    p = ba_synth.make_problem(6, 200, 6, seed=9)
    p["point"] = p["gt_point"].copy()
    p["point_fixed"] = np.ones(200, np.uint8); p["pose_fixed"] = np.ones(6, np.uint8); p["pose_fixed"][5] = 0
    p["edge_i"] = p["edge_i"][:0]; p["edge_j"] = p["edge_j"][:0]; p["edge_meas"] = p["edge_meas"][:0]; p["edge_info"] = p["edge_info"][:0]
    ba = mi355slam.BundleAdjuster(ctx, [p], max_iters=10); ba.solve()
    got, want = ba.download(0), oracle.ba_solve(p, 10, False)
    _check(p, got, want, strict_trajectory=False)       # a 6-dof problem converges to rounding well inside 10 iterations
    assert np.array_equal(got["point"], p["point"]) and np.array_equal(got["pose"][:5], p["pose"][:5])


def test_batch_of_c4_problems_runs_in_parallel(oracle, ctx):
    import mi355slam
    probs = [ba_synth.make_problem(50, 2000, 10, seed=100 + i) for i in range(3)]
    ba = mi355slam.BundleAdjuster(ctx, probs, max_iters=10); ba.solve()
    for i in (0, 2):
        _check(probs[i], ba.download(i), oracle.ba_solve(probs[i], 10, False))


def test_global_ba_sized_window(oracle, ctx):
    """globalBundleAdjust-sized problem (bundle_adjuster.cpp:493-604): 150 keyframes, current one fixed (:515), 12 LM iterations."""
    import mi355slam
    p = ba_synth.make_problem(150, 1500, 12, seed=77, fix_first=True)
    ba = mi355slam.BundleAdjuster(ctx, [p], max_iters=12); ba.solve()
    _check(p, ba.download(0), oracle.ba_solve(p, 12, False))


def test_global_ba_beyond_the_lds_panel(oracle, ctx):
    """More than 176 free poses: the Cholesky panel moves to global memory and the factorisation is spread over the team
    (cholesky_factor_team).  220 keyframes against the oracle at several team sizes, then 420 keyframes with a loop closure
    checked by its properties (the oracle's dense scalar Cholesky would take minutes there)."""
    import mi355slam
    p = ba_synth.make_problem(220, 2200, 12, seed=91, fix_first=True, yaw_total=0.05, z_drift=0.005)
    want = oracle.ba_solve(p, 8, False)
    for team, factor_team in ((0, 0), (1, 0), (3, 3), (32, 32), (32, 5), (16, 1)):
        ba = mi355slam.BundleAdjuster(ctx, [p], max_iters=8); ba.set_team(team); ba.set_factor_team(factor_team); ba.solve()
        _check(p, ba.download(0), want)
        ba.close()
    q = ba_synth.make_problem(420, 4000, 10, seed=92, fix_first=True, yaw_total=0.03, z_drift=0.003)
    extra = np.array([[419, 3], [300, 40]], np.int32)                    # loop-closure edges far off the band
    gp = q["gt_pose"]
    meas = [ba_synth._compose(gp[j], ba_synth._inverse(gp[i])) for i, j in extra]
    q["edge_i"] = np.concatenate([q["edge_i"], extra[:, 0]]); q["edge_j"] = np.concatenate([q["edge_j"], extra[:, 1]])
    q["edge_meas"] = np.concatenate([q["edge_meas"], np.array(meas).reshape(-1, 7)]); q["edge_info"] = np.concatenate([q["edge_info"], q["edge_info"][:2]])
    outs = []
    for team, factor_team in ((0, 0), (7, 7)):
        ba = mi355slam.BundleAdjuster(ctx, [q], max_iters=10); ba.set_team(team); ba.set_factor_team(factor_team); ba.solve()
        outs.append(ba.download(0)); ba.close()
    a, b = outs
    assert a["stats"]["chi2_final"] < 0.02 * a["stats"]["chi2_init"]
    r = ba_synth.residuals(q, a["pose"], a["point"])
    assert np.sqrt((r ** 2).mean()) < 1.2 / 500                               # the noise floor
    assert np.abs(r - ba_synth.residuals(q, b["pose"], b["point"])).max() < 1e-7  # team size does not change the solve
    assert a["stats"]["iters"] == b["stats"]["iters"] and a["stats"]["trials"] == b["stats"]["trials"]


def test_team_of_workgroups_matches_single_workgroup_and_oracle(oracle, ctx):
    """ms_ba_set_team: one problem spread over 1 .. 32 workgroups (grid barriers, agent-scope release / acquire) gives the
    oracle's result at every team size -- C4, a pose-only problem, a window with outliers and a batch of 3 with teams of 7."""
    import mi355slam
    c4 = ba_synth.make_problem(50, 2000, 10, seed=42)
    want = oracle.ba_solve(c4, 10, False)
    for team in (1, 2, 5, 16, 32):
        ba = mi355slam.BundleAdjuster(ctx, [c4], max_iters=10); ba.set_team(team); ba.solve()
        _check(c4, ba.download(0), want)
        ba.solve()                                                   # a second launch on the same (monotonic) barrier counter
        _check(c4, ba.download(0), want)
        ba.close()
    po = dict(c4); po["pose_fixed"] = np.ones(50, np.uint8); po["pose_fixed"][49] = 0; po["point_fixed"] = np.ones(2000, np.uint8)
    ba = mi355slam.BundleAdjuster(ctx, [po], max_iters=10); ba.set_team(8); ba.solve()
    _check(po, ba.download(0), oracle.ba_solve(po, 10, False), strict_trajectory=False)
    ba.close()
    probs = [ba_synth.make_problem(20, 400, 6, seed=200 + i, outlier_frac=0.05) for i in range(3)]
    ba = mi355slam.BundleAdjuster(ctx, probs, max_iters=8); ba.set_team(7); ba.solve()
    for i in range(3):
        _check(probs[i], ba.download(i), oracle.ba_solve(probs[i], 8, False))
    with pytest.raises(mi355slam.MsError):
        ba.set_team(65)
    ba.close()


def test_team_barriers_hold_beside_a_saturating_front_end_batch(oracle):
    """The workgroup hand-offs of a team solve with another stream keeping every CU busy (uneven barrier arrival, warm caches):
    every launch must reproduce the single-workgroup result and none may hang."""
    import mi355slam
    ca, cb = mi355slam.Context(0), mi355slam.Context(0)
    frames = np.stack([oracle.synth_frame(1280, 720, 1000 + i, 2 * (i % 8), i % 8) for i in range(8)])
    frames = np.concatenate([frames] * 8)
    buf = ca.upload(frames)
    ex = mi355slam.OrbExtractor(ca, 1280, 720, max_batch=64)
    prob = ba_synth.make_problem(50, 2000, 10, seed=42)
    ba = mi355slam.BundleAdjuster(cb, [prob], max_iters=10)
    ba.set_team(1); ba.solve(); cb.sync()
    ref = ba.download(0)
    for it in range(12):
        for _ in range(3): ex.extract(buf, n_frames=64, frame_stride=1280 * 720, row_stride=1280)
        ba.set_team((2, 7, 16, 32)[it % 4]); ba.solve()
        cb.sync(); ca.sync()
        out = ba.download(0)
        assert out["stats"]["iters"] == ref["stats"]["iters"] and out["stats"]["trials"] == ref["stats"]["trials"], it
        assert abs(out["stats"]["chi2_final"] - ref["stats"]["chi2_final"]) <= 1e-9 * abs(ref["stats"]["chi2_final"]), it
        assert np.abs(out["pose"] - ref["pose"]).max() < 1e-9 and np.abs(out["point"] - ref["point"]).max() < 1e-9, it
    ba.close(); ca.close(); cb.close()


def test_points_seen_by_more_than_64_keyframes_take_the_record_path(oracle, ctx):
    """The fused Schur pass packs a point's observations into the 64 lanes of a wave; a window in which a point has more free observations
    than that keeps the record-based path (Hpl / Y records, pose-pair segments, left-looking Cholesky).  Both paths must give the oracle's
    result -- here in one batch: a 72-keyframe window whose points are seen by 70 consecutive keyframes next to an ordinary one -- and ragged
    visibility (2 .. 40 observations per point, scattered over the window) must go through the fused path's sort-based batching."""
    import mi355slam
    wide = ba_synth.make_problem(72, 150, 70, seed=31)
    assert np.bincount(wide["obs_point"]).max() == 70
    rng = np.random.default_rng(5)
    rag = ba_synth.make_problem(40, 500, 6, seed=32)
    op, ol, uv, info = list(rag["obs_pose"]), list(rag["obs_point"]), list(rag["obs_uv"]), list(rag["obs_info"])
    seen = set(zip(op, ol))
    for l in range(0, 500, 3):                                        # every third point gets up to 34 more observations anywhere in the window
        for i in rng.choice(40, size=int(rng.integers(1, 35)), replace=False):
            q = ba_synth._R_from_quat(rag["gt_pose"][i, :4]) @ rag["gt_point"][l] + rag["gt_pose"][i, 4:]
            if q[2] < 0.5 or (int(i), l) in seen: continue
            seen.add((int(i), l)); op.append(int(i)); ol.append(l); uv.append(q[:2] / q[2] + rng.normal(0, 1 / 500, 2)); info.append(500.0 ** 2)
    rag["obs_pose"], rag["obs_point"] = np.array(op, np.int32), np.array(ol, np.int32)
    rag["obs_uv"], rag["obs_info"] = np.array(uv), np.array(info)
    assert 30 < np.bincount(rag["obs_point"]).max() <= 40
    probs = [wide, rag, ba_synth.make_problem(20, 300, 7, seed=33)]
    want = [oracle.ba_solve(p, 8, False) for p in probs]
    for team in (1, 4):
        ba = mi355slam.BundleAdjuster(ctx, probs, max_iters=8); ba.set_team(team); ba.solve()
        for i, p in enumerate(probs):
            _check(p, ba.download(i), want[i])
        ba.close()


def test_two_contexts_solve_with_teams_at_the_same_time(oracle):
    """SURVEY 8(b) threading: poseBundleAdjust on the front-end thread beside localBundleAdjust on the back-end thread
    (mapper.cpp:379-390 vs :268-269) = two handles on two contexts, both with teams whose grids together exceed the chip
    (2 x 4 x 40 workgroups of one per CU > 256).  Team launches of a process are chained per device, so neither may give up."""
    import threading
    import mi355slam
    ca, cb = mi355slam.Context(0), mi355slam.Context(0)
    probs = [ba_synth.make_problem(30, 600, 8, seed=300 + i) for i in range(4)]
    want = [oracle.ba_solve(p, 8, False) for p in probs]
    bas = [mi355slam.BundleAdjuster(c, probs, max_iters=8) for c in (ca, cb)]
    for b in bas: b.set_team(40)
    errs = []

    def run(b, c):
        try:
            for _ in range(6):
                b.solve()
            c.sync()
        except Exception as e:                                      # noqa: BLE001 -- reported below
            errs.append(e)
    th = [threading.Thread(target=run, args=(b, c)) for b, c in zip(bas, (ca, cb))]
    for t in th: t.start()
    for t in th: t.join()
    assert not errs, errs
    for b in bas:
        for i in range(4):
            _check(probs[i], b.download(i), want[i])
        assert b.team_fallbacks() == 0
        b.close()
    ca.close(); cb.close()


def test_team_barrier_give_up_falls_back_to_one_workgroup(oracle, ctx):
    """A team barrier that gives up (test hook: every barrier of the launch falls through at once, so the team's result is
    garbage) must not reach the caller: ms_ba_download repeats the solve with one workgroup per problem and returns that."""
    import mi355slam
    probs = [ba_synth.make_problem(20, 400, 6, seed=210 + i) for i in range(2)]
    ba = mi355slam.BundleAdjuster(ctx, probs, max_iters=8)
    ba.set_team(8); ba.debug_fail_team_barriers(True); ba.solve()
    for i in range(2):
        _check(probs[i], ba.download(i), oracle.ba_solve(probs[i], 8, False))
    assert ba.team_fallbacks() == 1
    ba.debug_fail_team_barriers(False); ba.solve()                  # the next launch uses the team again
    _check(probs[0], ba.download(0), oracle.ba_solve(probs[0], 8, False))
    assert ba.team_fallbacks() == 1
    ba.close()


def test_failed_solve_leaves_the_callers_arrays_untouched(ctx):
    """ms_ba_download reads the status first: MS_ERR_NUMERIC must not overwrite pose / point (the host mirrors pass the window's
    own arrays as outputs).  A point observed once from one pose with zero damping room: NaN measurement -> non-finite state."""
    import ctypes as C
    import mi355slam
    p = ba_synth.make_problem(4, 30, 3, seed=5)
    p["obs_uv"] = p["obs_uv"].copy(); p["obs_uv"][0, 0] = np.nan
    ba = mi355slam.BundleAdjuster(ctx, [p], max_iters=3)
    ba.solve()
    pose, point = np.full((4, 7), 7.5), np.full((30, 3), -2.5)
    rc = mi355slam.lib().ms_ba_download(ba._h, 0, pose.ctypes.data_as(C.c_void_p), point.ctypes.data_as(C.c_void_p), None, None)
    assert rc == -5                                                  # MS_ERR_NUMERIC, also without a result struct
    assert (pose == 7.5).all() and (point == -2.5).all()
    ba.close()


def test_envelope_with_loop_closure_and_scattered_covisibility(oracle, ctx):
    """The Cholesky skips what lies outside the envelope of the reduced camera matrix; a loop-closure edge between far keyframes,
    points seen by scattered keyframes and fixed poses in the middle must all widen / shift it correctly (batch and team)."""
    import mi355slam
    p = ba_synth.make_problem(40, 700, 6, seed=11)
    rng = np.random.default_rng(3)
    gt_pose, gt_point = p["gt_pose"], p["gt_point"]
    # 25 extra observations: old points re-observed by keyframes far from their run (covisibility off the band)
    op, ol, uv, info = list(p["obs_pose"]), list(p["obs_point"]), list(p["obs_uv"]), list(p["obs_info"])
    for _ in range(25):
        l, i = int(rng.integers(0, 700)), int(rng.integers(0, 40))
        q = ba_synth._R_from_quat(gt_pose[i, :4]) @ gt_point[l] + gt_pose[i, 4:]
        if q[2] < 0.5: continue
        op.append(i); ol.append(l); uv.append(q[:2] / q[2] + rng.normal(0, 1 / 500, 2)); info.append(500.0 ** 2)
    p["obs_pose"], p["obs_point"] = np.array(op, np.int32), np.array(ol, np.int32)
    p["obs_uv"], p["obs_info"] = np.array(uv), np.array(info)
    # a loop-closure edge between keyframes 3 and 37 (makeLoopClosureEdge, bundle_adjuster.cpp:87-111)
    M = ba_synth._compose(gt_pose[37], ba_synth._inverse(gt_pose[3]))
    p["edge_i"] = np.append(p["edge_i"], 3).astype(np.int32); p["edge_j"] = np.append(p["edge_j"], 37).astype(np.int32)
    p["edge_meas"] = np.vstack([p["edge_meas"], M[None]]); p["edge_info"] = np.vstack([p["edge_info"], (np.eye(6) * 400.0).reshape(1, 36)])
    p["pose_fixed"] = p["pose_fixed"].copy(); p["pose_fixed"][[0, 17, 18]] = 1
    want = oracle.ba_solve(p, 8, False)
    for team in (1, 6):
        ba = mi355slam.BundleAdjuster(ctx, [p, p], max_iters=8); ba.set_team(team); ba.solve()
        _check(p, ba.download(0), want); _check(p, ba.download(1), want)
        ba.close()


def test_randomised_windows_fuzz_tool():
    """tools/ba_fuzz.py on 120 random windows (2..70 keyframes, ragged visibility, fixed poses and points, outliers, loop closures, pose-only cases;
    pose-only batches; alone / batched / on teams of 2, 5, 16; some with forced rejections): residuals within 1e-7 of the oracle's (the tool's own bar; the contract is 1e-5), LM trajectory equal unless the solve had converged."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "ba_fuzz.py"), "120", "2024"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "0 mismatches" in r.stdout
    import re
    m = re.search(r"routes: pose_only=(\d+) one_pose=(\d+) general=(\d+)", r.stdout)
    assert m and all(int(k) > 0 for k in m.groups()), r.stdout[-2000:]                   # every solver was reached


def _pose_ba_problem(seed, n_pose=12, n_point=900, run=8, cur=6):
    return ba_synth.pose_only_from_window(ba_synth.make_problem(n_pose, n_point, run, seed=seed), cur, use_gt_points=True)


def _far_pose_ba_problem():
    """_pose_ba_problem(11) with the free pose rolled by 45 degrees and moved 3.9 m along its optical axis: the oracle rejects trials by data in the first
    three iterations (a start nearer the optimum is not enough: the Huber kernel's IRLS steps always gain there)."""
    p = _pose_ba_problem(11)
    p["pose"] = p["pose"].copy()
    p["pose"][0] = ba_synth._compose(ba_synth._pose(ba_synth._rotvec(np.radians(45.0) * np.array([0.0, 0.0, 1.0])), np.array([0.0, 0.0, -3.9])), p["pose"][0])
    return p


def test_pose_only_kernel_equals_the_general_solver_and_the_oracle(oracle, ctx, monkeypatch):
    """One free pose + fixed points goes to k_ba_pose_only (one workgroup keeps a trial in registers); the same problems through the general kernel
    (MS_BA_NO_POSE_KERNEL) and through the oracle: the same LM trajectory and end state.  With the odometry edge to the fixed previous keyframe, without any
    edge, with outliers (Huber active), and as a batch."""
    import mi355slam
    probs = [_pose_ba_problem(11), _pose_ba_problem(12, 20, 2500, 14, 9), _pose_ba_problem(13, 6, 60, 4, 3)]
    no_edge = dict(probs[0]); no_edge["edge_i"] = no_edge["edge_i"][:0]; no_edge["edge_j"] = no_edge["edge_j"][:0]; no_edge["edge_meas"] = no_edge["edge_meas"][:0]; no_edge["edge_info"] = no_edge["edge_info"][:0]
    outl = dict(probs[1]); outl["obs_uv"] = outl["obs_uv"].copy(); outl["obs_uv"][::9] += 0.05
    probs += [no_edge, outl]
    assert min(len(q["obs_pose"]) for q in probs[:2]) > 300
    wants = [oracle.ba_solve(q, 12, False) for q in probs]
    far = _far_pose_ba_problem()
    far3 = oracle.ba_solve(far, 3, False)
    assert far3["stats"]["trials"] > far3["stats"]["iters"]                                      # rejected by data, not by rounding
    ba = mi355slam.BundleAdjuster(ctx, probs, max_iters=12); ba.solve()
    fast = [ba.download(i) for i in range(len(probs))]
    monkeypatch.setenv("MS_BA_NO_POSE_KERNEL", "1")
    ba.solve()
    slow = [ba.download(i) for i in range(len(probs))]
    monkeypatch.delenv("MS_BA_NO_POSE_KERNEL")
    for i, q in enumerate(probs):
        _check(q, fast[i], wants[i], strict_trajectory=False)
        _check(q, slow[i], wants[i], strict_trajectory=False)
        assert np.abs(fast[i]["pose"] - slow[i]["pose"]).max() < 1e-8 and np.array_equal(fast[i]["point"], q["point"])
        assert fast[i]["stats"]["chi2_final"] < fast[i]["stats"]["chi2_init"]
        assert np.array_equal(fast[i]["pose"][1:], q["pose"][1:])                                   # the fixed keyframe did not move
    # the first iterations (far from convergence, where accept / reject is not decided by rounding) follow the oracle step for step
    for q in probs[:2] + [far]:
        w3 = oracle.ba_solve(q, 3, False)
        b3 = mi355slam.BundleAdjuster(ctx, [q], max_iters=3); b3.solve(); g3 = b3.download(0)
        _check(q, g3, w3)
        monkeypatch.setenv("MS_BA_NO_POSE_KERNEL", "1")
        b3.solve(); s3 = b3.download(0)
        monkeypatch.delenv("MS_BA_NO_POSE_KERNEL")
        _check(q, s3, w3)
        b3.close()
    ba.close()


def test_per_frame_pose_problems_through_recycled_handles(oracle, ctx):
    """The per-frame path (mapper_helpers.cpp:1043-1050: a NEW poseBundleAdjust problem per frame): handle objects, device blocks, the page-locked staging and result blocks
    are recycled from problem to problem -- small, large, single and batched problems in turn, each checked against the oracle.  Covers: results packed behind the launch
    (single problems up to 64 KB) and fetched the ordinary way (beyond, and batches); uploads staged without a wait (several problems side by side in the staging block) and
    the per-problem path (a batch beyond the block); more observations than k_ba_pose_only keeps in registers (192 threads x 8) and none at all in the last slots; a second
    solve of the same handle; a download without chi2."""
    import mi355slam
    small = _pose_ba_problem(31, 6, 60, 4, 3)
    mid = _pose_ba_problem(32)
    big = ba_synth.pose_only_from_window(ba_synth.make_problem(6, 4000, 6, seed=33), 3, use_gt_points=True)       # every point seen by every keyframe: 4000 observations of the free pose
    assert len(big["obs_pose"]) > 192 * 8 and len(small["obs_pose"]) < 192 < len(mid["obs_pose"])
    want = {id(q): oracle.ba_solve(q, 10, False) for q in (small, mid, big)}
    for rep, batch in enumerate([[small], [big], [mid], [small, mid, small], [mid] * 20, [small], [big, small], [mid] * 300, [small], [mid]] * 2):
        ba = mi355slam.BundleAdjuster(ctx, batch, max_iters=10)
        ba.solve()
        for i in (0, len(batch) - 1):
            _check(batch[i], ba.download(i), want[id(batch[i])], strict_trajectory=False)
        if rep % 3 == 0:                                                   # the same handle again: the eager results of the second launch, not the first's
            ba.solve()
            _check(batch[0], ba.download(0), want[id(batch[0])], strict_trajectory=False)
        ba.close()


def _stage1(p, cur):
    s = dict(p); s["pose_fixed"] = np.ones(len(p["pose"]), np.uint8); s["pose_fixed"][cur] = 0
    return s


def test_one_pose_kernel_equals_the_general_solver_and_the_oracle(oracle, ctx, monkeypatch):
    """Stage 1 of localBundleAdjust (bundle_adjuster.cpp:251-252, :322-333: only the current keyframe free, every point free) goes to k_ba_one_pose.  The same
    windows through the general kernel (MS_BA_NO_ONE_POSE_KERNEL) and through the oracle: the same LM trajectory and end state -- one workgroup per window,
    teams of 2 .. 16 workgroups, 1 .. 8 lanes per point, the current keyframe first / last / in the middle, some points fixed, outliers under the Huber
    kernel, a start far from the optimum (rejected steps), and the 50-keyframe window of the bench."""
    import mi355slam
    iters = 8
    base = ba_synth.make_problem(12, 400, 6, seed=7)
    far = _stage1(ba_synth.make_problem(12, 300, 8, seed=5), 11)
    far["point"] = far["point"] + np.random.default_rng(3).normal(0, 4.0, far["point"].shape)
    some_fixed = _stage1(ba_synth.make_problem(9, 250, 5, seed=12), 4)
    some_fixed["point_fixed"] = (np.arange(250) % 3 == 0).astype(np.uint8)
    outl = _stage1(ba_synth.make_problem(17, 111, 17, seed=4, outlier_frac=0.1), 16)
    probs = [_stage1(base, 11), _stage1(base, 0), _stage1(base, 5), far, some_fixed, outl, _stage1(ba_synth.make_problem(), 49)]
    wants = [oracle.ba_solve(q, iters, False) for q in probs]
    assert wants[3]["stats"]["trials"] > wants[3]["stats"]["iters"]                     # the far start rejects at least one step
    ba = mi355slam.BundleAdjuster(ctx, probs, max_iters=iters)
    monkeypatch.setenv("MS_BA_NO_ONE_POSE_KERNEL", "1")
    ba.solve()
    slow = [ba.download(i) for i in range(len(probs))]
    monkeypatch.delenv("MS_BA_NO_ONE_POSE_KERNEL")
    for team, lanes in ((1, None), (1, 2), (2, None), (5, 4), (16, None), (16, 1), (8, 8)):
        if lanes is None: monkeypatch.delenv("MS_BA_ONE_POSE_LANES", raising=False)
        else: monkeypatch.setenv("MS_BA_ONE_POSE_LANES", str(lanes))
        ba.set_team(team); ba.solve()
        for i, q in enumerate(probs):
            got = ba.download(i)
            _check(q, got, wants[i])
            assert np.abs(got["pose"] - slow[i]["pose"]).max() < 1e-8 and np.abs(got["point"] - slow[i]["point"]).max() < 1e-8
            fixed = q["pose_fixed"].astype(bool)
            assert np.array_equal(got["pose"][fixed], q["pose"][fixed])                 # the fixed keyframes did not move
            if q.get("point_fixed") is not None:
                pf = q["point_fixed"].astype(bool)
                assert np.array_equal(got["point"][pf], q["point"][pf])
        assert ba.team_fallbacks() == 0
    monkeypatch.delenv("MS_BA_ONE_POSE_LANES", raising=False)
    for i, q in enumerate(probs):
        _check(q, slow[i], wants[i])
    ba.close()
    # one window alone picks its team and lanes by itself
    one = mi355slam.BundleAdjuster(ctx, [probs[6]], max_iters=iters); one.solve()
    _check(probs[6], one.download(0), wants[6])
    one.close()
    # more keyframes than the LDS pose table takes (512): the poses are read from memory; more lanes than points on one workgroup (a lane group per point
    # without a team); and a window whose points outnumber the lanes of its team (several points per group, records in memory)
    long_w = ba_synth.make_problem(530, 120, 4, seed=21, z_drift=0.004)
    for k in ("edge_i", "edge_j", "edge_meas", "edge_info"): long_w[k] = long_w[k][-100:]
    long_w = _stage1(long_w, 529)
    small = _stage1(ba_synth.make_problem(5, 40, 4, seed=22), 2)
    for q, team in ((long_w, 1), (long_w, 3), (small, 1), (probs[6], 2)):
        b = mi355slam.BundleAdjuster(ctx, [q], max_iters=4); b.set_team(team); b.solve()
        _check(q, b.download(0), oracle.ba_solve(q, 4, False))
        b.close()
