"""The CPU oracle on the scenes of ba_scenes, against the extended-precision edge arithmetic of ba_ref_ld (no GPU).

Measured baseline: the largest relative gap between the oracle's chi2_init / chi2_final / chi2 per observation and ba_ref_ld evaluated at the state the
oracle returned, over every scene of a group, the three shapes (general, one free keyframe, one free keyframe with fixed points) and the short and the
full-length solve (per observation as ba_ref_ld.obs_gap measures it: relative, on the scale of 0.01 below that):

    group        chi2_init   chi2_final   per observation
    world        2.3e-15     6.6e-15      1.6e-12
    qsign        1.9e-15     3.1e-15      4.4e-13
    info         3.9e-15     3.8e-15      3.3e-13
    huber        1.7e-15     2.2e-15      5.3e-13
    edges        1.5e-14     5.1e-15      5.2e-13
    scale        1.4e-15     3.1e-15      6.4e-13
    near         9.1e-16     3.9e-15      1.3e-11
    degenerate   1.7e-15     2.6e-15      5.0e-13
    shape        2.2e-14     1.5e-14      3.8e-13
    mixed        2.1e-15     8.6e-15      3.0e-12

(ba_scenes.ORACLE_GAP holds the same numbers; test_oracle_agrees_with_extended_precision fails when the oracle is further away.)  The sums are a few ulp off;
a single observation's chi2 = info |uv - proj|^2 is a difference of two numbers of order 1 that leaves ~1e-3, squared, so 1e-16 becomes 1e-13 .. 1e-12, and
1e-11 for a point 5 cm in front of a camera.  This is the reference's own error; test_gpu_ba_domain.py takes its bars from it."""
import numpy as np
import pytest

import ba_ref_ld
import ba_scenes
import ba_synth

NAMES = [s.name for s in ba_scenes.scenes()]
MIN_GAIN = 1e-2             # the short solves' accept / reject decisions: every gain ratio at least this far from zero (rounding moves it by ~1e-12)
_measured = {}


def _solves(oracle, sc):
    for shape in ba_scenes.SHAPES:
        p = sc.shaped(shape)
        for iters in (sc.short_iters, ba_scenes.FULL_ITERS):
            yield shape, p, iters, oracle.ba_solve(p, iters, False)


def _scene_gaps(name, oracle):
    """The scene's largest gaps (cached); asserts them against the recorded baseline and the short solves' gains against MIN_GAIN."""
    if name in _measured: return _measured[name]
    sc = ba_scenes.scene(name)
    bar = ba_scenes.ORACLE_GAP[sc.group]
    worst = [0.0, 0.0, 0.0]
    for shape, p, iters, w in _solves(oracle, sc):
        st = w["stats"]
        assert np.isfinite(w["pose"]).all() and np.isfinite(w["point"]).all() and np.isfinite(st["chi2_final"])
        assert st["chi2_final"] < st["chi2_init"], (shape, iters, st)
        r0, r1 = ba_ref_ld.evaluate(p, p["pose"], p["point"]), ba_ref_ld.evaluate(p, w["pose"], w["point"])
        gaps = (ba_ref_ld.sum_gap(st["chi2_init"], r0["total"]), ba_ref_ld.sum_gap(st["chi2_final"], r1["total"]), ba_ref_ld.obs_gap(w["chi2"], r1["chi2_obs"]))
        print("%s %s iters=%d: gap to extended precision chi2_init %.1e chi2_final %.1e per observation %.1e; smallest gain ratio %.1e" % ((name, shape, iters) + gaps + (st["min_abs_gain"],)))
        for k in range(3):
            worst[k] = max(worst[k], gaps[k])
            assert gaps[k] <= bar[k], (shape, iters, k, gaps[k], bar[k])
        if iters == sc.short_iters:                  # the variant the GPU tests compare step for step: far from convergence, no decision near rounding
            assert iters <= 3 and st["stop"] == 0 and st["iters"] == iters and st["min_abs_gain"] > MIN_GAIN, (shape, st)
    _measured[name] = worst
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_oracle_agrees_with_extended_precision(name, oracle):
    _scene_gaps(name, oracle)


def _no_edge_window():
    return ba_scenes.no_edges(ba_scenes._base(101))


def _same_solve(oracle, a, b, iters, res_tol, chi2_tol):
    wa, wb = oracle.ba_solve(a, iters, False), oracle.ba_solve(b, iters, False)
    sa, sb = wa["stats"], wb["stats"]
    assert abs(sa["chi2_init"] - sb["chi2_init"]) <= chi2_tol * sa["chi2_init"]
    assert (sa["iters"], sa["trials"], sa["stop"]) == (sb["iters"], sb["trials"], sb["stop"])
    assert abs(sa["chi2_final"] - sb["chi2_final"]) <= chi2_tol * sa["chi2_final"]
    assert abs(sa["lam"] - sb["lam"]) <= 1e-6 * sa["lam"]
    ra, rb = ba_synth.residuals(a, wa["pose"], wa["point"]), ba_synth.residuals(b, wb["pose"], wb["point"])
    assert np.abs(ra - rb).max() < res_tol, np.abs(ra - rb).max()
    return wa, wb


@pytest.mark.parametrize("angle", [1.0, 2.0, 3.1])
def test_world_frame_does_not_matter_without_se3_edges(angle, oracle):
    """lambda I and the left-multiplicative pose update are invariant under a rigid change of world frame, so a window without SE3 edges takes the same LM
    trajectory and ends at the same residuals in any frame -- up to rounding: the moved window's coordinates are ~10 instead of ~1 and carry 1e-15, the
    reduced system's condition (~1e6 with the gauge held by damping alone) and three iterations multiply that: 1e-8 on the residuals, 1e-9 on the chi2."""
    rng = np.random.Generator(np.random.Philox(int(angle * 10)))
    a = _no_edge_window()
    b = ba_scenes.move_world(a, ba_scenes.random_rigid(rng, angle, 6.0))
    assert np.abs(b["pose"][:, 4:]).max() > 3 and min(2 * np.arccos(min(abs(q[3]), 1.0)) for q in b["pose"]) > angle - 0.3
    _same_solve(oracle, a, b, 3, 1e-8, 1e-9)
    _same_solve(oracle, a, ba_scenes.flip_quaternion_signs(b), 3, 1e-8, 1e-9)


@pytest.mark.parametrize("name", ["qsign_all", "qsign_half", "edges_large", "info_dense"])
def test_quaternion_sign_does_not_matter(name, oracle):
    """q and -q are the same rotation: every product the solver forms is even in q or is normalised to w >= 0 right away (SE3Quat::normalizeRotation), so a
    flipped window solves identically, SE3 edges included: the same trajectory over the full length, residuals to 1e-12."""
    sc = ba_scenes.scene(name)
    for shape in ba_scenes.SHAPES:
        a = sc.shaped(shape)
        rng = np.random.default_rng(5)
        b = ba_scenes.flip_quaternion_signs(a, rng.random(len(a["pose"])) < 0.5, rng.random(len(a["edge_i"])) < 0.5)
        assert (b["pose"][:, 3] * a["pose"][:, 3] < 0).any()
        _same_solve(oracle, a, b, ba_scenes.FULL_ITERS, 1e-12, 1e-13)


def test_catalogue_reaches_what_it_claims(oracle):
    S = {s.name: s for s in ba_scenes.scenes()}
    assert set(s.group for s in S.values()) == set(ba_scenes.GROUPS) == set(ba_scenes.ORACLE_GAP)
    for s in S.values():
        assert len(s.prob["pose"]) <= 20 and len(s.prob["point"]) <= 400
    angle = lambda q: 2 * np.arccos(min(abs(q[3]), 1.0))
    # world: every keyframe's orientation at least 0.9 rad from the identity, up to just under pi; metres of translation
    for name, a in (("world_1rad", 1.0), ("world_2rad", 2.0), ("world_3.1rad", 3.1)):
        ang = [angle(q) for q in S[name].prob["pose"]]
        assert a - 0.1 < min(ang) and max(ang) < np.pi and np.abs(S[name].prob["pose"][:, 4:]).max() > 3
    # qsign: both signs among the poses and the measurements
    for name in ("qsign_half", "qsign_world", "mixed"):
        p = S[name].prob
        assert (p["pose"][:, 3] < 0).any() and (p["pose"][:, 3] > 0).any() and (p["edge_meas"][:, 3] < 0).any() and (p["edge_meas"][:, 3] > 0).any()
    assert (S["qsign_all"].prob["pose"][:, 3] < 0).all()
    # info: full matrices, symmetric positive definite; the non-symmetric one is
    for name in ("info_dense", "info_nonsymmetric", "mixed"):
        W = S[name].prob["edge_info"].reshape(-1, 6, 6)
        off = np.abs(W[:, :3, 3:]).max(axis=(1, 2)) / np.sqrt(np.abs(W[:, 0, 0] * W[:, 3, 3]))
        assert off.min() > 0.05
        sym = np.array([np.array_equal(w, w.T) for w in W])
        assert sym.all() == (name == "info_dense") and all(np.linalg.eigvalsh(0.5 * (w + w.T)).min() > 0 for w in W)
    # edges: errors on both sides of se3_log's switch, tens of degrees, and one that is exactly the identity
    p = S["edges_small"].prob
    r = ba_ref_ld.evaluate(p, p["pose"], p["point"])
    d = np.array(r["d_edge"], np.float64)
    th = np.arccos(np.minimum(d, 1.0))
    for a in ba_scenes.SMALL_ANGLES:
        assert np.abs(th - a).min() < 1e-6
    assert ((d > 0.99999) & (th > 4.3e-3)).any() and ((d < 0.99999) & (th < 4.7e-3)).any()
    e, d_id = ba_ref_ld.se3_error(p["pose"][p["edge_i"][-1]], p["pose"][p["edge_j"][-1]], p["edge_meas"][-1])
    assert d_id == 1 and not e.any() and r["chi2_edge"][-1] == 0
    assert np.array_equal(oracle.ba_pose_edge(p["pose"][p["edge_i"][-1]], p["pose"][p["edge_j"][-1]], p["edge_meas"][-1])[0], np.zeros(6))
    p = S["edges_large"].prob
    th = np.arccos(np.array(ba_ref_ld.evaluate(p, p["pose"], p["point"])["d_edge"], np.float64))
    for a in ba_scenes.LARGE_ANGLES:
        assert np.abs(th - a).min() < 1e-6
    # huber: robustified and plain observations wherever the setting allows both
    for name, both in (("huber_0", False), ("huber_neg", False), ("huber_1e6", False), ("huber_0.5", True), ("huber_default", True), ("mixed", True)):
        p = S[name].prob
        for state in (p, oracle.ba_solve(p, ba_scenes.FULL_ITERS, False)):
            r = ba_ref_ld.evaluate(p, state["pose"], state["point"])
            robust = r["rho_obs"] < r["chi2_obs"]
            assert robust.any() == both and (~robust).any()
        assert r["chi2_obs"].max() < 1e12
    assert (ba_ref_ld.evaluate(S["huber_0"].prob, S["huber_0"].prob["pose"], S["huber_0"].prob["point"])["chi2_obs"] > 5.991).sum() > 20        # outliers are there
    # far from the optimum: the general shape's short solve rejects trials by data
    far = [s for s in S.values() if s.far]
    assert len(far) >= 2
    for s in far:
        st = oracle.ba_solve(s.prob, s.short_iters, False)["stats"]
        assert st["trials"] > st["iters"] and st["min_abs_gain"] > MIN_GAIN
    # scale
    assert np.abs(S["scale_1e3"].prob["point"]).max() > 4e3 and np.abs(S["scale_1e-3"].prob["point"]).max() < 2e-2
    # near: depths of 0.05 .. 0.2 in front of a camera, one point behind one
    p = S["near_points"].prob
    depth = lambda pose, X, o: (ba_synth._R_from_quat(pose[p["obs_pose"][o], :4]) @ X[p["obs_point"][o]] + pose[p["obs_pose"][o], 4:])[2]
    zs = np.array([depth(p["gt_pose"], p["gt_point"], o) for o in range(len(p["obs_pose"])) if p["obs_point"][o] in p["near"]])
    z0 = np.array([depth(p["pose"], p["point"], o) for o in range(len(p["obs_pose"]))])
    assert ((zs > 0.03) & (zs < 0.3)).sum() >= 10 and (zs < 0).any() and np.abs(zs).min() >= 0.03 and (z0 < 0).any() and (np.abs(z0) < 0.2).any()
    # degenerate: every feature
    p = S["degenerate"].prob; f = p["degenerate"]
    cnt = np.bincount(p["obs_point"], minlength=len(p["point"]))
    assert cnt[f["one_obs_point"]] == 1 and p["point_fixed"][f["one_obs_point"]] == 0
    assert cnt[f["no_obs_point"]] == 0 and p["point_fixed"][f["no_obs_point"]] == 0
    iso = f["isolated_pose"]
    assert p["pose_fixed"][iso] == 0 and not (p["obs_pose"] == iso).any() and not ((p["edge_i"] == iso) | (p["edge_j"] == iso)).any()
    a, b = f["double_edge"]
    assert (p["edge_i"][a], p["edge_j"][a]) == (p["edge_i"][b], p["edge_j"][b]) and not np.array_equal(p["edge_info"][a], p["edge_info"][b])
    k = f["fixed_edge"]
    assert p["pose_fixed"][p["edge_i"][k]] and p["pose_fixed"][p["edge_j"][k]]
    o = f["fixed_obs"]
    assert p["pose_fixed"][p["obs_pose"][o]] and p["point_fixed"][p["obs_point"][o]]
    a, b = f["double_obs"]
    assert (p["obs_pose"][a], p["obs_point"][a]) == (p["obs_pose"][b], p["obs_point"][b]) and not p["pose_fixed"][p["obs_pose"][a]] and not p["point_fixed"][p["obs_point"][a]]
    w = oracle.ba_solve(p, ba_scenes.FULL_ITERS, False)
    assert np.array_equal(w["pose"][iso], p["pose"][iso]) and np.array_equal(w["point"][f["no_obs_point"]], p["point"][f["no_obs_point"]])
    # shape
    p = S["pose_graph_only"].prob
    assert len(p["obs_pose"]) == 0 and len(p["point"]) == 0 and len(p["edge_i"]) > len(p["pose"])
    assert len(S["no_edges"].prob["edge_i"]) == 0 and len(S["no_edges"].prob["obs_pose"]) > 0


def test_every_scene_reaches_the_three_solvers():
    """route() is the host's rule; the shapes of a scene must land where they are meant to: the general kernel, k_ba_one_pose (stage 1's shape) and
    k_ba_pose_only (poseBundleAdjust's shape, which takes no team).  Only a window without points has nothing to offer k_ba_one_pose."""
    for s in ba_scenes.scenes():
        reached = set()
        for shape in ba_scenes.SHAPES:
            for team in (1, 4):
                r = ba_scenes.route([s.shaped(shape)], team)
                assert r == s.expected_route(shape, team), (s.name, shape, team, r)
                reached.add(r)
        assert reached == ({"general", "pose_only"} if s.name == "pose_graph_only" else {"general", "one_pose", "pose_only"}), (s.name, reached)


def test_measured_baseline_is_the_recorded_one(oracle, capsys):
    """The recorded ORACLE_GAP is the measured one rounded up, not a generous guess (at most twice what is measured)."""
    groups = {g: [0.0, 0.0, 0.0] for g in ba_scenes.GROUPS}
    for s in ba_scenes.scenes():
        groups[s.group] = [max(a, b) for a, b in zip(groups[s.group], _scene_gaps(s.name, oracle))]
    with capsys.disabled():
        print("\noracle vs extended precision, largest relative gap per group (chi2_init, chi2_final, per observation):")
        for g in ba_scenes.GROUPS:
            print("  %-11s %.1e %.1e %.1e" % ((g,) + tuple(groups[g])))
    for g in ba_scenes.GROUPS:
        for k in range(3):
            assert groups[g][k] <= ba_scenes.ORACLE_GAP[g][k] <= 2 * groups[g][k] + 1e-16, (g, k, groups[g][k])
