"""ms_sim3_optimize (OptimizeSim3Transform on the device) against the numpy restatement in tests/sim3_opt_ref.py with jacobian="analytic".

LM trajectories are reported, never asserted (except where they are forced: max_iters 0 and 1): optimize(20) has no convergence stop, and once
the minimum is reached every accept / reject decision is the sign of a gain at rounding level.  Parity is judged on the RETURNED state, for
every scene of sim3_opt_ref.gpu_scenes() without exception: chi2_init within n_edges * 2^-52 relative (one sweep, the same terms summed in
another order), chi2_final within 1e-10 relative (unless the minimum is a zero reached to rounding, sim3_opt_ref.zero_minimum), the
reprojection residuals of the returned Sim3 (both directions) within 1e-5, chi2_final <= chi2_init.  tests/test_sim3_opt_ref.py holds the
restatement itself, summed forward and reversed, to the same bars on the same scenes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import loop_ransac_ref as lref
import sim3_opt_ref as ref

pytestmark = pytest.mark.gpu
CHI2_REL = 1e-10
RESIDUAL = 1e-5


def state(r):
    return r["R12"], r["t12"], r["scale12"]


def compare(got, prob, want):
    """Asserts the bars of one scene; returns (trajectory differs, chi2_final gap or None, residual gap)."""
    n_edges = 2 * len(prob["pts1"])
    assert abs(got["chi2_init"] - want["chi2_init"]) <= n_edges * 2.0 ** -52 * want["chi2_init"]
    assert got["chi2_final"] <= got["chi2_init"]
    res = float(np.abs(ref.residuals(state(got), prob) - ref.residuals(state(want), prob)).max()) if n_edges else 0.0
    assert res < RESIDUAL
    gap = None
    if not ref.zero_minimum(want, prob):
        gap = abs(got["chi2_final"] - want["chi2_final"]) / want["chi2_final"]
        assert gap < CHI2_REL
    if prob["max_iters"] <= 1 or n_edges == 0:
        assert got["iters"] == want["iters"]
    if prob["max_iters"] == 0 or n_edges == 0:
        assert np.array_equal(got["R12"], prob["R12"]) and np.array_equal(got["t12"], prob["t12"]) and got["scale12"] == prob["scale12"]
        assert got["trials_total"] == 0 and got["chi2_final"] == got["chi2_init"]
    if prob["fix_scale"]:
        assert got["scale12"] == prob["scale12"]                       # not a single bit
    return (got["iters"], got["trials_total"]) != (want["iters"], want["trials_total"]), gap, res


GROUPS = ref.gpu_scenes()


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_every_generated_scene(ctx, name):
    """Match counts 0, 1, 3, 63, 64, 65, 500, 5000 and one beyond the register-resident size, fix_scale on and off, max_iters 0, 1, 20;
    batches of 1, 11 and 64 with empty problems in the middle; noise-free scenes; solves started AT the minimum."""
    import mi355slam
    probs = GROUPS[name]
    got = mi355slam.sim3_optimize(ctx, probs)
    out = [compare(g, p, ref.optimize(p)) for g, p in zip(got, probs)]
    gaps = [o[1] for o in out if o[1] is not None]
    print("%s: %d scenes, (iters, trials_total) differ in %d, largest chi2_final gap %.2e relative, largest residual gap %.2e" %
          (name, len(out), sum(o[0] for o in out), max(gaps) if gaps else 0.0, max(o[2] for o in out)))


def test_non_finite_input_returns_the_initial_estimate(ctx):
    import mi355slam
    rng = np.random.default_rng(21)
    good = ref.make_scene(rng, 300)
    for key, val in (("pts2", np.nan), ("obs1", np.inf), ("pts1", -np.inf)):
        bad = dict(good)
        bad[key] = good[key].copy()
        bad[key][17, 1] = val
        (g,), (h,) = mi355slam.sim3_optimize(ctx, [bad]), mi355slam.sim3_optimize(ctx, [good])
        assert np.array_equal(g["R12"], good["R12"]) and np.array_equal(g["t12"], good["t12"]) and g["scale12"] == good["scale12"]
        assert not np.isfinite(g["chi2_final"])
        assert h["chi2_final"] < h["chi2_init"]                       # and the context is fine afterwards


def test_calls_and_batch_positions_give_the_same_bits(ctx):
    import mi355slam
    rng = np.random.default_rng(22)
    probs = [ref.make_scene(rng, n, fix_scale=bool(i % 2)) for i, n in enumerate((40, 500, 3, 64, 2500, 65, 1, 777, 300, 20, 128))]
    key = lambda r: np.r_[r["R12"].ravel(), r["t12"], r["scale12"], r["chi2_init"], r["chi2_final"], r["lam"], r["iters"], r["trials_total"], r["chi2"]].tobytes()
    a, b = mi355slam.sim3_optimize(ctx, probs, chi2=True), mi355slam.sim3_optimize(ctx, probs, chi2=True)
    assert [key(x) for x in a] == [key(x) for x in b]
    for k in (7, 4):
        (alone,) = mi355slam.sim3_optimize(ctx, [probs[k]], chi2=True)
        assert key(alone) == key(a[k])                                  # alone and at position k of a batch of 11


def test_chi2_per_edge_sums_to_chi2_final(ctx):
    import mi355slam
    rng = np.random.default_rng(23)
    probs = [ref.make_scene(rng, n) for n in (1, 64, 500, 3000)]
    for g, p in zip(mi355slam.sim3_optimize(ctx, probs, chi2=True), probs):
        assert np.array_equal(g["chi2"], ref.edge_chi2(state(g), p))     # the restatement's operations, term for term
        rho, _ = ref.huber(g["chi2"], p["huber_delta"])
        assert (rho < g["chi2"]).any() or len(rho) < 10                  # some edges lie beyond delta
        assert abs(rho.sum() - g["chi2_final"]) <= len(rho) * 2.0 ** -52 * g["chi2_final"]


def _raw_call(ctx, prob, **over):
    """ms_sim3_optimize through ctypes with sentinel-filled outputs; returns (rc, result, chi2)."""
    import mi355slam as M
    P, keep = M.sim3_opt_pack([prob])
    for k, v in over.items():
        setattr(P[0], k, v)
    res = M.Sim3OptResultC()
    res.iters, res.chi2_final = 77, -3.0
    chi2 = np.full(2 * max(len(prob["pts1"]), 1), -5.0)
    rc = M.lib().ms_sim3_optimize(ctx._h, P, 1, C.byref(res), (C.c_void_p * 1)(chi2.ctypes.data))
    return rc, res, chi2


def test_invalid_arguments_are_rejected_and_nothing_is_written(ctx):
    rng = np.random.default_rng(24)
    p = ref.make_scene(rng, 30)
    for over in (dict(n_matches=-1), dict(max_iters=-1), dict(huber_delta=float("nan")), dict(huber_delta=float("inf")), dict(pts1=None),
                 dict(obs2=None), dict(info1=None)):
        rc, res, chi2 = _raw_call(ctx, p, **over)
        assert rc == -1 and res.iters == 77 and res.chi2_final == -3.0 and (chi2 == -5.0).all(), over
    rc, res, chi2 = _raw_call(ctx, p)
    assert rc == 0 and res.iters != 77 and res.chi2_final >= 0 and (chi2 >= 0).all()


def test_capacity_is_reported(ctx):
    import mi355slam
    rng = np.random.default_rng(25)
    p = ref.make_scene(rng, 10)
    rc, res, chi2 = _raw_call(ctx, p, n_matches=(1 << 20) + 1)
    assert rc == -4 and res.iters == 77 and (chi2 == -5.0).all()
    P, keep = mi355slam.sim3_opt_pack([p])
    res = mi355slam.Sim3OptResultC()
    assert mi355slam.lib().ms_sim3_optimize(ctx._h, P, 65536, C.byref(res), None) == -4


def test_allocations_stay_flat(ctx):
    import mi355slam
    L = mi355slam.lib()
    L.ms_debug_host_allocs.restype = C.c_longlong
    rng = np.random.default_rng(26)
    probs = [ref.make_scene(rng, n) for n in (500, 64, 3000, 3, 250, 700, 65, 90, 400, 20, 128)]
    mi355slam.sim3_optimize(ctx, probs, chi2=True)
    counts = []
    for k in range(50):
        mi355slam.sim3_optimize(ctx, probs[: 1 + k % 11], chi2=bool(k % 2))
        counts.append(L.ms_debug_host_allocs())
    assert len(set(counts)) == 1


def test_end_to_end_after_matcher_and_ransac(ctx):
    """The scene of test_gpu_loop_ransac.py::test_end_to_end_after_the_loop_closure_matcher, rebuilt: ms_match_loop_closure finds the
    correspondences, ms_loop_ransac the Sim3 (its scale rounded to float), ms_sim3_optimize refines it on the union inliers."""
    import mi355slam
    rng = np.random.default_rng(9)
    n = 800
    cam = (450.0, 450.0, 320.0, 240.0, 640, 480)
    R21, t21, s21 = lref.random_rotation(rng, 0.15), np.array([0.1, -0.05, 0.2]), 1.1
    prob = lref.make_scene(rng, n, R21=R21, t21=t21, s21=s21, cam=cam, n_iter=300, min_inliers=20)
    desc1 = rng.integers(0, 2**32, (n, 8), dtype=np.uint64).astype(np.uint32)
    flip = np.packbits(rng.random((n, 256)) < 0.03, axis=1, bitorder="little").view(np.uint32)
    perm = rng.permutation(n)
    desc2 = (desc1 ^ flip)[perm]
    ang1 = rng.uniform(0, 360, n).astype(np.float32)
    ang2 = ((ang1 + 15.0) % 360).astype(np.float32)[perm]
    bucket1 = (np.arange(n) % 40).astype(np.int32)
    f1 = mi355slam.FrameOnDevice(ctx, desc1, ang1, np.ones(n, np.uint8), bucket1)
    f2 = mi355slam.FrameOnDevice(ctx, desc2, ang2, np.ones(n, np.uint8), bucket1[perm])
    counts, matched = mi355slam.match_loop_closure(ctx, [f1], [f2], 0.75, True)
    i1 = np.flatnonzero(matched[0] >= 0)
    i2 = matched[0][i1]
    assert counts[0] == len(i1) > 0.9 * n and np.array_equal(perm[i2], i1)
    p = dict(prob, pts1=prob["pts1"][i1], pts2=prob["pts2"][perm][i2], thr1=prob["thr1"][i1], thr2=prob["thr2"][perm][i2])
    (g,) = mi355slam.loop_ransac(ctx, [p], rng=rng)
    assert g["ok"] and g["union"].sum() > 0.8 * len(i1)
    u = g["union"]
    p1, p2 = p["pts1"][u], p["pts2"][u]
    sigma2 = np.array([1.2 ** (2 * l) for l in range(8)], np.float32)
    opt = dict(pts1=p1, pts2=p2, obs1=p1[:, :2] / p1[:, 2:3], obs2=p2[:, :2] / p2[:, 2:3], info1=sigma2[rng.integers(0, 8, len(p1))],
               info2=sigma2[rng.integers(0, 8, len(p1))], huber_delta=float(np.float32(np.sqrt(1e-4))), fix_scale=False, max_iters=20,
               R12=g["R12"], t12=g["t12"], scale12=float(g["scale12"]))
    (r,) = mi355slam.sim3_optimize(ctx, [opt])
    assert r["chi2_final"] <= r["chi2_init"]
    truth = (R21.T, -(1 / s21) * R21.T @ t21, 1 / s21)
    dist = lambda S: float(np.abs(ref.smap(S, p2) - ref.smap(truth, p2)).max())
    print("end to end: %d matches, %d union inliers, chi2 %.3e -> %.3e, distance to the truth %.3e -> %.3e, %d iterations" %
          (len(i1), int(u.sum()), r["chi2_init"], r["chi2_final"], dist((g["R12"], g["t12"], float(g["scale12"]))), dist(state(r)), r["iters"]))
    assert dist(state(r)) <= dist((g["R12"], g["t12"], float(g["scale12"])))


def test_mirror_batch_equals_per_object_calls():
    import test_sim3_opt_abi
    out = subprocess.run([test_sim3_opt_abi.build_smoke(), "--gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "batch ok 11 problems" in out.stdout
