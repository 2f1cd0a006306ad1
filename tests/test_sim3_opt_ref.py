"""The numpy restatement of OptimizeSim3Transform (tests/sim3_opt_ref.py) against answers known by construction.  It is the specification
of ms_sim3_optimize, so it is checked on its own first: the group operations, the analytic Jacobian against differences of its own error
function, recovery of a known Sim3, the Huber kernel, the g2o-style numeric Jacobian against the analytic one, and -- for every scene the
GPU tests run -- that summing the edges in reversed order moves the RETURNED state by less than the bars the device is held to.

LM trajectories (iters, trials_total) are printed, never asserted: optimize(20) has no convergence stop, so once the minimum is reached every
accept / reject decision is the sign of a gain at rounding level, and another summation order legitimately takes another path."""
import numpy as np
import pytest

import sim3_opt_ref as ref

CHI2_REL = 1e-10          # chi2_final of two legitimate evaluations of the same solve (the bar tools/ba_fuzz.py uses when trajectories differ)
RESIDUAL = 1e-5           # the project's residual contract (BASELINE.json north star)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def test_exp_at_zero_is_the_identity():
    R, t, s = ref.sim3_exp(np.zeros(7))
    assert np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3)) and s == 1.0


def test_exp_of_a_times_exp_of_minus_a_is_the_identity():
    """R to rounding.  t carries the cancellation of g2o's general formulas just above their eps branches: (e^sigma - 1) / sigma has a
    relative rounding of 2^-53 / eps = 1.1e-11 at |sigma| = eps, (1 - cos theta) / theta^2 one of 2^-53 / eps^2 = 1.1e-6 times |Omega| = eps;
    both fall with growing argument, so 1e-10 |a| bounds the product of two exponentials.  Below eps the branch C = 1 drops sigma / 2 from
    (e^sigma - 1) / sigma in each factor, so there the product's translation is (1 - e^sigma) upsilon: up to eps |upsilon|."""
    rng = np.random.default_rng(0)
    for k in range(50):
        a = rng.normal(size=7) * (10.0 ** rng.uniform(-7, 0))
        if k % 5 == 0:
            a[:3] = 0
        if k % 7 == 0:
            a[6] = 0
        R, t, s = ref.mul(ref.sim3_exp(a), ref.sim3_exp(-a))
        scale = max(1.0, np.abs(a).max())
        assert np.abs(R - np.eye(3)).max() < 1e-13 * scale and abs(s - 1) < 1e-14
        assert np.abs(t).max() < 1e-10 * scale + (ref.EPS * np.abs(a[3:6]).max() if abs(a[6]) < ref.EPS else 0.0)


def test_small_branches_meet_the_general_formulas_at_eps():
    """At theta = eps and |sigma| = eps the branch formulas and the general ones differ by their first dropped Taylor term and by the
    cancellation of the general ones (1 - cos theta has an absolute rounding of 2^-53 against theta^2 / 2 = 5e-11: 2e-6 relative):
    the rotation terms are multiplied by |Omega| = eps, so R meets to eps * 1e-5 = 1e-10; C = 1 against (e^sigma - 1) / sigma = 1 + sigma / 2
    multiplies upsilon directly, so t meets to eps |upsilon| (1e-5 relative), the size of the jump g2o's branches really have."""
    rng = np.random.default_rng(1)
    for _ in range(20):
        w = rng.normal(size=3)
        w *= ref.EPS / np.linalg.norm(w)
        up = rng.normal(size=3)
        for sg in (ref.EPS, -ref.EPS, 0.3, 0.0):
            dx = np.r_[w, up, sg]
            small_sigma = abs(sg) < ref.EPS
            Ra, ta, sa = ref.sim3_exp(dx, force=(small_sigma, True))
            Rb, tb, sb = ref.sim3_exp(dx, force=(small_sigma, False))
            assert np.abs(Ra - Rb).max() < 1e-10 and np.abs(ta - tb).max() < ref.EPS * np.abs(up).max() and sa == sb
        for th in (0.2, 0.0):
            w2 = w * (th / ref.EPS)
            for sg in (ref.EPS, -ref.EPS):
                dx = np.r_[w2, up, sg]
                Ra, ta, sa = ref.sim3_exp(dx, force=(True, th < ref.EPS))
                Rb, tb, sb = ref.sim3_exp(dx, force=(False, th < ref.EPS))
                assert np.array_equal(Ra, Rb) and np.abs(ta - tb).max() < ref.EPS * np.abs(up).max() and sa == sb


def test_a_sim3_times_its_inverse_maps_points_to_themselves():
    rng = np.random.default_rng(2)
    for _ in range(20):
        S = ref.sim3_exp(rng.normal(size=7) * 0.5)
        p = rng.normal(size=(30, 3)) * 5
        assert np.abs(ref.smap(ref.mul(S, ref.inverse(S)), p) - p).max() < 1e-13
        assert np.abs(ref.smap(ref.inverse(S), ref.smap(S, p)) - p).max() < 1e-13
        A, B = ref.sim3_exp(rng.normal(size=7) * 0.5), S
        assert np.abs(ref.smap(ref.mul(A, B), p) - ref.smap(A, ref.smap(B, p))).max() < 1e-12


@pytest.mark.parametrize("fix", [False, True])
def test_analytic_jacobian_against_central_differences(fix):
    """Central differences of the restatement's own error function at step 1e-6: rounding about 2^-52 / 1e-6 = 2e-10, truncation about
    1e-12 (h^2 times a third derivative of order one), so 1e-7 relative to the Jacobian's scale is derived, not tuned.  Both edge types
    (even rows: edge 12, odd rows: edge 21)."""
    rng = np.random.default_rng(3 + fix)
    prob = ref.make_scene(rng, 40, fix_scale=fix)
    S = ref.initial(prob)
    Ja = ref.jacobians(S, prob, "analytic")
    Jn = ref.jacobians(S, prob, "g2o", step=1e-6)
    for rows in (slice(0, None, 2), slice(1, None, 2)):
        scale = max(1.0, np.abs(Ja[rows]).max())
        assert np.abs(Ja[rows] - Jn[rows]).max() < 1e-7 * scale
        assert np.abs(Ja[rows][:, :, :6]).max() > 0.1
    if fix:
        assert not Ja[:, :, 6].any() and not Jn[:, :, 6].any()
    else:
        assert np.abs(Ja[1::2, :, 6]).max() > 1e-3                   # the inverse edge sees the scale; the forward edge's projection does not
        assert np.abs(Ja[0::2, :, 6]).max() < 1e-12


def sim3_distance(S, T, pts):
    return float(np.abs(ref.smap(S, pts) - ref.smap(T, pts)).max())


@pytest.mark.parametrize("fix", [False, True])
def test_noise_free_scene_returns_to_the_truth(fix):
    rng = np.random.default_rng(5 + fix)
    for n in (10, 100):
        prob = ref.make_scene(rng, n, fix_scale=fix, noise=0.0, outliers=0.0)
        out = ref.optimize(prob)
        S = (out["R12"], out["t12"], out["scale12"])
        assert sim3_distance(ref.initial(prob), prob["truth"], prob["pts2"]) > 1e-2
        assert sim3_distance(S, prob["truth"], prob["pts2"]) < 1e-9
        assert out["chi2_final"] < 1e-18 * out["chi2_init"] or out["chi2_final"] < 1e-20
        if fix:
            assert np.float64(out["scale12"]).view(np.uint64) == np.float64(prob["scale12"]).view(np.uint64)   # not a single bit


def test_huber_lands_nearer_the_truth_than_no_kernel():
    rng = np.random.default_rng(7)
    nearer = 0
    for _ in range(10):
        prob = ref.make_scene(rng, 200, noise=0.0005, outliers=0.15)
        assert prob["outlier_mask"].sum() > 10
        a = ref.optimize(prob)
        b = ref.optimize(dict(prob, huber_delta=0.0))                # delta <= 0: the kernel is off
        da = sim3_distance((a["R12"], a["t12"], a["scale12"]), prob["truth"], prob["pts2"])
        db = sim3_distance((b["R12"], b["t12"], b["scale12"]), prob["truth"], prob["pts2"])
        nearer += da < db
    assert nearer == 10


def test_edges_of_the_contract():
    rng = np.random.default_rng(8)
    prob = ref.make_scene(rng, 50, max_iters=0)
    out = ref.optimize(prob)
    assert out["iters"] == 0 and out["trials_total"] == 0 and np.array_equal(out["R12"], prob["R12"]) and out["chi2_final"] == out["chi2_init"] > 0
    out = ref.optimize(ref.empty_problem())
    assert out["iters"] == 0 and out["chi2_init"] == 0 and out["scale12"] == 1.25 and np.array_equal(out["t12"], [0.1, 0.2, 0.3])
    one = ref.optimize(dict(prob, max_iters=1))
    assert one["iters"] == 1 and 1 <= one["trials_total"] <= 10 and one["chi2_final"] <= one["chi2_init"]
    bad = dict(prob, max_iters=20, pts2=prob["pts2"].copy())
    bad["pts2"][7, 1] = np.nan                                       # non-finite input: every trial rejected, the initial estimate comes back
    out = ref.optimize(bad)
    assert np.array_equal(out["R12"], prob["R12"]) and np.array_equal(out["t12"], prob["t12"]) and out["scale12"] == prob["scale12"]
    assert out["stop_reason"] == 1 and not np.isfinite(out["chi2_final"])


def test_numeric_and_analytic_jacobians_end_at_the_same_minimum():
    """g2o's central difference (step 1e-9, about 1e-7 of relative noise in J) against the analytic derivative: 40 scenes of 3-300 matches with
    10 % outliers, 20 iterations.  Judged on the returned state at the residual contract; the chi2 gap is printed (DESIGN 9.3 records it)."""
    rng = np.random.default_rng(9)
    worst_chi2, worst_res = 0.0, 0.0
    for i in range(40):
        prob = ref.make_scene(rng, int(rng.choice([3, 20, 64, 300])), fix_scale=bool(i % 2))
        a, g = ref.optimize(prob, "analytic"), ref.optimize(prob, "g2o")
        ra = ref.residuals((a["R12"], a["t12"], a["scale12"]), prob)
        rg = ref.residuals((g["R12"], g["t12"], g["scale12"]), prob)
        worst_chi2 = max(worst_chi2, rel(g["chi2_final"], a["chi2_final"]))
        worst_res = max(worst_res, np.abs(ra - rg).max())
        print("scene %2d n %3d fix %d: analytic %s g2o %s chi2 rel %.1e residuals %.1e" % (
            i, len(prob["pts1"]), prob["fix_scale"], (a["iters"], a["trials_total"]), (g["iters"], g["trials_total"]),
            rel(g["chi2_final"], a["chi2_final"]), np.abs(ra - rg).max()))
    print("numeric vs analytic Jacobian: largest chi2_final gap %.2e relative, largest residual gap %.2e" % (worst_chi2, worst_res))
    assert worst_res < RESIDUAL


def test_reversed_summation_stays_inside_the_bars_on_every_gpu_scene():
    """What the device is held to (tests/test_gpu_sim3_opt.py) must hold between two legitimate evaluations of the restatement itself: the
    edges summed forward and in reversed order, on EVERY scene the GPU tests generate, none left out.  chi2_init within n_edges * 2^-52
    relative, chi2_final within 1e-10 relative unless the minimum is a zero reached to rounding (listed), residuals within 1e-5."""
    differ, total, worst_chi2, worst_res, zeros = 0, 0, 0.0, 0.0, []
    for name, probs in ref.gpu_scenes().items():
        for k, prob in enumerate(probs):
            f, r = ref.optimize(prob, order=1), ref.optimize(prob, order=-1)
            n_edges = 2 * len(prob["pts1"])
            assert abs(f["chi2_init"] - r["chi2_init"]) <= n_edges * 2.0 ** -52 * f["chi2_init"], (name, k)
            assert f["chi2_final"] <= f["chi2_init"] and r["chi2_final"] <= r["chi2_init"], (name, k)
            rf = ref.residuals((f["R12"], f["t12"], f["scale12"]), prob)
            rr = ref.residuals((r["R12"], r["t12"], r["scale12"]), prob)
            res = float(np.abs(rf - rr).max()) if n_edges else 0.0
            assert res < RESIDUAL, (name, k, res)
            if ref.zero_minimum(f, prob):
                zeros.append("%s[%d] (n = %d)" % (name, k, len(prob["pts1"])))
            else:
                assert rel(r["chi2_final"], f["chi2_final"]) < CHI2_REL, (name, k)
                worst_chi2 = max(worst_chi2, rel(r["chi2_final"], f["chi2_final"]))
            worst_res = max(worst_res, res)
            if prob["max_iters"] <= 1 or n_edges == 0:
                assert f["iters"] == r["iters"] == (min(prob["max_iters"], 1) if n_edges else 0), (name, k)
            total += 1
            differ += (f["iters"], f["trials_total"]) != (r["iters"], r["trials_total"])
    print("forward vs reversed on %d scenes: (iters, trials_total) differ in %d; largest chi2_final gap %.2e relative, largest residual gap %.2e" %
          (total, differ, worst_chi2, worst_res))
    print("zero minimum (residual bar only): " + ", ".join(zeros))
    assert total >= 130
