"""ms_loop_ransac (LoopRansac::ransacSolve on the device) against the numpy restatement in tests/loop_ransac_ref.py, samples given explicitly.

Per hypothesis, the inlier counts must be equal wherever the restatement flags nothing (no decision within 1e-6 of its threshold or of the
image border, no degenerate top eigen-gap).  Per problem, when every count is equal and nothing up to the winner is flagged, the winner,
its count, ok and both masks must be equal, R12 / t12 to 1e-9 relative and scale12 to one float ulp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loop_ransac_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(ctx, probs, samples):
    import mi355slam
    return mi355slam.loop_ransac(ctx, [dict(p, samples=s) for p, s in zip(probs, samples)], hyp_counts=True)


def compare(got, prob, want):
    """Asserts what must be exact; returns whether the whole problem was strict."""
    flagged = want["near"] | want["degenerate"]
    assert np.array_equal(got["counts"][~flagged], want["counts"][~flagged])
    if want["early"]:
        assert not got["ok"] and got["count"] == 0 and got["best_iter"] == -1 and not got["union"].any() and not got["best"].any()
        return True
    b = want["best_iter"]
    upto = slice(0, b + 1) if b >= 0 else slice(0, len(flagged))
    strict = np.array_equal(got["counts"], want["counts"]) and not (want["near"][upto] | (want["degenerate"][upto] & (want["counts"][upto] > 0))).any()
    if not strict:
        return False
    assert (got["best_iter"], got["count"], got["ok"]) == (b, want["count"], want["ok"])
    assert np.array_equal(got["union"], want["union"]) and np.array_equal(got["best"], want["best"])
    if b >= 0:
        assert np.abs(got["R12"] - want["R12"]).max() <= 1e-9 * max(1.0, np.abs(want["R12"]).max())
        assert np.abs(got["t12"] - want["t12"]).max() <= 1e-9 * max(1.0, np.abs(want["t12"]).max())
        assert abs(int(np.float32(got["scale12"]).view(np.int32)) - int(np.float32(want["scale12"]).view(np.int32))) <= 1
    else:
        assert not got["union"].any() and not got["best"].any()
    return True


def check_batch(ctx, probs, samples):
    got = run(ctx, probs, samples)
    strict = [compare(g, p, ref.ransac_solve(p, s)) for g, p, s in zip(got, probs, samples)]
    return got, strict


def scene(rng, n, it, **kw):
    kw.setdefault("noise_px", 0.1)            # inlier errors well inside the thresholds: few decisions near them
    kw.setdefault("outliers", 0.3)
    return ref.make_scene(rng, n, n_iter=it, **kw)


def test_match_counts_and_iterations(ctx):
    rng = np.random.default_rng(1)
    probs = [scene(rng, n, it, min_inliers=3) for n in (3, 4, 63, 64, 65, 500, 5000) for it in (1, 300, 1000)]
    samples = [ref.draw(rng, len(p["pts1"]), p["n_iter"]) for p in probs]
    got, strict = check_batch(ctx, probs, samples)
    assert np.mean(strict) >= 0.95
    assert got[-1]["ok"] and got[-1]["count"] > 2500          # 5000 matches, 70 % inliers


@pytest.mark.parametrize("dof", [0, 1])
@pytest.mark.parametrize("fix", [False, True])
def test_dof_and_fix_scale(ctx, dof, fix):
    rng = np.random.default_rng(10 + 2 * dof + fix)
    probs = [scene(rng, n, it, dof=dof, fix_scale=fix, s21=1.0 if fix else 1.1) for n, it in ((500, 300), (64, 1000), (65, 300), (2000, 100))]
    samples = [ref.draw(rng, len(p["pts1"]), p["n_iter"]) for p in probs]
    got, strict = check_batch(ctx, probs, samples)
    assert np.mean(strict) >= 0.95
    assert all(g["ok"] for g in got)


@pytest.mark.parametrize("batch", [1, 11, 64])
def test_mixed_batches_with_early_returns(ctx, batch):
    rng = np.random.default_rng(100 + batch)
    probs = []
    for i in range(batch):
        n = int(rng.choice([3, 4, 40, 64, 65, 200, 500, 1500]))
        it = int(rng.choice([1, 100, 300]))
        p = scene(rng, n, it, dof=int(rng.integers(0, 2)), fix_scale=bool(rng.integers(0, 2)), behind=0.1,
                  t21=rng.normal(scale=0.6, size=3), min_inliers=int(rng.integers(0, 12)))   # larger shifts push points off the image
        if batch > 1 and i in (batch // 2, batch // 2 + 1):           # early returns in the middle of the batch
            p = dict(p, min_inliers=n + 1) if i == batch // 2 else {k: (v[:2] if isinstance(v, np.ndarray) else v) for k, v in p.items()}
        probs.append(p)
    samples = [None if (len(p["pts1"]) < 3 or len(p["pts1"]) < p["min_inliers"]) else ref.draw(rng, len(p["pts1"]), p["n_iter"]) for p in probs]
    got, strict = check_batch(ctx, probs, samples)
    assert np.mean(strict) >= 0.95
    if batch > 1:
        for i in (batch // 2, batch // 2 + 1):
            assert not got[i]["ok"] and got[i]["best_iter"] == -1 and not got[i]["counts"].any()


def test_coincident_and_collinear_samples_score_nothing(ctx):
    rng = np.random.default_rng(3)
    for dof in (0, 1):
        for fix in (False, True):
            p = scene(rng, 50, 3, dof=dof, fix_scale=fix, outliers=0.0, noise_px=0.0, min_inliers=1)
            p["pts2"][10:] = -np.abs(p["pts2"][10:])                 # only matches 0-9 can ever count
            p["pts1"][0:3] = [1.25, -0.5, 4.0]                        # coincident in both keyframes (exact: the centred points are 0)
            p["pts2"][0:3] = [0.75, 0.25, 3.5]
            p["pts1"][3:6] = [[0.0, 0.0, 3.0], [0.5, 0.0, 3.0], [1.0, 0.0, 3.0]]    # collinear in both, spacings that disagree
            p["pts2"][3:6] = [[0.0, 0.0, 3.0], [0.25, 0.0, 3.0], [1.0, 0.0, 3.0]]
            samples = np.array([[0, 1, 2], [3, 4, 5], [2, 0, 1]], np.int32)
            (g,) = run(ctx, [p], [samples])
            assert list(g["counts"]) == [0, 0, 0] and g["best_iter"] == -1 and not g["ok"] and not g["union"].any()


def test_all_hypotheses_at_zero(ctx):
    rng = np.random.default_rng(4)
    p = scene(rng, 300, 200, min_inliers=0)
    p["pts2"][:, 2] = -p["pts2"][:, 2]                                # every keyframe-2 point behind its camera
    (g,) = run(ctx, [p], [ref.draw(rng, 300, 200)])
    assert g["best_iter"] == -1 and g["count"] == 0 and not g["counts"].any()
    assert g["ok"]                                                    # 0 >= min_inliers = 0, as in the reference
    assert not g["union"].any() and not g["best"].any() and not g["R12"].any() and g["scale12"] == 0


def test_ties_go_to_the_earliest_iteration(ctx):
    rng = np.random.default_rng(5)
    p = scene(rng, 400, 6, noise_px=0.0)
    s = ref.draw(rng, 400, 6)
    s[5] = s[3]                                                      # the same triplet twice: the same count
    s[4] = s[3][[2, 0, 1]]                                           # and in another order
    want = ref.ransac_solve(p, s)
    (g,) = run(ctx, [p], [s])
    assert g["counts"][3] == g["counts"][4] == g["counts"][5]
    assert g["best_iter"] == int(np.argmax(g["counts"])) == want["best_iter"]


def test_allocations_stay_flat(ctx):
    import mi355slam
    L = mi355slam.lib()
    L.ms_debug_host_allocs.restype = C.c_longlong
    rng = np.random.default_rng(6)
    probs = [scene(rng, n, 300) for n in (500, 64, 1000, 3, 250, 700, 65, 90, 400, 20, 128)]
    samples = [ref.draw(rng, len(p["pts1"]), 300) for p in probs]
    run(ctx, probs, samples)
    counts = []
    for k in range(50):
        sub = probs[: 1 + k % 11]
        run(ctx, sub, samples[: len(sub)])
        counts.append(L.ms_debug_host_allocs())
    assert len(set(counts)) == 1


def _raw_call(ctx, p, samples):
    """ms_loop_ransac through ctypes with caller outputs filled with a sentinel; returns (rc, result, union, best, counts)."""
    import mi355slam as M
    pts1, pts2 = np.ascontiguousarray(p["pts1"]), np.ascontiguousarray(p["pts2"])
    thr1, thr2 = np.ascontiguousarray(p["thr1"], np.float32), np.ascontiguousarray(p["thr2"], np.float32)
    smp = np.ascontiguousarray(samples, np.int32)
    prob = M.LoopRansacProblemC(len(pts1), pts1.ctypes.data, pts2.ctypes.data, thr1.ctypes.data, thr2.ctypes.data, M.Pinhole(*p["cam1"]),
                                M.Pinhole(*p["cam2"]), len(smp), smp.ctypes.data, 0, 0, 3)
    res = M.LoopRansacResultC()
    res.best_iter = 77
    um, bm, cn = np.full(len(pts1), 9, np.uint8), np.full(len(pts1), 9, np.uint8), np.full(len(smp), -5, np.int32)
    ptr = lambda a: (C.c_void_p * 1)(a.ctypes.data)
    rc = M.lib().ms_loop_ransac(ctx._h, C.byref(prob), 1, C.byref(res), ptr(um), ptr(bm), ptr(cn))
    return rc, res, um, bm, cn


def test_invalid_samples_are_rejected_and_nothing_is_written(ctx):
    rng = np.random.default_rng(7)
    p = scene(rng, 30, 4)
    good = ref.draw(rng, 30, 4)
    for bad in ([0, 1, 30], [-1, 2, 3], [4, 4, 5], [6, 7, 6]):
        s = good.copy()
        s[2] = bad
        rc, res, um, bm, cn = _raw_call(ctx, p, s)
        assert rc == -1 and res.best_iter == 77 and (um == 9).all() and (bm == 9).all() and (cn == -5).all()
    rc, res, um, bm, cn = _raw_call(ctx, p, good)
    assert rc == 0 and res.best_iter != 77 and (um <= 1).all() and (cn >= 0).all()


def test_capacity_is_reported(ctx):
    import mi355slam
    rng = np.random.default_rng(8)
    p = scene(rng, 10, (1 << 20) + 1)
    with pytest.raises(mi355slam.MsError, match=r"\(-4\)"):
        mi355slam.loop_ransac(ctx, [dict(p, samples=np.tile(np.array([[0, 1, 2]], np.int32), (p["n_iter"], 1)))])


def test_end_to_end_after_the_loop_closure_matcher(ctx):
    """Two keyframes of one scene: M1 (ms_match_loop_closure) finds the correspondences from the descriptors, the RANSAC recovers the Sim3."""
    import mi355slam
    rng = np.random.default_rng(9)
    n = 800
    cam = (450.0, 450.0, 320.0, 240.0, 640, 480)
    R21, t21, s21 = ref.random_rotation(rng, 0.15), np.array([0.1, -0.05, 0.2]), 1.1
    prob = ref.make_scene(rng, n, R21=R21, t21=t21, s21=s21, cam=cam, n_iter=300, min_inliers=20)
    desc1 = rng.integers(0, 2**32, (n, 8), dtype=np.uint64).astype(np.uint32)
    flip = np.packbits(rng.random((n, 256)) < 0.03, axis=1, bitorder="little").view(np.uint32)
    perm = rng.permutation(n)                                        # keyframe 2 lists its keypoints in another order
    desc2 = (desc1 ^ flip)[perm]
    ang1 = rng.uniform(0, 360, n).astype(np.float32)
    ang2 = ((ang1 + 15.0) % 360).astype(np.float32)[perm]
    bucket1 = (np.arange(n) % 40).astype(np.int32)
    f1 = mi355slam.FrameOnDevice(ctx, desc1, ang1, np.ones(n, np.uint8), bucket1)
    f2 = mi355slam.FrameOnDevice(ctx, desc2, ang2, np.ones(n, np.uint8), bucket1[perm])
    counts, matched = mi355slam.match_loop_closure(ctx, [f1], [f2], 0.75, True)
    m = matched[0]
    i1 = np.flatnonzero(m >= 0)
    i2 = m[i1]
    assert counts[0] == len(i1) > 0.9 * n and np.array_equal(perm[i2], i1)       # every match is a true correspondence
    p = dict(prob, pts1=prob["pts1"][i1], pts2=prob["pts2"][perm][i2], thr1=prob["thr1"][i1], thr2=prob["thr2"][perm][i2])
    (g,) = mi355slam.loop_ransac(ctx, [p], rng=rng)
    assert g["ok"] and g["count"] > 0.8 * len(i1)                   # the rest leave keyframe 2's image
    assert np.abs(g["R12"] - R21.T).max() < 1e-9
    assert abs(float(g["scale12"]) - 1 / s21) < 1e-6
    assert np.abs(g["t12"] - (-(1 / s21) * R21.T @ t21)).max() < 1e-6


def test_mirror_batch_equals_per_object_solves():
    import test_loop_ransac_abi
    out = subprocess.run([test_loop_ransac_abi.build_smoke(), "--gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "batch ok 11 objects" in out.stdout
