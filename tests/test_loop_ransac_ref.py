"""CPU checks of the numpy restatement of LoopRansac::ransacSolve (tests/loop_ransac_ref.py) on cases whose answers are known by construction."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_ransac_ref as ref  # noqa: E402

CAM = (400.0, 410.0, 320.0, 240.0, 640, 480)


def _triplet(R, t, s, P1):
    return P1, s * P1 @ R.T + t


def test_known_sim3_is_recovered_from_a_noise_free_triplet():
    rng = np.random.default_rng(11)
    for _ in range(20):
        R = ref.random_rotation(rng)
        t = rng.normal(size=3)
        s = 1.25                                              # a float32 value, so the float rounding of the scale loses nothing
        P1, P2 = _triplet(R, t, s, rng.normal(size=(3, 3)) * 2.0)
        R21, t21, s21, deg = ref.solve_triplet(P1, P2, 0)
        assert not deg
        assert s21 == np.float32(s)
        assert np.abs(R21 - R).max() < 1e-9 and np.abs(t21 - t).max() < 1e-9


def test_known_z_rotation_is_recovered_from_a_noise_free_triplet():
    rng = np.random.default_rng(12)
    for theta in (-2.5, -0.3, 0.0, 0.7, 3.0):
        R = ref.rot_z(theta)
        t = rng.normal(size=3)
        P1, P2 = _triplet(R, t, 0.75, rng.normal(size=(3, 3)))
        R21, t21, s21, _ = ref.solve_triplet(P1, P2, 1)
        assert s21 == np.float32(0.75)
        assert np.abs(R21 - R).max() < 1e-9 and np.abs(t21 - t).max() < 1e-9


def test_fix_scale_keeps_the_translation_of_the_unfixed_scale():
    rng = np.random.default_rng(13)
    R, t = ref.random_rotation(rng), rng.normal(size=3)
    P1, P2 = _triplet(R, t, 2.0, rng.normal(size=(3, 3)) + 3.0)
    A21, t21, A12, t12, R12, s12, _ = ref.hypothesis(P1, P2, 0, fix_scale=True)
    assert s12 == np.float32(1.0)
    assert np.abs(A21 - R).max() < 1e-9                       # s21 = 1
    assert np.abs(t21 - t).max() < 1e-9                       # ... but t21 = c2 - 2 R c1, the unfixed scale's
    c1, c2 = P1.mean(0), P2.mean(0)
    assert np.abs(t21 - (c2 - R @ c1)).max() > 1e-3
    assert np.allclose(t12, -R12 @ t21, rtol=0, atol=1e-12)


def _two_groups():
    """Matches 0-3 follow T1 (a shift of 1 m along x), matches 4-9 follow the identity; both groups lie in front of the camera."""
    rng = np.random.default_rng(14)
    z = rng.uniform(3.0, 6.0, 10)
    u, v = rng.uniform(100, 540, 10), rng.uniform(100, 380, 10)
    p1 = np.stack([(u - CAM[2]) / CAM[0] * z, (v - CAM[3]) / CAM[1] * z, z], 1)
    p2 = p1.copy()
    p2[:4, 0] += 1.0
    thr = np.full(10, ref.CHI_SQ_2D, np.float32)
    return dict(pts1=p1, pts2=p2, thr1=thr, thr2=thr, cam1=CAM, cam2=CAM, dof=0, fix_scale=False, min_inliers=5, n_iter=3)


def test_union_mask_differs_from_the_best_hypothesis_mask():
    prob = _two_groups()
    samples = np.array([[0, 1, 2], [4, 5, 6], [1, 2, 3]], np.int32)
    r = ref.ransac_solve(prob, samples)
    assert list(r["counts"]) == [4, 6, 4]
    assert r["best_iter"] == 1 and r["count"] == 6 and r["ok"]
    assert list(np.flatnonzero(r["best"])) == [4, 5, 6, 7, 8, 9]
    assert list(np.flatnonzero(r["union"])) == list(range(10))      # iteration 0's inliers stay in the never-cleared vector
    # the earliest of tied iterations wins: a repeat of iteration 1 at the end changes nothing
    r2 = ref.ransac_solve(dict(prob, n_iter=4), np.vstack([samples, [[7, 8, 9]]]))
    assert r2["best_iter"] == 1 and r2["counts"][3] == 6


def test_early_return_reads_no_samples():
    prob = _two_groups()
    for p in (dict(prob, pts1=prob["pts1"][:2], pts2=prob["pts2"][:2], thr1=prob["thr1"][:2], thr2=prob["thr2"][:2]), dict(prob, min_inliers=11)):
        r = ref.ransac_solve(p, None)                         # samples are never touched
        assert r["early"] and not r["ok"] and r["count"] == 0 and r["best_iter"] == -1 and not r["union"].any()


def test_coincident_samples_score_nothing():
    prob = _two_groups()
    prob["pts1"][:3] = [1.25, -0.5, 4.0]                      # exactly representable: the centred points are exactly 0, the scale 0 / 0
    prob["pts2"][:3] = [1.25, -0.5, 4.0]
    for dof in (0, 1):
        for fix in (False, True):
            r = ref.ransac_solve(dict(prob, dof=dof, fix_scale=fix, n_iter=1), np.array([[0, 1, 2]], np.int32))
            assert r["counts"][0] == 0 and r["best_iter"] == -1


def test_generated_scene_is_solved():
    rng = np.random.default_rng(15)
    prob = ref.make_scene(rng, 200, noise_px=0.3, outliers=0.3, n_iter=50)
    r = ref.ransac_solve(prob, ref.draw(rng, 200, 50))
    assert r["ok"] and r["count"] > 100
