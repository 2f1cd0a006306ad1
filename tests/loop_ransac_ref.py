"""Numpy restatement of LoopRansac::ransacSolve (loop_ransac.cpp:47-314) with the pinhole camera of include/mi355slam.h, and a scene
generator for it.

float64 throughout, with the reference's two float roundings: the scale numer / denom is rounded to float32 (:191, :309) and s12 = 1 / s21
is a float32 division (:88).  The thresholds are float32 values compared against double errors (:222).  The largest eigenvector of Horn's N
comes from numpy.linalg.eigh.  Beside the decisions it reports, for every (hypothesis, match), whether the decision lies near its threshold
(|err - thr| <= 1e-6 thr) and, for every hypothesis, whether the top eigen-gap of N is degenerate (<= 1e-9 relative): there another exact
solver may legitimately decide differently."""
import numpy as np

CHI_SQ_2D = np.float32(9.21034)
NEAR = 1e-6
DEGENERATE = 1e-9


def project(cam, A, t, p):
    """p_c = A p + t (row by row, left to right), u = fx (x / z) + cx, v = fy (y / z) + cy; visible iff z > 0 and the pixel is in the image."""
    fx, fy, cx, cy, w, h = cam
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    px = A[0, 0] * x + A[0, 1] * y + A[0, 2] * z + t[0]
    py = A[1, 0] * x + A[1, 1] * y + A[1, 2] * z + t[1]
    pz = A[2, 0] * x + A[2, 1] * y + A[2, 2] * z + t[2]
    with np.errstate(all="ignore"):
        u = fx * (px / pz) + cx
        v = fy * (py / pz) + cy
        vis = (pz > 0) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
    return u, v, vis


def quat_to_rot(q):
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def solve_triplet(P1, P2, dof):
    """(R21, t21, s21 as float32, degenerate) from 3 x 3 arrays of points (rows = samples): computeSim3 (:112-196) or computeRotZ (:277-314)."""
    with np.errstate(all="ignore"):
        c1 = (P1[0] + P1[1] + P1[2]) / 3.0
        c2 = (P2[0] + P2[1] + P2[2]) / 3.0
        a1, a2 = P1 - c1, P2 - c2
        degenerate = False
        if dof == 1:
            C = np.float64(sum(a1[k, 0] * a2[k, 0] + a1[k, 1] * a2[k, 1] for k in range(3)))
            S = np.float64(sum(a1[k, 0] * a2[k, 1] - a1[k, 1] * a2[k, 0] for k in range(3)))
            h = np.sqrt(C * C + S * S)
            ct, st = C / h, S / h
            R = np.array([[ct, -st, 0.0], [st, ct, 0.0], [0.0, 0.0, 1.0]])
        else:
            M = a1.T @ a2                     # M[i, j] = sum_k a1[k, i] a2[k, j]
            Sxx, Sxy, Sxz = M[0]
            Syx, Syy, Syz = M[1]
            Szx, Szy, Szz = M[2]
            N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                          [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                          [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                          [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
            if not np.all(np.isfinite(N)):
                R, degenerate = np.full((3, 3), np.nan), True
            else:
                ev, V = np.linalg.eigh(N)
                scale = max(abs(ev).max(), 1e-300)
                degenerate = bool(ev[3] - ev[2] <= DEGENERATE * scale)
                q = V[:, 3] / np.linalg.norm(V[:, 3])
                R = quat_to_rot(q)
        numer = np.float64(np.sum(a2 * (a1 @ R.T)))
        denom = np.float64(np.sum(a1 * a1))
        s21 = np.float32(numer / denom)                        # 0 / 0 is NaN here, as in C++
        t21 = c2 - (float(s21) * R) @ c1
    return R, t21, s21, degenerate


def hypothesis(P1, P2, dof, fix_scale):
    """The hypothesis of one iteration as count_inliers sees it: (A21, t21, A12, t12, R12, s12, degenerate)."""
    R21, t21, s21, deg = solve_triplet(P1, P2, dof)
    if fix_scale:
        s21 = np.float32(1.0)
    with np.errstate(all="ignore"):
        s12 = np.float32(1.0) / s21
        R12 = R21.T.copy()
        t12 = (-float(s12) * R12) @ t21
        return float(s21) * R21, t21, float(s12) * R12, t12, R12, s12, deg


def inliers(prob, hyp):
    """(inlier mask, near-threshold mask) of one hypothesis over all matches (:198-229)."""
    A21, t21, A12, t12 = hyp[:4]
    p1, p2 = prob["pts1"], prob["pts2"]
    thr1, thr2 = prob["thr1"].astype(np.float64), prob["thr2"].astype(np.float64)
    I = np.eye(3)
    z = np.zeros(3)
    r1u, r1v, vs1 = project(prob["cam1"], I, z, p1)
    r2u, r2v, vs2 = project(prob["cam2"], I, z, p2)
    u2, v2, vis1 = project(prob["cam2"], A21, t21, p1)
    u1, v1, vis2 = project(prob["cam1"], A12, t12, p2)
    with np.errstate(all="ignore"):
        e2 = (u2 - r2u) ** 2 + (v2 - r2v) ** 2
        e1 = (u1 - r1u) ** 2 + (v1 - r1v) ** 2
        vis = vis1 & vis2 & vs1 & vs2
        inl = vis & (e2 < thr2) & (e1 < thr1)
        near = vis & ((np.abs(e2 - thr2) <= NEAR * thr2) | (np.abs(e1 - thr1) <= NEAR * thr1))
        near |= _near_border(prob["cam2"], u2, v2) | _near_border(prob["cam1"], u1, v1)   # a cross projection on the image border is as fragile
    return inl, near


def _near_border(cam, u, v):
    w, h = cam[4], cam[5]
    tol = NEAR * max(w, h)
    with np.errstate(all="ignore"):
        return (np.abs(u) <= tol) | (np.abs(u - w) <= tol) | (np.abs(v) <= tol) | (np.abs(v - h) <= tol)


def ransac_solve(prob, samples):
    """ransacSolve with explicit samples ([n_iter, 3]).  Returns ok, count, best_iter, R12, t12, scale12, union, best (masks), counts,
    near (per hypothesis: some match decided within NEAR of its threshold), degenerate (per hypothesis)."""
    n, it = len(prob["pts1"]), int(prob["n_iter"])
    out = dict(ok=False, count=0, best_iter=-1, R12=np.zeros((3, 3)), t12=np.zeros(3), scale12=np.float32(0), union=np.zeros(n, bool),
               best=np.zeros(n, bool), counts=np.zeros(it, np.int32), near=np.zeros(it, bool), degenerate=np.zeros(it, bool), early=False)
    if n < 3 or n < prob["min_inliers"]:                       # :52-54, no sample is drawn
        out["early"] = True
        return out
    acc = np.zeros(n, bool)                                    # the never-cleared inlier vector of :64
    for i in range(it):
        s = samples[i]
        hyp = hypothesis(prob["pts1"][s], prob["pts2"][s], prob["dof"], prob["fix_scale"])
        inl, near = inliers(prob, hyp)
        acc |= inl
        c = int(inl.sum())
        out["counts"][i], out["near"][i], out["degenerate"][i] = c, bool(near.any()), hyp[6]
        if out["count"] < c:
            out.update(count=c, best_iter=i, R12=hyp[4], t12=hyp[3], scale12=hyp[5], union=acc.copy(), best=inl)
    out["ok"] = out["count"] >= prob["min_inliers"]
    return out


def random_rotation(rng, max_angle=np.pi):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-max_angle, max_angle)
    return quat_to_rot(np.r_[np.cos(a / 2), np.sin(a / 2) * axis])


def rot_z(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def make_scene(rng, n, R21=None, t21=None, s21=1.0, noise_px=0.0, outliers=0.0, cam=(450.0, 450.0, 320.0, 240.0, 640, 480), levels=8,
               scale_factor=1.2, dof=0, fix_scale=False, min_inliers=10, n_iter=100, behind=0.0):
    """A problem whose keyframe-2 points are s21 R21 p1 + t21 (the relation the solver estimates), seen by one pinhole camera in both keyframes.
    Points lie in front of camera 1 inside its image; noise_px perturbs the keyframe-2 points by about that many pixels; a fraction `outliers`
    of the matches get unrelated keyframe-2 points; a fraction `behind` get keyframe-1 points behind the camera.  Octaves are random in [0, levels)."""
    fx, fy, cx, cy, w, h = cam
    if R21 is None:
        R21 = random_rotation(rng, 0.2) if dof == 0 else rot_z(rng.uniform(-0.5, 0.5))     # keyframe 2 still sees most of the scene
    if t21 is None:
        t21 = rng.normal(scale=0.2, size=3)
    z = rng.uniform(2.0, 8.0, n)
    u, v = rng.uniform(5, w - 5, n), rng.uniform(5, h - 5, n)
    p1 = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    p2 = s21 * p1 @ np.asarray(R21).T + t21
    if noise_px:
        p2 = p2 + rng.normal(scale=noise_px / fx, size=p2.shape) * p2[:, 2:3]
    k = rng.random(n) < outliers
    p2[k] = p2[k][rng.permutation(int(k.sum()))] + rng.normal(scale=0.5, size=(int(k.sum()), 3))
    b = rng.random(n) < behind
    p1[b, 2] = -p1[b, 2]
    sigma2 = np.array([(scale_factor ** (2 * l)) for l in range(levels)], np.float32)
    thr1 = CHI_SQ_2D * sigma2[rng.integers(0, levels, n)]
    thr2 = CHI_SQ_2D * sigma2[rng.integers(0, levels, n)]
    return dict(pts1=p1, pts2=p2, thr1=thr1.astype(np.float32), thr2=thr2.astype(np.float32), cam1=cam, cam2=cam, dof=dof, fix_scale=fix_scale,
                min_inliers=min_inliers, n_iter=n_iter)


def draw(rng, n, it):
    if n < 3 or it == 0:
        return np.zeros((it, 3), np.int32)
    return np.stack([rng.choice(n, 3, replace=False) for _ in range(it)]).astype(np.int32)
