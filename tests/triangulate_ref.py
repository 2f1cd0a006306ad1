"""The specification of ms_triangulate: triangulateMapPoint and triangulateMapPointFirstLastObs (mapper_helpers.cpp:600-812)
restated in float64 numpy, one rounded IEEE operation after the other in one fixed order.  The kernel follows this file operation for
operation and is written to give the same bits; the GPU test holds triangulated positions to a tolerance that is derived
(POSITION_REL_DIFF below), never read off the device, and everything else to equality.

What the reference leaves to libraries outside its tree is pinned here:
  camera        the pinhole stand-in ms_pinhole: normalizePixel = ((double(x) - cx) / fx, (double(y) - cy) / fy), always true;
                kp.bearing = (xn, yn, 1) / sqrt(xn^2 + yn^2 + 1); cameraToWorldRotation = R^T; cameraCenter = -R^T t;
                reproject = the ms_pinhole rule (p_c = R p + t, visible iff z > 0 and (u, v) in [0, w) x [0, h)) narrowed to float32
  sums          a sum over a point's observations is taken in rounds of GROUP = 16: the 16 terms of a round (missing ones are +0.0) are
                added as a tree ((i, i + 8), (i, i + 4), (i, i + 2), (0, 1)), the rounds' sums are added to 0.0 in order; every other
                sum runs left to right as written
  N-view        theia::TriangulateNView: A = sum_i C_i^T C_i, C_i = P_i - p_i (p_i^T P_i), p_i = the unit bearing, P_i = rows 0-2 of
                poseCW; the eigenvector of A's smallest eigenvalue
  two views     theia::Triangulate: Lindstrom's niter2 correction of the two normalized points, then the DLT null vector as the smallest
                eigenvector of D^T D
  midpoint      theia::TriangulateMidpoint: (sum_i (I - d_i d_i^T)) X = sum_i (I - d_i d_i^T) o_i, solved by elimination without
                interchanges (the matrix is symmetric positive semidefinite); it fails when a pivot is not above PIVOT_REL times the
                largest entry's magnitude
  eigen-solve   cyclic Jacobi, JACOBI_SWEEPS sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); the first smallest diagonal
                entry names the vector.  A result with a non-finite component or a fourth component of 0 is a failed triangulation.
"""
import numpy as np

F = np.float32
D = np.float64

TME, MIDPOINT, FIRST_LAST = 0, 1, 2                          # MS_TRI_*
NOT_TRIANGULATED, UNSURE, TRIANGULATED = 0, 1, 2             # the status output
FLAG_OF_STATUS = (0, 2, 3)                                   # the 9.6 flag encoding of the three
(R_NONE, R_FEW_OBSERVATIONS, R_ANGLE, R_SOLVER, R_DEPTH, R_REPROJECTION, R_FEW_PASSING, R_DENSE_SKIP) = range(8)
CHI2_INV2D = 5.991                                           # mapper_helpers.cpp:26, a double
GROUP = 16
JACOBI_SWEEPS = 10
PIVOT_REL = 1e-10

# The largest relative difference |p - q| / |q| over the fixtures of the GPU test (every scene of FIXTURES, every mode, with and without
# depth) between the position of this restatement (pinned Jacobi / elimination) and a LAPACK evaluation of the same definitions
# (numpy.linalg.eigh, svd and solve; solver="lapack").  Measured with
#     python tests/triangulate_ref.py --measure
# The GPU test allows the device 100 times this value: both differences come from the conditioning of the same problems.
POSITION_REL_DIFF = 1.43e-12                                 # measured: 1.421e-12
GPU_POSITION_TOLERANCE = 100.0 * POSITION_REL_DIFF


def settings(n_levels=8, scale_factor=1.2, min_angle_two_obs=1.0, min_angle_multiple_obs=3.0, rel_reprojection_threshold=0.004,
             dense_stereo_depth=False):
    sf = [F(1.0)]
    for _ in range(1, n_levels):
        sf.append(F(sf[-1] * F(scale_factor)))
    return dict(level_sigma_sq=np.array([s * s for s in sf], F), min_angle_two_obs=float(min_angle_two_obs),
                min_angle_multiple_obs=float(min_angle_multiple_obs), rel_reprojection_threshold=float(F(rel_reprojection_threshold)),
                dense_stereo_depth=bool(dense_stereo_depth))


def cos_of_degrees(deg):
    return D(np.cos(D(deg) * D(np.pi) / D(180.0)))           # std::cos(minAngleDeg * M_PI / 180.0)


# ---------------------------------------------------------------------------------------------------- per-observation quantities
def observe(poses, cams, kf, x, y):
    """Everything the passes read of a list of observations, as arrays over the list: P [n, 12], normalized point, bearing, world ray,
    camera centre."""
    kf = np.asarray(kf, np.int64)
    cam = np.asarray(cams, D).reshape(-1, 6)[kf]
    xn = (np.asarray(x, F).astype(D) - cam[:, 2]) / cam[:, 0]
    yn = (np.asarray(y, F).astype(D) - cam[:, 3]) / cam[:, 1]
    return observe_normalized(np.asarray(poses, D).reshape(-1, 12)[kf], cam, xn, yn)


def observe_normalized(P, cam, xn, yn):
    """observe() from the normalized points on (what the solver tests call with points no pixel grid has rounded)."""
    nrm = np.sqrt(xn * xn + yn * yn + 1.0)
    b = [xn / nrm, yn / nrm, 1.0 / nrm]
    ray = [P[:, j] * b[0] + P[:, 4 + j] * b[1] + P[:, 8 + j] * b[2] for j in range(3)]
    centre = [-(P[:, j] * P[:, 3] + P[:, 4 + j] * P[:, 7] + P[:, 8 + j] * P[:, 11]) for j in range(3)]
    return dict(P=P, cam=cam, xn=xn, yn=yn, b=b, ray=ray, centre=centre)


def tree_sum(v):
    v = np.asarray(v, D)
    rounds = (len(v) + GROUP - 1) // GROUP
    w = np.zeros(rounds * GROUP, D)
    w[:len(v)] = v
    w = w.reshape(rounds, GROUP)
    a = w[:, :8] + w[:, 8:]
    a = a[:, :4] + a[:, 4:]
    a = a[:, :2] + a[:, 2:]
    a = a[:, 0] + a[:, 1]
    acc = D(0.0)
    for r in a:
        acc = acc + r
    return acc


def depth_position(o, i, depth):
    """depth * kf.cameraToWorldRotation() * kp.bearing + kf.cameraCenter(), :622 / :746"""
    d = D(F(depth))
    P = o["P"][i]
    b = [o["b"][k][i] for k in range(3)]
    return [(d * P[j]) * b[0] + (d * P[4 + j]) * b[1] + (d * P[8 + j]) * b[2] + o["centre"][j][i] for j in range(3)]


def min_pair_dot(o, idx=None):
    """The smallest dot product over the pairs i < j of the world rays (+inf without a pair; a NaN product is never the smallest):
    checkTriangulationAngle(rays, a) is min_pair_dot < cos(a)."""
    r = [c if idx is None else c[idx] for c in o["ray"]]
    n = len(r[0])
    if n < 2:
        return D(np.inf)
    dots = r[0][:, None] * r[0][None, :] + r[1][:, None] * r[1][None, :] + r[2][:, None] * r[2][None, :]
    d = dots[np.triu_indices(n, 1)]
    d = d[~np.isnan(d)]
    return D(d.min()) if len(d) else D(np.inf)


# ---------------------------------------------------------------------------------------------------- solvers
def jacobi(A):
    """Cyclic Jacobi on a symmetric n x n matrix (a list of rows of float64).  Returns (diagonal, V): V's columns are the vectors."""
    with np.errstate(all="ignore"):
        return _jacobi([[D(a) for a in row] for row in A])


def _jacobi(A):
    n = len(A)
    V = [[D(1.0) if i == j else D(0.0) for j in range(n)] for i in range(n)]
    for _ in range(JACOBI_SWEEPS):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p][q]
                if not (apq != 0.0):
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                A[p][p] = A[p][p] - t * apq
                A[q][q] = A[q][q] + t * apq
                A[p][q] = A[q][p] = D(0.0)
                for k in range(n):
                    if k != p and k != q:
                        akp, akq = A[k][p], A[k][q]
                        A[k][p] = A[p][k] = c * akp - s * akq
                        A[k][q] = A[q][k] = s * akp + c * akq
                for k in range(n):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return [A[i][i] for i in range(n)], V


def smallest_eigenvector(A, solver):
    n = len(A)
    if solver == "lapack":
        M = np.array(A, D)
        if not np.all(np.isfinite(M)):
            return [D(np.nan)] * n
        w, v = np.linalg.eigh(M)
        return [D(x) for x in v[:, 0]]
    w, V = jacobi(A)
    at = 0
    for k in range(1, n):
        if w[k] < w[at]:
            at = k
    return [V[k][at] for k in range(n)]


def homogeneous_ok(h):
    return bool(np.all(np.isfinite(np.array(h, D))) and h[3] != 0.0)


def triangulate_nview(o, solver="jacobi"):
    """theia::TriangulateNView over all observations of o."""
    P, b = o["P"], o["b"]
    q = [b[0] * P[:, c] + b[1] * P[:, 4 + c] + b[2] * P[:, 8 + c] for c in range(4)]                 # p^T P
    Cm = [[P[:, 4 * r + c] - b[r] * q[c] for c in range(4)] for r in range(3)]
    A = [[None] * 4 for _ in range(4)]
    for c1 in range(4):
        for c2 in range(c1, 4):
            A[c1][c2] = A[c2][c1] = tree_sum(Cm[0][c1] * Cm[0][c2] + Cm[1][c1] * Cm[1][c2] + Cm[2][c1] * Cm[2][c2])
    h = smallest_eigenvector(A, solver)
    return homogeneous_ok(h), h


def lindstrom(E, x, xp):
    """niter2 for x^T E x' = 0: x, xp = the two normalized points (two components each).  Returns the corrected pair."""
    x, xp = [D(x[0]), D(x[1])], [D(xp[0]), D(xp[1])]
    n = [E[a][0] * xp[0] + E[a][1] * xp[1] + E[a][2] for a in range(2)]                               # S E x'
    m = [E[0][a] * x[0] + E[1][a] * x[1] + E[2][a] for a in range(2)]                                 # S E^T x
    a = n[0] * (E[0][0] * m[0] + E[0][1] * m[1]) + n[1] * (E[1][0] * m[0] + E[1][1] * m[1])
    b = (n[0] * n[0] + n[1] * n[1] + m[0] * m[0] + m[1] * m[1]) * 0.5
    c = x[0] * n[0] + x[1] * n[1] + (E[2][0] * xp[0] + E[2][1] * xp[1] + E[2][2])
    d = np.sqrt(b * b - a * c)
    lam = c / (b + d)
    dx = [lam * n[0], lam * n[1]]
    dxp = [lam * m[0], lam * m[1]]
    n = [n[k] - (E[k][0] * dxp[0] + E[k][1] * dxp[1]) for k in range(2)]
    m = [m[k] - (E[0][k] * dx[0] + E[1][k] * dx[1]) for k in range(2)]
    lam = lam * (2.0 * d / (n[0] * n[0] + n[1] * n[1] + m[0] * m[0] + m[1] * m[1]))
    return [x[0] - lam * n[0], x[1] - lam * n[1]], [xp[0] - lam * m[0], xp[1] - lam * m[1]]


def essential_21(P1, P2):
    """E with x2^T E x1 = 0: [t21]x R21, R21 = R2 R1^T, t21 = t2 - R21 t1."""
    R21 = [[P2[4 * a] * P1[4 * b] + P2[4 * a + 1] * P1[4 * b + 1] + P2[4 * a + 2] * P1[4 * b + 2] for b in range(3)] for a in range(3)]
    t = [P2[4 * a + 3] - (R21[a][0] * P1[3] + R21[a][1] * P1[7] + R21[a][2] * P1[11]) for a in range(3)]
    return [[t[1] * R21[2][c] - t[2] * R21[1][c] for c in range(3)],
            [t[2] * R21[0][c] - t[0] * R21[2][c] for c in range(3)],
            [t[0] * R21[1][c] - t[1] * R21[0][c] for c in range(3)]]


def triangulate_two_view(o, i1, i2, solver="jacobi", parts=None):
    """theia::Triangulate(pose1, pose2, point1, point2) for the observations i1 and i2 of o."""
    P1, P2 = o["P"][i1], o["P"][i2]
    with np.errstate(all="ignore"):
        E = essential_21(P1, P2)
        x2, x1 = lindstrom(E, [o["xn"][i2], o["yn"][i2]], [o["xn"][i1], o["yn"][i1]])
        rows = []
        for P, x in ((P1, x1), (P2, x2)):
            rows.append([x[0] * P[8 + c] - P[c] for c in range(4)])
            rows.append([x[1] * P[8 + c] - P[4 + c] for c in range(4)])
        if parts is not None:
            parts.update(E=E, x1=x1, x2=x2, rows=rows)
        if solver == "lapack":
            M = np.array(rows, D)
            h = [D(v) for v in np.linalg.svd(M)[2][3]] if np.all(np.isfinite(M)) else [D(np.nan)] * 4
        else:
            G = [[None] * 4 for _ in range(4)]
            for c1 in range(4):
                for c2 in range(c1, 4):
                    G[c1][c2] = G[c2][c1] = rows[0][c1] * rows[0][c2] + rows[1][c1] * rows[1][c2] + rows[2][c1] * rows[2][c2] + rows[3][c1] * rows[3][c2]
            h = smallest_eigenvector(G, solver)
    return homogeneous_ok(h), h


def triangulate_midpoint(o, solver="jacobi", quantities=None):
    """theia::TriangulateMidpoint(origins, rays).  quantities collects (pivot, threshold) pairs."""
    d, c = o["ray"], o["centre"]
    m = {}
    for a in range(3):
        for b in range(a, 3):
            m[a, b] = m[b, a] = (1.0 if a == b else 0.0) - d[a] * d[b]
    rhs = [tree_sum(m[a, 0] * c[0] + m[a, 1] * c[1] + m[a, 2] * c[2]) for a in range(3)]
    M = {k: tree_sum(v) for k, v in m.items() if k[0] <= k[1]}
    m00, m01, m02, m11, m12, m22 = M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]
    if solver == "lapack":
        full = np.array([[m00, m01, m02], [m01, m11, m12], [m02, m12, m22]], D)
        if not np.all(np.isfinite(full)) or not np.all(np.isfinite(np.array(rhs, D))) or np.linalg.matrix_rank(full) < 3:
            return False, [D(0.0)] * 4
        return True, [D(v) for v in np.linalg.solve(full, np.array(rhs, D))] + [D(1.0)]
    big = D(0.0)
    for v in (m00, m01, m02, m11, m12, m22):
        if np.abs(v) > big:
            big = np.abs(v)
    thr = PIVOT_REL * big
    fail = (False, [D(0.0)] * 4)

    def pivot_ok(p):
        if quantities is not None:
            quantities.append(("pivot", p, thr))
        return bool(p > thr)
    if not pivot_ok(m00):
        return fail
    l10, l20 = m01 / m00, m02 / m00
    a11, a12, r1 = m11 - l10 * m01, m12 - l10 * m02, rhs[1] - l10 * rhs[0]
    a22, r2 = m22 - l20 * m02, rhs[2] - l20 * rhs[0]
    if not pivot_ok(a11):
        return fail
    l21 = a12 / a11
    a22, r2 = a22 - l21 * a12, r2 - l21 * r1
    if not pivot_ok(a22):
        return fail
    z = r2 / a22
    y = (r1 - a12 * z) / a11
    x = (rhs[0] - m01 * y - m02 * z) / m00
    return True, [x, y, z, D(1.0)]


# ---------------------------------------------------------------------------------------------------- the checks
def camera_point(P, X):
    return [P[4 * r] * X[0] + P[4 * r + 1] * X[1] + P[4 * r + 2] * X[2] + P[4 * r + 3] for r in range(3)]


def check_reprojection(o, i, X, px, py, octave, focal, S, quantities=None):
    """checkReprojectionError, :576-598, with the reference's types."""
    P, (fx, fy, cx, cy, w, h) = o["P"][i], o["cam"][i]
    pc = camera_point(P, X)
    u = fx * (pc[0] / pc[2]) + cx
    v = fy * (pc[1] / pc[2]) + cy
    if quantities is not None:
        quantities += [("z", pc[2], np.abs(P[8] * X[0]) + np.abs(P[9] * X[1]) + np.abs(P[10] * X[2]) + np.abs(P[11])),
                       ("u", u, w), ("v", v, h)]
    if not (pc[2] > 0.0 and u >= 0.0 and u < w and v >= 0.0 and v < h):
        return False
    du, dv = F(u) - F(px), F(v) - F(py)
    sq = du * du + dv * dv                                                                            # float32
    ls = S["level_sigma_sq"]
    rel_sigma_base = D(F(int(focal)) * F(S["rel_reprojection_threshold"]))                            # an int times a float, widened
    sigma2 = D(F(ls[octave]) / F(ls[len(ls) // 2])) * rel_sigma_base * rel_sigma_base
    limit = D(CHI2_INV2D) * sigma2
    if quantities is not None:
        quantities.append(("reprojection", D(sq), limit))
    return bool(D(sq) <= limit)


# ---------------------------------------------------------------------------------------------------- one map point
def triangulate_point(pos, was, kf, x, y, octave, depth, poses, cams, focal, S, mode, solver="jacobi", quantities=None):
    """One call of triangulateMapPoint (TME, MIDPOINT) or triangulateMapPointFirstLastObs (FIRST_LAST).  pos = the point's position on entry;
    depth = the observations' depths or None.  Returns (position, status, reason, n_pass)."""
    pos = [D(v) for v in pos]
    n = len(kf)
    if n < 2:
        return pos, NOT_TRIANGULATED, R_FEW_OBSERVATIONS, 0
    with np.errstate(all="ignore"):
        o = observe(poses, cams, kf, x, y)
        cos_two, cos_multi = cos_of_degrees(S["min_angle_two_obs"]), cos_of_degrees(S["min_angle_multiple_obs"])

        def note(name, value, threshold):
            if quantities is not None:
                quantities.append((name, value, threshold))

        if mode == FIRST_LAST:
            last = n - 1
            if depth is not None and depth[last] > 0:
                pos = depth_position(o, last, depth[last])                                            # :746
            else:
                if S["dense_stereo_depth"]:
                    return pos, NOT_TRIANGULATED, R_DENSE_SKIP, 0                                     # :748
                dot = min_pair_dot(o, [0, last])
                note("angle", dot, cos_two)
                if not dot < cos_two:
                    return pos, NOT_TRIANGULATED, R_ANGLE, 0
                ok, h = triangulate_two_view(o, 0, last, solver)
                if not ok:
                    return pos, NOT_TRIANGULATED, R_SOLVER, 0
                pos = [h[0] / h[3], h[1] / h[3], h[2] / h[3]]                                         # :776
            n_new = 0
            for i in range(n):
                n_new += check_reprojection(o, i, pos, x[i], y[i], octave[i], focal[kf[i]], S, quantities)
            if n_new < 2:
                return pos, NOT_TRIANGULATED, R_FEW_PASSING, n_new                                    # :809
            return pos, (TRIANGULATED if n > 2 else UNSURE), R_NONE, n_new

        status_if_ok = UNSURE
        first_depth = -1
        if depth is not None and not was:
            for i in range(n):
                if depth[i] > 0:
                    first_depth = i
                    break
        if first_depth >= 0:
            pos = depth_position(o, first_depth, depth[first_depth])                                  # :622, stays written
            X = pos
        else:
            dot = min_pair_dot(o)
            if n > 2:
                note("angle", dot, cos_multi)
            if n > 2 and dot < cos_multi:
                status_if_ok = TRIANGULATED
            else:
                note("angle", dot, cos_two)
                if not dot < cos_two:
                    return pos, NOT_TRIANGULATED, R_ANGLE, 0
            if mode == MIDPOINT:
                ok, h = triangulate_midpoint(o, solver, quantities)
            elif n == 2:
                ok, h = triangulate_two_view(o, 0, 1, solver)
            else:
                ok, h = triangulate_nview(o, solver)
            if not ok:
                return pos, NOT_TRIANGULATED, R_SOLVER, 0
            X = [h[0] / h[3], h[1] / h[3], h[2] / h[3]]
        for i in range(n):
            z = camera_point(o["P"][i], X)[2]
            if not z > 0.0:
                P = o["P"][i]
                note("z", z, np.abs(P[8] * X[0]) + np.abs(P[9] * X[1]) + np.abs(P[10] * X[2]) + np.abs(P[11]))
                return pos, NOT_TRIANGULATED, R_DEPTH, 0
            if not check_reprojection(o, i, X, x[i], y[i], octave[i], focal[kf[i]], S, quantities):
                return pos, NOT_TRIANGULATED, R_REPROJECTION, 0
        return X, status_if_ok, R_NONE, 0


def triangulate(mp_pos, mp_flags, poses, cams, focal, prob, S, mode, solver="jacobi", quantities=None):
    """ms_triangulate: returns (mp_pos, mp_flags, status, reason, n_pass) with the listed rows of copies of the two tables rewritten.
    prob: rows, was_triangulated, obs_start, obs_kf, obs_x, obs_y, obs_octave, obs_depth (or None)."""
    mp_pos = np.array(mp_pos, D).reshape(-1, 3).copy()
    mp_flags = None if mp_flags is None else np.array(mp_flags, np.uint8).copy()
    rows, start = np.asarray(prob["rows"], np.int64), np.asarray(prob["obs_start"], np.int64)
    x, y = np.asarray(prob["obs_x"], F), np.asarray(prob["obs_y"], F)
    kf, octv = np.asarray(prob["obs_kf"], np.int64), np.asarray(prob["obs_octave"], np.int64)
    depth = None if prob.get("obs_depth") is None else np.asarray(prob["obs_depth"], F)
    status, reason, n_pass = np.zeros(len(rows), np.uint8), np.zeros(len(rows), np.uint8), np.zeros(len(rows), np.int32)
    for r, row in enumerate(rows):
        s = slice(start[r], start[r + 1])
        q = None if quantities is None else []
        p, status[r], reason[r], n_pass[r] = triangulate_point(mp_pos[row], bool(prob["was_triangulated"][r]), kf[s], x[s], y[s], octv[s],
                                                               None if depth is None else depth[s], poses, cams, focal, S, mode, solver, q)
        mp_pos[row] = p
        if mp_flags is not None:
            mp_flags[row] = FLAG_OF_STATUS[status[r]]
        if quantities is not None:
            quantities.append(q)
    return mp_pos, mp_flags, status, reason, n_pass


# ---------------------------------------------------------------------------------------------------- fixtures
N_KF, N_MP = 70, 1100
SLOT_HUGE, SLOT_NAN = 68, 69                                 # a keyframe whose translation overflows the solvers, one with a NaN rotation
OBS_COUNTS = (0, 1, 2, 3, 15, 16, 17, 33, 65, 300)
POINTS_PER_CALL = (1, 3, 4, 5, 63, 64, 65, 1003)
SEED = 20262                                                 # 20261 has a pair of rays within 4e-8 of the two-observation angle (entry 902)


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def make_keyframes(rng, n_kf=N_KF, special=True):
    """A corridor of cameras 0.1 apart that look down +z with small rotations.  Returns poses [n_kf, 12], cams [n_kf, 6], focal [n_kf]."""
    poses, cams = np.zeros((n_kf, 12)), np.zeros((n_kf, 6))
    for k in range(n_kf):
        R = rotation(*(rng.uniform(-0.015, 0.015, 3)))
        c = np.array([0.1 * k, rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)])
        poses[k] = np.concatenate([R, (-R @ c)[:, None]], axis=1).reshape(12)
        f = rng.uniform(480.0, 520.0)
        cams[k] = (f, f * rng.uniform(0.99, 1.01), rng.uniform(310.0, 330.0), rng.uniform(230.0, 250.0), 640, 480)
    if special and n_kf > SLOT_NAN:
        poses[SLOT_HUGE, 3::4] = (1e200, -1e200, 1e200)
        poses[SLOT_NAN, 0] = np.nan
    return poses, cams, np.rint(cams[:, 0]).astype(np.int32)


def project(poses, cams, k, X):
    """(u, v, range) of X in keyframe k; the range is what keyPointDepth holds: the distance along the unit bearing."""
    P = poses[k].reshape(3, 4)
    pc = P[:, :3] @ X + P[:, 3]
    return cams[k, 0] * pc[0] / pc[2] + cams[k, 2], cams[k, 1] * pc[1] / pc[2] + cams[k, 3], float(np.linalg.norm(pc))


KINDS = ("clean", "clean", "clean", "clean", "noisy", "outlier", "behind", "far", "huge", "nan")


def make_scene(seed=SEED, n_points=POINTS_PER_CALL[-1], obs_counts=OBS_COUNTS, n_levels=8, kinds=KINDS, n_mp=N_MP):
    """A map of n_mp rows and a batch of n_points of them (in a shuffled order) over the corridor, with every observation count of
    obs_counts and every kind of point: clean / noisy pixels, one outlier pixel, a point behind its cameras, a far point (small angle),
    an observation from the keyframe whose translation overflows or from the one with a NaN rotation.  A third of the points carry a depth
    on the first, a middle or the last observation."""
    rng = np.random.default_rng(seed)
    poses, cams, focal = make_keyframes(rng)
    rows = rng.permutation(n_mp)[:n_points].astype(np.int32)
    mp_pos = rng.uniform(-50.0, 50.0, (n_mp, 3))                                                      # what the rows hold on entry
    mp_flags = rng.integers(0, 4, n_mp).astype(np.uint8)
    usable = SLOT_HUGE
    start, kf, x, y, octv, depth, was = [0], [], [], [], [], [], []
    for r in range(n_points):
        n = obs_counts[r % len(obs_counts)]
        if n > 100 and not (r < 40 or r % 250 == 9):         # the very long lists only a few times
            n = 8
        kind = kinds[(r // len(obs_counts) + r) % len(kinds)]
        k0 = int(rng.integers(8, usable - 8))
        window = np.arange(k0 - 8, k0 + 9)
        ks = np.sort(rng.choice(window, n, replace=n > len(window)))
        zc = rng.uniform(3.0, 10.0) * (-1.0 if kind == "behind" else 1.0) * (400.0 if kind == "far" else 1.0)
        Pk = poses[k0].reshape(3, 4)
        X = Pk[:, :3].T @ (np.array([rng.uniform(-0.2, 0.2) * zc, rng.uniform(-0.15, 0.15) * zc, zc]) - Pk[:, 3])
        if kind in ("huge", "nan") and n >= 2:
            ks[-1] = SLOT_HUGE if kind == "huge" else SLOT_NAN
        sigma = dict(noisy=0.4).get(kind, 0.02)
        depth_at = {0: 0, 1: n // 2, 2: n - 1}.get(int(rng.integers(0, 9)), -1)
        for i, k in enumerate(ks):
            if k >= usable:
                u, v, z = rng.uniform(200.0, 400.0), rng.uniform(150.0, 300.0), 5.0
            else:
                u, v, z = project(poses, cams, k, X)
            u += rng.normal(0.0, sigma); v += rng.normal(0.0, sigma)
            if kind == "outlier" and i == n // 2:
                u += 25.0
            kf.append(k); x.append(u); y.append(v)
            octv.append(int(rng.integers(0, n_levels)))
            has_depth = i == depth_at and k < usable                                                  # none from the two special keyframes
            depth.append(z * (1.0 + rng.normal(0.0, 1e-3)) if has_depth else (0.0 if rng.integers(0, 2) else -1.0))
        start.append(len(kf))
        was.append(int(rng.integers(0, 2)))
    prob = dict(rows=rows, was_triangulated=np.array(was, np.uint8), obs_start=np.array(start, np.int32), obs_kf=np.array(kf, np.int32),
                obs_x=np.array(x, F), obs_y=np.array(y, F), obs_octave=np.array(octv, np.int32), obs_depth=np.array(depth, F))
    return dict(poses=poses, cams=cams, focal=focal, mp_pos=mp_pos, mp_flags=mp_flags, prob=prob)


def sub_problem(prob, entries, with_depth=True):
    """The problem of the listed entries of prob, in that order."""
    entries = list(entries)
    start = np.asarray(prob["obs_start"])
    obs = np.concatenate([np.arange(start[e], start[e + 1]) for e in entries] + [np.zeros(0, np.int64)]).astype(np.int64)
    out = dict(rows=np.asarray(prob["rows"])[entries], was_triangulated=np.asarray(prob["was_triangulated"])[entries],
               obs_start=np.concatenate([[0], np.cumsum([start[e + 1] - start[e] for e in entries])]).astype(np.int32))
    for k in ("obs_kf", "obs_x", "obs_y", "obs_octave"):
        out[k] = np.asarray(prob[k])[obs]
    out["obs_depth"] = np.asarray(prob["obs_depth"])[obs] if with_depth and prob.get("obs_depth") is not None else None
    return out


FIXTURES = tuple((mode, with_depth, dense) for mode in (TME, MIDPOINT, FIRST_LAST) for with_depth in (True, False) for dense in (False, True)
                 if not dense or (mode == FIRST_LAST and with_depth))
_CACHE = {}


def fixture(mode, with_depth, dense=False, solver="jacobi"):
    """The restatement's answer for one fixture of the GPU test over the whole scene (computed once): a dict with scene, prob, settings, and
    pos, flags, status, reason, n_pass and quantities (per entry, the decision quantities as (name, value, threshold))."""
    key = (mode, with_depth, dense, solver)
    if key not in _CACHE:
        if "scene" not in _CACHE:
            _CACHE["scene"] = make_scene()
        sc = _CACHE["scene"]
        prob = sub_problem(sc["prob"], range(len(sc["prob"]["rows"])), with_depth)
        S = settings(dense_stereo_depth=dense)
        q = []
        pos, flags, status, reason, n_pass = triangulate(sc["mp_pos"], sc["mp_flags"], sc["poses"], sc["cams"], sc["focal"], prob, S, mode, solver, q)
        _CACHE[key] = dict(scene=sc, prob=prob, settings=S, pos=pos, flags=flags, status=status, reason=reason, n_pass=n_pass, quantities=q)
    return _CACHE[key]


def margin(name, value, threshold):
    """How far a decision quantity stays from its threshold, relative: inf for a value that is not finite (every comparison with it is
    false whatever the rounding)."""
    value, threshold = float(value), float(threshold)
    if not np.isfinite(value) or not np.isfinite(threshold):
        return np.inf
    if name == "z":                                          # against 0, relative to the magnitude of the terms of the sum
        return abs(value) / threshold if threshold > 0 else np.inf
    if name in ("u", "v"):                                   # against both image borders, relative to the image size
        return min(abs(value), abs(value - threshold)) / threshold
    return abs(value - threshold) / abs(threshold) if threshold != 0 else np.inf


def relative_difference(p, q):
    """The largest |p - q| / |q| (maximum norms, row by row) of two [n, 3] position arrays; they must be finite in the same places."""
    p, q = np.asarray(p, D).reshape(-1, 3), np.asarray(q, D).reshape(-1, 3)
    assert np.array_equal(np.isfinite(p), np.isfinite(q))
    fin = np.isfinite(q).all(axis=1)
    size = np.abs(q[fin]).max(axis=1, initial=0.0)
    diff = np.abs(p[fin] - q[fin]).max(axis=1, initial=0.0)
    assert np.all(diff[size == 0.0] == 0.0)
    keep = size > 0.0
    return float(np.max(diff[keep] / size[keep])) if keep.any() else 0.0


def measure_position_difference():
    worst = 0.0
    for mode, with_depth, dense in FIXTURES:
        a, b = fixture(mode, with_depth, dense), fixture(mode, with_depth, dense, solver="lapack")
        same = (a["status"] == b["status"]) & (a["reason"] == b["reason"])
        rows = np.asarray(a["prob"]["rows"])[same]
        worst = max(worst, relative_difference(a["pos"][rows], b["pos"][rows]))
        print("mode %d depth %d dense %d: %d of %d decisions equal, running maximum %.3e" % (mode, with_depth, dense, same.sum(), len(same), worst))
    return worst


if __name__ == "__main__":
    import sys
    if "--measure" in sys.argv:
        print("POSITION_REL_DIFF measured: %.3e" % measure_position_difference())
