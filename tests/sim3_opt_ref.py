"""Numpy restatement of OptimizeSim3Transform (optimize_transform.cpp:63-155): the refinement of one g2o::Sim3 on all matches of a loop
candidate, with a scene generator for it.  g2o is not part of the reference tree, so this file IS the specification of ms_sim3_optimize
(DESIGN 9.3); it is written from the algorithm: g2o's sim3.h, types_seven_dof_expmap and optimization_algorithm_levenberg.

The unknown is S12 = (r, t, s), S.map(p) = s * (r * p) + t (sim3.h).  Per match (optimize_transform.cpp:101-143), with p1 / p2 the matched map
points in keyframe 1's / 2's camera frame (fixed vertices), obs = bearing.xy / bearing.z, focal lengths 1 and principal points 0:
  edge 12 (EdgeSim3ProjectXYZ)         e = obs1 - proj(S12.map(p2))
  edge 21 (EdgeInverseSim3ProjectXYZ)  e = obs2 - proj(S12^-1.map(p1))
  proj(y) = (y.x / y.z, y.y / y.z): a plain division, no visibility test
  information = levelSigmaSq[octave] * I2 (:122, :137: the reference multiplies by levelSigmaSq, NOT by its inverse; kept), a float widened
  RobustKernelHuber, delta = (double)(float)sqrt(loopClosureInlierThreshold) (:72-73, :125), as oracle/ba.c:172-176 restates it:
    chi2 = info * |e|^2; rho = chi2, w = 1 up to delta^2; beyond it rho = 2 sqrt(chi2) delta - delta^2, w = delta / sqrt(chi2);
    H += J^T (w info) J, b += -J^T (w info) e (g2o leaves the second-order term of the kernel out).
Update (VertexSim3Expmap::oplusImpl): S <- Sim3::exp(dx) * S, dx = (omega[3], upsilon[3], sigma); with fix_scale dx[6] = 0 first.
LM: optimizer.optimize(max_iters) on OptimizationAlgorithmLevenberg, the schedule of oracle/ba.c:415-462, on the 7 x 7 system
(H + lambda I) dx = b solved by Cholesky; a failed factorisation is a rejected trial.

Edges are numbered as ms_sim3_optimize returns them: edge 12 of match i is 2 i, edge 21 is 2 i + 1.

Choices that the sources leave open, made here:
  * the exponential's small-angle rotation is I + Omega + Omega^2 / 2 (g2o versions differ in that term by at most eps^2 / 2);
  * with fix_scale column 6 of every Jacobian is zero, so H[6][6] = lambda only and dx[6] = b[6] / lambda = 0 exactly;
  * the Cholesky is the plain row-by-row one, a pivot that is not a finite positive number fails it (g2o: Eigen's LDLT / LLT `info()`);
  * a failed solve gives chi2_trial = DBL_MAX and scale = 1e-3, as oracle/ba.c:436-444;
  * the rotation is kept as a matrix and never re-orthonormalised (g2o keeps a quaternion and normalises it: a difference of rounding size);
  * no match, or max_iters = 0: g2o has no active edge / runs no iteration; the estimate comes back unchanged with 0 iterations;
  * the returned chi2_final is the robust chi2 of the returned state; iters, trials_total, stop_reason, lambda as oracle/ba.c reports them.

jacobian = "analytic" (the device's specification) uses the derivative of the left update; "g2o" is what g2o really does for these two
edges, which do not implement linearizeOplus: central differences with step 1e-9 through oplus (base_binary_edge.hpp).  order = -1 sums
the edges in reversed order (what a parallel reduction may legitimately do)."""
import numpy as np

EPS = 1e-5            # sim3.h: the branches of the exponential
DBL_MAX = np.finfo(np.float64).max


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_coeffs(theta, sigma, force=None):
    """(a, b2, A, B, C, s) of Sim3::exp: R = I + a Omega + b2 Omega^2, t = (A Omega + B Omega^2 + C I) upsilon, s = exp(sigma).
    force = (small_sigma, small_theta) overrides the eps branches (continuity tests)."""
    s = np.exp(sigma)
    small_sigma, small_theta = (abs(sigma) < EPS, theta < EPS) if force is None else force
    if small_theta:
        a, b2 = 1.0, 0.5
    else:
        a, b2 = np.sin(theta) / theta, (1.0 - np.cos(theta)) / (theta * theta)
    if small_sigma:
        C = 1.0
        if small_theta:
            A, B = 0.5, 1.0 / 6.0
        else:
            A, B = (1.0 - np.cos(theta)) / (theta * theta), (theta - np.sin(theta)) / (theta * theta * theta)
    else:
        C = (s - 1.0) / sigma
        if small_theta:
            A = ((sigma - 1.0) * s + 1.0) / (sigma * sigma)
            B = ((0.5 * sigma * sigma - sigma + 1.0) * s - 1.0) / (sigma * sigma * sigma)
        else:
            ca, cb, cc = s * np.sin(theta), s * np.cos(theta), theta * theta + sigma * sigma
            A = (ca * sigma + (1.0 - cb) * theta) / (theta * cc)
            B = (C - ((cb - 1.0) * sigma + ca * theta) / cc) / (theta * theta)
    return a, b2, A, B, C, s


def sim3_exp(dx, force=None):
    """Sim3::exp of (omega, upsilon, sigma) -> (R [3, 3], t [3], s)."""
    dx = np.asarray(dx, np.float64)
    om, up, sg = dx[:3], dx[3:6], dx[6]
    theta = np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    O = skew(om)
    O2 = O @ O
    a, b2, A, B, C, s = exp_coeffs(theta, sg, force)
    I = np.eye(3)
    return I + a * O + b2 * O2, (A * O + B * O2 + C * I) @ up, s


def mul(a, b):
    """(A * B) = (A.r B.r, A.s (A.r B.t) + A.t, A.s B.s)"""
    return a[0] @ b[0], a[2] * (a[0] @ b[1]) + a[1], a[2] * b[2]


def inverse(S):
    """S^-1 = (r^-1, -(1 / s) (r^-1 t), 1 / s)"""
    R, t, s = S
    return R.T.copy(), -(1.0 / s) * (R.T @ t), 1.0 / s


def smap(S, p):
    """S.map for points in rows: s (R p) + t"""
    R, t, s = S
    return s * (np.asarray(p) @ R.T) + t


def initial(prob):
    return np.array(prob["R12"], np.float64).reshape(3, 3), np.array(prob["t12"], np.float64).reshape(3), float(prob["scale12"])


def mapped(S, prob):
    """y = S.map(p2) = s (R p2) + t and z = S^-1.map(p1) = (1 / s) (R^T (p1 - t)), rows per match.  Written out term by term, left to right, so
    that the device's sweep (csrc/sim3_opt.hip edge_errors) performs the same IEEE operations: chi2_init then differs only by summation order."""
    R, t, s = S
    x, y, z = prob["pts2"][:, 0], prob["pts2"][:, 1], prob["pts2"][:, 2]
    Y = np.stack([s * (R[i, 0] * x + R[i, 1] * y + R[i, 2] * z) + t[i] for i in range(3)], 1)
    q0, q1, q2 = prob["pts1"][:, 0] - t[0], prob["pts1"][:, 1] - t[1], prob["pts1"][:, 2] - t[2]
    inv_s = 1.0 / s
    Z = np.stack([inv_s * (R[0, i] * q0 + R[1, i] * q1 + R[2, i] * q2) for i in range(3)], 1)
    return Y, Z


def residuals(S, prob):
    """[2 n, 2] reprojection errors in edge order (12, 21 per match)"""
    n = len(prob["pts1"])
    out = np.zeros((2 * n, 2))
    if n == 0:
        return out
    with np.errstate(all="ignore"):
        y, z = mapped(S, prob)
        out[0::2] = prob["obs1"] - y[:, :2] / y[:, 2:3]
        out[1::2] = prob["obs2"] - z[:, :2] / z[:, 2:3]
    return out


def edge_info(prob):
    n = len(prob["pts1"])
    info = np.zeros(2 * n)
    info[0::2] = np.asarray(prob["info1"], np.float32).astype(np.float64)
    info[1::2] = np.asarray(prob["info2"], np.float32).astype(np.float64)
    return info


def edge_chi2(S, prob):
    """chi2 = info |e|^2 per edge (before the robust kernel)"""
    e = residuals(S, prob)
    with np.errstate(all="ignore"):
        return edge_info(prob) * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])


def huber(chi2, delta):
    """(rho, w) per edge"""
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi2)
        inside = (delta <= 0) | (chi2 <= delta * delta)
        rho = np.where(inside, chi2, 2.0 * sq * delta - delta * delta)
        w = np.where(inside, 1.0, delta / sq)
    return rho, w


def robust_chi2(S, prob, order=1):
    rho, _ = huber(edge_chi2(S, prob), prob["huber_delta"])
    return float(np.sum(rho[::order])) if len(rho) else 0.0


def _dproj(y):
    """[n, 2, 3] derivative of proj at the rows of y"""
    with np.errstate(all="ignore"):
        iz = 1.0 / y[:, 2]
        D = np.zeros((len(y), 2, 3))
        D[:, 0, 0] = iz
        D[:, 1, 1] = iz
        D[:, 0, 2] = -(y[:, 0] * iz) * iz
        D[:, 1, 2] = -(y[:, 1] * iz) * iz
    return D


def _gen(p):
    """[n, 3, 7]: d(exp(dx) p) / d dx at 0 = [-[p]x | I | p]"""
    n = len(p)
    G = np.zeros((n, 3, 7))
    G[:, 0, 1], G[:, 0, 2] = p[:, 2], -p[:, 1]
    G[:, 1, 0], G[:, 1, 2] = -p[:, 2], p[:, 0]
    G[:, 2, 0], G[:, 2, 1] = p[:, 1], -p[:, 0]
    G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
    G[:, :, 6] = p
    return G


def jacobians(S, prob, jacobian="analytic", step=1e-9):
    """[2 n, 2, 7] de / d dx of every edge under S <- exp(dx) S; column 6 is zero under fix_scale.  step: the central difference's (g2o: 1e-9)"""
    R, t, s = S
    n = len(prob["pts1"])
    J = np.zeros((2 * n, 2, 7))
    if n == 0:
        return J
    with np.errstate(all="ignore"):
        if jacobian == "analytic":
            y, z = mapped(S, prob)
            J[0::2] = -np.einsum("nik,nkc->nic", _dproj(y), _gen(y))
            M = np.einsum("nik,kj->nij", _dproj(z), (1.0 / s) * R.T)             # -dproj(z) * (-(1 / s) R^T)
            J[1::2] = np.einsum("nik,nkc->nic", M, _gen(prob["pts1"]))
        elif jacobian == "g2o":
            h = step
            for d in range(7):
                dx = np.zeros(7)
                dx[d] = h
                ep = residuals(mul(sim3_exp(_fixed(dx, prob)), S), prob)
                dx[d] = -h
                em = residuals(mul(sim3_exp(_fixed(dx, prob)), S), prob)
                J[:, :, d] = (ep - em) / (2.0 * h)
        else:
            raise ValueError(jacobian)
    if prob["fix_scale"]:
        J[:, :, 6] = 0.0
    return J


def _fixed(dx, prob):
    dx = np.array(dx, np.float64)
    if prob["fix_scale"]:
        dx[6] = 0.0
    return dx


def linearise(S, prob, jacobian="analytic", order=1):
    """(H [7, 7], b [7], robust chi2) at S"""
    e = residuals(S, prob)
    J = jacobians(S, prob, jacobian)
    info = edge_info(prob)
    with np.errstate(all="ignore"):
        chi2 = info * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
        rho, w = huber(chi2, prob["huber_delta"])
        wi = w * info
        J, e, wi, rho = J[::order], e[::order], wi[::order], rho[::order]
        H = np.einsum("nia,n,nib->ab", J, wi, J)
        b = -np.einsum("nia,n,ni->a", J, wi, e)
    return H, b, (float(np.sum(rho)) if len(rho) else 0.0)


def cholesky_solve(A, b):
    """x of A x = b by the plain Cholesky, or None where a pivot is not a finite positive number"""
    n = len(b)
    L = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[j, j] - np.dot(L[j, :j], L[j, :j])
            if not (d > 0) or not np.isfinite(d):
                return None
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, n):
                L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
        y = np.zeros(n)
        for i in range(n):
            y[i] = (b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
        x = np.zeros(n)
        for i in range(n - 1, -1, -1):
            x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x


def optimize(prob, jacobian="analytic", order=1):
    """OptimizeSim3Transform on one problem.  Returns R12, t12, scale12, chi2_init, chi2_final, lam, iters, trials_total, stop_reason."""
    S = initial(prob)
    n = len(prob["pts1"])
    max_iters = int(prob["max_iters"])
    lam, ni = 0.0, 2.0
    it, trials, stop = 0, 0, 0
    chi2_init = robust_chi2(S, prob, order)
    with np.errstate(all="ignore"):
        while n > 0 and it < max_iters:
            H, b, current = linearise(S, prob, jacobian, order)
            if it == 0:
                lam, ni = 1e-5 * float(np.max(np.abs(np.diag(H)))), 2.0            # computeLambdaInit (a NaN diagonal gives a NaN lambda)
            rho, q = 0.0, 0
            while True:
                dx = cholesky_solve(H + lam * np.eye(7), b)
                if dx is not None:
                    T = mul(sim3_exp(_fixed(dx, prob)), S)
                    temp = robust_chi2(T, prob, order)
                    scale = float(np.sum(dx * (lam * dx + b))) + 1e-3
                else:
                    temp, scale = DBL_MAX, 1e-3
                rho = (current - temp) / scale
                if rho > 0 and np.isfinite(temp):
                    alpha = min(1.0 - (2.0 * rho - 1.0) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    current = temp
                    S = T
                else:
                    lam *= ni
                    ni *= 2.0
                    if not np.isfinite(lam):
                        break
                q += 1
                trials += 1
                if not (rho < 0 and q < 10):
                    break
            it += 1
            if q == 10 or rho == 0 or not np.isfinite(lam):                        # Terminate
                stop = 1
                break
    return dict(R12=S[0], t12=S[1], scale12=S[2], chi2_init=chi2_init, chi2_final=robust_chi2(S, prob, order), lam=lam, iters=it,
                trials_total=trials, stop_reason=stop)


# ---------------------------------------------------------------------------------------------------------------- scenes
def random_sim3(rng, angle=0.2, shift=0.2, scale=1.0):
    w = rng.normal(size=3)
    w *= angle / np.linalg.norm(w)
    return sim3_exp(np.r_[w, 0, 0, 0, 0])[0], rng.normal(scale=shift, size=3), float(scale)


def make_scene(rng, n, fix_scale=False, noise=0.002, outliers=0.1, perturb=1.0, max_iters=20, levels=8, scale_factor=1.2, inlier_threshold=1e-4,
               truth=None):
    """n matches of one scene seen from two keyframes related by truth = S12 (p1 = S12.map(p2)), observations with Gaussian noise (normalised
    image coordinates) and a share of outliers in image 1, octaves random, started from truth perturbed by exp(perturb * small dx).
    The problem dict carries the truth as prob["truth"]."""
    if truth is None:
        truth = random_sim3(rng, scale=1.0 if fix_scale else 1.1)
    R, t, s = truth
    p2 = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 8, n)].reshape(n, 3)
    p1 = s * p2 @ R.T + t
    o1 = p1[:, :2] / p1[:, 2:3] + rng.normal(scale=noise, size=(n, 2)) if noise else p1[:, :2] / p1[:, 2:3]
    o2 = p2[:, :2] / p2[:, 2:3] + rng.normal(scale=noise, size=(n, 2)) if noise else p2[:, :2] / p2[:, 2:3]
    k = rng.random(n) < outliers
    o1[k] += rng.normal(scale=0.1, size=(int(k.sum()), 2))
    sigma2 = np.array([scale_factor ** (2 * l) for l in range(levels)], np.float32)       # levelSigmaSq
    i1, i2 = sigma2[rng.integers(0, levels, n)], sigma2[rng.integers(0, levels, n)]
    d = perturb * np.r_[rng.normal(scale=0.02, size=3), rng.normal(scale=0.05, size=3), 0.0 if fix_scale else 0.03 * rng.normal()]
    R0, t0, s0 = mul(sim3_exp(d), truth)
    return dict(pts1=p1, pts2=p2, obs1=o1, obs2=o2, info1=i1.astype(np.float32), info2=i2.astype(np.float32),
                huber_delta=float(np.float32(np.sqrt(inlier_threshold))), fix_scale=bool(fix_scale), max_iters=int(max_iters),
                R12=R0, t12=t0, scale12=float(s0), truth=truth, outlier_mask=k)


def empty_problem(max_iters=20, fix_scale=False):
    z3, z2 = np.zeros((0, 3)), np.zeros((0, 2))
    return dict(pts1=z3, pts2=z3, obs1=z2, obs2=z2, info1=np.zeros(0, np.float32), info2=np.zeros(0, np.float32), huber_delta=0.01,
                fix_scale=fix_scale, max_iters=max_iters, R12=np.eye(3), t12=np.array([0.1, 0.2, 0.3]), scale12=1.25, truth=None,
                outlier_mask=np.zeros(0, bool))


RESIDENT = 2048          # matches k_sim3_opt keeps in registers (csrc/sim3_opt.hip: kThreads * kSlots); beyond it they stream from memory
COUNTS = (0, 1, 3, 63, 64, 65, 500, 5000, RESIDENT + 1)


def gpu_scenes():
    """Every scene the GPU tests run, by group name: {name: [problems]}.  tests/test_sim3_opt_ref.py runs the restatement forward and reversed on
    all of them; tests/test_gpu_sim3_opt.py runs the device on all of them.  1 and 3 matches are generated without outliers: 2 or 6 edges and 7
    unknowns fit exactly, so chi2_final is a zero reached to rounding (listed by zero_minimum())."""
    rng = np.random.default_rng(2026)
    groups = {}
    for fix in (False, True):
        for iters in (0, 1, 20):
            probs = []
            for n in COUNTS:
                if n == 0:
                    probs.append(empty_problem(iters, fix))
                else:
                    probs.append(make_scene(rng, n, fix_scale=fix, max_iters=iters, outliers=0.0 if n <= 3 else 0.1))
            groups["counts_fix%d_it%d" % (fix, iters)] = probs
    for batch in (1, 11, 64):
        probs = []
        for i in range(batch):
            n = int(rng.choice([1, 3, 20, 64, 65, 200, 500, 1500]))
            fix = bool(rng.integers(0, 2))
            if batch > 1 and i in (batch // 2, batch // 2 + 1):
                probs.append(empty_problem(20, fix))                    # empty problems in the middle of the batch
            else:
                probs.append(make_scene(rng, n, fix_scale=fix, outliers=0.0 if n <= 3 else 0.1))
        groups["batch%d" % batch] = probs
    groups["noise_free"] = [make_scene(rng, n, fix_scale=f, noise=0.0, outliers=0.0) for n in (20, 300) for f in (False, True)]
    # started AT the minimum of a noise-free scene: whatever path the solve takes through Terminate
    groups["at_minimum"] = [make_scene(rng, n, fix_scale=f, noise=0.0, outliers=0.0, perturb=0.0) for n in (20, 300) for f in (False, True)]
    return groups


def zero_minimum(want, prob):
    """A minimum that is zero to rounding: a relative bar on chi2_final means nothing there, only the residual bar applies.  Either the solve
    took chi2 down by twelve orders of magnitude (noise-free scenes, 1 match that 7 unknowns fit exactly), or it never rose above rounding in the
    first place (a noise-free scene started AT its minimum): every residual below 2^-40, seven orders under the residual contract and 2^12 above
    the rounding of an observation of size one, i.e. chi2_final <= n_edges * max(info) * 2^-80."""
    n_edges = 2 * len(prob["pts1"])
    if n_edges == 0:
        return True
    floor = n_edges * float(max(np.max(prob["info1"]), np.max(prob["info2"]))) * 2.0 ** -80
    return want["chi2_final"] <= 1e-12 * want["chi2_init"] or want["chi2_final"] <= floor
