"""The bundle adjuster's edge arithmetic in extended precision (numpy.longdouble: 80-bit x87 on x86-64, eps 1.08e-19), and nothing else: no solver.

Written from the formulas, not from oracle/ba.c: rotation matrices instead of quaternion products, no normalisation between the factors.  Evaluated at a
state that a solver RETURNED it arbitrates chi2_per_obs, chi2_initial and chi2_final without depending on the LM trajectory that led there.

  R(q)        Eigen's toRotationMatrix for q = (x, y, z, w), q used as given
  e_proj      uv - (R X + t).xy / (R X + t).z                       (EdgeSE3ProjectXYZ, fx = fy = 1, cx = cy = 0)
  e_se3       log(Tj^-1 M Ti) = (omega, V^-1 t), (rotation, translation) order, with SE3Quat::log's two branches: d = (tr R - 1) / 2;
              |d| > 0.99999: omega = vee(R - R^T) / 2, V^-1 = I - Om / 2 + Om^2 / 12; else theta = acos d, omega = theta / (2 sqrt(1 - d^2)) vee(R - R^T),
              V^-1 = I - Om / 2 + (1 - theta / (2 tan(theta / 2))) / theta^2 Om^2
  rho         Huber: chi2 if delta <= 0 or chi2 <= delta^2, else 2 sqrt(chi2) delta - delta^2 (projection edges only; SE3 edges are not robustified)
  chi2        info |e_proj|^2 per observation; e^T W e per SE3 edge with W row-major as given; total = sum rho + sum e^T W e"""
import numpy as np

LD = np.longdouble
LOG_SWITCH = LD("0.99999")


def rot(q):
    x, y, z, w = (LD(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], LD)


def _hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], LD)


def proj_error(pose, X, uv):
    c = rot(pose[:4]) @ np.asarray(X, LD) + np.asarray(pose[4:], LD)
    return np.asarray(uv, LD) - c[:2] / c[2]


def se3_log(R, t):
    """(omega, V^-1 t) and the d that chose the branch."""
    d = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    vee = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], LD)
    if abs(d) > LOG_SWITCH:
        om = vee / 2
        Om = _hat(om)
        Vi = np.eye(3, dtype=LD) - Om / 2 + (Om @ Om) / 12
    else:
        th = np.arccos(d)
        om = th / (2 * np.sqrt(1 - d * d)) * vee
        Om = _hat(om)
        Vi = np.eye(3, dtype=LD) - Om / 2 + (1 - th / (2 * np.tan(th / 2))) / (th * th) * (Om @ Om)
    return np.concatenate([om, Vi @ t]), d


def se3_error(Ti, Tj, M):
    """log(Tj^-1 M Ti) and d."""
    Ri, Rj, Rm = rot(Ti[:4]), rot(Tj[:4]), rot(M[:4])
    ti, tj, tm = (np.asarray(v[4:], LD) for v in (Ti, Tj, M))
    return se3_log(Rj.T @ Rm @ Ri, Rj.T @ (Rm @ ti + tm - tj))


def huber_rho(chi2, delta):
    delta = LD(delta)
    if delta <= 0 or chi2 <= delta * delta: return chi2
    return 2 * np.sqrt(chi2) * delta - delta * delta


def evaluate(prob, pose, point):
    """At the state (pose, point): dict(chi2_obs [n_obs], rho_obs [n_obs], chi2_edge [n_edge], d_edge [n_edge], total) in longdouble."""
    Rs = [rot(T[:4]) for T in pose]
    n = len(prob["obs_pose"])
    chi2, rho = np.zeros(n, LD), np.zeros(n, LD)
    for o in range(n):
        i, l = prob["obs_pose"][o], prob["obs_point"][o]
        c = Rs[i] @ np.asarray(point[l], LD) + np.asarray(pose[i][4:], LD)
        e = np.asarray(prob["obs_uv"][o], LD) - c[:2] / c[2]
        chi2[o] = LD(prob["obs_info"][o]) * (e[0] * e[0] + e[1] * e[1])
        rho[o] = huber_rho(chi2[o], prob["huber_delta"])
    ne = len(prob["edge_i"])
    ce, de = np.zeros(ne, LD), np.zeros(ne, LD)
    for k in range(ne):
        e, de[k] = se3_error(pose[prob["edge_i"][k]], pose[prob["edge_j"][k]], prob["edge_meas"][k])
        ce[k] = e @ (np.asarray(prob["edge_info"][k], LD).reshape(6, 6) @ e)
    return dict(chi2_obs=chi2, rho_obs=rho, chi2_edge=ce, d_edge=de, total=rho.sum() + ce.sum())


CHI2_FLOOR = 1e-2


def obs_gap(chi2, ref):
    """The largest |chi2 - ref| / max(ref, CHI2_FLOOR) over the observations: relative, except that an observation whose chi2 is below 0.01 (a residual that
    happens to be a hundredth of its sigma: its relative error is unbounded, it is a difference of two numbers of order 1) is measured on the scale of 0.01."""
    if len(ref) == 0: return 0.0
    ref = np.asarray(ref, LD)
    return float((np.abs(np.asarray(chi2, LD) - ref) / np.maximum(ref, LD(CHI2_FLOOR))).max())


def sum_gap(total, ref):
    return float(abs(LD(total) - ref) / abs(ref)) if ref != 0 else float(abs(LD(total)))
