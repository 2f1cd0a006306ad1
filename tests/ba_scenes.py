"""Bundle-adjustment windows outside the corridor of ba_synth: transforms that take a ba_synth problem and return a new, equally valid one, and a named
catalogue scenes() built from them on small windows (<= 20 keyframes, <= 400 points: the oracle stays fast).  Plain numpy, no GPU.

What ba_synth never produces and these do: a world frame rotated by 1 rad .. just under pi and moved by metres (move_world); quaternions of either sign
(flip_quaternion_signs); full 6 x 6 information matrices, one of them not symmetric (dense_edge_info); Huber off / tight / wide (huber); SE3 edge errors
on both sides of se3_log's |d| > 0.99999 switch, at tens of degrees, and exactly the identity (edge_errors); kilometres and millimetres (rescale); points
a few centimetres in front of a camera and one behind it (near_points); vertices without edges, doubled edges, constant edges (degenerate); a pose graph
without points and a window without SE3 edges (pose_graph_only, no_edges).  Every scene is also offered with ONE free keyframe (stage 1 of
localBundleAdjust: k_ba_one_pose) and with one free keyframe and every point fixed (poseBundleAdjust: k_ba_pose_only); route() is the host's routing rule."""
import numpy as np

import ba_synth
from ba_route import route          # tools/ba_route.py: the host's routing rule, one copy shared with tools/ba_fuzz.py

_compose, _inverse, _pose, _rotvec, _R = ba_synth._compose, ba_synth._inverse, ba_synth._pose, ba_synth._rotvec, ba_synth._R_from_quat


def _copy(p):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}


def _point_fixed(p):
    return np.zeros(len(p["point"]), np.uint8) if p.get("point_fixed") is None else p["point_fixed"].astype(np.uint8)


def random_rigid(rng, angle, shift=5.0):
    """A rigid motion: rotation by `angle` about a random axis, translation of `shift` metres in a random direction."""
    a, t = rng.normal(size=3), rng.normal(size=3)
    return _pose(_rotvec(angle * a / np.linalg.norm(a)), shift * t / np.linalg.norm(t))


def move_world(p, G):
    """The same window in another world frame x' = G x: pose' = pose G^-1, point' = G point (gt_* likewise).  The SE3 measurements relate camera frames
    (Tj Ti^-1) and do not change."""
    q = _copy(p)
    Gi, Rg, tg = _inverse(G), _R(G[:4]), G[4:]
    for k in ("pose", "gt_pose"):
        if k in q: q[k] = np.array([_compose(T, Gi) for T in p[k]]).reshape(-1, 7)
    for k in ("point", "gt_point"):
        if k in q: q[k] = p[k] @ Rg.T + tg
    return q


def flip_quaternion_signs(p, pose_mask=None, edge_mask=None):
    """The same rotations written with the other quaternion: q -> -q on the chosen poses and edge measurements (default: all)."""
    q = _copy(p)
    pm = np.ones(len(q["pose"]), bool) if pose_mask is None else np.asarray(pose_mask, bool)
    em = np.ones(len(q["edge_meas"]), bool) if edge_mask is None else np.asarray(edge_mask, bool)
    q["pose"][pm, :4] *= -1.0
    q["edge_meas"][em, :4] *= -1.0
    return q


def dense_edge_info(p, rng, nonsymmetric=()):
    """Every 6 x 6 information matrix becomes a full symmetric positive (semi-)definite one, W' = D^1/2 B B^T D^1/2 with D the old diagonal and B = I + 0.45 N
    (off-diagonal entries and rotation-translation cross blocks of the size of the diagonal).  The edges listed in `nonsymmetric` also get an antisymmetric
    part D^1/2 (A - A^T) D^1/2: e^T W e is unchanged by it, W e and J^T W J are not, so the solver and the oracle must agree on what row-major W means."""
    q = _copy(p)
    for k in range(len(q["edge_info"])):
        W = q["edge_info"][k].reshape(6, 6)
        s = np.sqrt(np.diag(W))
        B = np.eye(6) + 0.45 * rng.normal(size=(6, 6))
        Wn = (B @ B.T) * np.outer(s, s)
        Wn = 0.5 * (Wn + Wn.T)
        if k in nonsymmetric:
            A = 0.2 * rng.normal(size=(6, 6))
            Wn = Wn + (A - A.T) * np.outer(s, s)
        q["edge_info"][k] = Wn.reshape(36)
    return q


def huber(p, delta):
    q = _copy(p); q["huber_delta"] = float(delta)
    return q


SMALL_ANGLES = (3e-3, 4.4e-3, 4.6e-3, 6e-3)                                    # rad: se3_log switches at acos(0.99999) = 4.472 mrad
LARGE_ANGLES = tuple(np.radians([20.0, 100.0, 170.0]))


def edge_errors(p, angles, rng, edges=None, offset=0.05):
    """Edge k (edges[n] for the n-th angle, default: spread over the chain) gets the measurement M = Tj E Ti^-1 with E a rotation by the angle about a random
    axis and a translation of `offset` (1 + angle) metres: at the initial state its error log(Tj^-1 M Ti) is E to rounding."""
    q = _copy(p)
    ne = len(q["edge_i"])
    edges = [(n * max(ne // len(angles), 1)) % ne for n in range(len(angles))] if edges is None else edges
    for ang, k in zip(angles, edges):
        a, t = rng.normal(size=3), rng.normal(size=3)
        E = _pose(_rotvec(ang * a / np.linalg.norm(a)), offset * (1 + ang) * t / np.linalg.norm(t))
        Ti, Tj = q["pose"][q["edge_i"][k]], q["pose"][q["edge_j"][k]]
        q["edge_meas"][k] = _compose(Tj, _compose(E, _inverse(Ti)))
    return q


def identity_error_edge(p, cur):
    """One more vertex: a FIXED bit copy of keyframe `cur`'s pose, tied to `cur` by an edge with the identity as measurement (the stage-2 prior of
    localBundleAdjust, bundle_adjuster.cpp:341-370, here with a full-rank information): Tj^-1 M Ti is exactly the identity at the initial state."""
    q = _copy(p)
    n = len(q["pose"])
    q["pose"] = np.vstack([q["pose"], q["pose"][cur:cur + 1]])
    if "gt_pose" in q: q["gt_pose"] = np.vstack([q["gt_pose"], q["gt_pose"][cur:cur + 1]])
    q["pose_fixed"] = np.append(q["pose_fixed"], 1).astype(np.uint8)
    q["edge_i"] = np.append(q["edge_i"], n).astype(np.int32); q["edge_j"] = np.append(q["edge_j"], cur).astype(np.int32)
    q["edge_meas"] = np.vstack([q["edge_meas"], [[0, 0, 0, 1, 0, 0, 0]]])
    q["edge_info"] = np.vstack([q["edge_info"], np.diag([4e4] * 3 + [1e3] * 3).reshape(1, 36)])
    return q


def rescale(p, s):
    """The same scene in other units, x' = s x: translations, points and the measurements' translations times s, the translation block of the information by
    1 / s^2 and its rotation-translation cross blocks by 1 / s (e^T W e is unchanged).  The image measurements are ratios and stay."""
    q = _copy(p)
    for k in ("pose", "gt_pose", "edge_meas"):
        if k in q: q[k][:, 4:] *= s
    for k in ("point", "gt_point"):
        if k in q: q[k] *= s
    sc = np.concatenate([np.ones(3), np.full(3, 1.0 / s)])
    q["edge_info"] = (q["edge_info"].reshape(-1, 6, 6) * np.outer(sc, sc)).reshape(-1, 36)
    return q


def near_points(p, rng, n_near=6):
    """n_near points move to depth 0.05 .. 0.2 in front of one of their cameras and one more to 0.05 BEHIND one (g2o does not test cheirality while it
    optimises); all their measurements are redrawn from the moved point (noise 1 / 500), those from cameras that would see it within 0.03 of their own focal
    plane are dropped, and the initial estimate sits within 5 % of the depth of the true position."""
    q = _copy(p)
    n_obs_of = np.bincount(q["obs_point"], minlength=len(q["point"]))
    chosen = rng.choice(np.flatnonzero(n_obs_of >= 2), size=n_near + 1, replace=False)
    keep = np.ones(len(q["obs_pose"]), bool)
    for n, l in enumerate(chosen):
        obs = np.flatnonzero(q["obs_point"] == l)
        anchor = int(q["obs_pose"][obs[int(rng.integers(0, len(obs)))]])
        depth = -0.05 if n == n_near else float(rng.uniform(0.05, 0.2))
        Xc = np.array([rng.uniform(-0.3, 0.3) * depth, rng.uniform(-0.3, 0.3) * depth, depth])
        Ta = q["gt_pose"][anchor]
        X = _R(Ta[:4]).T @ (Xc - Ta[4:])
        q["gt_point"][l] = X
        q["point"][l] = X + 0.05 * abs(depth) * rng.normal(size=3) / np.sqrt(3)
        for o in obs:
            T = q["gt_pose"][q["obs_pose"][o]]
            c = _R(T[:4]) @ X + T[4:]
            if abs(c[2]) < 0.03 and q["obs_pose"][o] != anchor: keep[o] = False
            else: q["obs_uv"][o] = c[:2] / c[2] + rng.normal(0, 1 / 500, 2)
    for k in ("obs_pose", "obs_point", "obs_uv", "obs_info"): q[k] = q[k][keep]
    q["near"] = chosen
    return q


def _normalised_like_a_solver(quat):
    """A quaternion as a solve leaves it: a fixed point of SE3Quat::normalizeRotation (w >= 0; divided by sqrt(x^2 + y^2 + z^2 + w^2) summed in that order)."""
    quat = np.array(quat, np.float64)
    for _ in range(20):
        if quat[3] < 0: quat = -quat
        nxt = quat / np.sqrt(((quat[0] * quat[0] + quat[1] * quat[1]) + quat[2] * quat[2]) + quat[3] * quat[3])
        if np.array_equal(nxt, quat): return quat
        quat = nxt
    raise AssertionError("normalisation did not settle")


def degenerate(p, rng):
    """Everything a graph builder may hand over and ba_synth never does.  The returned problem carries `degenerate`, a dict that names each feature:
      one_obs_point   a free point with ONE observation                    no_obs_point    a free point with none (appended)
      isolated_pose   a free pose without observations or edges (appended; must come back bit for bit: its quaternion is a fixed point of the normalisation)
      double_edge     two SE3 edges on the same pair (different information)   fixed_edge      an edge between two fixed poses (0 and 1)
      fixed_obs       an observation whose pose and point are both fixed    double_obs      an observation listed twice"""
    q = _copy(p)
    assert len(q["edge_i"]) >= 2 and (q["edge_i"][0], q["edge_j"][0]) == (1, 0)
    q["pose_fixed"][[0, 1]] = 1
    for k in (0, 1): q["pose"][k] = q["gt_pose"][k]
    feat = dict(fixed_edge=0)
    pf = _point_fixed(q)
    o_fixed = int(np.flatnonzero(q["obs_pose"] == 0)[0]); pf[q["obs_point"][o_fixed]] = 1
    cnt = np.bincount(q["obs_point"], minlength=len(q["point"]))
    l_one = int(np.flatnonzero((cnt >= 3) & (pf == 0))[-1])
    keep = np.ones(len(q["obs_pose"]), bool); keep[np.flatnonzero(q["obs_point"] == l_one)[1:]] = False
    for k in ("obs_pose", "obs_point", "obs_uv", "obs_info"): q[k] = q[k][keep]
    feat["one_obs_point"] = l_one
    feat["fixed_obs"] = int(np.flatnonzero((q["obs_pose"] == 0) & (pf[q["obs_point"]] != 0))[0])
    free_obs = np.flatnonzero((q["pose_fixed"][q["obs_pose"]] == 0) & (pf[q["obs_point"]] == 0) & (q["obs_point"] != l_one))
    o_dup = int(free_obs[len(free_obs) // 2])
    for k in ("obs_pose", "obs_point", "obs_uv", "obs_info"): q[k] = np.concatenate([q[k], q[k][o_dup:o_dup + 1]])
    feat["double_obs"] = (o_dup, len(q["obs_pose"]) - 1)
    k_dup = len(q["edge_i"]) // 2
    q["edge_i"] = np.append(q["edge_i"], q["edge_i"][k_dup]).astype(np.int32); q["edge_j"] = np.append(q["edge_j"], q["edge_j"][k_dup]).astype(np.int32)
    q["edge_meas"] = np.vstack([q["edge_meas"], q["edge_meas"][k_dup:k_dup + 1]]); q["edge_info"] = np.vstack([q["edge_info"], 0.25 * q["edge_info"][k_dup:k_dup + 1]])
    feat["double_edge"] = (k_dup, len(q["edge_i"]) - 1)
    feat["no_obs_point"] = len(q["point"])
    lonely = np.array([1.0, -2.0, 7.0])
    q["point"] = np.vstack([q["point"], lonely]); q["gt_point"] = np.vstack([q["gt_point"], lonely]); pf = np.append(pf, 0).astype(np.uint8)
    feat["isolated_pose"] = len(q["pose"])
    iso = _pose(_rotvec(np.array([0.3, -1.1, 0.4])), np.array([0.5, 0.25, -2.0]))
    iso[:4] = _normalised_like_a_solver(iso[:4])
    q["pose"] = np.vstack([q["pose"], iso]); q["gt_pose"] = np.vstack([q["gt_pose"], iso]); q["pose_fixed"] = np.append(q["pose_fixed"], 0).astype(np.uint8)
    q["point_fixed"] = pf
    q["degenerate"] = feat
    return q


def pose_graph_only(p, rng):
    """Only the keyframes and their SE3 edges: n_obs = 0, n_point = 0 (what globalBundleAdjust builds on a fresh map).  Two loop-closure edges (last -> first
    keyframe, middle -> second; ground truth disturbed by 5 mrad and 2 cm) close the chain, so the graph is over-determined and its chi2 does not end at 0."""
    q = _copy(p)
    n = len(q["pose"])
    for a, b in ((n - 1, 0), (n // 2, 1)):
        D = _pose(_rotvec(rng.normal(0, 5e-3, 3)), rng.normal(0, 0.02, 3))
        M = _compose(D, _compose(q["gt_pose"][b], _inverse(q["gt_pose"][a])))
        q["edge_i"] = np.append(q["edge_i"], a).astype(np.int32); q["edge_j"] = np.append(q["edge_j"], b).astype(np.int32)
        q["edge_meas"] = np.vstack([q["edge_meas"], M]); q["edge_info"] = np.vstack([q["edge_info"], np.diag([4e4] * 3 + [1e4] * 3).reshape(1, 36)])
    q["point"] = np.zeros((0, 3)); q["gt_point"] = np.zeros((0, 3)); q["point_fixed"] = None
    q["obs_pose"] = np.zeros(0, np.int32); q["obs_point"] = np.zeros(0, np.int32); q["obs_uv"] = np.zeros((0, 2)); q["obs_info"] = np.zeros(0)
    return q


def no_edges(p):
    q = _copy(p)
    q["edge_i"] = q["edge_i"][:0]; q["edge_j"] = q["edge_j"][:0]; q["edge_meas"] = q["edge_meas"][:0]; q["edge_info"] = q["edge_info"][:0]
    return q


def far_start(p, rng, sigma=1.0, angle=0.15):
    """A start far from the optimum: the points' initial estimates thrown off by sigma metres and every free keyframe turned by `angle` rad about a random
    axis, so that damped trials are rejected by data."""
    q = _copy(p); q["point"] = q["point"] + rng.normal(0, sigma, q["point"].shape)
    for i in np.flatnonzero(q["pose_fixed"] == 0):
        a = rng.normal(size=3)
        q["pose"][i] = _compose(_pose(_rotvec(angle * a / np.linalg.norm(a)), np.zeros(3)), q["pose"][i])
    return q


# ---------------------------------------------------------------- the three shapes
def as_general(p):
    return p


def as_one_pose(p, cur):
    """Stage 1 of localBundleAdjust (test_gpu_ba._stage1): only keyframe `cur` free."""
    s = _copy(p); s["pose_fixed"] = np.ones(len(p["pose"]), np.uint8); s["pose_fixed"][cur] = 0
    return s


def as_pose_only(p, cur):
    """poseBundleAdjust's shape on the whole window (tools/ba_fuzz.py's idiom; ba_synth.pose_only_from_window is this with the other keyframes' observations
    and edges left out): only keyframe `cur` free and every point fixed.  Everything else stays, as constants of the chi2."""
    s = as_one_pose(p, cur); s["point_fixed"] = np.ones(len(p["point"]), np.uint8)
    return s


SHAPES = ("general", "one_pose", "pose_only")
SHORT_ITERS, FULL_ITERS = 2, 10


class Scene:
    """name, group, the window, the keyframe the two special shapes free, `far` (the general shape's short solve rejects trials by data) and the length of
    the short, far-from-convergence solve that is compared step for step (FULL_ITERS for the full-length one)."""

    def __init__(self, name, group, prob, cur, far=False, short_iters=SHORT_ITERS):
        self.name, self.group, self.prob, self.cur, self.far, self.short_iters = name, group, prob, cur, far, short_iters

    def shaped(self, shape):
        return {"general": as_general(self.prob), "one_pose": as_one_pose(self.prob, self.cur), "pose_only": as_pose_only(self.prob, self.cur)}[shape]

    def expected_route(self, shape, team):
        """What route() must say for this shape: the special shapes reach their kernels unless the window has no free point to give k_ba_one_pose (then it
        is poseBundleAdjust's shape), and k_ba_pose_only takes no team."""
        if shape == "general": return "general"
        q = self.shaped(shape)
        no_free_point = len(q["point"]) == 0 or (q.get("point_fixed") is not None and bool(np.all(q["point_fixed"] != 0)))
        if shape == "one_pose" and not no_free_point: return "one_pose"
        return "pose_only" if team <= 1 else "general"


def _base(seed, n_pose=10, n_point=120, run=5, **kw):
    return ba_synth.make_problem(n_pose, n_point, run, seed=seed, fix_first=True, **kw)


_CACHE = []


def scenes():
    """The catalogue (built once): a list of Scene.  Groups: world, qsign, info, huber, edges, scale, near, degenerate, shape, mixed."""
    if _CACHE: return _CACHE
    rng = np.random.Generator(np.random.Philox(20260))
    S = []
    base = _base(101)
    outl = _base(102, 12, 160, 6, outlier_frac=0.12)
    for name, ang in (("world_1rad", 1.0), ("world_2rad", 2.0), ("world_3.1rad", 3.1)):
        S.append(Scene(name, "world", move_world(base, random_rigid(rng, ang, 4.0 + ang)), 9))
    S.append(Scene("qsign_all", "qsign", flip_quaternion_signs(base), 9))
    half = np.arange(10) % 2 == 1
    S.append(Scene("qsign_half", "qsign", flip_quaternion_signs(base, half, np.arange(9) % 2 == 0), 4))
    S.append(Scene("qsign_world", "qsign", flip_quaternion_signs(move_world(base, random_rigid(rng, 2.6)), ~half, np.arange(9) % 3 == 0), 5))
    S.append(Scene("info_dense", "info", dense_edge_info(base, rng), 9))
    S.append(Scene("info_nonsymmetric", "info", dense_edge_info(base, rng, nonsymmetric=(3, 8)), 9))       # edge 8 = (9, 8) touches keyframe 9
    for name, d in (("huber_0", 0.0), ("huber_neg", -1.0), ("huber_0.5", 0.5), ("huber_1e6", 1e6), ("huber_default", ba_synth.HUBER_DELTA)):
        S.append(Scene(name, "huber", huber(outl, d), 11))
    small = identity_error_edge(edge_errors(base, SMALL_ANGLES, rng, edges=[1, 3, 6, 8], offset=0.002), 9)
    S.append(Scene("edges_small", "edges", small, 9))
    S.append(Scene("edges_large", "edges", edge_errors(base, LARGE_ANGLES, rng, edges=[2, 5, 8]), 9, far=True))
    S.append(Scene("scale_1e3", "scale", rescale(base, 1e3), 9))
    S.append(Scene("scale_1e-3", "scale", rescale(base, 1e-3), 9))
    S.append(Scene("near_points", "near", near_points(_base(103, 10, 120, 5), rng), 5))
    S.append(Scene("degenerate", "degenerate", degenerate(_base(104, 10, 120, 5), rng), 6))
    S.append(Scene("pose_graph_only", "shape", pose_graph_only(base, rng), 9, short_iters=1))
    S.append(Scene("no_edges", "shape", no_edges(base), 9))
    S.append(Scene("far_start", "mixed", far_start(move_world(_base(105, 8, 100, 5), random_rigid(rng, 2.2)), rng, 0.8), 7))
    mixed = move_world(_base(106, 14, 200, 6, outlier_frac=0.05), random_rigid(rng, 2.9, 8.0))
    mixed = edge_errors(dense_edge_info(mixed, rng, nonsymmetric=(12,)), (4.4e-3, 4.6e-3, np.radians(35.0)), rng, edges=[4, 9, 12])
    mixed = huber(flip_quaternion_signs(mixed, np.arange(14) % 3 == 0, np.arange(13) % 2 == 1), 1.5)
    S.append(Scene("mixed", "mixed", mixed, 13, far=True))
    _CACHE.extend(S)
    return _CACHE


def scene(name):
    return next(s for s in scenes() if s.name == name)


GROUPS = ("world", "qsign", "info", "huber", "edges", "scale", "near", "degenerate", "shape", "mixed")

# The oracle's own distance from ba_ref_ld, per group: the largest relative gap of (chi2_init, chi2_final, chi2 per observation as ba_ref_ld.obs_gap measures it)
# over every scene of the group, the three shapes and the short and the full-length solve, each evaluated at the state the oracle returned.  Measured by
# tests/test_ba_scenes_ref.py (which fails if the oracle is further away than this) and rounded up to two digits.  It is the REFERENCE's error: the GPU tests
# allow the solver four times as much, and for the sums never less than n_terms * 2^-52 (test_gpu_ba_domain.py).
ORACLE_GAP = {
    "world": (2.3e-15, 6.6e-15, 1.6e-12), "qsign": (1.9e-15, 3.1e-15, 4.4e-13), "info": (3.9e-15, 3.8e-15, 3.3e-13), "huber": (1.7e-15, 2.2e-15, 5.3e-13),
    "edges": (1.5e-14, 5.1e-15, 5.2e-13), "scale": (1.4e-15, 3.1e-15, 6.4e-13), "near": (9.1e-16, 3.9e-15, 1.3e-11), "degenerate": (1.7e-15, 2.6e-15, 5.0e-13),
    "shape": (2.2e-14, 1.5e-14, 3.8e-13), "mixed": (2.1e-15, 8.6e-15, 3.0e-12),
}
