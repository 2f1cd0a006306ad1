"""Restatement of the two writers of the device map-point table -- the specification of ms_map_refresh and ms_loop_correct.

File:line relative to the reference tree:
  refresh        MapPoint::updateDescriptor map_point.cpp:75-116, MapPoint::updateDistanceAndNorm map_point.cpp:158-172, as
                 mapper_helpers.cpp:1062-1077 runs them for the map points of a new keyframe
  loop_correct   LoopCloser::correctLoop loop_closer.cpp:398-503, interpolateSim3 :69-76, se3ToSim3 / sim3ToSe3 :52-66
Types as the reference has them: positions, poses, camera centres and the normal's sum in float64; the normal, the viewing distances and the
scale factors in float32.  Python floats and numpy scalars round every operation on its own, sums are written in the order they are made.

The Sim3 algebra (matrix -> quaternion, quaternion -> matrix, product, inverse, map) is mi355slam::Sim3's (host/mi355slam/optimize_transform.hpp),
operation for operation; slerp is Eigen's QuaternionBase::slerp.  acos and sin are the two functions whose last bits belong to the math
library: `nudge`, when given, moves each of their results by a chosen number of ulps, which is how the tolerance of the interpolated poses is
measured (interpolation_tolerance).

A refresh problem is a dict: rows [n_rows], obs_start [n_rows + 1], obs_kf [n_obs], obs_desc [n_obs] (-1: keyframe without descriptors),
first_octave [n_rows]; the table is project_gate_ref's dict (pos, norm, min_dist, max_dist, desc); kf_pose is [n_kf, 12] float64 (rows 0-2 of
poseCW, row-major); pool is [n_pool, 8] uint32.  Also here: the scene generators the tests draw from."""
import math

import numpy as np

from project_gate_ref import camera_centre

F = np.float32
MEDOID_MAX_OBS = 256
EPS = 2.220446049250313e-16


# ------------------------------------------------------------------------------------------------ refresh
def pose_centre(P):
    P = np.asarray(P, np.float64).reshape(3, 4)
    return camera_centre(P[:, :3], P[:, 3])


def sq_norm3(v):
    """Eigen's unrolled redux of three elements: x^2 + (y^2 + z^2)."""
    return v[0] * v[0] + (v[1] * v[1] + v[2] * v[2])


def normalized(v):
    """Eigen's normalized(): divided by the square root of the squared norm when that is > 0, otherwise as it is."""
    z = sq_norm3(v)
    return v / np.sqrt(z) if z > 0 else v


def medoid_of(desc):
    """:88-115 on [n, 8] uint32: the index whose median Hamming distance (sorted[(n - 1) / 2], self included) is smallest; the first wins
    ties; only a median < 256 replaces index 0."""
    d = np.asarray(desc, np.uint32).reshape(-1, 8)
    n = len(d)
    bits = np.unpackbits(d.view(np.uint8), axis=1).astype(np.int32)
    dist = bits @ (1 - bits.T) + (1 - bits) @ bits.T
    med = np.sort(dist, axis=1)[:, (n - 1) // 2]
    best, best_idx = 256, 0
    for i in range(n):
        if med[i] < best:
            best, best_idx = med[i], i
    return best_idx


def refresh(table, kf_pose, pool, prob, sf, medoid_fn=medoid_of):
    """Returns (table', medoid): a copy of the table with the problem's rows refreshed, and per row entry the chosen observation's position
    in the row's list (-1: no observation has a descriptor; -2: more than MEDOID_MAX_OBS have one; the row keeps its descriptor in both).
    pool = None skips the descriptor half (medoid all -1)."""
    out = {k: np.array(v, copy=True) for k, v in table.items()}
    kf_pose = np.asarray(kf_pose, np.float64).reshape(-1, 12)
    centre = np.array([pose_centre(P) for P in kf_pose]).reshape(-1, 3)
    sf = np.asarray(sf, F)
    rows, start = np.asarray(prob["rows"]), np.asarray(prob["obs_start"])
    medoid = np.full(len(rows), -1, np.int32)
    for r, row in enumerate(rows):
        obs = np.asarray(prob["obs_kf"][start[r]:start[r + 1]])
        n = len(obs)
        assert n > 0                                            # observations.at(firstKf.id), :168
        p = np.asarray(table["pos"], np.float64).reshape(-1, 3)[row]
        norm_sum = np.zeros(3)                                  # :159
        for k in obs:                                           # :160-163, in list order
            norm_sum = norm_sum + normalized(centre[k] - p)
        out["norm"][row] = norm_sum.astype(F) / F(n)            # :164
        dist = F(np.sqrt(sq_norm3(centre[obs[0]] - p)))         # :167
        s = sf[prob["first_octave"][r]]
        out["max_dist"][row] = dist * s                         # :170
        out["min_dist"][row] = (dist * s) / sf[-1]              # :171
        if pool is None or prob.get("obs_desc") is None:
            continue
        od = np.asarray(prob["obs_desc"][start[r]:start[r + 1]])
        have = np.nonzero(od != -1)[0]                          # :78-84
        if len(have) == 0:
            continue                                            # :86
        if len(have) > MEDOID_MAX_OBS:
            medoid[r] = -2
            continue
        b = medoid_fn(np.asarray(pool, np.uint32).reshape(-1, 8)[od[have]])
        medoid[r] = have[b]
        out["desc"][row] = np.asarray(pool, np.uint32).reshape(-1, 8)[od[have[b]]]    # :115
    return out, medoid


# ------------------------------------------------------------------------------------------------ Sim3 as (q = (w, x, y, z), t, s), Python floats
def q_normalized(q):
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return tuple(v / n for v in q) if n > 0.0 else tuple(q)


def q_of_matrix(R):
    """Sim3(R, t, s): R row-major, 9 floats."""
    tr = R[0] + R[4] + R[8]
    if tr > 0.0:
        w4 = 2.0 * math.sqrt(tr + 1.0)
        q = (0.25 * w4, (R[7] - R[5]) / w4, (R[2] - R[6]) / w4, (R[3] - R[1]) / w4)
    elif R[0] > R[4] and R[0] > R[8]:
        x4 = 2.0 * math.sqrt(1.0 + R[0] - R[4] - R[8])
        q = ((R[7] - R[5]) / x4, 0.25 * x4, (R[1] + R[3]) / x4, (R[2] + R[6]) / x4)
    elif R[4] > R[8]:
        y4 = 2.0 * math.sqrt(1.0 + R[4] - R[0] - R[8])
        q = ((R[2] - R[6]) / y4, (R[1] + R[3]) / y4, 0.25 * y4, (R[5] + R[7]) / y4)
    else:
        z4 = 2.0 * math.sqrt(1.0 + R[8] - R[0] - R[4])
        q = ((R[3] - R[1]) / z4, (R[2] + R[6]) / z4, (R[5] + R[7]) / z4, 0.25 * z4)
    return q_normalized(q)


def matrix_of_q(q):
    w, x, y, z = q
    return (1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y))


def rotate(q, p):
    R = matrix_of_q(q)
    return (R[0] * p[0] + R[1] * p[1] + R[2] * p[2], R[3] * p[0] + R[4] * p[1] + R[5] * p[2], R[6] * p[0] + R[7] * p[1] + R[8] * p[2])


def s3_mul(a, b):
    (aq, at, as_), (bq, bt, bs) = a, b
    q = q_normalized((aq[0] * bq[0] - aq[1] * bq[1] - aq[2] * bq[2] - aq[3] * bq[3], aq[0] * bq[1] + aq[1] * bq[0] + aq[2] * bq[3] - aq[3] * bq[2],
                      aq[0] * bq[2] - aq[1] * bq[3] + aq[2] * bq[0] + aq[3] * bq[1], aq[0] * bq[3] + aq[1] * bq[2] - aq[2] * bq[1] + aq[3] * bq[0]))
    rt = rotate(aq, bt)
    return q, tuple(as_ * rt[j] + at[j] for j in range(3)), as_ * bs


def s3_inverse(a):
    q, t, s = a
    qi = (q[0], -q[1], -q[2], -q[3])
    rt = rotate(qi, t)
    si = 1.0 / s
    return qi, tuple(-si * rt[j] for j in range(3)), si


def s3_map(a, p):
    q, t, s = a
    r = rotate(q, p)
    return tuple(s * r[j] + t[j] for j in range(3))


def ulps(x, k):
    """x moved by k units in the last place."""
    x = float(x)
    for _ in range(abs(k)):
        x = float(np.nextafter(x, math.inf if k > 0 else -math.inf))
    return x


def s3_interpolate(T, lam, nudge=None):
    """interpolateSim3(identity, T, lam), :69-76.  nudge = (a, b, c, d): ulps added to acos(|d|), sin(theta), sin((1 - lam) theta), sin(lam theta)."""
    q, t, s = T
    nd = nudge or (0, 0, 0, 0)
    one = 1.0 - EPS
    d = q[0]                                                    # identity . T.r
    ad = abs(d)
    if ad >= one:
        scale0, scale1 = 1.0 - lam, lam
    else:
        theta = ulps(math.acos(ad), nd[0])
        sin_theta = ulps(math.sin(theta), nd[1])
        scale0 = ulps(math.sin((1.0 - lam) * theta), nd[2]) / sin_theta
        scale1 = ulps(math.sin(lam * theta), nd[3]) / sin_theta
    if d < 0.0:
        scale1 = -scale1
    qi = q_normalized((scale0 * 1.0 + scale1 * q[0], scale0 * 0.0 + scale1 * q[1], scale0 * 0.0 + scale1 * q[2], scale0 * 0.0 + scale1 * q[3]))
    return qi, tuple(0.0 + lam * (t[j] - 0.0) for j in range(3)), 1.0 + lam * (s - 1.0)


def s3_of_pose(P):
    """se3ToSim3: P = 12 floats, rows 0-2 of poseCW."""
    return q_of_matrix((P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10])), (P[3], P[7], P[11]), 1.0


def pose_of_s3(a):
    """sim3ToSe3: the scale is dropped."""
    R = matrix_of_q(a[0])
    t = a[1]
    return (R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2])


def as_s3(T):
    T = [float(v) for v in T]
    return tuple(T[0:4]), tuple(T[4:7]), T[7]


def correct_poses(kf_pose, T, prob, nudge=None):
    """Stage A: (corrected pose table, previous poses of the corrected entries [n_corr, 12])."""
    out = np.array(kf_pose, np.float64, copy=True).reshape(-1, 12)
    T = as_s3(T)
    prev = np.zeros((len(prob["kf_slot"]), 12))
    for i, slot in enumerate(prob["kf_slot"]):
        P = [float(v) for v in out[slot]]
        prev[i] = P                                             # :398-401
        Tl = T if prob["kf_rigid"][i] else s3_interpolate(T, float(prob["kf_lambda"][i]), nudge)       # :427, :459
        out[slot] = pose_of_s3(s3_mul(s3_of_pose(P), Tl))       # :427, :463
    return out, prev


def move_points(pos, kf_pose_after, prev, prob):
    """Stage B, :492-503: every listed point moves with its reference keyframe."""
    out = np.array(pos, np.float64, copy=True).reshape(-1, 3)
    xfer = {}
    for j, row in enumerate(prob["mp_row"]):
        ref = int(prob["mp_ref"][j])
        if ref not in xfer:
            corrected = s3_of_pose([float(v) for v in np.asarray(kf_pose_after).reshape(-1, 12)[prob["kf_slot"][ref]]])     # :500
            previous = s3_of_pose([float(v) for v in prev[ref]])                                                          # :501
            q, t, s = s3_mul(s3_inverse(corrected), previous)
            xfer[ref] = (matrix_of_q(q), t, s)
        R, t, s = xfer[ref]
        x, y, z = (float(v) for v in out[row])
        out[row] = (s * (R[0] * x + R[1] * y + R[2] * z) + t[0], s * (R[3] * x + R[4] * y + R[5] * z) + t[1], s * (R[6] * x + R[7] * y + R[8] * z) + t[2])
    return out


def loop_correct(kf_pose, pos, T, prob, nudge=None):
    after, prev = correct_poses(kf_pose, T, prob, nudge)
    return after, move_points(pos, after, prev, prob)


# ------------------------------------------------------------------------------------------------ scenes
def quat_axis_angle(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return q_normalized((math.cos(angle / 2),) + tuple(math.sin(angle / 2) * a))


def random_pose(rng, spread=5.0):
    q = quat_axis_angle(rng.normal(size=3), rng.uniform(-math.pi, math.pi))
    return np.array(pose_of_s3((q, tuple(rng.uniform(-spread, spread, 3)), 1.0)))


def scale_factors(levels=8, f=1.2):
    """static_settings.cpp:9-16: sf[0] = 1, sf[i] = sf[i - 1] * f in float32."""
    sf = np.ones(levels, F)
    for i in range(1, levels):
        sf[i] = sf[i - 1] * F(f)
    return sf


REFRESH_LENGTHS = (1, 2, 3, 63, 64, 65, 256, 257)


def make_refresh_scene(seed=5, n_kf=40, n_mp=400, n_rows=300, n_pool=6000):
    """40 keyframes, 300 of 400 rows.  List lengths: REFRESH_LENGTHS first (longer than n_kf by repeating keyframes -- the kernels do not care
    that a std::map cannot), then 1-12 at random.  Special rows: entry 8 repeats one keyframe, entry 9 has a zero term (a camera centre on the
    point), entry 10 is octave 0 and entry 11 the last level, entry 12 has obs_desc = -1 throughout, entry 13 has some -1."""
    rng = np.random.default_rng(seed)
    sf = scale_factors()
    kf_pose = np.stack([random_pose(rng) for _ in range(n_kf)])
    table = dict(pos=rng.uniform(-8, 8, (n_mp, 3)), norm=rng.normal(size=(n_mp, 3)).astype(F), min_dist=rng.uniform(0.1, 1, n_mp).astype(F),
                 max_dist=rng.uniform(5, 50, n_mp).astype(F), desc=rng.integers(0, 2 ** 32, (n_mp, 8), dtype=np.uint64).astype(np.uint32))
    protos = rng.integers(0, 2 ** 32, (n_mp, 8), dtype=np.uint64).astype(np.uint32)
    pool = protos[rng.integers(0, n_mp, n_pool)] ^ np.where(rng.random((n_pool, 8)) < 0.3, 1 << rng.integers(0, 32, (n_pool, 8)), 0).astype(np.uint32)
    rows = rng.permutation(n_mp)[:n_rows].astype(np.int32)
    lengths = list(REFRESH_LENGTHS) + [int(v) for v in rng.integers(1, 13, n_rows - len(REFRESH_LENGTHS))]
    obs_kf, obs_desc, octave = [], [], []
    for r, n in enumerate(lengths):
        kf = np.sort(rng.permutation(n_kf)[:n]) if n <= n_kf else np.sort(rng.integers(0, n_kf, n))
        od = rng.integers(0, n_pool, n)
        if r == 8:
            kf[:] = kf[0]
        if r == 12:
            od[:] = -1
        if r == 13:
            od[::2] = -1
        obs_kf.append(kf.astype(np.int32)); obs_desc.append(od.astype(np.int32)); octave.append(int(rng.integers(0, len(sf))))
    octave[10], octave[11] = 0, len(sf) - 1
    table["pos"][rows[9]] = pose_centre(kf_pose[obs_kf[9][1 if len(obs_kf[9]) > 1 else 0]])      # the term of that observation is the zero vector
    start = np.zeros(n_rows + 1, np.int32)
    start[1:] = np.cumsum(lengths)
    prob = dict(rows=rows, obs_start=start, obs_kf=np.concatenate(obs_kf), obs_desc=np.concatenate(obs_desc), first_octave=np.array(octave, np.int32))
    return dict(table=table, kf_pose=kf_pose, pool=pool, prob=prob, sf=sf, lengths=lengths)


def sub_problem(prob, entries):
    """The problem restricted to the given row entries, in the given order."""
    start = prob["obs_start"]
    cut = [np.arange(start[e], start[e + 1]) for e in entries]
    s = np.zeros(len(entries) + 1, np.int32)
    s[1:] = np.cumsum([len(c) for c in cut])
    sel = np.concatenate(cut + [np.zeros(0, np.int64)]).astype(np.int64)
    return dict(rows=prob["rows"][entries], obs_start=s, obs_kf=prob["obs_kf"][sel], obs_desc=prob["obs_desc"][sel], first_octave=prob["first_octave"][entries])


SCAN_TRIP = 1024                                             # rows whose descriptor counts k_refresh_dscan scans in one trip
SCAN_CASES = ((1024, False), (1025, False), (2100, False), (2100, True))      # (n_rows, longest_last): one trip exactly, one row more, three trips


def make_scan_scene(n_rows, longest_last=False):
    """The refresh fixture at n_rows rows for the device form (ms_map_refresh_lists), whose descriptor lists are counted on the device and
    scanned SCAN_TRIP rows per trip.  Device-built lists hold obs_desc = -1 for the keyframes without descriptors only, so two such slots
    (40, 41) are added and every observation the fixture gives obs_desc = -1 (entries 12 and 13) becomes an observation by them, behind the
    row's others (the lists are in slot order).  Entry 12 (no descriptor at all) changes places with entry 1023 and entry 13 (some) with
    entry 1024 where there is one: equal neighbouring descriptor offsets on the two sides of the first trip's end.  longest_last: the lists
    of 256 and 257 descriptors (entries 6 and 7: the longest with a medoid, and the `-2`) change places with entries n_rows - 40 and
    n_rows - 39, in the last trip.  Returns the scene of make_refresh_scene with kf_pose of 42 slots and prob in that order."""
    sc = make_refresh_scene(n_mp=2600, n_rows=n_rows, n_pool=20000)
    rng = np.random.default_rng(78)
    n_kf = len(sc["kf_pose"])
    sc["kf_pose"] = np.concatenate([sc["kf_pose"], np.stack([random_pose(rng) for _ in range(2)])])
    old = sc["prob"]
    obs_kf, obs_desc = [], []
    for a, b in zip(old["obs_start"][:-1], old["obs_start"][1:]):
        kf, od = old["obs_kf"][a:b], old["obs_desc"][a:b]
        bare = int((od == -1).sum())
        obs_kf.append(np.concatenate([kf[od != -1], np.full((bare + 1) // 2, n_kf), np.full(bare // 2, n_kf + 1)]).astype(np.int32))
        obs_desc.append(np.concatenate([od[od != -1], np.full(bare, -1)]).astype(np.int32))
    prob = dict(old, obs_kf=np.concatenate(obs_kf), obs_desc=np.concatenate(obs_desc))
    order = np.arange(n_rows)
    swaps = [(12, SCAN_TRIP - 1), (13, SCAN_TRIP)] + ([(6, n_rows - 40), (7, n_rows - 39)] if longest_last else [])
    for a, b in swaps:
        if b < n_rows:
            order[[a, b]] = order[[b, a]]
    sc["prob"] = sub_problem(prob, order)
    sc["lengths"] = np.diff(sc["prob"]["obs_start"]).tolist()
    return sc


def descriptor_counts(prob):
    """Per row entry: how many of its observations have a descriptor."""
    return np.add.reduceat((np.asarray(prob["obs_desc"]) != -1).astype(np.int64), prob["obs_start"][:-1])


LOOP_LAMBDAS = (0.0, 1e-9, 0.5, 1.0)


def loop_transforms():
    """The Sim3s of the loop scenes (w, x, y, z, t, s): a usual correction, one within 1e-9 of identity (slerp's linear branch), a 179 degree
    rotation, one whose quaternion has w < 0 (the sign flip), the identity."""
    near = q_normalized((1.0, 3e-10, -2e-10, 1e-10))
    return dict(usual=quat_axis_angle((0.2, 1.0, -0.3), 0.31) + (0.8, -0.4, 1.7, 1.07),
                near_identity=near + (1e-9, -1e-9, 5e-10, 1.0 + 1e-9),
                rot179=quat_axis_angle((1.0, 0.5, 0.2), math.radians(179.0)) + (-1.2, 0.3, 0.6, 0.95),
                negative_w=tuple(-v for v in quat_axis_angle((0.0, 0.3, 1.0), 0.7)) + (0.1, 0.2, -0.3, 1.02),
                identity=(1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0))


def make_loop_scene(seed=9, n_kf=48, n_corr=24, n_mp=700, n_pts=500):
    """48 keyframe slots of which 24 are corrected (the first 6 rigidly, the next 4 at LOOP_LAMBDAS, the others at random lambdas), 500 of 700
    points, each with one of the corrected keyframes as its reference."""
    rng = np.random.default_rng(seed)
    kf_pose = np.stack([random_pose(rng) for _ in range(n_kf)])
    pos = rng.uniform(-8, 8, (n_mp, 3))
    rigid = np.zeros(n_corr, np.uint8); rigid[:6] = 1
    lam = rng.uniform(0, 1, n_corr); lam[6:10] = LOOP_LAMBDAS
    prob = dict(kf_slot=rng.permutation(n_kf)[:n_corr].astype(np.int32), kf_rigid=rigid, kf_lambda=lam,
                mp_row=rng.permutation(n_mp)[:n_pts].astype(np.int32), mp_ref=rng.integers(0, n_corr, n_pts).astype(np.int32))
    return dict(kf_pose=kf_pose, pos=pos, prob=prob)


# The tolerance of the interpolated poses and of everything computed from them: the largest change of any output over the loop
# scenes when each acos / sin result of the slerp moves by up to 2 ulp (the bound the ROCm device library documents for the float64
# functions), times 4 for the accumulation through the quaternion product.  tests/test_map_refresh_ref.py measures it and holds it under the
# recorded value, which the GPU tests use.
# Measured on make_loop_scene() over loop_transforms(): poses 4.44e-15 (pose entries up to 5 in size), points 6.57e-14; recorded, rounded up:
TOL_POSE, TOL_POINT = 5e-15, 7e-14
NUDGES = [(a, b, c, d) for a in (-2, 0, 2) for b in (-2, 0, 2) for c in (-2, 0, 2) for d in (-2, 0, 2)]


def interpolation_tolerance(scene, transforms):
    worst_pose = worst_point = 0.0
    for T in transforms:
        base_pose, base_pos = loop_correct(scene["kf_pose"], scene["pos"], T, scene["prob"])
        for nd in NUDGES:
            if nd == (0, 0, 0, 0):
                continue
            pose, pos = loop_correct(scene["kf_pose"], scene["pos"], T, scene["prob"], nudge=nd)
            worst_pose = max(worst_pose, float(np.abs(pose - base_pose).max()))
            worst_point = max(worst_point, float(np.abs(pos - base_pos).max()))
    return 4.0 * worst_pose, 4.0 * worst_point
