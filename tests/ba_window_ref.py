"""The specification of ms_ba_window_lists and ms_ba_window_apply, restated in numpy: the local BA window of localBundleAdjust
(bundle_adjuster.cpp:214-290) gathered from the map tables, and the solver's answer written back into them (:376-390, :326-331).

A scene is a dict of the tables: kf_mp [n_kf, stride] int32 (Keyframe::mapPoints as table rows, -1 none; valid iff 0 <= r < n_mp), kf_id
[n_kf] (-1 = empty slot), mp_flags [n_mp] uint8 (3 TRIANGULATED, 2 UNSURE, 0 NOT_TRIANGULATED), mp_pos [n_mp, 3], poses [n_kf, 12] (rows 0-2
of poseCW), kp (x, y, depth float32, octave int32, [n_kf, stride]), cams [n_kf, 6] (fx, fy, cx, cy, width, height), focal [n_kf] int32, sigma
[n_levels] float32 and n_obs [n_mp] int32, the whole-map observation counts.

Operation order.  Pose k = g2o::SE3Quat(R, t) of the local keyframe k: Eigen's quaternion of a rotation matrix (trace = (m00 + m11) + m22;
the four branches in Eigen's order of operations), then normalizeRotation: negated when w < 0, divided by sqrt(((x x + y y) + z z) + w w).
obs_uv = ((double)x - cx) / fx, ((double)y - cy) / fy; obs_info = (double)focal * (double)focal / (double)sigma[octave].  The pose written
back is Eigen's toRotationMatrix of the quaternion as given.  Every float64 operation is a single IEEE operation, so the device results
equal these bit for bit; scalars are Python floats, arrays numpy float64."""
import math

import numpy as np

import obs_lists_ref as OL

CHI2_THRESHOLD = 5.991                                       # bundle_adjuster.cpp:378
LOCAL, NEIGHBOR = 0, 1
N_LEVELS = 8


# ---- poses
def quat_of_matrix(R):
    """R: 9 floats, row-major.  (x, y, z, w) of g2o::SE3Quat(R, t)."""
    R = [float(v) for v in R]
    q = [0.0] * 4
    t = (R[0] + R[4]) + R[8]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[7] - R[5]) * t
        q[1] = (R[2] - R[6]) * t
        q[2] = (R[3] - R[1]) * t
        branch = 3
    else:
        i = 0
        if R[4] > R[0]:
            i = 1
        if R[8] > R[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[3 * k + j] - R[3 * j + k]) * t
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t
        branch = i
    flipped = q[3] < 0.0
    if flipped:
        q = [-v for v in q]
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [v / n for v in q], branch, flipped


def pose_of_matrix(P):
    """P: 12 floats, rows 0-2 of poseCW.  qx, qy, qz, qw, tx, ty, tz."""
    P = [float(v) for v in P]
    q, _, _ = quat_of_matrix([P[4 * a + b] for a in range(3) for b in range(3)])
    return q + [P[3], P[7], P[11]]


def matrix_of_pose(s):
    """rows 0-2 of to_homogeneous_matrix(): Eigen's toRotationMatrix of (x, y, z, w) as given."""
    x, y, z, w = (float(v) for v in s[:4])
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy, float(s[4]),
            txy + twz, 1.0 - (txx + tzz), tyz - twx, float(s[5]),
            txz - twy, tyz + twx, 1.0 - (txx + tyy), float(s[6])]


# ---- gather
def local_rows(sc, slots):
    """localMapPoints: the valid TRIANGULATED entries of the slots, ascending (ms_map_point_union with require = 1)."""
    e = np.asarray(sc["kf_mp"], np.int64)[np.asarray(slots, np.int64)].reshape(-1)
    e = e[(e >= 0) & (e < sc["n_mp"])]
    e = np.unique(e)
    return e[(sc["mp_flags"][e] & 1) != 0].astype(np.int32)


def lists_of(sc, slots):
    """What ms_observation_lists leaves for the rows of the union over `slots`."""
    sel = OL.select(OL.FROM_ROWS, rows_in=local_rows(sc, slots))
    return OL.observation_lists(sc["kf_mp"], sc["n_mp"], sc["kf_id"], sc["mp_flags"], sc["kp"], np.full(len(sc["kf_id"]), -1, np.int32), sel, N_LEVELS)


def gather(sc, local_slot, current_index, lists=None):
    """ms_ba_window_lists.  lists: the observation lists (lists_of(sc, local_slot) when None).  Returns the host outputs pose, point,
    obs_point, obs_pose, obs_uv, obs_info, n_edge, n_current, the device outputs edge_slot, edge_kp, edge_point, and rows, local_slot,
    current_index, n_rows, n_obs for apply()."""
    local_slot = np.asarray(local_slot, np.int32).reshape(-1)
    n_kf = len(sc["kf_id"])
    assert len(set(local_slot.tolist())) == len(local_slot) and all(0 <= s < n_kf and sc["kf_id"][s] >= 0 for s in local_slot) and 0 <= current_index < len(local_slot)
    L = lists_of(sc, local_slot) if lists is None else lists
    rows, n_rows, n_obs = L["rows"], L["n_rows"], L["n_obs"]
    index = np.full(n_kf, -1, np.int64)
    index[local_slot] = np.arange(len(local_slot))
    k_all = index[L["obs_kf"]]
    keep = np.nonzero(k_all >= 0)[0]                         # list order: rows ascending, inside a row ascending KfId, then keypoint
    k = k_all[keep]
    p_all = np.repeat(np.arange(n_rows), np.diff(L["obs_start"].astype(np.int64)))
    cams = np.asarray(sc["cams"], np.float64)[local_slot]
    x, y = L["obs_x"][keep].astype(np.float64), L["obs_y"][keep].astype(np.float64)
    uv = np.stack([(x - cams[k, 2]) / cams[k, 0], (y - cams[k, 3]) / cams[k, 1]], 1) if len(keep) else np.zeros((0, 2))
    focal = np.asarray(sc["focal"], np.int32)[local_slot].astype(np.float64)[k]
    info = focal * focal / np.asarray(sc["sigma"], np.float32).astype(np.float64)[L["obs_octave"][keep]]
    pose = np.array([pose_of_matrix(sc["poses"][s]) for s in local_slot], np.float64).reshape(-1, 7)
    return dict(pose=pose, point=np.asarray(sc["mp_pos"], np.float64)[rows].reshape(-1, 3), obs_point=p_all[keep].astype(np.int32), obs_pose=k.astype(np.int32),
                obs_uv=uv, obs_info=info, n_edge=len(keep), n_current=int((k == current_index).sum()),
                edge_slot=L["obs_kf"][keep].astype(np.int32), edge_kp=L["obs_kp"][keep].astype(np.int32), edge_point=p_all[keep].astype(np.int32),
                rows=rows, local_slot=local_slot, current_index=int(current_index), n_rows=n_rows, n_obs=n_obs, keep=keep)


def literal_gather(sc, local_slot, current_index):
    """The same window, walked the way bundle_adjuster.cpp:214-290 does: dictionaries of keyframes and map points, `observations` ordered
    by KfId (a slot that binds a row twice observes it twice, in keypoint order: the tables' multiplicity convention)."""
    n_mp = sc["n_mp"]
    keyframes = {int(sc["kf_id"][s]): dict(slot=s, mapPoints=[int(r) if 0 <= r < n_mp else -1 for r in sc["kf_mp"][s]]) for s in range(len(sc["kf_id"])) if sc["kf_id"][s] >= 0}
    mapPoints = {}
    for kf_id in sorted(keyframes):
        for j, r in enumerate(keyframes[kf_id]["mapPoints"]):
            if r != -1:
                mapPoints.setdefault(r, dict(observations={}))["observations"].setdefault(kf_id, []).append(j)
    localKeyframes = sorted((int(sc["kf_id"][s]) for s in local_slot), reverse=True)          # std::set<KfId, std::greater<KfId>>
    assert [keyframes[k]["slot"] for k in localKeyframes] == [int(s) for s in local_slot], "local_slot is not in descending KfId"
    current_id = localKeyframes[current_index]
    localMapPoints, n_current = set(), 0
    for kf_id in localKeyframes:                             # :198-223
        for r in keyframes[kf_id]["mapPoints"]:
            if r == -1:
                continue
            if sc["mp_flags"][r] == 3:
                if kf_id == current_id:
                    n_current += 1
                localMapPoints.add(r)
    vertex = {kf_id: i for i, kf_id in enumerate(localKeyframes)}      # :245-254
    pose = [pose_of_matrix(sc["poses"][keyframes[kf_id]["slot"]]) for kf_id in localKeyframes]
    point, obs_point, obs_pose, uv, info, edges = [], [], [], [], [], []
    for p, r in enumerate(sorted(localMapPoints)):           # :259-290
        point.append([float(v) for v in sc["mp_pos"][r]])
        for kf_id in sorted(mapPoints[r]["observations"]):
            if kf_id not in vertex:
                continue
            s = keyframes[kf_id]["slot"]
            fx, fy, cx, cy = (float(v) for v in sc["cams"][s][:4])
            for j in mapPoints[r]["observations"][kf_id]:
                obs_point.append(p); obs_pose.append(vertex[kf_id])
                uv.append([(float(sc["kp"]["x"][s, j]) - cx) / fx, (float(sc["kp"]["y"][s, j]) - cy) / fy])
                f = float(int(sc["focal"][s]))
                info.append(f * f / float(sc["sigma"][int(sc["kp"]["octave"][s, j])]))
                edges.append((s, j, p))
    return dict(pose=np.array(pose).reshape(-1, 7), point=np.array(point).reshape(-1, 3), obs_point=np.array(obs_point, np.int32), obs_pose=np.array(obs_pose, np.int32),
                obs_uv=np.array(uv).reshape(-1, 2), obs_info=np.array(info, np.float64), n_edge=len(edges), n_current=n_current,
                edge_slot=np.array([e[0] for e in edges], np.int32), edge_kp=np.array([e[1] for e in edges], np.int32),
                edge_point=np.array([e[2] for e in edges], np.int32), rows=np.array(sorted(localMapPoints), np.int32))


# ---- apply
def state_of(sc):
    return {k: np.array(sc[k]) for k in ("kf_mp", "n_obs", "mp_flags", "mp_pos", "poses")}


def apply(state, window, pose, point, chi2, mode):
    """ms_ba_window_apply on a copy of `state` (kf_mp, n_obs, mp_flags, mp_pos, poses).  Returns (state, erased_edge, n_stale): an edge
    whose table entry no longer names its row is skipped and counted."""
    st = {k: np.array(v) for k, v in state.items()}
    rows, local_slot = window["rows"].astype(np.int64), window["local_slot"]
    pose, point = np.asarray(pose, np.float64).reshape(-1, 7), np.asarray(point, np.float64).reshape(-1, 3)
    erased, n_stale = np.zeros(0, np.int32), 0
    if mode == LOCAL:
        slot, kp, row = window["edge_slot"].astype(np.int64), window["edge_kp"].astype(np.int64), rows[window["edge_point"]]
        stale = st["kf_mp"][slot, kp] != row
        with np.errstate(invalid="ignore"):
            erase = ~stale & (np.asarray(chi2, np.float64) > CHI2_THRESHOLD)     # strict; a NaN keeps the edge
        n_stale = int(stale.sum())
        erased = np.nonzero(erase)[0].astype(np.int32)
        st["kf_mp"][slot[erase], kp[erase]] = -1
        np.subtract.at(st["n_obs"], row[erase], 1)
        lost = np.unique(row[erase])
        st["mp_flags"][lost[st["n_obs"][lost] <= 2]] = 2
    st["mp_pos"][rows] = point[:len(rows)]
    for k, s in enumerate(local_slot):
        if mode == LOCAL or k == window["current_index"]:
            st["poses"][s] = matrix_of_pose(pose[k])
    return st, erased, n_stale


def literal_apply(state, window, pose, point, chi2, mode):
    """The loop of :376-390 edge by edge, with the `<= 2` test after each erase."""
    st = {k: np.array(v) for k, v in state.items()}
    erased = []
    if mode == LOCAL:
        for e in range(len(window["edge_slot"])):
            if chi2[e] > CHI2_THRESHOLD:
                s, j, r = int(window["edge_slot"][e]), int(window["edge_kp"][e]), int(window["rows"][window["edge_point"][e]])
                st["kf_mp"][s, j] = -1
                st["n_obs"][r] -= 1
                if st["n_obs"][r] <= 2:
                    st["mp_flags"][r] = 2
                erased.append(e)
    for p, r in enumerate(window["rows"]):
        st["mp_pos"][r] = point[p]
    for k, s in enumerate(window["local_slot"]):
        if mode == LOCAL or k == window["current_index"]:
            st["poses"][s] = matrix_of_pose(pose[k])
    return st, np.array(erased, np.int32), 0


# ---- scenes
def sigma_levels():
    return (np.cumprod(np.concatenate([[np.float32(1)], np.full(N_LEVELS - 1, np.float32(1.2))])).astype(np.float32) ** 2).astype(np.float32)


def rotation(rng, angle):
    v = rng.normal(size=3)
    v = v / np.linalg.norm(v) * angle
    th = np.linalg.norm(v)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]) / max(th, 1e-300)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def finish(sc, rng, lists_per_slot, noise=0.3):
    """The tables of a scene whose slots list the given rows: keypoints in a shuffled order, pixels = the projection of the true point
    through the slot's true pose and camera plus noise (float32), table poses and positions slightly off the truth."""
    n_kf, stride, n_mp = sc["n_kf"], sc["stride"], sc["n_mp"]
    c = np.stack([0.25 * np.arange(n_kf) - 0.125 * n_kf, 0.05 * np.sin(0.3 * np.arange(n_kf)), 0.02 * np.arange(n_kf)], 1)
    Rs = np.stack([rotation(rng, 0.03) for _ in range(n_kf)])
    true_pos = np.stack([rng.uniform(-3, 3, n_mp), rng.uniform(-2, 2, n_mp), rng.uniform(4, 10, n_mp)], 1)
    cams = np.zeros((n_kf, 6))
    cams[:] = (500.0, 502.5, 320.0, 241.5, 640, 480)
    cams[1::2] = (458.654, 457.296, 367.215, 248.375, 752, 480)                # two distinct cameras
    focal = np.where(np.arange(n_kf) % 2 == 0, 501, 457).astype(np.int32)
    kf_mp = np.full((n_kf, stride), -1, np.int32)
    kp = dict(x=(rng.random((n_kf, stride)) * 640).astype(np.float32), y=(rng.random((n_kf, stride)) * 480).astype(np.float32),
              octave=rng.integers(0, N_LEVELS, (n_kf, stride)).astype(np.int32), depth=np.full((n_kf, stride), -1, np.float32))
    for s, l in enumerate(lists_per_slot):
        assert len(l) <= stride, (s, len(l))
        row = np.full(stride, -1, np.int64)
        row[:len(l)] = l
        kf_mp[s] = rng.permutation(row).astype(np.int32)
        j = np.nonzero((kf_mp[s] >= 0) & (kf_mp[s] < n_mp))[0]
        pc = (true_pos[kf_mp[s, j]] - c[s]) @ Rs[s].T
        assert (pc[:, 2] > 0.5).all()
        kp["x"][s, j] = (cams[s, 0] * pc[:, 0] / pc[:, 2] + cams[s, 2] + rng.normal(0, noise, len(j))).astype(np.float32)
        kp["y"][s, j] = (cams[s, 1] * pc[:, 1] / pc[:, 2] + cams[s, 3] + rng.normal(0, noise, len(j))).astype(np.float32)
    poses = np.zeros((n_kf, 12))
    for s in range(n_kf):
        R = rotation(rng, 0.004) @ Rs[s]
        t = -R @ (c[s] + rng.normal(0, 0.01, 3))
        poses[s] = np.concatenate([R, t[:, None]], 1).reshape(12)
    sc.update(kf_mp=kf_mp, kp=kp, cams=cams, focal=focal, poses=poses, mp_pos=true_pos + rng.normal(0, 0.01, true_pos.shape), sigma=sigma_levels(),
              true=dict(c=c, R=Rs, pos=true_pos))
    start, _, _ = OL.transpose(kf_mp, n_mp, sc["kf_id"])
    sc["n_obs"] = np.diff(start).astype(np.int32)
    return sc


BASE_EMPTY, BASE_NON_LOCAL = 5, (1, 7, 10)
BASE_KF_ID = (30, 4, 12, 50, 8, -1, 44, 20, 2, 38, 16, 26)
BASE_LOCAL = (3, 6, 9, 0, 11, 2, 4, 8)                       # descending KfId; slot 3 is the current keyframe
BASE_TWICE = (300, 3)                                        # row 300 is observed by every keyframe and bound twice in slot 3: 12 observations
# rows for the apply tests: row -> (local observers, other observers, the local observers whose edge is erased)
BASE_APPLY = {301: ((3, 6), (), ()),                         # count 2, loses nothing: keeps flag 3
              302: ((3, 9), (1, 7), (3, 9)),                 # 4 -> 2: UNSURE; the other keyframes' observations count
              303: ((3, 6, 0), (10,), (6,)),                 # 4 -> 3: keeps 3
              304: ((6, 9, 11), (), (6, 9, 11)),             # 3 -> 0
              305: ((3, 0, 2, 4), (1,), (0, 4)),             # 5 -> 3
              306: ((8,), (7,), (8,)),                       # 2 -> 1
              307: ((2, 4), (10,), ()),                      # count 3, loses nothing
              308: ((3, 6, 9, 0, 11), (), (3, 6, 9, 0, 11))}  # 5 -> 0
BASE_UNLISTED = 309                                          # TRIANGULATED, observed by slots 1 and 7 only: not in the window


def base_scene(seed=61):
    """12 slots x 96, 400 map points (GPU test 1).  Slot 5 is empty (kf_id -1) and still holds stale entries; slots 1, 7, 10 hold keyframes
    that are not local; the 8 local slots in descending KfId are not in slot order.  Rows 0 .. 199 have 1 .. 11 observers drawn over the
    occupied slots and flags 0, 2, 3; row 300 has 12 observations; rows 301 .. 308 are the cases of the apply tests; slot 7 also carries
    entries outside [0, n_mp)."""
    rng = np.random.default_rng(seed)
    sc = dict(n_kf=12, stride=96, n_mp=400, kf_id=np.array(BASE_KF_ID, np.int32))
    occupied = [s for s in range(12) if s != BASE_EMPTY]
    lists = [[] for _ in range(12)]
    flags = np.zeros(400, np.uint8)
    for r in range(200):
        n = 1 + r % 11 if r < 44 else int(rng.choice([1, 2, 2, 3, 3, 4, 5, 6, 8]))
        for s in rng.permutation(occupied)[:n]:
            if len(lists[s]) < 70:
                lists[s].append(r)
        flags[r] = (3, 3, 2, 0, 3)[r % 5]
    for s in occupied:
        lists[s].append(BASE_TWICE[0])
    lists[BASE_TWICE[1]].append(BASE_TWICE[0])
    for r, (loc, other, _) in BASE_APPLY.items():
        for s in loc + other:
            lists[s].append(r)
    for s in (1, 7):
        lists[s].append(BASE_UNLISTED)
    flags[300:310] = 3
    lists[BASE_EMPTY] = [300, 301, 302, 3, 4, 5]
    lists[7] += [400, 401, -2 ** 31]
    sc["mp_flags"] = flags
    sc = finish(sc, rng, lists)
    for r, (_, _, gone) in BASE_APPLY.items():               # gross outliers: the observations the apply tests erase lie 25 pixels off
        for s in gone:
            sc["kp"]["x"][s, sc["kf_mp"][s] == r] += np.float32(25.0)
    return sc


def base_conditions(sc, w):
    """What the base scene promises (asserted by the CPU tests on the restatement)."""
    local = set(BASE_LOCAL)
    assert [int(sc["kf_id"][s]) for s in BASE_LOCAL] == sorted((int(sc["kf_id"][s]) for s in BASE_LOCAL), reverse=True) and list(BASE_LOCAL) != sorted(BASE_LOCAL)
    assert sc["kf_id"][BASE_EMPTY] == -1 and all(sc["kf_id"][s] >= 0 and s not in local for s in BASE_NON_LOCAL) and len(local) == 8
    assert set(np.unique(sc["mp_flags"]).tolist()) == {0, 2, 3} and (sc["mp_flags"][w["rows"]] == 3).all()
    n_all = sc["n_obs"][w["rows"]]
    n_loc = np.bincount(w["edge_point"], minlength=w["n_rows"])
    assert set(range(1, 13)) <= set(n_all.tolist()), sorted(set(n_all.tolist()))
    assert (n_loc >= 1).all() and (n_loc == n_all).any() and (n_loc < n_all).any() and set(range(1, 9)) <= set(n_loc.tolist())
    assert sc["mp_flags"][BASE_UNLISTED] == 3 and sc["n_obs"][BASE_UNLISTED] == 2 and BASE_UNLISTED not in w["rows"]          # 0 local observations: not listed
    assert (sc["kf_mp"][BASE_TWICE[1]] == BASE_TWICE[0]).sum() == 2 and sc["n_obs"][BASE_TWICE[0]] == 12
    assert set(sc["kp"]["octave"][w["edge_slot"], w["edge_kp"]].tolist()) == set(range(N_LEVELS))
    assert len({tuple(c) for c in sc["cams"][list(BASE_LOCAL)]}) == 2
    assert 0 < w["n_current"] < w["n_edge"] < w["n_obs"]
    assert list(w["rows"]) == sorted(set(w["rows"].tolist()))


def base_chi2(sc, w):
    """The chi2 of the apply tests: the edges BASE_APPLY names are erased with the next float64 above the threshold or +inf; among the
    others one is exactly at the threshold, one NaN and one 0 (all kept); the rest stay below."""
    rng = np.random.default_rng(5)
    chi2 = rng.uniform(0.0, 5.9, w["n_edge"])
    row = w["rows"][w["edge_point"]]
    k = 0
    for r, (_, _, gone) in BASE_APPLY.items():
        for s in gone:
            e = np.nonzero((row == r) & (w["edge_slot"] == s))[0]
            assert len(e) == 1
            chi2[e[0]] = (np.nextafter(CHI2_THRESHOLD, np.inf), np.inf)[k % 2]
            k += 1
    kept = np.nonzero((row == 301) | (row == 307))[0]
    chi2[kept[0]], chi2[kept[1]], chi2[kept[2]] = CHI2_THRESHOLD, np.nan, 0.0
    return chi2


def apply_conditions(sc, w, chi2, after):
    n0, n1, f1 = sc["n_obs"], after["n_obs"], after["mp_flags"]
    want = {301: (2, 2, 3), 302: (4, 2, 2), 303: (4, 3, 3), 304: (3, 0, 2), 305: (5, 3, 3), 306: (2, 1, 2), 307: (3, 3, 3), 308: (5, 0, 2)}
    for r, (before, now, flag) in want.items():
        assert (n0[r], n1[r], f1[r]) == (before, now, flag), (r, n0[r], n1[r], f1[r])
    assert (chi2 == CHI2_THRESHOLD).sum() == 1 and np.isnan(chi2).sum() == 1 and np.isinf(chi2).sum() > 0 and (chi2 == np.nextafter(CHI2_THRESHOLD, np.inf)).sum() > 0


GATHER_TRIP, APPLY_TRIP = 256 * 256, 128 * 256              # what one trip of the offsets scan covers: 256 workgroups of 256 observations / of 128 edges
BIG_KF, BIG_STRIDE, BIG_ROWS, BIG_PER_ROW, BIG_LOCAL = 24, 3000, 6000, 12, 13


def big_scene(seed=67):
    """24 slots x 3000, 6000 TRIANGULATED rows of 12 observations each = 72 000 listed observations (281 workgroups: the offsets scan takes
    a second trip), 13 slots local."""
    rng = np.random.default_rng(seed)
    sc = dict(n_kf=BIG_KF, stride=BIG_STRIDE, n_mp=BIG_ROWS, kf_id=(rng.permutation(BIG_KF) * 3 + 1).astype(np.int32))
    lists = [[] for _ in range(BIG_KF)]
    for r in range(0, BIG_ROWS, 2):                          # a pair of rows shares out the 24 slots: every slot is exactly full
        order = rng.permutation(BIG_KF)
        for i, s in enumerate(order):
            lists[s].append(r + (i >= BIG_PER_ROW))
    sc["mp_flags"] = np.full(BIG_ROWS, 3, np.uint8)
    sc = finish(sc, rng, lists)
    order = np.argsort(-sc["kf_id"].astype(np.int64))
    sc["local"] = order[:BIG_LOCAL].astype(np.int32)         # the 13 newest keyframes, descending KfId
    return sc


def big_conditions(sc, w):
    assert w["n_obs"] == BIG_ROWS * BIG_PER_ROW > 65536 and w["n_rows"] == BIG_ROWS
    keep = w["keep"]                                         # positions of the kept edges among the listed observations
    assert (keep < 65536).any() and (keep >= 65536).any()
    carry = int((keep < 65536).sum())                        # what the second trip of the offsets scan starts from
    assert 0 < carry < w["n_edge"] and (np.nonzero(keep >= 65536)[0] >= carry).all()
    return carry


def big_chi2(w):
    """A chi2 per edge of the big window, about a quarter of them above the threshold."""
    return np.random.default_rng(9).uniform(0, 8, w["n_edge"])


def round_trip_margin():
    """The restatement's own error on the round trip pose -> quaternion -> pose: the largest element-wise difference it shows on the base
    scene's local poses after a re-orthonormalisation (the nearest rotation, by SVD)."""
    sc, _ = cached("base")
    margin = 0.0
    for s in BASE_LOCAL:
        M = sc["poses"][s].reshape(3, 4)[:, :3]
        U, _, Vt = np.linalg.svd(M)
        O = U @ Vt
        q, _, _ = quat_of_matrix(O.reshape(9))
        back = np.array(matrix_of_pose(q + [0.0, 0.0, 0.0])).reshape(3, 4)[:, :3]
        margin = max(margin, float(np.abs(back - O).max()))
    return margin


_CACHE = {}


def cached(name):
    """base / big: (scene, window) computed once and shared; callers must not change them."""
    if name not in _CACHE:
        sc = base_scene() if name == "base" else big_scene()
        _CACHE[name] = (sc, gather(sc, BASE_LOCAL if name == "base" else sc["local"], 0))
    return _CACHE[name]
