"""The specification of ms_loop_usable_mask, ms_loop_pairs and ms_loop_sim3_lists: the three pieces of
LoopCloser::tryLoopClosure (loop_closer.cpp:126-378) between its batched solvers, restated twice.

  *_map      on a map of dicts as the reference holds it: mapPoints[id] = dict(position, status, observations {kfId: kpId}),
             keyframes[id] = dict(mapPoints [kp] -> id or -1, poseCW 3 x 4, keyPoints x / y / octave, cam fx fy cx cy w h).  A map-point id is
             its table row; a keyframe id is NOT its slot (slot_of).
  *_tables   on the device tables' arrays (tables(S)), derived from the same map plus `stale`: entries of kf_mp that still name a row whose
             mp_live is 0 -- the map knows nothing of them, the tables must drop them.

Arithmetic (numpy evaluates it as written, without contraction): the camera-frame point is ((R[i][0] p0 + R[i][1] p1) + R[i][2] p2) + t_i in
float64; a threshold is the float32 product 9.21034f * levelSigmaSq[octave]; an observation is ((x - cx) / fx, (y - cy) / fy) of the float32
pixel in float64; an information is levelSigmaSq[octave]."""
import numpy as np

TRIP = 256                                                   # keypoints per trip of the walk, candidates per trip of the offsets scan
CHI_SQ_2D = np.float32(9.21034)
TRIANGULATED, UNSURE, NOT_TRIANGULATED = 3, 2, 0             # mp_flags: bit 0 = TRIANGULATED, bit 1 = neither NOT_TRIANGULATED nor BAD
DROPS = ("no match", "r1 absent", "r2 absent", "same row", "dead row")
PAIR_ARRAYS = ("kp1", "kp2", "row1", "row2", "pts1", "pts2", "thr1", "thr2")
SIM3_ARRAYS = ("pts1", "pts2", "obs1", "obs2", "info1", "info2", "row1", "row2")


def cam_point(P, p):
    """poseCW * p for P [..., 3, 4] and p [..., 3] in the pinned operation order."""
    P, p = np.asarray(P, np.float64), np.asarray(p, np.float64)
    return ((P[..., :, 0] * p[..., None, 0] + P[..., :, 1] * p[..., None, 1]) + P[..., :, 2] * p[..., None, 2]) + P[..., :, 3]


def level_sigma_sq(n_levels, f=1.2):
    s = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        s[i] = s[i - 1] * np.float32(f)
    return (s * s).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the map form
def usable_mask_map(S, kf_id, require):
    """keyframe_matcher.cpp:79-84 / :94-96, and the mps argument of matchMapPointsSim3 (:568-571)."""
    kf = S["keyframes"][kf_id]
    n = len(kf["mapPoints"])
    usable, tri_row = np.zeros(n, np.uint8), np.full(n, -1, np.int32)
    for k, mp_id in enumerate(kf["mapPoints"]):
        if mp_id == -1:
            continue
        tri = S["mapPoints"][mp_id]["status"] == TRIANGULATED
        usable[k] = 1 if (tri or not require) else 0
        if tri:
            tri_row[k] = mp_id
    return usable, tri_row


def _empty_pairs(n_cand):
    return dict(pair_start=[0], kp1=[], kp2=[], row1=[], row2=[], pts1=[], pts2=[], thr1=[], thr2=[])


def _finish(w, spec):
    for k, (dt, width) in spec.items():
        w[k] = np.array(w[k], dt).reshape((-1, width) if width > 1 else (-1,))
    return w


_PAIR_SPEC = dict(pair_start=(np.int32, 1), kp1=(np.int32, 1), kp2=(np.int32, 1), row1=(np.int32, 1), row2=(np.int32, 1), pts1=(np.float64, 3), pts2=(np.float64, 3),
                  thr1=(np.float32, 1), thr2=(np.float32, 1))
_SIM3_SPEC = dict(pts1=(np.float64, 3), pts2=(np.float64, 3), obs1=(np.float64, 2), obs2=(np.float64, 2), info1=(np.float32, 1), info2=(np.float32, 1),
                  row1=(np.int32, 1), row2=(np.int32, 1))


def pairs_map(S, matched=None):
    """loop_closer.cpp:203-213, then the LoopRansac constructor (loop_ransac.cpp:17-41), candidate by candidate."""
    matched = S["matched"] if matched is None else matched
    cur = S["keyframes"][S["cur_id"]]
    sig = S["level_sigma_sq"]
    w = _empty_pairs(len(S["cand_ids"]))
    reasons = []                                             # per candidate: per keypoint of cur, None (kept) or the drop reason as the MAP sees it
    for c, cand_id in enumerate(S["cand_ids"]):
        cand = S["keyframes"][cand_id]
        matches, why = [], []
        for i, m in enumerate(matched[c]):
            if m < 0:
                why.append("no match")
                continue
            id1, id2 = cur["mapPoints"][i], cand["mapPoints"][m]
            if id1 != -1 and id2 != -1 and id1 != id2:
                matches.append((id1, id2))
                why.append(None)
            else:
                why.append("r1 absent" if id1 == -1 else "r2 absent" if id2 == -1 else "same row")
        reasons.append(why)
        for id1, id2 in matches:
            mp1, mp2 = S["mapPoints"][id1], S["mapPoints"][id2]
            k1, k2 = mp1["observations"][S["cur_id"]], mp2["observations"][cand_id]
            w["kp1"].append(k1); w["kp2"].append(k2); w["row1"].append(id1); w["row2"].append(id2)
            w["pts1"].append(cam_point(cur["poseCW"], mp1["position"]))
            w["pts2"].append(cam_point(cand["poseCW"], mp2["position"]))
            w["thr1"].append(CHI_SQ_2D * sig[cur["keyPoints"]["octave"][k1]])
            w["thr2"].append(CHI_SQ_2D * sig[cand["keyPoints"]["octave"][k2]])
        w["pair_start"].append(len(w["kp1"]))
    w = _finish(w, _PAIR_SPEC)
    w["n_pairs"] = int(w["pair_start"][-1])
    w["cur_pose"] = np.array(cur["poseCW"], np.float64).reshape(12)
    w["cand_pose"] = np.array([S["keyframes"][k]["poseCW"] for k in S["cand_ids"]], np.float64).reshape(-1, 12)
    w["reasons"] = reasons
    return w


def sim3_lists_map(S, lists):
    """optimize_transform.cpp:44-59 and :101-142 for the match lists `lists` = per candidate a list of (MpId, MpId)."""
    cur = S["keyframes"][S["cur_id"]]
    sig = S["level_sigma_sq"]
    w = {k: [] for k in _SIM3_SPEC}

    def obs(kf, k):
        fx, fy, cx, cy = kf["cam"][:4]
        return ((np.float64(kf["keyPoints"]["x"][k]) - cx) / fx, (np.float64(kf["keyPoints"]["y"][k]) - cy) / fy)

    for cand_id, matches in zip(S["cand_ids"], lists):
        cand = S["keyframes"][cand_id]
        for id1, id2 in matches:
            mp1, mp2 = S["mapPoints"][id1], S["mapPoints"][id2]
            k1, k2 = mp1["observations"][S["cur_id"]], mp2["observations"][cand_id]
            w["row1"].append(id1); w["row2"].append(id2)
            w["pts1"].append(cam_point(cur["poseCW"], mp1["position"]))
            w["pts2"].append(cam_point(cand["poseCW"], mp2["position"]))
            w["obs1"].append(obs(cur, k1)); w["obs2"].append(obs(cand, k2))
            w["info1"].append(sig[cur["keyPoints"]["octave"][k1]]); w["info2"].append(sig[cand["keyPoints"]["octave"][k2]])
    return _finish(w, _SIM3_SPEC)


def keypoint_lists(S, lists):
    """The (kp1, kp2, match_start) form of the match lists that ms_loop_sim3_lists takes (loop_closer.cpp:258-264)."""
    kp1, kp2, start = [], [], [0]
    for cand_id, matches in zip(S["cand_ids"], lists):
        for id1, id2 in matches:
            kp1.append(S["mapPoints"][id1]["observations"][S["cur_id"]])
            kp2.append(S["mapPoints"][id2]["observations"][cand_id])
        start.append(len(kp1))
    return np.array(kp1, np.int32), np.array(kp2, np.int32), np.array(start, np.int32)


# ---------------------------------------------------------------------------------------------------------------- the tables form
def tables(S):
    """The device tables of the map S (and its stale entries): kf_mp [n_kf, stride], mp_flags, mp_live, mp_pos, kf_pose [n_kf, 12], kp_x / kp_y /
    kp_octave [n_kf, stride], cams [n_kf, 6]."""
    n_kf, stride, n_mp = S["n_kf"], S["stride"], S["n_mp"]
    t = dict(kf_mp=np.full((n_kf, stride), -1, np.int32), mp_flags=np.zeros(n_mp, np.uint8), mp_live=np.zeros(n_mp, np.uint8), mp_pos=np.zeros((n_mp, 3), np.float64),
             kf_pose=np.zeros((n_kf, 12), np.float64), kp_x=np.zeros((n_kf, stride), np.float32), kp_y=np.zeros((n_kf, stride), np.float32),
             kp_octave=np.zeros((n_kf, stride), np.int32), cams=np.zeros((n_kf, 6), np.float64), n_kp=np.zeros(n_kf, np.int32))
    t["kf_pose"][:, [0, 5, 10]] = 1.0
    t["cams"][:] = (500.0, 500.0, 320.0, 240.0, 640, 480)
    for mp_id, mp in S["mapPoints"].items():
        t["mp_flags"][mp_id], t["mp_live"][mp_id], t["mp_pos"][mp_id] = mp["status"], 1, mp["position"]
    for row, pos in S["dead"].items():                       # rows that were culled: their flags and positions linger, mp_live is 0
        t["mp_flags"][row], t["mp_pos"][row] = TRIANGULATED, pos
    for kf_id, kf in S["keyframes"].items():
        s, n = S["slot_of"][kf_id], len(kf["mapPoints"])
        t["kf_mp"][s, :n] = kf["mapPoints"]
        t["kf_pose"][s] = np.asarray(kf["poseCW"], np.float64).reshape(12)
        t["kp_x"][s, :n], t["kp_y"][s, :n], t["kp_octave"][s, :n] = kf["keyPoints"]["x"], kf["keyPoints"]["y"], kf["keyPoints"]["octave"]
        t["cams"][s], t["n_kp"][s] = kf["cam"], n
    for slot, kp, row in S["stale"]:
        assert t["kf_mp"][slot, kp] == -1 and not t["mp_live"][row]
        t["kf_mp"][slot, kp] = row
    return t


def present(t, r):
    r = np.asarray(r)
    ok = (r >= 0) & (r < len(t["mp_live"]))
    return ok & (t["mp_live"][np.where(ok, r, 0)] != 0)


def usable_mask_tables(t, slot, n_kp, require):
    r = t["kf_mp"][slot, :n_kp]
    there = present(t, r)
    tri = there & ((t["mp_flags"][np.where(there, r, 0)] & 1) != 0)
    return (there & (tri | (not require))).astype(np.uint8), np.where(tri, r, -1).astype(np.int32)


def pairs_tables(S, t, matched=None):
    matched = S["matched"] if matched is None else matched
    cur, sig = S["cur"], S["level_sigma_sq"]
    w = _empty_pairs(len(S["cand_slot"]))
    parts = {k: [] for k in PAIR_ARRAYS}
    for c, slot in enumerate(S["cand_slot"]):
        m = np.asarray(matched[c], np.int32)
        i = np.arange(len(m))
        has = m >= 0
        r1 = t["kf_mp"][cur, i]
        r2 = np.where(has, t["kf_mp"][slot, np.where(has, m, 0)], -1)
        keep = has & present(t, r1) & present(t, r2) & (r1 != r2)
        i, m, r1, r2 = i[keep], m[keep], r1[keep], r2[keep]
        parts["kp1"].append(i); parts["kp2"].append(m); parts["row1"].append(r1); parts["row2"].append(r2)
        parts["pts1"].append(cam_point(t["kf_pose"][cur].reshape(3, 4), t["mp_pos"][r1]).reshape(-1, 3))
        parts["pts2"].append(cam_point(t["kf_pose"][slot].reshape(3, 4), t["mp_pos"][r2]).reshape(-1, 3))
        parts["thr1"].append(CHI_SQ_2D * sig[t["kp_octave"][cur, i]]); parts["thr2"].append(CHI_SQ_2D * sig[t["kp_octave"][slot, m]])
        w["pair_start"].append(w["pair_start"][-1] + int(keep.sum()))
    for k in PAIR_ARRAYS:
        w[k] = np.concatenate(parts[k]) if parts[k] else []
    w = _finish(w, _PAIR_SPEC)
    w["n_pairs"] = int(w["pair_start"][-1])
    w["cur_pose"] = t["kf_pose"][cur].copy()
    w["cand_pose"] = t["kf_pose"][np.asarray(S["cand_slot"], np.int64)].reshape(-1, 12).copy()
    return w


def sim3_lists_tables(S, t, kp1, kp2, match_start):
    cur, sig = S["cur"], S["level_sigma_sq"]
    slot = np.repeat(np.asarray(S["cand_slot"], np.int64), np.diff(match_start))
    r1, r2 = t["kf_mp"][cur, kp1], t["kf_mp"][slot, kp2]
    w = dict(row1=r1, row2=r2)
    w["pts1"] = cam_point(t["kf_pose"][cur].reshape(3, 4), t["mp_pos"][r1]).reshape(-1, 3)
    w["pts2"] = cam_point(t["kf_pose"][slot].reshape(-1, 3, 4), t["mp_pos"][r2]).reshape(-1, 3)

    def obs(s, k):
        cam = t["cams"][s].reshape(-1, 6) if np.ndim(s) else t["cams"][s][None]
        return np.stack([(t["kp_x"][s, k].astype(np.float64) - cam[:, 2]) / cam[:, 0], (t["kp_y"][s, k].astype(np.float64) - cam[:, 3]) / cam[:, 1]], axis=-1)

    w["obs1"], w["obs2"] = obs(cur, kp1), obs(slot, kp2)
    w["info1"], w["info2"] = sig[t["kp_octave"][cur, kp1]], sig[t["kp_octave"][slot, kp2]]
    return _finish(w, _SIM3_SPEC)


# ---------------------------------------------------------------------------------------------------------------- scenes
def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def scene(n_kf, stride, n_mp, cur, n_kp_cur, cand_slot, n_kp_cand, n_levels=8, seed=1, p_bound=0.8, p_match=0.7, empty_first_trip=()):
    """A map with a current keyframe in slot `cur` and candidates in cand_slot (n_kp_cand keypoints each), the matcher's output `matched` for
    each pair, and the conditions the device tests rely on: in every trip of TRIP keypoints of the current keyframe, against every candidate
    of at least 16 keypoints, each reason of DROPS occurs.  empty_first_trip: candidates (indices) whose first trip keeps no pair."""
    rng = np.random.default_rng(seed)
    cand_slot, n_kp_cand = list(cand_slot), list(n_kp_cand)
    n_kp = rng.integers(1, stride + 1, n_kf)
    n_kp[cur] = n_kp_cur
    for s, n in zip(cand_slot, n_kp_cand):
        n_kp[s] = n
    n_dead = max(8, n_mp // 50)
    dead_rows = rng.choice(n_mp, n_dead, replace=False)
    live_rows = np.setdiff1d(np.arange(n_mp), dead_rows)
    n_trips = (n_kp_cur + TRIP - 1) // TRIP
    n_big = sum(n >= 16 for n in n_kp_cand)
    n_spare = 3 * n_trips * (n_big + 1) + 8 + sum(n for n in n_kp_cand if n <= 2)
    # same_rows: rows the current keyframe and every large candidate list; spare: rows no random binding uses, each handed out once
    same_rows, spare, free_rows = live_rows[:n_trips], [int(r) for r in live_rows[n_trips:n_trips + n_spare]], live_rows[n_trips + n_spare:]
    bind = {}
    for s in range(n_kf):
        n_b = min(int(p_bound * n_kp[s]), len(free_rows))
        b = np.full(n_kp[s], -1, np.int64)
        if n_b:
            b[rng.choice(n_kp[s], n_b, replace=False)] = rng.choice(free_rows, n_b, replace=False)
        bind[s] = b
    for s, n in zip(cand_slot, n_kp_cand):                   # a short candidate has every keypoint bound, so that it can have a pair
        if n <= 2:
            bind[s][:] = [spare.pop() for _ in range(n)]
    # the forced keypoints of the current keyframe, five per trip: no match | unbound | bound | bound to a shared row | the dead row's pair.  The
    # dead row sits on the current keyframe's side in the even trips and on the candidate's side in the odd ones.
    stale, forced = [], []
    for tr in range(n_trips):
        lo, hi = tr * TRIP, min((tr + 1) * TRIP, n_kp_cur)
        if hi - lo < 5:
            forced.append(None)
            continue
        i = lo + rng.choice(hi - lo, 5, replace=False)
        bind[cur][i[0]] = spare.pop()
        bind[cur][i[1]] = -1
        bind[cur][i[2]] = spare.pop()
        bind[cur][i[3]] = same_rows[tr]
        if tr % 2 == 0:
            bind[cur][i[4]] = -1
            stale.append((cur, int(i[4]), int(dead_rows[tr % n_dead])))
        else:
            bind[cur][i[4]] = spare.pop()
        forced.append(i)
    taken = set(int(k) for f in forced if f is not None for k in f)
    matched = []
    for c, (s, n) in enumerate(zip(cand_slot, n_kp_cand)):
        m = np.full(n_kp_cur, -1, np.int32)
        targets = [int(k) for k in rng.permutation(n)]
        big = n >= 16
        if big:
            for tr, i in enumerate(forced):
                if i is None:
                    continue
                t = [targets.pop() for _ in range(4)]
                m[i[1]], m[i[2]], m[i[3]], m[i[4]] = t
                bind[s][t[0]] = spare.pop()
                bind[s][t[1]] = -1
                bind[s][t[2]] = same_rows[tr]
                if tr % 2 == 0:
                    bind[s][t[3]] = spare.pop()
                else:
                    bind[s][t[3]] = -1
                    stale.append((s, t[3], int(dead_rows[(tr + c) % n_dead])))
        eligible = [i for i in range(n_kp_cur) if not (big and i in taken) and not (not big and bind[cur][i] < 0) and not (c in empty_first_trip and i < TRIP)]
        for i in rng.choice(eligible, min(len(targets), int(np.ceil(p_match * len(eligible)))), replace=False) if eligible else ():
            m[i] = targets.pop()
        matched.append(m)
    # the map
    poses = {s: np.concatenate([_rotation(rng), rng.uniform(-2, 2, (3, 1))], axis=1) for s in range(n_kf)}
    slot_of = {100 + 3 * ((s * 7) % n_kf): s for s in range(n_kf)} if np.gcd(7, n_kf) == 1 else {100 + 3 * s: s for s in range(n_kf)}
    id_of = {s: k for k, s in slot_of.items()}
    map_points, keyframes = {}, {}
    for s in range(n_kf):
        n = int(n_kp[s])
        keyframes[id_of[s]] = dict(mapPoints=[int(r) for r in bind[s]], poseCW=poses[s],
                                   keyPoints=dict(x=rng.uniform(0, 640, n).astype(np.float32), y=rng.uniform(0, 480, n).astype(np.float32),
                                                  octave=rng.integers(0, n_levels, n).astype(np.int32)),
                                   cam=(rng.uniform(400, 600), rng.uniform(400, 600), rng.uniform(300, 340), rng.uniform(220, 260), 640, 480))
        for k, r in enumerate(bind[s]):
            if r >= 0:
                mp = map_points.setdefault(int(r), dict(position=rng.uniform(-5, 5, 3), status=int(rng.choice((TRIANGULATED, TRIANGULATED, UNSURE, NOT_TRIANGULATED))),
                                                        observations={}))
                assert id_of[s] not in mp["observations"]
                mp["observations"][id_of[s]] = k
    return dict(n_kf=n_kf, stride=stride, n_mp=n_mp, n_levels=n_levels, level_sigma_sq=level_sigma_sq(n_levels), mapPoints=map_points, keyframes=keyframes, slot_of=slot_of,
                cur=cur, cur_id=id_of[cur], n_kp_cur=n_kp_cur, cand_slot=np.array(cand_slot, np.int32), cand_ids=[id_of[s] for s in cand_slot],
                n_kp_cand=np.array(n_kp_cand, np.int32), matched=matched, stale=stale, dead={int(r): rng.uniform(-5, 5, 3) for r in dead_rows},
                forced=forced)


def match_lists(S, w, seed=3):
    """Final match lists per candidate as (MpId, MpId): every other pair of `w` (the RANSAC inliers' stand-in) plus, as what matchMapPointsSim3
    appends, pairs of bound keypoints the matcher did not join."""
    rng = np.random.default_rng(seed)
    cur = S["keyframes"][S["cur_id"]]
    lists = []
    for c, cand_id in enumerate(S["cand_ids"]):
        lo, hi = w["pair_start"][c], w["pair_start"][c + 1]
        lst = [(int(w["row1"][e]), int(w["row2"][e])) for e in range(lo, hi, 2)]
        used1, used2 = {a for a, _ in lst}, {b for _, b in lst}
        extra1 = [r for r in cur["mapPoints"] if r != -1 and r not in used1]
        extra2 = [r for r in S["keyframes"][cand_id]["mapPoints"] if r != -1 and r not in used2]
        n_extra = min(len(extra1), len(extra2), 7)
        if n_extra:
            lst += list(zip([int(extra1[k]) for k in rng.choice(len(extra1), n_extra, replace=False)],
                            [int(extra2[k]) for k in rng.choice(len(extra2), n_extra, replace=False)]))
        lists.append(lst)
    return lists


def drop_reasons(S, t, w):
    """Per candidate and keypoint of the current keyframe: None (kept) or the reason of DROPS, with the dead rows told from the absent ones."""
    out = []
    for c, slot in enumerate(S["cand_slot"]):
        why = list(w["reasons"][c])
        for i, m in enumerate(S["matched"][c]):
            if m < 0:
                continue
            r1, r2 = t["kf_mp"][S["cur"], i], t["kf_mp"][slot, m]
            if (r1 >= 0 and not t["mp_live"][r1]) or (r2 >= 0 and not t["mp_live"][r2]):
                assert why[i] in ("r1 absent", "r2 absent")
                why[i] = "dead row"
        out.append(why)
    return out


def chain_scene(seed=21, n_pts=420, n_extra=30, n_levels=4):
    """A geometric scene for the whole chain, in tables form: n_pts world points seen by the current keyframe (slot 0, rows [0, n_pts)) and by
    two candidates (slots 1 and 2, with rows of their own for the same physical points: the two ends of a loop), pixels = the float32
    projections, descriptors = the point's with a few bits flipped, the BoW node = point index % 24 -- but every tenth point sits in another
    node in the candidates, so the BoW-guided matcher leaves it to matchMapPointsSim3.  A point's keypoints share their octave and the row's
    max_dist predicts it.  Every keyframe has n_extra unbound keypoints besides; some rows are UNSURE.  Returns (S, t, frames): frames[slot] =
    dict(desc, angle, bucket); S["mp_table"] = the map-point table of the gates (pos, norm, min_dist, max_dist, desc)."""
    rng = np.random.default_rng(seed)
    n_kf, stride, n_mp = 3, n_pts + n_extra, 3 * n_pts
    X = np.stack([rng.uniform(-2, 2, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(4, 8, n_pts)], axis=1)
    base_desc = rng.integers(0, 2 ** 32, (n_pts, 8), dtype=np.uint64).astype(np.uint32)
    t = dict(kf_mp=np.full((n_kf, stride), -1, np.int32), mp_flags=np.full(n_mp, TRIANGULATED, np.uint8), mp_live=np.ones(n_mp, np.uint8), mp_pos=np.zeros((n_mp, 3)),
             kf_pose=np.zeros((n_kf, 12)), kp_x=np.zeros((n_kf, stride), np.float32), kp_y=np.zeros((n_kf, stride), np.float32),
             kp_octave=np.zeros((n_kf, stride), np.int32), cams=np.tile(np.array([500.0, 500.0, 320.0, 240.0, 640, 480]), (n_kf, 1)),
             n_kp=np.full(n_kf, stride, np.int32))
    t["mp_flags"][rng.choice(n_mp, n_mp // 10, replace=False)] = UNSURE
    octave = rng.integers(0, n_levels, n_pts)
    table = dict(pos=t["mp_pos"], norm=np.zeros((n_mp, 3), np.float32), min_dist=np.full(n_mp, 0.1, np.float32), max_dist=np.zeros(n_mp, np.float32),
                 desc=np.zeros((n_mp, 8), np.uint32))
    frames = []
    for s in range(n_kf):
        a = rng.uniform(-0.04, 0.04, 3) * (s > 0)
        Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        P = np.concatenate([Rx @ Ry, (rng.uniform(-0.25, 0.25, (3, 1)) * (s > 0))], axis=1)
        t["kf_pose"][s] = P.reshape(12)
        rows = s * n_pts + rng.permutation(n_pts)            # keypoint k of the slot sees world point k through row rows[k]
        t["mp_pos"][rows] = X + rng.normal(0, 1e-4, X.shape) * (s > 0)
        t["kf_mp"][s, :n_pts] = rows
        pc = cam_point(P, t["mp_pos"][rows])
        t["kp_x"][s, :n_pts] = (500.0 * pc[:, 0] / pc[:, 2] + 320.0).astype(np.float32)
        t["kp_y"][s, :n_pts] = (500.0 * pc[:, 1] / pc[:, 2] + 240.0).astype(np.float32)
        t["kp_x"][s, n_pts:], t["kp_y"][s, n_pts:] = rng.uniform(0, 640, n_extra), rng.uniform(0, 480, n_extra)
        t["kp_octave"][s] = np.concatenate([octave, rng.integers(0, n_levels, n_extra)])
        table["max_dist"][rows] = (np.sqrt((pc * pc).sum(axis=1)) * 1.2 ** (octave - 0.5)).astype(np.float32)   # predictScaleLevel gives octave from nearby
        table["desc"][rows] = base_desc
        desc = np.concatenate([base_desc, rng.integers(0, 2 ** 32, (n_extra, 8), dtype=np.uint64).astype(np.uint32)])
        bucket = np.arange(stride) % 24
        if s > 0:
            bucket[3:n_pts:10] = (bucket[3:n_pts:10] + 7) % 24
        flip = np.zeros_like(desc)
        for _ in range(6):
            flip[np.arange(stride), rng.integers(0, 8, stride)] |= (np.uint32(1) << rng.integers(0, 32, stride).astype(np.uint32))
        frames.append(dict(desc=desc ^ flip, angle=np.concatenate([np.linspace(0, 359, n_pts), rng.uniform(0, 360, n_extra)]).astype(np.float32),
                           bucket=bucket.astype(np.int32)))
    S = dict(n_kf=n_kf, stride=stride, n_mp=n_mp, n_levels=n_levels, level_sigma_sq=level_sigma_sq(n_levels), cur=0, n_kp_cur=stride,
             cand_slot=np.array([1, 2], np.int32), n_kp_cand=np.array([stride, stride], np.int32), mp_table=table)
    return S, t, frames


_SCENES = {}
SCENES = ("base", "cands257", "small")


def gpu_scene(name):
    """The scenes of the device tests, built once: S with S['tables'], S['want'] (pairs), S['lists'] / S['want_sim3'] (the final match lists)."""
    if name not in _SCENES:
        if name == "base":                                   # three trips of the walk; a candidate without a pair between two others; a first trip that keeps nothing
            S = scene(12, 640, 3000, cur=4, n_kp_cur=600, cand_slot=(9, 2, 7, 0, 11), n_kp_cand=(600, 0, 257, 1, 256), seed=11, empty_first_trip=(2,))
        elif name == "cands257":                             # the offsets scan over the candidates past its first trip
            S = scene(300, 8, 2000, cur=299, n_kp_cur=8, cand_slot=range(257), n_kp_cand=[8] * 257, seed=12, p_match=0.9)
        elif name == "small":
            S = scene(4, 16, 60, cur=1, n_kp_cur=16, cand_slot=(3, 0), n_kp_cand=(16, 12), seed=13, p_match=0.9, p_bound=0.9)
        else:
            raise KeyError(name)
        S["tables"] = tables(S)
        S["want"] = pairs_map(S)
        S["lists"] = match_lists(S, S["want"])
        S["want_sim3"] = sim3_lists_map(S, S["lists"])
        _SCENES[name] = S
    return _SCENES[name]
