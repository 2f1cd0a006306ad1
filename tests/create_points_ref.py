"""The specification of ms_create_points_lists, ms_create_points_bind and ms_unbound_mask: createNewMapPoints
(mapper_helpers.cpp:271-318) restated twice.

  sequential()   the function as the reference runs it, with Keyframe and MapPoint objects as dicts (mapPoints per keyframe; observations
                 keyed and sorted by KfId), one adjacent keyframe after the other and one match after the other: the matcher reads
                 `mapPoints[kp] == -1` live, the point is built (:293-301), triangulated (:308, triangulate_ref.triangulate_point) and, on
                 success, registered and bound with the descriptor rule of map_point.cpp:75-116 (:309-316).
  staged()       the same steps in table form, as the device chain runs them: masks (ms_unbound_mask, once), then per adjacent the matcher
                 on the masks, lists (ms_create_points_lists), triangulate (ms_triangulate_lists), bind (ms_create_points_bind).

They are equal because the matches of one adjacent name every keypoint at most once: no match reads what another match of the same adjacent
wrote, and between adjacents the masks carry exactly what `mapPoints[kp] == -1` would give.  tests/test_create_points_ref.py holds them
equal on the fixture.  The matcher is the oracle's (mso.match_triangulation, mso.create_E21).

A scene is a dict: kf_mp [n_kf, stride], kf_id, n_kp [n_kf], poses [n_kf, 12], cams [n_kf, 6], focal, kp (x, y, octave, depth, each
[n_kf, stride]), angle [n_kf, stride], node [n_kf, stride], desc_base [n_kf], pool [n_pool, 8], table (pos, norm, min_dist, max_dist, desc),
mp_flags, mp_live, n_obs, mp_track [n_mp], S (triangulate_ref.settings), sf (scale factors), thr_deg.

A row that fails its triangulation is handed back: it stays mp_live = 0 and mp_flags = 0.  Its mp_pos holds whatever triangulateMapPoint
left in the discarded MapPoint (the entry value, or the depth position of :622); both restatements keep that in the table, as the device
does, so that mp_pos can be compared over the whole table."""
import numpy as np

import map_refresh_ref as MR
import triangulate_ref as TR

F = np.float32
INVALID, CAPACITY = -1, -4                                   # MS_ERR_INVALID, MS_ERR_CAPACITY
TABLES = ("kf_mp", "mp_flags", "mp_live", "n_obs", "mp_track")
FIELDS = ("pos", "norm", "min_dist", "max_dist", "desc")
LISTS = ("rows", "obs_start", "n_obs_row", "first_octave", "was_triangulated", "obs_kf", "obs_kp", "obs_octave", "obs_desc", "obs_x", "obs_y", "obs_depth")


def oracle():
    """The CPU oracle, built on first use."""
    if "mso" not in _CACHE:
        import mso
        mso.build()
        _CACHE["mso"] = mso
    return _CACHE["mso"]


def copy_state(sc):
    st = dict(sc)
    for k in TABLES:
        st[k] = np.array(sc[k], copy=True)
    st["table"] = {k: np.array(v, copy=True) for k, v in sc["table"].items()}
    return st


def snapshot(st, masks):
    out = {k: st[k].copy() for k in TABLES}
    out["table"] = {k: v.copy() for k, v in st["table"].items()}
    out["masks"] = {s: m.copy() for s, m in masks.items()}
    return out


def same_state(a, b):
    """Every table of two states (or snapshots) bit for bit."""
    bits = lambda v: np.ascontiguousarray(v).view(np.uint8)
    return all(np.array_equal(a[k], b[k]) for k in TABLES) and all(np.array_equal(bits(a["table"][k]), bits(b["table"][k])) for k in FIELDS)


def same_masks(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[s], b[s]) for s in a)


def bearings(sc, slot):
    """KeyPoint::bearing of the slot's keypoints: the unit vector of the normalized pixel, float64."""
    n = int(sc["n_kp"][slot])
    fx, fy, cx, cy = sc["cams"][slot][:4]
    xn = (sc["kp"]["x"][slot, :n].astype(np.float64) - cx) / fx
    yn = (sc["kp"]["y"][slot, :n].astype(np.float64) - cy) / fy
    b = np.stack([xn, yn, np.ones(n)], axis=1)
    return b / np.linalg.norm(b, axis=1)[:, None]


def descriptors(sc, slot):
    n = int(sc["n_kp"][slot])
    return sc["pool"][sc["desc_base"][slot]:sc["desc_base"][slot] + n]


def essential(sc, current, adj):
    """The call order of keyframe_matcher.cpp:171-175: create_E_21(kf2.R, kf2.t, kf1.R, kf1.t)."""
    P1, P2 = sc["poses"][current].reshape(3, 4), sc["poses"][adj].reshape(3, 4)
    return oracle().create_E21(P2[:, :3], P2[:, 3], P1[:, :3], P1[:, 3])


def match(sc, current, adj, usable1, usable2):
    """matchForTriangulationDBoW of the pair; matched [n_kp(current)], -1 none."""
    n1, n2 = int(sc["n_kp"][current]), int(sc["n_kp"][adj])
    _, m = oracle().match_triangulation(descriptors(sc, current), sc["angle"][current, :n1], sc["kp"]["octave"][current, :n1], bearings(sc, current), usable1,
                                        sc["node"][current, :n1], descriptors(sc, adj), sc["angle"][adj, :n2], bearings(sc, adj), usable2, sc["node"][adj, :n2],
                                        essential(sc, current, adj), sc["sf"], sc["thr_deg"], True)
    return m.astype(np.int32)


# ---------------------------------------------------------------------------------------------------- the sequential restatement
def sequential(sc, current, adjacent, free_rows, mode=TR.TME):
    """:271-318.  Returns (state, per adjacent: None for the skipped slot or a dict)."""
    st = copy_state(sc)
    n_mp = len(st["mp_live"])
    keyframes = [dict(id=int(st["kf_id"][s]), slot=s, mapPoints=[int(v) if 0 <= v < n_mp else -1 for v in st["kf_mp"][s, :st["n_kp"][s]]]) for s in range(len(st["kf_id"]))]
    slot_of = {kf["id"]: kf["slot"] for kf in keyframes}
    cur = keyframes[current]
    initial1 = np.array([mp == -1 for mp in cur["mapPoints"]], np.uint8)
    free = [int(r) for r in free_rows]
    i32 = lambda a: np.array(a, np.int32)
    results = []
    for adj_slot in adjacent:
        if adj_slot == current:                              # :281
            results.append(None)
            continue
        adj = keyframes[adj_slot]
        usable1 = np.array([mp == -1 for mp in cur["mapPoints"]], np.uint8)     # keyframe_matcher.cpp:205-221, read live
        usable2 = np.array([mp == -1 for mp in adj["mapPoints"]], np.uint8)
        matched = match(sc, current, adj_slot, usable1, usable2)
        would = match(sc, current, adj_slot, initial1, usable2)
        pairs = [(kp1, int(kp2)) for kp1, kp2 in enumerate(matched) if kp2 >= 0]                         # :282-290, ascending kp1
        assert len(pairs) <= len(free)
        rows = free[:len(pairs)]
        status, reason, created = [], [], []
        for i, (kp1, kp2) in enumerate(pairs):
            row = free[i]
            assert not st["mp_live"][row] and cur["mapPoints"][kp1] == -1 and adj["mapPoints"][kp2] == -1
            mp = dict(observations={cur["id"]: kp1, adj["id"]: kp2}, status=TR.NOT_TRIANGULATED)        # :293-301
            obs = sorted(mp["observations"].items())                                                     # std::map<KfId, KpId>
            slots = i32([slot_of[k] for k, _ in obs]); js = i32([j for _, j in obs])
            kp = st["kp"]
            pos, s, r, _ = TR.triangulate_point(st["table"]["pos"][row], False, slots, kp["x"][slots, js], kp["y"][slots, js], kp["octave"][slots, js],
                                                kp["depth"][slots, js], st["poses"], st["cams"], st["focal"], st["S"], mode)              # :308
            st["table"]["pos"][row] = pos
            st["mp_flags"][row] = TR.FLAG_OF_STATUS[s]
            status.append(s); reason.append(r)
            if s == TR.NOT_TRIANGULATED:                     # :309: the point is dropped, the row stays free
                continue
            cur["mapPoints"][kp1] = row; adj["mapPoints"][kp2] = row                                     # :310-311
            st["kf_mp"][current, kp1] = row; st["kf_mp"][adj_slot, kp2] = row
            st["mp_live"][row], st["n_obs"][row], st["mp_track"][row] = 1, 2, -1
            base = st["desc_base"][slots]                                                                # updateDescriptor, map_point.cpp:75-116
            d = st["pool"][(base + js)[base >= 0]]
            if len(d):
                st["table"]["desc"][row] = d[MR.medoid_of(d)]
            created.append((row, kp1, kp2))
        taken = {c[0] for c in created}
        free = [r for r in free if r not in taken]
        masks = {kf["slot"]: np.array([mp == -1 for mp in kf["mapPoints"]], np.uint8) for kf in keyframes}
        results.append(dict(slot=adj_slot, matched=matched, n_matches=len(pairs), match_kp1=i32([p[0] for p in pairs]), match_kp2=i32([p[1] for p in pairs]),
                            rows=i32(rows), status=np.array(status, np.uint8), reason=np.array(reason, np.uint8),
                            created_rows=i32([c[0] for c in created]), created_kp1=i32([c[1] for c in created]), created_kp2=i32([c[2] for c in created]),
                            masked=int(((would >= 0) & (matched < 0) & (usable1 == 0) & (initial1 == 1)).sum()), state=snapshot(st, masks)))
    return st, results


# ---------------------------------------------------------------------------------------------------- the staged restatement
def unbound_mask(kf_mp, n_mp, slot, n_kp):
    """ms_unbound_mask of one slot: 1 where the entry is not a row of the table."""
    e = kf_mp[slot, :n_kp].astype(np.int64)
    return (~((e >= 0) & (e < n_mp))).astype(np.uint8)


def lists_of(st, current, adj, matched, new_rows, n_mp=None, desc_base=None, n_levels=None, cap_rows=None, cap_obs=None):
    """ms_create_points_lists: (rc, n_matches, lists dict or None, match_kp1, match_kp2, violations)."""
    n_mp = len(st["mp_live"]) if n_mp is None else n_mp
    desc_base = st["desc_base"] if desc_base is None else desc_base
    n_levels = len(st["S"]["level_sigma_sq"]) if n_levels is None else n_levels
    n2 = int(st["n_kp"][adj])
    matched = np.asarray(matched, np.int32)
    v = dict(range=0, twice=0, bound=0, live=0, octave=0)
    pairs, named = [], set()
    for j, m in enumerate(matched):
        if m == -1:
            continue
        if not 0 <= m < n2:
            v["range"] += 1
            continue
        v["twice"] += int(m) in named
        named.add(int(m))
        v["bound"] += int(0 <= st["kf_mp"][current, j] < n_mp) + int(0 <= st["kf_mp"][adj, m] < n_mp)
        if n_levels > 0:
            v["octave"] += int(not 0 <= st["kp"]["octave"][current, j] < n_levels) + int(not 0 <= st["kp"]["octave"][adj, m] < n_levels)
        if len(pairs) < len(new_rows):
            v["live"] += bool(st["mp_live"][new_rows[len(pairs)]])
        pairs.append((j, int(m)))
    n = len(pairs)
    i32 = lambda a: np.array(a, np.int32)
    if any(v.values()):
        return INVALID, n, None, None, None, v
    cap_rows = n if cap_rows is None else cap_rows
    cap_obs = 2 * n if cap_obs is None else cap_obs
    if n > len(new_rows) or n > cap_rows or 2 * n > cap_obs:
        return CAPACITY, n, None, None, None, v
    cur_first = st["kf_id"][current] < st["kf_id"][adj]
    L = {k: [] for k in LISTS}
    for i, (j, m) in enumerate(pairs):
        L["rows"].append(new_rows[i]); L["obs_start"].append(2 * i); L["n_obs_row"].append(2); L["was_triangulated"].append(0)
        for s, p in (((current, j), (adj, m)) if cur_first else ((adj, m), (current, j))):
            L["obs_kf"].append(s); L["obs_kp"].append(p)
            for k in ("x", "y", "octave", "depth"):
                L["obs_" + k].append(st["kp"][k][s, p])
            L["obs_desc"].append(desc_base[s] + p if desc_base[s] >= 0 else -1)
        L["first_octave"].append(L["obs_octave"][2 * i])
    L["obs_start"].append(2 * n)
    dt = dict(was_triangulated=np.uint8, obs_x=F, obs_y=F, obs_depth=F)
    L = {k: np.array(a, dt.get(k, np.int32)) for k, a in L.items()}
    return 0, n, L, i32([p[0] for p in pairs]), i32([p[1] for p in pairs]), v


def triangulate_lists(st, L, mode):
    """ms_triangulate_lists on a state in place: mp_pos and mp_flags of the listed rows.  Returns (status, reason)."""
    prob = dict(rows=L["rows"], was_triangulated=L["was_triangulated"], obs_start=L["obs_start"], obs_kf=L["obs_kf"], obs_x=L["obs_x"], obs_y=L["obs_y"],
                obs_octave=L["obs_octave"], obs_depth=L["obs_depth"])
    pos, flags, status, reason, _ = TR.triangulate(st["table"]["pos"], st["mp_flags"], st["poses"], st["cams"], st["focal"], prob, st["S"], mode)
    st["table"]["pos"], st["mp_flags"] = pos, flags
    return status, reason


def bind(st, current, adj, L, match_kp1, match_kp2, masks, with_pool=True):
    """ms_create_points_bind on a state and the masks in place.  Returns (created_rows, created_kp1, created_kp2)."""
    created = []
    for i, row in enumerate(L["rows"]):
        if st["mp_flags"][row] == 0:
            continue
        kp1, kp2 = int(match_kp1[i]), int(match_kp2[i])
        st["kf_mp"][current, kp1] = row; st["kf_mp"][adj, kp2] = row
        st["mp_live"][row], st["n_obs"][row], st["mp_track"][row] = 1, 2, -1
        if with_pool:
            for d in L["obs_desc"][2 * i:2 * i + 2]:         # the FIRST observation with a descriptor
                if d != -1:
                    st["table"]["desc"][row] = st["pool"][d]
                    break
        if masks is not None:
            masks[current][kp1] = 0; masks[adj][kp2] = 0
        created.append((row, kp1, kp2))
    i32 = lambda a: np.array(a, np.int32)
    return i32([c[0] for c in created]), i32([c[1] for c in created]), i32([c[2] for c in created])


def staged(sc, current, adjacent, free_rows, mode=TR.TME):
    st = copy_state(sc)
    n_mp = len(st["mp_live"])
    masks = {s: unbound_mask(st["kf_mp"], n_mp, s, int(st["n_kp"][s])) for s in range(len(st["kf_id"]))}
    free = [int(r) for r in free_rows]
    results = []
    for adj in adjacent:
        if adj == current:
            results.append(None)
            continue
        matched = match(sc, current, adj, masks[current], masks[adj])
        rc, n, L, kp1, kp2, _ = lists_of(st, current, adj, matched, free)
        assert rc == 0
        status, reason = triangulate_lists(st, L, mode)
        rows, c1, c2 = bind(st, current, adj, L, kp1, kp2, masks)
        taken = set(rows.tolist())
        free = [r for r in free if r not in taken]
        results.append(dict(slot=adj, matched=matched, n_matches=n, match_kp1=kp1, match_kp2=kp2, rows=L["rows"], lists=L, status=status, reason=reason,
                            created_rows=rows, created_kp1=c1, created_kp2=c2, state=snapshot(st, masks)))
    return st, results


# ---------------------------------------------------------------------------------------------------- the scene
N_KF, STRIDE, N_MP, TRIP = 6, 320, 1024, 256
CURRENT = 2
ADJACENT = (3, 0, CURRENT, 5, 4)                             # four adjacents and the current slot itself once (:281)
KF_ID = (4, 2, 8, 12, 10, 6)                                 # not in slot order; slots 3 and 4 are younger than the current keyframe
N_KP = (200, 100, 300, 280, 150, 320)
EMPTY_SLOT = 4                                               # shares no vocabulary node with the current keyframe
N_EXISTING = 30
# kind -> (how many, depth range, the slots that see it besides the current one)
KINDS = dict(near_3=(20, (2.0, 4.5), (3,)), near_0=(15, (2.0, 8.0), (0,)), near_5=(15, (2.0, 12.0), (5,)), far=(10, (60.0, 100.0), (3, 0, 5)),
             mid=(10, (7.0, 9.0), (3, 0)), twice=(10, (2.0, 4.5), (3, 5)), off_line=(10, (2.0, 4.5), (3,)), flipped=(10, (2.0, 3.0), (3,)),
             with_depth=(10, (2.0, 8.0), (0,)), existing=(N_EXISTING, (2.0, 8.0), (3, 0)))


def make_scene(seed=5):
    """Six keyframes of the corridor of triangulate_ref.make_keyframes (0.1 apart along x), stride 320, 1024 rows; the current keyframe in
    slot 2 with 300 keypoints.  True 3-D points are projected into the keyframes that see them; the observations of a point share a
    vocabulary node and carry its descriptor with up to 8 flipped bits (every other pair of descriptors is about 128 bits apart), so the
    matcher pairs exactly them.  Kinds of points, by depth and by who sees them:
      near_3 / near_0 / near_5   close enough for the two-observation angle against that adjacent                     -> created
      far           seen by three adjacents, too far for any baseline                                                 -> angle failure, three times
      mid           too far for slot 3 (baseline 0.1), close enough for slot 0 (0.2)                                  -> fails, then created
      twice         seen by slots 3 and 5                                                                             -> created against 3, masked against 5
      off_line      the adjacent keypoint 8 px off the epipolar line at octave 0 (inside the matcher's 2 degrees)     -> reprojection failure
      flipped       the adjacent keypoint sees the point mirrored through the current camera centre                   -> negative depth
      with_depth    the current keypoint carries a keyPointDepth                                                      -> the depth branch of :621
      existing      map points of rows [0, 30), bound in slots 2, 3 and 0                                             -> masked from the start
    Slot 4's keypoints lie in vocabulary nodes of their own: no match.  Slot 1 is a bystander."""
    rng = np.random.default_rng(seed)
    poses, cams, focal = TR.make_keyframes(rng, N_KF, special=False)
    kf_id, n_kp = np.array(KF_ID, np.int32), np.array(N_KP, np.int32)
    kp = dict(x=(rng.random((N_KF, STRIDE)) * 640).astype(F), y=(rng.random((N_KF, STRIDE)) * 480).astype(F),
              octave=rng.integers(0, 8, (N_KF, STRIDE)).astype(np.int32), depth=np.full((N_KF, STRIDE), -1.0, F))
    angle = (rng.random((N_KF, STRIDE)) * 360).astype(F)
    node = rng.integers(100, 140, (N_KF, STRIDE)).astype(np.int32)
    node[EMPTY_SLOT] += 100
    desc_base = (rng.permutation(N_KF) * STRIDE).astype(np.int32)
    pool = rng.integers(0, 2 ** 32, (N_KF * STRIDE, 8), dtype=np.uint64).astype(np.uint32)
    kf_mp = np.full((N_KF, STRIDE), -1, np.int32)
    table = dict(pos=rng.uniform(-50, 50, (N_MP, 3)), norm=rng.normal(0, 1, (N_MP, 3)).astype(F), min_dist=rng.uniform(0.5, 1, N_MP).astype(F),
                 max_dist=rng.uniform(20, 30, N_MP).astype(F), desc=rng.integers(0, 2 ** 32, (N_MP, 8), dtype=np.uint64).astype(np.uint32))
    mp_flags, mp_live = np.zeros(N_MP, np.uint8), np.zeros(N_MP, np.uint8)
    mp_live[:120] = 1; mp_flags[:120] = rng.choice([0, 2, 3, 3], 120)
    mp_flags[:N_EXISTING] = 3
    n_obs = rng.integers(0, 9, N_MP).astype(np.int32)
    mp_track = rng.integers(-1, 5000, N_MP).astype(np.int32)
    order = {s: iter(rng.permutation(N_KP[s]).tolist()) for s in range(N_KF)}      # the keypoints of a slot are dealt in a shuffled order
    Pc = poses[CURRENT].reshape(3, 4)
    centre = np.asarray(MR.pose_centre(poses[CURRENT]), np.float64)
    kind_of, point = {}, 0
    for kind, (count, (z0, z1), seen) in KINDS.items():
        for _ in range(count):
            zc = rng.uniform(z0, z1)
            X = Pc[:, :3].T @ (np.array([rng.uniform(-0.2, 0.2) * zc, rng.uniform(-0.15, 0.15) * zc, zc]) - Pc[:, 3])
            d0 = rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)
            a0, octave = rng.random() * 360, int(rng.integers(0, 8))
            for s in (CURRENT,) + seen:
                j = next(order[s])
                u, v, rng_depth = TR.project(poses, cams, s, X)
                kp["x"][s, j], kp["y"][s, j] = u + rng.normal(0, 0.02), v + rng.normal(0, 0.02)
                kp["octave"][s, j] = 0 if kind == "off_line" else octave
                angle[s, j] = a0 + rng.normal(0, 0.5)
                node[s, j] = point % 16
                d = d0.copy()
                for b in rng.integers(0, 256, int(rng.integers(0, 9))):
                    d[b // 32] ^= np.uint32(1) << np.uint32(b % 32)
                pool[desc_base[s] + j] = d
                if s == CURRENT:
                    kind_of[int(j)] = kind
                    if kind == "with_depth":
                        kp["depth"][s, j] = rng_depth * (1.0 + rng.normal(0, 1e-3))
                elif kind == "off_line":
                    kp["y"][s, j] += F(8.0)
                elif kind == "flipped":              # the pixel of the point mirrored through the current camera centre: the rays meet behind both cameras
                    kp["x"][s, j], kp["y"][s, j], _ = TR.project(poses, cams, s, 2.0 * centre - X)
                if kind == "existing":
                    kf_mp[s, j] = point - sum(c for k, (c, _, _) in KINDS.items() if k != "existing")
                    table["pos"][kf_mp[s, j]] = X
            point += 1
    free = np.flatnonzero(mp_live == 0)
    free_rows = rng.permutation(free[free >= 200])[:260].astype(np.int32)       # more than any adjacent matches, in no order
    return dict(kf_mp=kf_mp, kf_id=kf_id, n_kp=n_kp, poses=poses, cams=cams, focal=focal, kp=kp, angle=angle, node=node, desc_base=desc_base, pool=pool, table=table,
                mp_flags=mp_flags, mp_live=mp_live, n_obs=n_obs, mp_track=mp_track, S=TR.settings(), sf=MR.scale_factors(), thr_deg=2.0, kind_of=kind_of), free_rows


def case_counts(sc, results):
    """How often the sequential restatement reached each case the tests rely on."""
    done = [r for r in results if r is not None]
    failed_kp, created_kp = set(), set()
    fails_then_created = 0
    for r in done:
        ok = r["status"] != TR.NOT_TRIANGULATED
        fails_then_created += len(failed_kp & set(r["match_kp1"][ok].tolist()))
        failed_kp |= set(r["match_kp1"][~ok].tolist())
        created_kp |= set(r["created_kp1"].tolist())
    reasons = np.concatenate([r["reason"] for r in done])
    depth_branch = sum(int((sc["kp"]["depth"][CURRENT, r["match_kp1"]] > 0).sum()) for r in done)
    return dict(created=sum(len(r["created_rows"]) for r in done), angle=int((reasons == TR.R_ANGLE).sum()),
                depth_or_reprojection=int(((reasons == TR.R_DEPTH) | (reasons == TR.R_REPROJECTION)).sum()), negative_depth=int((reasons == TR.R_DEPTH).sum()),
                reprojection=int((reasons == TR.R_REPROJECTION).sum()), depth_branch=depth_branch, fails_then_created=fails_then_created,
                masked_later=sum(r["masked"] for r in done), empty_adjacent=sum(r["n_matches"] == 0 for r in done),
                second_trip=sum(int((r["match_kp1"] >= TRIP).sum()) for r in done), flipped_order=sum(len(r["created_rows"]) for r in done if KF_ID[r["slot"]] > KF_ID[CURRENT]),
                skipped=sum(r is None for r in results))


_CACHE = {}


def fixture():
    """(scene, free_rows, sequential state, sequential results, case counts), computed once.  Every case is a condition of the fixture: a
    test that could skip one would hide it."""
    if "fixture" not in _CACHE:
        sc, free_rows = make_scene()
        st, results = sequential(sc, CURRENT, ADJACENT, free_rows)
        counts = case_counts(sc, results)
        assert all(counts[k] > 0 for k in ("created", "angle", "depth_or_reprojection", "depth_branch", "fails_then_created", "masked_later", "empty_adjacent", "second_trip",
                                           "flipped_order")) and counts["skipped"] == 1, counts
        _CACHE["fixture"] = (sc, free_rows, st, results, counts)
    return _CACHE["fixture"]
