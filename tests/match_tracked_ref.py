"""The specification of ms_match_tracked and ms_match_tracked_finish: matchTrackedFeatures (mapper_helpers.cpp:67-142) restated
over the device map tables, one keypoint after the other in the reference's order, with keyPointToTrackId and trackIdToMapPoint as dicts.

The gates, the FIRST_LAST triangulation, the refresh and the medoid are the restatements the repository already has: project_gate_ref.gate_view
(mode SEARCH = Keyframe::isInFrustum), triangulate_ref.check_reprojection / triangulate_point, map_refresh_ref.refresh / medoid_of.

Two forms, which tests/test_match_tracked_ref.py holds equal on every scene:
  sequential()   the function as the reference runs it: walk, triangulate, update, keypoint by keypoint
  walk() -> triangulate_tracked() -> finish()   the stages of the device chain (ms_match_tracked | ms_observation_lists + ms_triangulate_lists |
                 ms_match_tracked_finish + the refresh).  They are equal because every tracked keypoint resolves to its own map point
                 (MapPoint::addObservation asserts it, map_point.cpp:66): no step of one keypoint reads what another keypoint's step wrote.

A state is a dict: kf_mp [n_kf, stride], kf_id, poses [n_kf, 12], cams [n_kf, 6], focal, kp (x, y, octave, depth, each [n_kf, stride]), desc_base
[n_kf], pool [n_pool, 8], table (pos, norm, min_dist, max_dist, desc), mp_flags, mp_live, mp_track [n_mp], track_row [n_track], track_base, S
(triangulate_ref.settings), sf (scale factors), view_cos_limit.  A frame is a dict: slot, kp_track [n_kp] (-1 for none)."""
import numpy as np

import map_refresh_ref as MR
import project_gate_ref as PG
import triangulate_ref as TR

F = np.float32
NO_TRACK, CREATED, TRACKED, CHECKED, FRUSTUM, REPROJECTION, NO_DESCRIPTORS = range(7)
INVALID, CAPACITY = -1, -4                                   # MS_ERR_INVALID, MS_ERR_CAPACITY
TABLES = ("kf_mp", "mp_flags", "mp_live", "mp_track", "track_row")
FIELDS = ("pos", "norm", "min_dist", "max_dist", "desc")


def copy_state(sc):
    st = dict(sc)
    for k in TABLES:
        st[k] = np.array(sc[k], copy=True)
    st["table"] = {k: np.array(v, copy=True) for k, v in sc["table"].items()}
    return st


def presence(sc, t):
    """(row, reason): reason 0 present | 1 no entry | 2 entry outside the table | 3 mp_live == 0 | 4 mp_track differs.  A culled or recycled row counts as
    erased (mapdb.cpp:166-173)."""
    i = t - sc["track_base"]
    r = int(sc["track_row"][i])
    if r == -1:
        return -1, 1
    if not 0 <= r < len(sc["mp_live"]):
        return -1, 2
    if not sc["mp_live"][r]:
        return -1, 3
    if sc["mp_track"][r] != t:
        return -1, 4
    return r, 0


def observations(st, r):
    """MapPoint::observations of row r: (slots, js) in ascending KfId (then j), the slots with kf_id >= 0 only."""
    slots, js = np.nonzero(st["kf_mp"] == r)
    keep = st["kf_id"][slots] >= 0
    slots, js = slots[keep], js[keep]
    order = np.lexsort((js, st["kf_id"][slots]))
    return slots[order], js[order]


def in_frustum(st, slot, r):
    """Keyframe::isInFrustum (keyframe.cpp:247-262) = the SEARCH gates, statuses 1, 2 and 4."""
    P = st["poses"][slot].reshape(3, 4)
    view = dict(R=P[:, :3], t=P[:, 3], cam=tuple(st["cams"][slot]), threshold=0.0, view_cos_limit=st["view_cos_limit"], mode=PG.SEARCH, indices=np.array([r], np.int32))
    status = int(PG.gate_view(st["table"], view, st["sf"], 1.2)["status"][0])
    assert status in (PG.KEPT, PG.NOT_VISIBLE, PG.DISTANCE, PG.ANGLE)
    return status == PG.KEPT


def reprojection_ok(st, slot, j, r):
    x, y = st["kp"]["x"][slot, j], st["kp"]["y"][slot, j]
    with np.errstate(all="ignore"):
        o = TR.observe(st["poses"], st["cams"], [slot], [x], [y])
        return TR.check_reprojection(o, 0, [TR.D(v) for v in st["table"]["pos"][r]], x, y, int(st["kp"]["octave"][slot, j]), st["focal"][slot], st["S"])


def triangulate_first_last(st, r):
    """triangulateMapPointFirstLastObs (:724-810) of row r from the table as it is; returns the status."""
    slots, js = observations(st, r)
    kp = st["kp"]
    pos, status, _, _ = TR.triangulate_point(st["table"]["pos"][r], bool(st["mp_flags"][r] & 2), slots, kp["x"][slots, js], kp["y"][slots, js], kp["octave"][slots, js],
                                             kp["depth"][slots, js], st["poses"], st["cams"], st["focal"], st["S"], TR.FIRST_LAST)
    st["table"]["pos"][r] = pos
    st["mp_flags"][r] = TR.FLAG_OF_STATUS[status]
    return status


def descriptors_of(st, r):
    slots, js = observations(st, r)
    base = st["desc_base"][slots]
    have = base >= 0
    return st["pool"][(base + js)[have]]


def update_descriptor(st, r):
    """MapPoint::updateDescriptor (map_point.cpp:76-115): the general medoid."""
    d = descriptors_of(st, r)
    if len(d):
        st["table"]["desc"][r] = d[MR.medoid_of(d)]


def update_descriptor_two_observations(st, r):
    """What ms_match_tracked_finish does for an UNSURE row: the first descriptor.  n = 2: index (unsigned)(0.5 * (n - 1)) = 0 of each sorted
    row of distances is the distance to itself, 0; `<` keeps the first.  Asserted against the general rule on every call."""
    d = descriptors_of(st, r)
    if len(d):
        assert len(d) <= 2 and MR.medoid_of(d) == 0
        st["table"]["desc"][r] = d[0]


def update_distance_and_norm(st, r):
    slots, js = observations(st, r)
    prob = dict(rows=np.array([r]), obs_start=np.array([0, len(slots)]), obs_kf=slots, first_octave=np.array([st["kp"]["octave"][slots[0], js[0]]]))
    out, _ = MR.refresh(st["table"], st["poses"], None, prob, st["sf"])
    for k in ("norm", "min_dist", "max_dist"):
        st["table"][k][r] = out[k][r]


def _walk(sc, frame, new_rows, whole):
    """The loop of :76-141.  whole = False leaves out everything behind the binding (:90, :121-124): the tables as ms_match_tracked leaves them."""
    st = copy_state(sc)
    slot, kp_track = int(frame["slot"]), np.asarray(frame["kp_track"], np.int32)
    has_desc = st["desc_base"][slot] >= 0
    n_mp, n_levels = len(st["mp_live"]), len(st["S"]["level_sigma_sq"])
    key_point_to_track = {v: int(t) for v, t in enumerate(kp_track) if t >= 0}
    track_to_map_point = {}                                  # mapDB.trackIdToMapPoint, as the tables hold it
    for t in key_point_to_track.values():
        r, reason = presence(sc, t)
        if not reason:
            track_to_map_point[t] = r
    outcome = np.zeros(len(kp_track), np.uint8)
    created_rows, created_kp, tracked, checked, unsure = [], [], [], [], []
    violations = dict(bound=0, live=0, octave=0)
    for v in range(len(kp_track)):
        if v not in key_point_to_track:
            continue
        t = key_point_to_track[v]
        octave_ok = 0 <= st["kp"]["octave"][slot, v] < n_levels
        violations["octave"] += not octave_ok
        if t in track_to_map_point:
            r = track_to_map_point[t]
            if (sc["mp_flags"][r] & 1) == 0:                 # :85
                outcome[v] = TRACKED
                tracked.append(r)
                violations["bound"] += 0 <= sc["kf_mp"][slot, v] < n_mp
                st["kf_mp"][slot, v] = r
                if whole and triangulate_first_last(st, r) != TR.NOT_TRIANGULATED:
                    update_descriptor(st, r)                 # :811
            else:
                if not octave_ok:
                    outcome[v] = REPROJECTION
                    continue
                if not in_frustum(st, slot, r):
                    outcome[v] = FRUSTUM
                    continue
                if not reprojection_ok(st, slot, v, r):
                    outcome[v] = REPROJECTION
                    continue
                outcome[v] = CHECKED
                checked.append(r)
                violations["bound"] += 0 <= sc["kf_mp"][slot, v] < n_mp
                st["kf_mp"][slot, v] = r
            if whole and (st["mp_flags"][r] & 1):            # :121
                if has_desc:
                    update_descriptor(st, r)
                update_distance_and_norm(st, r)
        elif has_desc:                                       # :126-139
            outcome[v] = CREATED
            violations["bound"] += 0 <= sc["kf_mp"][slot, v] < n_mp
            k = len(created_kp)
            created_kp.append(v)
            if k < len(new_rows):
                r = int(new_rows[k])
                created_rows.append(r)
                violations["live"] += bool(sc["mp_live"][r])
                st["kf_mp"][slot, v] = r
                st["mp_live"][r], st["mp_flags"][r], st["mp_track"][r] = 1, 0, t
                st["track_row"][t - st["track_base"]] = r
                st["table"]["desc"][r] = st["pool"][st["desc_base"][slot] + v]
        else:
            outcome[v] = NO_DESCRIPTORS
    counts = [len(created_kp), len(tracked), len(checked), int((outcome == FRUSTUM).sum()), int((outcome == REPROJECTION).sum())]
    rc = 0
    if any(violations.values()):
        rc = INVALID
    elif len(created_kp) > len(new_rows):
        rc = CAPACITY
    if rc:
        st = copy_state(sc)                                  # nothing but `outcome` is written
    i32 = lambda a: np.array(a, np.int32)
    return dict(rc=rc, state=st, outcome=outcome, created_rows=i32(created_rows), created_kp=i32(created_kp), tracked_rows=i32(tracked), checked_rows=i32(checked),
                counts=counts, violations=violations, has_desc=bool(has_desc))


def sequential(sc, frame, new_rows):
    return _walk(sc, frame, new_rows, True)


def walk(sc, frame, new_rows):
    return _walk(sc, frame, new_rows, False)


def triangulate_tracked(st, tracked_rows):
    """Stage 2 on a state in place: FIRST_LAST for the just-tracked rows (each from its own observations).  Returns the statuses."""
    return np.array([triangulate_first_last(st, int(r)) for r in tracked_rows], np.uint8)


def finish(st, tracked_rows, checked_rows, has_desc):
    """Stage 3 on a state in place: the two-observation descriptor rule for the UNSURE rows, then the refresh of :121-124 -- one pass over the
    tracked-and-TRIANGULATED rows followed by the checked rows when the frame has descriptors; otherwise the tracked ones with the descriptor
    half (the updateDescriptor of :811) and the checked ones without.  Returns refresh_rows as ms_match_tracked_finish packs them."""
    for r in tracked_rows:
        if st["mp_flags"][r] == 2:
            update_descriptor_two_observations(st, int(r))
    promoted = [int(r) for r in tracked_rows if st["mp_flags"][r] & 1]
    for r in promoted:
        update_descriptor(st, r)
        update_distance_and_norm(st, r)
    for r in checked_rows:
        if has_desc:
            update_descriptor(st, int(r))
        update_distance_and_norm(st, int(r))
    return np.array(promoted + ([int(r) for r in checked_rows] if has_desc else []), np.int32)


def staged(sc, frame, new_rows):
    w = walk(sc, frame, new_rows)
    if w["rc"]:
        return w
    w["status"] = triangulate_tracked(w["state"], w["tracked_rows"])
    w["refresh_rows"] = finish(w["state"], w["tracked_rows"], w["checked_rows"], w["has_desc"])
    return w


def same_state(a, b):
    """Every table of two states bit for bit."""
    bits = lambda v: np.ascontiguousarray(v).view(np.uint8)
    return all(np.array_equal(a[k], b[k]) for k in TABLES) and all(np.array_equal(bits(a["table"][k]), bits(b["table"][k])) for k in FIELDS)


# ---------------------------------------------------------------------------------------------------- the scene
N_KF, STRIDE, N_MP, N_KP, N_TRACK, TRACK_BASE = 12, 640, 2000, 600, 1400, 1000
CURRENT = N_KF - 1
NO_DESC_SLOT = 3                                             # an older keyframe without descriptors
TRIP = 256
# the kinds of tracked keypoints and how many the current frame has of each
KINDS = dict(checked=70, behind=10, too_far=10, turned_away=10, off_pixel=30, two_obs=40, two_obs_off=10, many_obs=40, many_obs_off=10, far_point=10, with_depth=10,
             absent=40, culled=10, recycled=10, out_of_table=4)


def make_scene(seed=11, n_kp=N_KP, stride=STRIDE, n_mp=N_MP, n_track=N_TRACK, filled=1500, scale=1):
    """12 keyframes in a corridor (triangulate_ref.make_keyframes), stride 640, 2000 rows of which the first ~1500 hold map points, the
    current frame in slot 11 with 600 keypoints, 314 of them tracked, of every kind of KINDS:
      checked       a TRIANGULATED point whose keypoint lies on its projection                                   -> 3
      behind / too_far / turned_away   a TRIANGULATED point behind the camera, beyond maxViewingDistance, with its normal turned away -> 4
      off_pixel     a TRIANGULATED point whose keypoint lies 25 px off                                           -> 5
      two_obs / many_obs   a point that is not TRIANGULATED, seen by one / by two to five older keyframes          -> 2, then UNSURE / TRIANGULATED
      *_off, far_point     the same with the current keypoint 25 px off the epipolar line, or 400 times as far away -> 2, then NOT_TRIANGULATED (mostly)
      with_depth    a just-tracked point whose current keypoint carries a depth                                  -> 2
      absent        track_row holds -1                                                                           -> 1 (6 without descriptors)
      culled        track_row names a row with mp_live == 0 that still carries the track id (ms_map_cull)        -> 1 / 6
      recycled      track_row names a live row that belongs to another track now                                 -> 1 / 6
      out_of_table  track_row holds n_mp, n_mp + 1, INT32_MIN, -2                                                -> 1 / 6
    The kinds are dealt to the keypoints in a shuffled order.  kf_id is not monotone in the slot; slot 3 has no descriptors.
    The arguments make the same scene at another size (tools/match_tracked_probe.py): `scale` times as many keypoints of every kind among
    n_kp, rows [0, filled) of n_mp holding map points."""
    rng = np.random.default_rng(seed)
    poses, cams, focal = TR.make_keyframes(rng, N_KF, special=False)
    kf_id = (2 * np.arange(N_KF) + 1).astype(np.int32)
    kf_id[2], kf_id[6] = kf_id[6], kf_id[2]
    kp = dict(x=(rng.random((N_KF, stride)) * 640).astype(F), y=(rng.random((N_KF, stride)) * 480).astype(F),
              octave=rng.integers(0, 8, (N_KF, stride)).astype(np.int32), depth=np.full((N_KF, stride), -1.0, F))
    desc_base = (rng.permutation(N_KF) * stride).astype(np.int32)
    desc_base[NO_DESC_SLOT] = -1
    pool = rng.integers(0, 2 ** 32, (N_KF * stride, 8), dtype=np.uint64).astype(np.uint32)
    kf_mp = np.full((N_KF, stride), -1, np.int32)
    used = np.zeros(N_KF, np.int64)                          # keypoints handed out per older slot
    table = dict(pos=rng.uniform(-50, 50, (n_mp, 3)), norm=np.zeros((n_mp, 3), F), min_dist=np.zeros(n_mp, F), max_dist=np.zeros(n_mp, F),
                 desc=rng.integers(0, 2 ** 32, (n_mp, 8), dtype=np.uint64).astype(np.uint32))
    mp_flags, mp_live = np.zeros(n_mp, np.uint8), np.zeros(n_mp, np.uint8)
    mp_track = np.full(n_mp, -1, np.int32)
    track_row = np.full(n_track, -1, np.int32)
    centre = np.array([MR.pose_centre(P) for P in poses])
    ids = iter((TRACK_BASE + rng.permutation(n_track)).tolist())
    Pc = poses[CURRENT].reshape(3, 4)

    def new_point(r, n_prev, flags, far=False):
        """A live row r in front of the current camera, seen by n_prev older keyframes at its projections; returns its position."""
        zc = rng.uniform(3.0, 10.0) * (400.0 if far else 1.0)
        X = Pc[:, :3].T @ (np.array([rng.uniform(-0.25, 0.25) * zc, rng.uniform(-0.18, 0.18) * zc, zc]) - Pc[:, 3])
        for k in np.sort(rng.choice(CURRENT, n_prev, replace=False)):
            j = used[k]; used[k] += 1
            u, v, _ = TR.project(poses, cams, k, X)
            kp["x"][k, j], kp["y"][k, j] = u + rng.normal(0, 0.02), v + rng.normal(0, 0.02)
            kf_mp[k, j] = r
        d = np.linalg.norm(centre[CURRENT] - X)
        table["pos"][r] = X
        table["norm"][r] = ((centre[CURRENT] - X) / d + rng.normal(0, 0.05, 3)).astype(F)
        table["min_dist"][r], table["max_dist"][r] = d / 3.0, d * 1.5
        mp_flags[r], mp_live[r] = flags, 1
        return X

    kinds = [k for k, n in KINDS.items() for _ in range(scale * n)]
    slots_j = rng.permutation(n_kp)[:len(kinds)]             # the keypoints that carry a track, in a shuffled order
    kp_track = np.full(n_kp, -1, np.int32)
    kind_of = {}
    r = 0
    for kind, j in zip(kinds, slots_j):
        t = next(ids)
        kp_track[j] = t
        kind_of[int(j)] = kind
        if kind == "absent":
            continue
        if kind == "out_of_table":
            track_row[t - TRACK_BASE] = (n_mp, n_mp + 1, -2 ** 31, -2)[j % 4]
            continue
        triangulated = kind in ("checked", "behind", "too_far", "turned_away", "off_pixel", "culled", "recycled")
        n_prev = 1 if kind.startswith("two_obs") else int(rng.integers(2, 6))
        X = new_point(r, n_prev, 3 if triangulated else (2 if n_prev > 1 and rng.random() < 0.5 else 0), far=kind == "far_point")
        mp_track[r] = t
        track_row[t - TRACK_BASE] = r
        u, v, rng_depth = TR.project(poses, cams, CURRENT, X)
        kp["x"][CURRENT, j], kp["y"][CURRENT, j] = u + rng.normal(0, 0.02), v + rng.normal(0, 0.02)
        if kind == "behind":
            table["pos"][r] = centre[CURRENT] - (X - centre[CURRENT])
        elif kind == "too_far":
            table["max_dist"][r] = table["min_dist"][r] * 1.01
        elif kind == "turned_away":
            table["norm"][r] = -table["norm"][r]
        elif kind in ("off_pixel", "two_obs_off", "many_obs_off"):
            kp["y"][CURRENT, j] += F(25.0)
        elif kind == "with_depth":
            kp["depth"][CURRENT, j] = rng_depth * (1.0 + rng.normal(0, 1e-3))
        elif kind == "culled":
            mp_live[r] = 0
        elif kind == "recycled":
            mp_track[r] = next(ids)
        r += 1
    while r < filled:                                          # the rest of the map: points of other tracks, not in this frame
        new_point(r, int(rng.integers(1, 6)), int(rng.choice([0, 2, 3, 3])))
        mp_track[r] = next(ids) if rng.random() < 0.7 else -1
        if mp_track[r] >= 0:
            track_row[mp_track[r] - TRACK_BASE] = r
        r += 1
    assert used.max() <= stride
    free = np.flatnonzero(mp_live == 0)
    new_rows = rng.permutation(free[free >= filled])[:80 * scale].astype(np.int32)          # more than the frame creates, in no order
    sc = dict(kf_mp=kf_mp, kf_id=kf_id, poses=poses, cams=cams, focal=focal, kp=kp, desc_base=desc_base, pool=pool, table=table, mp_flags=mp_flags, mp_live=mp_live,
              mp_track=mp_track, track_row=track_row, track_base=TRACK_BASE, S=TR.settings(), sf=MR.scale_factors(), view_cos_limit=0.5, kind_of=kind_of)
    return sc, dict(slot=CURRENT, kp_track=kp_track), new_rows


def without_descriptors(sc):
    """The scene with a current frame for which hasFeatureDescriptors() is false."""
    out = dict(sc, desc_base=sc["desc_base"].copy())
    out["desc_base"][CURRENT] = -1
    return out


def first_trip_empty(frame):
    """The frame with no tracked keypoint among its first 256."""
    t = frame["kp_track"].copy()
    t[:TRIP] = -1
    return dict(frame, kp_track=t)


_CACHE = {}


def fixture(name):
    """The scenes of the tests and their expected results, computed once: 'desc', 'no_desc', 'empty_trip' -> (scene, frame, new_rows, staged result)."""
    if not _CACHE:
        sc, frame, new_rows = make_scene()
        for key, s, f in (("desc", sc, frame), ("no_desc", without_descriptors(sc), frame), ("empty_trip", sc, first_trip_empty(frame))):
            _CACHE[key] = (s, f, new_rows, staged(s, f, new_rows))
    return _CACHE[name]
