"""The specification of ms_observation_count and ms_map_cull, restated in numpy: the transpose of the keyframe table kf_mp
[n_kf, stride] (slot -> map-point rows, Keyframe::mapPoints) and the two culling passes of addKeyframeCommonInner on it (cullMapPoints,
mapper_helpers.cpp:349-373; cullKeyframes, :433-482).  Integer work plus one float64 subtraction; the device results equal these bit for bit.

An entry r is valid iff 0 <= r < n_mp.  mp_flags [n_mp] uint8, bit 0 = TRIANGULATED; mp_live [n_mp] uint8, non-zero = the row holds a map
point; kf_id [n_kf] int32, -1 for an empty slot; kf_t [n_kf] float64.  tests/test_map_cull_ref.py holds these functions against a
sequential dictionary model written the way the reference writes its loops."""
import numpy as np

NONE = -1
EMPTY, AGED, ORPHANED = 1, 2, 3                              # removed_why


def valid(kf_mp, n_mp):
    a = np.asarray(kf_mp, np.int64)
    return (a >= 0) & (a < n_mp)


def observation_count(kf_mp, n_mp, kf_id):
    """n_obs [n_mp] (valid entries equal to the row over the slots with kf_id >= 0, with multiplicity), first_slot / last_slot [n_mp] (the
    slot with the smallest / largest kf_id among those that list the row, -1 for none)."""
    kf_mp = np.asarray(kf_mp, np.int32)
    kf_id = np.asarray(kf_id, np.int32)
    n_obs = np.zeros(n_mp, np.int32)
    first, last = np.full(n_mp, NONE, np.int32), np.full(n_mp, NONE, np.int32)
    order = [k for k in np.argsort(kf_id, kind="stable") if kf_id[k] >= 0]
    for k in order:                                          # ascending id: the last writer is the largest
        r = kf_mp[k][valid(kf_mp[k], n_mp)]
        np.add.at(n_obs, r, 1)
        last[r] = k
    for k in order[::-1]:
        first[kf_mp[k][valid(kf_mp[k], n_mp)]] = k
    return n_obs, first, last


def settings(current_slot, cull_points=1, min_age=0.0, min_obs_for_ba=2, max_critical_ratio=0.5, ratio_float32=0):
    return dict(current_slot=int(current_slot), cull_points=int(cull_points), min_age=float(min_age), min_obs_for_ba=int(min_obs_for_ba),
                max_critical_ratio=float(max_critical_ratio), ratio_float32=int(ratio_float32))


def ratio_test(n_critical, n_map_points, ratio, ratio_float32):
    """nCritical < nMapPoints * keyframeCullMaxCriticalRatio (:476) in the parameter's type."""
    if ratio_float32:
        return bool(np.float32(n_critical) < np.float32(n_map_points) * np.float32(ratio))
    return bool(np.float64(n_critical) < np.float64(n_map_points) * np.float64(ratio))


def age_of(kf_t, current_slot, first_slot):
    """const int obsAge = currentKeyframe.t - first.t: the float64 difference truncated toward zero."""
    return int(np.trunc(np.float64(kf_t[current_slot]) - np.float64(kf_t[first_slot])))


def map_cull(kf_mp, mp_flags, mp_live, n_mp, kf_id, kf_t, cand, cand_keep, s):
    """Returns a dict: kf_mp, mp_flags (None when none were given), mp_live, n_obs after both passes, removed_rows (ascending) and removed_why,
    cand_removed [n_cand] in the caller's order, n_removed_kf, and `trace`: per walked candidate (slot, nMapPoints, nCritical, removed)."""
    kf_mp = np.array(kf_mp, np.int32)
    kf_id = np.asarray(kf_id, np.int32)
    kf_t = np.asarray(kf_t, np.float64)
    flags = None if mp_flags is None else np.array(mp_flags, np.uint8)
    live = np.array(mp_live, np.uint8)
    cand = [int(c) for c in cand]
    keep = [0] * len(cand) if cand_keep is None else [int(x) for x in cand_keep]
    cur = s["current_slot"]
    n_obs, first, _ = observation_count(kf_mp, n_mp, kf_id)
    why = np.zeros(n_mp, np.uint8)
    if s["cull_points"]:
        in_cur = np.zeros(n_mp, bool)
        in_cur[kf_mp[cur][valid(kf_mp[cur], n_mp)]] = True
        for r in range(n_mp):
            if not live[r]:
                continue
            if n_obs[r] == 0:
                why[r] = EMPTY
            elif not in_cur[r] and float(age_of(kf_t, cur, first[r])) > s["min_age"] and (flags[r] & 1) == 0:
                why[r] = AGED
    gone = why != 0
    ok = valid(kf_mp, n_mp)
    kf_mp[ok & np.append(gone, False)[np.where(ok, kf_mp, n_mp)]] = NONE
    n_obs[gone] = 0
    cand_removed = np.zeros(len(cand), np.uint8)
    trace = []
    for i in sorted((i for i in range(len(cand)) if not keep[i]), key=lambda i: -int(kf_id[cand[i]])):
        k = cand[i]
        rows = kf_mp[k][valid(kf_mp[k], n_mp)]
        n_map_points, n_critical = len(rows), int((n_obs[rows] <= s["min_obs_for_ba"]).sum())
        remove = ratio_test(n_critical, n_map_points, s["max_critical_ratio"], s["ratio_float32"])
        trace.append((k, n_map_points, n_critical, remove))
        if not remove:
            continue
        np.subtract.at(n_obs, rows, 1)
        orphan = np.unique(rows[(n_obs[rows] == 0) & (live[rows] != 0)])
        why[orphan] = ORPHANED
        kf_mp[k] = NONE
        cand_removed[i] = 1
        # an orphan has no entry left in a slot with kf_id >= 0; an entry in an empty slot goes as well (every entry equal to the row)
        ok = valid(kf_mp, n_mp)
        kf_mp[ok & np.isin(kf_mp, orphan)] = NONE
    gone = why != 0
    live[gone] = 0
    if flags is not None:
        flags[gone] = 0
    rows = np.nonzero(gone)[0].astype(np.int32)
    return dict(kf_mp=kf_mp, mp_flags=flags, mp_live=live, n_obs=n_obs, removed_rows=rows, removed_why=why[rows], cand_removed=cand_removed,
                n_removed_kf=int(cand_removed.sum()), trace=trace)


N_KF, STRIDE, N_MP = 70, 100, 1003
CURRENT = 69


def make_scene(seed=11, n_kf=N_KF, stride=STRIDE, n_mp=N_MP):
    """A seeded map in the sizes of covis_ref.make_scene.  Slot k holds KfId 3 * k + 1 at t = k seconds, except slot 13 (empty: kf_id -1, all
    -1 but two stale entries) and slot 5, which holds the OLDEST KfId 0 (so the order of ids is not the order of slots; slots 45 and 60 have their ids exchanged).  Rows are observed
    by runs of consecutive slots (rows 900 .. 924 also by an old slot and the current one); rows 950 .. 989 have no observation at all, rows 990 .. 1002 are free (not live).  Slot 20 carries the
    out-of-range entries n_mp, n_mp + 1.  Returns a dict of the inputs of map_cull (cand: 20 candidate slots in shuffled order)."""
    rng = np.random.default_rng(seed)
    lists = [[] for _ in range(n_kf)]
    for r in range(950):
        n = int(rng.choice([1, 1, 2, 3, 4, 6, 8]))
        k0 = int(rng.integers(0, n_kf))
        for k in range(k0, min(k0 + n, n_kf)):
            if k != 13 and len(lists[k]) < stride - 4:
                lists[k].append(r)
    for r in range(900, 925):                                # rows that an old keyframe and the current one both list
        for k in (r % 23, CURRENT):
            if r not in lists[k]:
                lists[k].append(r)
    kf_mp = np.full((n_kf, stride), NONE, np.int32)
    for k, l in enumerate(lists):
        row = np.full(stride, NONE, np.int32)
        row[:len(l)] = l
        if k == 20:
            row[len(l):len(l) + 3] = (n_mp, n_mp + 1, n_mp)
        kf_mp[k] = rng.permutation(row)
    kf_mp[13, :2] = (3, 951)                                 # stale entries of an empty slot: not observations
    kf_id = (3 * np.arange(n_kf) + 1).astype(np.int32)
    kf_id[13], kf_id[5] = -1, 0
    kf_id[45], kf_id[60] = kf_id[60], kf_id[45]              # two candidates whose order by id is not their order by slot
    kf_t = np.arange(n_kf).astype(np.float64) + 0.25 * rng.random(n_kf)
    kf_t[5] = -1.5
    mp_flags = rng.integers(0, 4, n_mp).astype(np.uint8)
    mp_live = np.ones(n_mp, np.uint8)
    mp_live[990:] = 0
    mp_live[rng.choice(950, 12, replace=False)] = 0          # a few observed rows that hold no map point
    cand = rng.permutation(np.array([k for k in range(30, 69)], np.int32))[:20].astype(np.int32)
    cand_keep = np.zeros(20, np.uint8)
    cand_keep[[2, 11]] = 1
    return dict(kf_mp=kf_mp, mp_flags=mp_flags, mp_live=mp_live, n_mp=n_mp, kf_id=kf_id, kf_t=kf_t, cand=cand, cand_keep=cand_keep)


def scene_settings(cull_points=1, ratio_float32=0):
    return settings(CURRENT, cull_points=cull_points, min_age=20.0, min_obs_for_ba=2, max_critical_ratio=0.3, ratio_float32=ratio_float32)


def run_scene(scene, s, n_cand=None):
    n = len(scene["cand"]) if n_cand is None else n_cand
    return map_cull(scene["kf_mp"], scene["mp_flags"], scene["mp_live"], scene["n_mp"], scene["kf_id"], scene["kf_t"], scene["cand"][:n], scene["cand_keep"][:n], s)


LARGE_N_KF, LARGE_STRIDE = 12, 2048
LARGE_TRIP = 256 * 256                                       # rows whose block totals k_cull_offsets scans in one trip
LARGE_N_MP = (LARGE_TRIP, LARGE_TRIP + 1, LARGE_TRIP + 300)  # exactly one trip; one row into the second; a second trip of two blocks


def large_scene(n_mp, seed=5):
    """A table of 12 slots x 2048 entries over n_mp > 65 000 rows, so that the 256-row blocks of the removed-row compaction number more than
    the 256 whose totals are scanned at a time.  Entries as the GPU tests' random tables draw them: -1, the valid rows, n_mp and n_mp + 1.
    Slot k is at t = 3 k seconds, the ids are shuffled, every non-current slot is a candidate and none is kept.  Most rows have no
    observation; the last row is live and has none, so it is removed whatever else is.  Returns the inputs of map_cull plus `current`."""
    rng = np.random.default_rng(seed)
    n_kf, stride = LARGE_N_KF, LARGE_STRIDE
    kf_mp = rng.integers(-1, n_mp + 2, (n_kf, stride)).astype(np.int32)
    kf_mp[rng.random((n_kf, stride)) < 0.3] = -1
    kf_mp[kf_mp == n_mp - 1] = -1
    kf_mp[:, 7] = n_mp + (np.arange(n_kf) & 1)               # among so many rows the draw may leave the two out-of-range values out
    kf_id = rng.permutation(3 * n_kf)[:n_kf].astype(np.int32)
    current = int(rng.integers(0, n_kf))
    kf_id[current] = 3 * n_kf
    kf_t = 3.0 * np.arange(n_kf)
    cand = rng.permutation([k for k in range(n_kf) if k != current]).astype(np.int32)
    mp_flags = rng.integers(0, 4, n_mp).astype(np.uint8)
    mp_live = ((rng.random(n_mp) < 0.85) * rng.integers(1, 256, n_mp)).astype(np.uint8)
    mp_live[n_mp - 1] = 1
    return dict(kf_mp=kf_mp, mp_flags=mp_flags, mp_live=mp_live, n_mp=n_mp, kf_id=kf_id, kf_t=kf_t, cand=cand, cand_keep=np.zeros(len(cand), np.uint8),
                current=current)


def large_settings(scene, ratio_float32=0):
    return settings(scene["current"], cull_points=1, min_age=10.0, min_obs_for_ba=1, max_critical_ratio=0.9, ratio_float32=ratio_float32)


FILL_N_KF, FILL_STRIDE, FILL_N_MP, FILL_N_CAND = 304, 8, 200, 300
FILL_FIRST = 256 - 2                                         # the first candidate whose entry of the result block [2 + n_cand] lies behind the rows' one workgroup


def fill_scene(seed=8):
    """200 rows (one 256-row workgroup) and 300 candidates: the device's result block of 2 + 300 words is longer than the rows, so the launch
    that zeroes both has to be sized by the block.  Returns (scene, settings): about nine observations per row and min_obs_for_ba = 8, so that
    candidates are removed and kept all along the caller's order."""
    rng = np.random.default_rng(seed)
    n_kf, stride, n_mp = FILL_N_KF, FILL_STRIDE, FILL_N_MP
    kf_mp = rng.integers(-1, n_mp + 2, (n_kf, stride)).astype(np.int32)
    kf_mp[rng.random((n_kf, stride)) < 0.3] = -1
    kf_id = rng.permutation(3 * n_kf)[:n_kf].astype(np.int32)
    current = int(rng.integers(0, n_kf))
    kf_id[current] = 3 * n_kf
    kf_t = np.round(rng.normal(0, 8, n_kf), 2)
    cand = rng.permutation([k for k in range(n_kf) if k != current])[:FILL_N_CAND].astype(np.int32)
    scene = dict(kf_mp=kf_mp, mp_flags=rng.integers(0, 4, n_mp).astype(np.uint8), mp_live=np.ones(n_mp, np.uint8), n_mp=n_mp, kf_id=kf_id, kf_t=kf_t, cand=cand,
                 cand_keep=np.zeros(len(cand), np.uint8), current=current)
    return scene, settings(current, cull_points=1, min_age=2.0, min_obs_for_ba=8, max_critical_ratio=0.6)


def fill_second_call(scene, first):
    """The scene again with cand_keep = 1 for every candidate that the first call removed at positions >= FILL_FIRST: those never reach the
    device, and their cand_removed is the zero the call wrote itself."""
    keep = np.zeros(len(scene["cand"]), np.uint8)
    keep[FILL_FIRST:] = first["cand_removed"][FILL_FIRST:]
    return dict(scene, cand_keep=keep)


def find_ratio_pair(scene, s):
    """Settings (differing in ratio_float32 alone) under which some candidate of the scene is decided differently in float32 and in float64:
    a ratio nCritical / nMapPoints of one of the walked candidates, where the two products round to different sides of nCritical."""
    for k, n_map_points, n_critical, _ in run_scene(scene, s)["trace"]:
        if n_map_points == 0:
            continue
        for ratio in (n_critical / n_map_points, float(np.float32(n_critical / n_map_points))):
            a, b = dict(s, max_critical_ratio=ratio, ratio_float32=0), dict(s, max_critical_ratio=ratio, ratio_float32=1)
            if not np.array_equal(run_scene(scene, a)["cand_removed"], run_scene(scene, b)["cand_removed"]):
                return a, b
    return None
