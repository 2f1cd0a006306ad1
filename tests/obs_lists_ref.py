"""The specification of ms_observation_lists, restated in numpy: MapPoint::observations (`std::map<KfId, KpId>`) of chosen rows
of the map-point table as CSR lists, read off the keyframe table kf_mp [n_kf, stride] (slot -> map-point rows, Keyframe::mapPoints) and the
keypoint table parallel to it.  Integer work and copies: the device results equal these bit for bit.

An entry r is valid iff 0 <= r < n_mp.  kf_id [n_kf] int32, -1 for an empty slot (its entries are stale: no observations); mp_flags [n_mp]
uint8, bit 0 = TRIANGULATED, bit 1 = neither NOT_TRIANGULATED nor BAD.  tests/test_obs_lists_ref.py holds this against a dictionary model
written the way the reference builds `observations`."""
import numpy as np

FROM_ROWS, FROM_SLOT = 0, 1
ALL, REFRESH, RETRIANGULATE = 0, 1, 2
INT32_MIN = -2 ** 31


def select(source, filter=ALL, drop_empty=0, slot=-1, rows_in=None):
    return dict(source=int(source), filter=int(filter), drop_empty=int(drop_empty), slot=int(slot),
                rows_in=None if rows_in is None else np.asarray(rows_in, np.int32).reshape(-1))


def transpose(kf_mp, n_mp, kf_id):
    """The observations of every row: (start [n_mp + 1], slot, j), a row's run ordered by (kf_id of the slot, j); slots with kf_id < 0 and
    entries outside [0, n_mp) left out, entries of one slot naming the same row all kept."""
    kf_mp = np.asarray(kf_mp, np.int32).reshape(len(kf_id), -1)
    kf_id = np.asarray(kf_id, np.int32)
    order = [k for k in np.argsort(kf_id, kind="stable") if kf_id[k] >= 0]
    rows, slots, js = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for k in order:
        e = kf_mp[k].astype(np.int64)
        j = np.nonzero((e >= 0) & (e < n_mp))[0]
        rows.append(e[j]); slots.append(np.full(len(j), k, np.int64)); js.append(j)
    rows, slots, js = np.concatenate(rows), np.concatenate(slots), np.concatenate(js)
    by_row = np.argsort(rows, kind="stable")                 # stable: inside a row the (kf_id, j) order stays
    start = np.zeros(n_mp + 1, np.int64)
    start[1:] = np.cumsum(np.bincount(rows, minlength=n_mp)[:n_mp])
    return start, slots[by_row], js[by_row]


def selected_rows(kf_mp, n_mp, mp_flags, n_obs, sel):
    """The kept rows in order: the selection's valid entries at their first occurrence, then the filter, then drop_empty."""
    src = np.asarray(kf_mp, np.int32)[sel["slot"]] if sel["source"] == FROM_SLOT else (sel["rows_in"] if sel["rows_in"] is not None else np.zeros(0, np.int32))
    src = src.astype(np.int64)
    src = src[(src >= 0) & (src < n_mp)]
    _, first = np.unique(src, return_index=True)
    rows = src[np.sort(first)]
    if sel["filter"] == REFRESH:
        rows = rows[(mp_flags[rows] & 2) != 0]
    elif sel["filter"] == RETRIANGULATE:
        rows = rows[((mp_flags[rows] & 1) == 0) | (n_obs[rows] >= 2)]
    if sel["drop_empty"]:
        rows = rows[n_obs[rows] > 0]
    return rows


def observation_lists(kf_mp, n_mp, kf_id, mp_flags, kp, desc_base, sel, n_levels=0, transposed=None):
    """kp: dict of x, y, depth (float32) and octave (int32), [n_kf, stride] each; desc_base [n_kf] int32.  Returns a dict of every output
    array of ms_obs_lists plus n_rows, n_obs and violations (gathered octaves outside [0, n_levels), stored clamped; none counted for
    n_levels == 0).  `transposed` = transpose(kf_mp, n_mp, kf_id) when the caller has it already."""
    kf_mp = np.asarray(kf_mp, np.int32).reshape(len(kf_id), -1)
    flags = np.zeros(n_mp, np.uint8) if mp_flags is None else np.asarray(mp_flags, np.uint8)
    start, slots, js = transposed if transposed is not None else transpose(kf_mp, n_mp, kf_id)
    n_all = np.diff(start)
    rows = selected_rows(kf_mp, n_mp, flags, n_all, sel)
    n_row = n_all[rows]
    obs_start = np.zeros(len(rows) + 1, np.int64)
    obs_start[1:] = np.cumsum(n_row)
    take = np.concatenate([np.arange(start[r], start[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    s, j = slots[take], js[take]
    octave = np.asarray(kp["octave"], np.int32)[s, j].astype(np.int64)
    violations = 0
    if n_levels > 0:
        violations = int(((octave < 0) | (octave >= n_levels)).sum())
        octave = np.clip(octave, 0, n_levels - 1)
    base = np.asarray(desc_base, np.int64)[s]
    first_octave = np.zeros(len(rows), np.int64)
    some = n_row > 0
    first_octave[some] = octave[obs_start[:-1][some]]
    return dict(rows=rows.astype(np.int32), obs_start=obs_start.astype(np.int32), n_obs_row=n_row.astype(np.int32), first_octave=first_octave.astype(np.int32),
                was_triangulated=((flags[rows] & 2) != 0).astype(np.uint8), obs_kf=s.astype(np.int32), obs_kp=j.astype(np.int32), obs_octave=octave.astype(np.int32),
                obs_desc=np.where(base < 0, -1, base + j).astype(np.int32), obs_x=np.asarray(kp["x"], np.float32)[s, j], obs_y=np.asarray(kp["y"], np.float32)[s, j],
                obs_depth=np.asarray(kp["depth"], np.float32)[s, j], n_rows=len(rows), n_obs=int(obs_start[-1]), violations=violations)


ROW_ARRAYS = ("rows", "obs_start", "n_obs_row", "first_octave", "was_triangulated")
OBS_ARRAYS = ("obs_kf", "obs_kp", "obs_octave", "obs_desc", "obs_x", "obs_y", "obs_depth")
N_LEVELS = 8


def keypoint_table(rng, n_kf, stride):
    """A keypoint table and descriptor bases for a map of n_kf x stride: distinct pixels (so a wrong gather shows), octaves in [0, N_LEVELS),
    a depth for every third keypoint (-1 = none); every seventh slot has no descriptors, the others' bases are not in slot order."""
    kp = dict(x=(rng.random((n_kf, stride)) * 640).astype(np.float32), y=(rng.random((n_kf, stride)) * 480).astype(np.float32),
              octave=rng.integers(0, N_LEVELS, (n_kf, stride)).astype(np.int32),
              depth=np.where(rng.integers(0, 3, (n_kf, stride)) == 0, rng.random((n_kf, stride)) * 20 + 0.5, -1.0).astype(np.float32))
    base = (rng.permutation(n_kf) * stride).astype(np.int32)
    base[::7] = -1
    return kp, base


A_KF, A_STRIDE, A_MP = 70, 100, 1003                         # the sizes of the cull fixture
A_EMPTY = (13, 27, 41)
A_TWICE = (30, 7)                                            # slot 30 lists row 7 twice
A_LENGTHS = {900: 63, 901: 64, 902: 65, 903: 1, 904: 2}     # rows with exactly that many observations; rows 950 .. 1002 have none
A_CURRENT = 69


def scene_a(seed=23):
    """70 slots x 100.  kf_id is a permutation-like order that is not monotone in the slot (slot 5 holds the oldest id, 45 and 60 are
    exchanged); slots 13, 27, 41 are empty and still hold stale entries (rows 900 .. 904 and 951 among them); slot 20 carries the entries
    n_mp, n_mp + 1 and INT32_MIN besides -1; slot 30 lists row 7 twice; rows 900 .. 904 have 63, 64, 65, 1 and 2 observations, rows 950 ..
    1002 none; the other rows are observed by runs of consecutive slots.  Slot 69 (the current keyframe) lists rows of every kind."""
    rng = np.random.default_rng(seed)
    n_kf, stride, n_mp = A_KF, A_STRIDE, A_MP
    live = [k for k in range(n_kf) if k not in A_EMPTY]
    lists = [[] for _ in range(n_kf)]
    for r in range(900):
        n = int(rng.choice([1, 1, 2, 3, 4, 6, 8]))
        k0 = int(rng.integers(0, n_kf))
        for k in range(k0, min(k0 + n, n_kf)):
            if k not in A_EMPTY and len(lists[k]) < stride - 12:
                lists[k].append(r)
    others = [k for k in live if k != A_CURRENT]
    for r, n in A_LENGTHS.items():                           # the current keyframe's selection meets long and short lists: it observes all but row 902
        who = list(rng.permutation(others)[:n]) if r == 902 else [A_CURRENT] + list(rng.permutation(others)[:n - 1])
        for k in who:
            lists[int(k)].append(r)
    if 7 not in lists[A_TWICE[0]]:
        lists[A_TWICE[0]].append(7)
    lists[A_TWICE[0]].append(7)
    for k in A_EMPTY:
        lists[k] = [900, 901, 902, 903, 904, 951, 3]
    kf_mp = np.full((n_kf, stride), -1, np.int32)
    for k, l in enumerate(lists):
        row = np.full(stride, -1, np.int64)
        row[:len(l)] = l
        if k == 20:
            row[len(l):len(l) + 4] = (n_mp, n_mp + 1, INT32_MIN, n_mp)
        kf_mp[k] = rng.permutation(row).astype(np.int32)
    kf_id = (3 * np.arange(n_kf) + 1).astype(np.int32)
    kf_id[list(A_EMPTY)] = -1
    kf_id[5] = 0
    kf_id[45], kf_id[60] = kf_id[60], kf_id[45]
    kp, base = keypoint_table(rng, n_kf, stride)
    return dict(kf_mp=kf_mp, n_mp=n_mp, kf_id=kf_id, mp_flags=rng.integers(0, 4, n_mp).astype(np.uint8), kp=kp, desc_base=base, lengths=dict(A_LENGTHS))


B_KF, B_STRIDE, B_MP = 1100, 8, 70000
B_LENGTHS = {5: 1025, 6: 1100, 8: 300}


def scene_b(seed=29):
    """1100 slots x 8, every slot with a keyframe, ids a permutation of the slots.  Row 6 is observed by every slot, row 5 by 1025 of them
    and row 8 by 300: the lists that are sorted from global memory and through LDS.  70 000 map points, so a whole-map selection packs 274
    blocks of rows and scans their totals in two trips."""
    rng = np.random.default_rng(seed)
    n_kf, stride, n_mp = B_KF, B_STRIDE, B_MP
    kf_mp = np.full((n_kf, stride), -1, np.int32)
    kf_mp[:, 3:] = rng.integers(9, n_mp, (n_kf, stride - 3))
    kf_mp[rng.random((n_kf, stride)) < 0.2] = -1
    col = rng.integers(0, 3, n_kf)                           # rows 5, 6 and 8 sit in columns 0 .. 2, in a different one per slot
    for i, (r, n) in enumerate(B_LENGTHS.items()):
        who = rng.permutation(n_kf)[:n]
        kf_mp[who, (col[who] + i) % 3] = r
    kp, base = keypoint_table(rng, n_kf, stride)
    return dict(kf_mp=kf_mp, n_mp=n_mp, kf_id=rng.permutation(n_kf).astype(np.int32) * 2 + 1, mp_flags=rng.integers(0, 4, n_mp).astype(np.uint8), kp=kp,
                desc_base=base, lengths=dict(B_LENGTHS))


C_KF, C_STRIDE, C_MP, C_LONG = 66, 1040, 1100, 1030


def scene_c(seed=31):
    """66 slots x 1040, ids a permutation of the slots.  Row r < 1030 is observed by every slot but slot r % 66: 1030 lists of 65
    observations, six more than the 1024 workgroups that sort the lists longer than a wave, so some of them sort a second list through the
    LDS that held their first.  Rows 1030 .. 1099 have up to three observations."""
    rng = np.random.default_rng(seed)
    n_kf, stride, n_mp = C_KF, C_STRIDE, C_MP
    kf_mp = np.full((n_kf, stride), -1, np.int32)
    for k in range(n_kf):
        rows = [r for r in range(C_LONG) if r % n_kf != k] + rng.integers(C_LONG, n_mp, 3).tolist()
        row = np.full(stride, -1, np.int32)
        row[:len(rows)] = rows
        kf_mp[k] = rng.permutation(row)
    short = kf_mp >= C_LONG
    kf_mp[short & (rng.random(kf_mp.shape) < 0.5)] = -1
    kp, base = keypoint_table(rng, n_kf, stride)
    return dict(kf_mp=kf_mp, n_mp=n_mp, kf_id=rng.permutation(n_kf).astype(np.int32) * 2 + 1, mp_flags=rng.integers(0, 4, n_mp).astype(np.uint8), kp=kp,
                desc_base=base, lengths={r: n_kf - 1 for r in range(C_LONG)})


def run_scene(scene, sel, n_levels=N_LEVELS):
    if "transposed" not in scene:
        scene["transposed"] = transpose(scene["kf_mp"], scene["n_mp"], scene["kf_id"])
    return observation_lists(scene["kf_mp"], scene["n_mp"], scene["kf_id"], scene["mp_flags"], scene["kp"], scene["desc_base"], sel, n_levels, scene["transposed"])
