"""The specification of ms_map_extract in numpy: the partial map copy of copyMap (mapper.cpp:281-326), that is
MapDB(mapDB, activeKeyframes) (mapdb.cpp:116-159) with MapPoint(mp, activeKeyframes) (map_point.cpp:22-43), on the map tables, and the scenes
the GPU tests run.  Everything is integers and copied bits: a comparison with this file is bit for bit.

Source tables, a dict: kf_mp [n_kf, stride] int32, kf_id [n_kf] int32 (-1: an empty slot), mp_flags [n_mp] uint8, mp_live [n_mp] uint8 or
None (every row live), mp_pos [n_mp, 3] float64, mp_norm [n_mp, 3] float32, mp_min_dist / mp_max_dist [n_mp] float32, mp_desc [n_mp, 8]
uint32, mp_track [n_mp] int32 or None, kp_x / kp_y / kp_depth float32 and kp_octave int32 [n_kf, stride] (all four or None), kf_pose [n_kf, 12]
float64 or None, track_row [n_track] int32 or None with track_base, desc_pool [pool_size, 8] uint32 or None with desc_base [n_kf] int32 and
n_kp [n_kf] int32 (the keypoints of each slot)."""
import numpy as np

OK, INVALID, CAPACITY = 0, -1, -4
ROW_FIELDS = ("mp_pos", "mp_norm", "mp_min_dist", "mp_max_dist", "mp_desc", "mp_flags", "mp_track")       # copied bit for bit
KP_FIELDS = ("kp_x", "kp_y", "kp_octave", "kp_depth")
DTYPES = dict(kf_mp=np.int32, mp_flags=np.uint8, mp_live=np.uint8, mp_pos=np.float64, mp_norm=np.float32, mp_min_dist=np.float32, mp_max_dist=np.float32,
              mp_desc=np.uint32, mp_track=np.int32, kp_x=np.float32, kp_y=np.float32, kp_octave=np.int32, kp_depth=np.float32, kf_pose=np.float64,
              track_row=np.int32, desc_pool=np.uint32, n_obs=np.int32, row_src=np.int32, row_dst=np.int32)
DST = tuple(DTYPES)                                          # every array a destination can have


def sizes(t, n_kf_dst, n_mp_dst, pool_size_dst=0):
    n_kf, stride = t["kf_mp"].shape
    return dict(n_kf=n_kf, stride=stride, n_mp=len(t["mp_flags"]), track_base=int(t.get("track_base", 0)), n_track=0 if t["track_row"] is None else len(t["track_row"]),
                pool_size=0 if t["desc_pool"] is None else len(t["desc_pool"]), n_kf_dst=n_kf_dst, n_mp_dst=n_mp_dst, pool_size_dst=pool_size_dst)


def dst_shape(name, z):
    """The shape of a destination array for the sizes z."""
    w = dict(mp_pos=3, mp_norm=3, mp_desc=8, kf_pose=12, desc_pool=8).get(name, 1)
    if name in ("kf_mp",) + KP_FIELDS:
        return (z["n_kf_dst"], z["stride"])
    n = z["n_kf_dst"] if name == "kf_pose" else z["n_track"] if name == "track_row" else z["pool_size_dst"] if name == "desc_pool" else z["n_mp"] if name == "row_dst" else z["n_mp_dst"]
    return (n, w) if w > 1 else (n,)


def dst_names(t, outputs=True):
    """The arrays a destination of these source tables has."""
    return [k for k in DST if k in ("kf_mp", "mp_live") or (k in t and t[k] is not None) or (outputs and k in ("n_obs", "row_src", "row_dst"))]


def fresh_dst(t, z, fill=0, outputs=True):
    """A destination filled with a byte pattern."""
    return {k: np.frombuffer(bytes([fill]) * (int(np.prod(dst_shape(k, z))) * np.dtype(DTYPES[k]).itemsize), DTYPES[k]).reshape(dst_shape(k, z)).copy()
            for k in dst_names(t, outputs)}


def present(t, r):
    """(uint32)r < n_mp and live, the rule of DESIGN 9.18, for an int64 array of entries"""
    n_mp = len(t["mp_flags"])
    ok = (r >= 0) & (r < n_mp)
    if t["mp_live"] is not None and n_mp:
        ok = ok & (t["mp_live"][np.where(ok, r, 0)] != 0)
    return ok


def extract(t, active, z, dst=None):
    """ms_map_extract.  z = sizes(...); dst = the destination arrays before the call (default: zeros).  Returns dict(rc, counts [5],
    dst_desc_base [n_active], and every destination array as it is afterwards)."""
    active = [int(s) for s in active]
    n_mp, stride, n_a = z["n_mp"], z["stride"], len(active)
    out = {k: np.array(v, copy=True) for k, v in (fresh_dst(t, z) if dst is None else dst).items()}
    e = np.asarray(t["kf_mp"], np.int64)[active].reshape(n_a, stride) if n_a else np.zeros((0, stride), np.int64)
    valid = (e >= 0) & (e < n_mp)
    keep = present(t, e)
    cnt = np.bincount(e[keep], minlength=n_mp).astype(np.int32)
    row_src = np.nonzero(cnt > 0)[0].astype(np.int32)        # ascending source rows: the walk of std::set<MpId>
    n_rows = len(row_src)
    row_dst = np.full(n_mp, -1, np.int32)
    row_dst[row_src] = np.arange(n_rows, dtype=np.int32)
    # the pool offsets and the track count do not depend on the capacity verdict
    base, n_desc = np.full(n_a, -1, np.int32), 0
    if t["desc_pool"] is not None:
        for i, s in enumerate(active):
            if t["desc_base"][s] >= 0:
                base[i] = n_desc
                n_desc += int(t["n_kp"][s])
    track_dst = None
    if t["track_row"] is not None:
        tr = np.asarray(t["track_row"], np.int64)
        ok = present(t, tr)
        safe = np.where(ok, tr, 0)
        ok = ok & (np.asarray(t["mp_track"], np.int64)[safe] == z["track_base"] + np.arange(len(tr))) & (row_dst[safe] >= 0) if n_mp else ok & False
        track_dst = np.where(ok, row_dst[safe] if n_mp else -1, -1).astype(np.int32)
    counts = np.array([n_rows, int(keep.sum()), int((valid & ~keep).sum()), 0 if track_dst is None else int((track_dst >= 0).sum()), n_desc], np.int32)
    out.update(counts=counts, dst_desc_base=base)
    if n_rows > z["n_mp_dst"]:
        out["rc"] = CAPACITY                                 # every verdict before any write
        return out
    for k in ROW_FIELDS:
        if k in out:
            out[k][:n_rows] = t[k][row_src]
    out["mp_live"][:n_rows] = 1
    out["mp_live"][n_rows:] = 0
    out["mp_flags"][n_rows:] = 0
    if "mp_track" in out:
        out["mp_track"][n_rows:] = -1
    if "n_obs" in out:
        out["n_obs"][:n_rows] = cnt[row_src]
        out["n_obs"][n_rows:] = 0
    if "row_src" in out:
        out["row_src"][:n_rows] = row_src
    if "row_dst" in out:
        out["row_dst"][:] = row_dst
    out["kf_mp"][:n_a] = np.where(keep, row_dst[np.where(keep, e, 0)] if n_mp else -1, -1)
    out["kf_mp"][n_a:] = -1
    for k in KP_FIELDS:
        if k in out:
            out[k][:n_a] = t[k][active]
            out[k][n_a:] = 0
    if "kf_pose" in out and n_a:
        out["kf_pose"][:n_a] = t["kf_pose"][active]
    if track_dst is not None:
        out["track_row"][:] = track_dst
    if "desc_pool" in out:
        for i, s in enumerate(active):
            if base[i] >= 0:
                n = int(t["n_kp"][s])
                out["desc_pool"][base[i]:base[i] + n] = t["desc_pool"][t["desc_base"][s]:t["desc_base"][s] + n]
    out["rc"] = OK
    return out


def cut_links(t, active):
    """mapdb.cpp:124-129 on slots: (previous, next) per active slot as DESTINATION slots, -1 where the neighbour is not active."""
    where = {int(s): i for i, s in enumerate(active)}
    return [(where.get(int(t["previous"][s]), -1), where.get(int(t["next"][s]), -1)) for s in active]


def occupied(t):
    """The full copy's active list: every slot with kf_id >= 0, by ascending KfId."""
    slots = [s for s in range(len(t["kf_id"])) if t["kf_id"][s] >= 0]
    return sorted(slots, key=lambda s: int(t["kf_id"][s]))


# ---------------------------------------------------------------------------------------------------------------------------- scenes
def _tables(kf_mp, kf_id, n_mp, seed, n_track=0, track_base=0, pool=True):
    rng = np.random.default_rng(seed)
    kf_mp = np.array(kf_mp, np.int32)
    n_kf, stride = kf_mp.shape
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    t = dict(kf_mp=kf_mp, kf_id=np.asarray(kf_id, np.int32), mp_flags=rng.integers(1, 4, n_mp).astype(np.uint8), mp_live=np.ones(n_mp, np.uint8),
             mp_pos=rng.standard_normal((n_mp, 3)), mp_norm=f32(n_mp, 3), mp_min_dist=f32(n_mp), mp_max_dist=f32(n_mp),
             mp_desc=rng.integers(0, 2 ** 32, (n_mp, 8), dtype=np.uint32), mp_track=np.full(n_mp, -1, np.int32), kp_x=f32(n_kf, stride), kp_y=f32(n_kf, stride),
             kp_octave=rng.integers(0, 8, (n_kf, stride)).astype(np.int32), kp_depth=f32(n_kf, stride), kf_pose=rng.standard_normal((n_kf, 12)),
             track_row=np.full(n_track, -1, np.int32), track_base=track_base, desc_pool=None, desc_base=np.full(n_kf, -1, np.int32),
             n_kp=np.full(n_kf, stride, np.int32))
    order = sorted((s for s in range(n_kf) if kf_id[s] >= 0), key=lambda s: kf_id[s])
    t["previous"], t["next"] = np.full(n_kf, -1, np.int32), np.full(n_kf, -1, np.int32)      # the chain in KfId order, as slots
    for a, b in zip(order, order[1:]):
        t["next"][a], t["previous"][b] = b, a
    if pool:
        t["desc_pool"] = rng.integers(0, 2 ** 32, (n_kf * stride + 5, 8), dtype=np.uint32)
        t["desc_base"] = (3 + stride * rng.permutation(n_kf)).astype(np.int32)      # slices in no particular order
    return t


def every_kind():
    """Scene 1: 6 slots x 8 on 24 rows; slots 4, 0, 2 are active, given in that order (not slot order); slot 3 is empty with a stale entry."""
    kf = np.full((6, 8), -1, np.int32)
    kf[0] = [3, 7, -1, 24, 11, 11, -5, 9]                   # 3 shared with slot 2; 11 twice; -1, >= n_mp, < -1; 9 is valid but not live
    kf[2] = [3, 15, 20, -1, 2, 30, 17, 9]                   # 15 shared with the inactive slot 1; 9 again
    kf[4] = [22, 0, -1, -1, 7, 19, 21, -1]                  # 7 shared with slot 0; row 0 is a row like any other
    kf[1] = [15, 5, 6, 13, -1, -1, 23, -1]                  # inactive: 5, 6, 13, 23 must not appear
    kf[5] = [5, 13, 1, -1, -1, -1, -1, -1]                  # inactive
    kf[3] = [8, 3, -1, -1, -1, -1, -1, -1]                  # empty slot: stale entries
    t = _tables(kf, [40, 31, 52, -1, 37, 60], 24, 21, n_track=12, track_base=500)
    t["mp_live"][[9, 12]] = 0
    t["mp_flags"][9] = 3
    # tracks: 500 -> row 3 present; 501 -> row 7 but the row was reused for track 900 (stale); 502 -> row 5 present but inactive; 503 -> row 9 not live;
    # 504 -> row 20 present; 505 -> out of range; row 11 has no track
    t["mp_track"][[3, 7, 5, 9, 20]] = [500, 900, 502, 503, 504]
    t["track_row"][:6] = [3, 7, 5, 9, 20, 77]
    t["desc_base"][0] = -1                                   # an active slot without descriptors
    t["n_kp"][:] = [8, 6, 5, 0, 7, 8]
    return dict(t=t, active=[4, 0, 2], n_kf_dst=5, n_mp_dst=20, pool_size_dst=14)


def second_trip(k_block=256):
    """Scene 2: more source rows than one trip of block_offsets covers (k_block workgroups of k_block rows), active rows on both sides of the trip's
    edge; 4 slots x 96, two active: the output stays a few hundred rows."""
    rng = np.random.default_rng(22)
    n_mp = k_block * k_block + 3 * k_block + 17
    kf = np.where(rng.random((4, 96)) < 0.85, rng.integers(0, n_mp, (4, 96)), -1).astype(np.int32)
    edge = k_block * k_block
    kf[1, :6] = [edge - 1, edge, edge + 1, n_mp - 1, 0, edge + k_block]
    kf[3, :3] = [edge, edge - k_block, n_mp - 1]
    t = _tables(kf, [5, 9, 7, 11], n_mp, 23, n_track=64, track_base=0, pool=False)
    t["mp_live"][rng.choice(n_mp, n_mp // 20, replace=False)] = 0
    t["mp_live"][[edge - 1, edge, edge + 1, n_mp - 1, 0]] = 1
    rows = kf[1, :6]
    t["mp_track"][rows] = np.arange(6)
    t["track_row"][:6] = rows
    return dict(t=t, active=[1, 3], n_kf_dst=3, n_mp_dst=200, pool_size_dst=0, k_block=k_block)


def optional_absent():
    """Scene 3: mp_live, mp_track, track_row, the keypoint arrays, the poses and the pool are None; the three optional outputs too."""
    rng = np.random.default_rng(24)
    kf = np.where(rng.random((5, 300)) < 0.7, rng.integers(-2, 420, (5, 300)), -1).astype(np.int32)
    t = _tables(kf, [4, 6, 2, 9, -1], 400, 25, pool=False)
    for k in ("mp_live", "mp_track", "track_row", "kf_pose") + KP_FIELDS:
        t[k] = None
    return dict(t=t, active=[2, 0, 3], n_kf_dst=3, n_mp_dst=400, pool_size_dst=0, outputs=False)


SCENES = dict(every_kind=every_kind, second_trip=second_trip, optional_absent=optional_absent)
_cache = {}


def cached(name):
    """(scene, sizes, extract(scene) on a zero destination), computed once and shared; none is to be changed."""
    if name not in _cache:
        sc = SCENES[name]()
        z = sizes(sc["t"], sc["n_kf_dst"], sc["n_mp_dst"], sc["pool_size_dst"])
        _cache[name] = (sc, z, extract(sc["t"], sc["active"], z, fresh_dst(sc["t"], z, 0, sc.get("outputs", True))))
    return _cache[name]


def scene_conditions(name, sc, z, want):
    """What each scene is there to hit."""
    t, kf, active = sc["t"], sc["t"]["kf_mp"], sc["active"]
    rows = want["row_src"][:want["counts"][0]].tolist() if "row_src" in want else None
    if name == "every_kind":
        assert active != sorted(active) and rows == [0, 2, 3, 7, 11, 15, 17, 19, 20, 21, 22]
        assert not {5, 6, 13, 23, 1, 8, 9} & set(rows)                                                   # inactive slots only, the stale entry, not live
        assert want["n_obs"][:11].tolist() == [1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1] and want["counts"].tolist() == [11, 14, 2, 2, 5 + 7]
        assert want["kf_mp"][1].tolist() == [2, 3, -1, -1, 4, 4, -1, -1] and (want["kf_mp"][3:] == -1).all()
        assert want["track_row"].tolist() == [2, -1, -1, -1, 8] + [-1] * 7 and want["dst_desc_base"].tolist() == [0, -1, 7]
        assert want["mp_track"][:11].tolist().count(-1) == 8 and t["kf_id"][3] < 0 and kf[3, 1] == 3
    elif name == "second_trip":
        k = sc["k_block"]
        assert z["n_mp"] > k * k and min(rows) < k * k <= max(rows) and k * k in rows and k * k - 1 in rows and 100 < len(rows) <= z["n_mp_dst"]
        assert want["counts"][2] > 0 and want["counts"][3] >= 5
    elif name == "optional_absent":
        assert rows is None and not {"mp_track", "track_row", "kf_pose", "n_obs", "row_dst"} & set(want) and want["counts"][0] > 200
        assert (kf[active] >= 400).any() and (kf[active] < -1).any() and want["counts"][2] == 0 and (want["dst_desc_base"] == -1).all()
