"""The specification of ms_covisibility and ms_map_point_union, restated in numpy: set algebra over the keyframe table
kf_mp [n_kf, stride] (slot -> map-point rows, Keyframe::mapPoints).  Integer work only; the device results equal these bit for bit.

An entry r is valid iff 0 <= r < n_mp (the kernels' (uint32)r < n_mp); every other value is "none".  mp_flags [n_mp] uint8: bit 0 =
TRIANGULATED, bit 1 = neither NOT_TRIANGULATED nor BAD.  tests/test_covis_ref.py holds these functions against sequential dictionary /
set models written the way the reference writes its loops (keyframe.cpp:192-230, mapper_helpers.cpp:241-261, loop_closer.cpp:418-433)."""
import numpy as np

NONE = -1


def valid(kf_mp, n_mp):
    a = np.asarray(kf_mp, np.int64)
    return (a >= 0) & (a < n_mp)


def _passes(rows, mp_flags, require):
    if not require:
        return np.ones(len(rows), bool)
    return (np.asarray(mp_flags, np.uint8)[rows] & require) == require


def query_set(kf_mp, n_mp, mp_flags, slot, require):
    """S(q): the valid entries of `slot` that pass `require`, as a membership mask over the rows."""
    row = np.asarray(kf_mp[slot], np.int64)
    r = row[valid(row, n_mp)]
    member = np.zeros(n_mp, bool)
    member[r[_passes(r, mp_flags, require)]] = True
    return member


def covisibility(kf_mp, n_mp, mp_flags, queries):
    """queries: (slot, force_a, force_b, min_covis, require).  Returns count [n_q, n_kf] int32, the neighbour slots of every query
    (ascending) and their numbers."""
    kf_mp = np.asarray(kf_mp, np.int32)
    n_kf = kf_mp.shape[0]
    ok = valid(kf_mp, n_mp)
    idx = np.where(ok, kf_mp, n_mp)                          # invalid entries look at a member that is never set
    count = np.zeros((len(queries), n_kf), np.int32)
    neighbours = []
    for q, (slot, fa, fb, min_covis, require) in enumerate(queries):
        member = np.append(query_set(kf_mp, n_mp, mp_flags, slot, require), False)
        count[q] = member[idx].sum(axis=1) if kf_mp.size else 0
        k = np.arange(n_kf)
        is_nb = (k != slot) & ((k == fa) | (k == fb) | ((count[q] >= 1) & (count[q] >= min_covis)))
        neighbours.append(k[is_nb].astype(np.int32))
    return count, neighbours, np.array([len(n) for n in neighbours], np.int32)


def map_point_union(kf_mp, n_mp, mp_flags, kf_list, problems):
    """problems: (first, count, exclude_slot, require) over kf_list.  Returns, per problem, the rows in ascending order and for each the
    smallest position of the problem's list whose slot lists it."""
    kf_mp = np.asarray(kf_mp, np.int32)
    rows_out, owner_out = [], []
    for first, count, exclude, require in problems:
        owner = np.full(n_mp, np.iinfo(np.int32).max, np.int64)
        for p in range(count - 1, -1, -1):                   # descending, so the smallest position is written last
            row = np.asarray(kf_mp[kf_list[first + p]], np.int64)
            r = row[valid(row, n_mp)]
            owner[r[_passes(r, mp_flags, require)]] = p
        if exclude != NONE:
            row = np.asarray(kf_mp[exclude], np.int64)
            owner[row[valid(row, n_mp)]] = np.iinfo(np.int32).max
        rows = np.nonzero(owner != np.iinfo(np.int32).max)[0]
        rows_out.append(rows.astype(np.int32))
        owner_out.append(owner[rows].astype(np.int32))
    return rows_out, owner_out, np.array([len(r) for r in rows_out], np.int32)


def make_scene(seed=5, n_kf=70, stride=100, n_mp=1003, max_obs=8, empty_slot=13, odd_slot=20, odd_entries=None):
    """A seeded map: every row is observed by up to max_obs consecutive slots (at most once per slot, the reference's invariant), entries
    shuffled within a slot, slot `empty_slot` emptied, three out-of-range entries placed in slot `odd_slot` (odd_entries; by default
    n_mp, n_mp + 1, n_mp).  Returns kf_mp [n_kf, stride] int32 and mp_flags [n_mp] uint8."""
    rng = np.random.default_rng(seed)
    lists = [[] for _ in range(n_kf)]
    for r in range(n_mp):
        n = int(rng.integers(1, max_obs + 1))
        k0 = int(rng.integers(0, n_kf))
        for k in range(k0, min(k0 + n, n_kf)):
            if len(lists[k]) < stride - 3:
                lists[k].append(r)
    kf_mp = np.full((n_kf, stride), NONE, np.int32)
    for k, l in enumerate(lists):
        if k == empty_slot:
            continue
        row = np.full(stride, NONE, np.int32)
        row[:len(l)] = l
        if k == odd_slot:
            row[len(l):len(l) + 3] = odd_entries if odd_entries is not None else (n_mp, n_mp + 1, n_mp)
        kf_mp[k] = rng.permutation(row)
    mp_flags = rng.integers(0, 4, n_mp).astype(np.uint8)
    return kf_mp, mp_flags


def scene_queries(n_kf, min_covis, require, forced, empty_slot=13):
    """Every slot as a query.  forced: 'chain' (slot - 1, slot + 1), 'none', or 'self' (the slot itself and the empty slot)."""
    out = []
    for s in range(n_kf):
        if forced == "chain":
            fa, fb = s - 1, (s + 1 if s + 1 < n_kf else NONE)
        elif forced == "none":
            fa, fb = NONE, NONE
        else:
            fa, fb = s, empty_slot
        out.append((s, fa, fb, min_covis, require))
    return out


MIN_COVIS = (-3, 0, 1, 5, 15)
REQUIRE = (0, 1)
FORCED = ("chain", "none", "self")
