"""The specification of ms_map_fuse and ms_map_replace_pairs, in two forms that tests/test_map_fuse_ref.py holds equal:

  sequential   the reference's data structures: a dict of map points, each with its observation dict, status bits and track id; the
               keyframes' mapPoints lists; trackIdToMapPoint.  replaceDuplication (keyframe_matcher.cpp:424-526, behind its gates),
               MapPoint::replaceWith (map_point.cpp:118-156) and the merge loop of loop_closer.cpp:531-546 written out.
  tables       numpy over the device tables (kf_mp, mp_flags, mp_live, n_obs, mp_track, track_row), the rules of include/mi355slam.h.

Both are fed the per-entry candidate keypoint (`candidates` derives it from kept_entry / top_idx / top_dist as the kernel does), so the walk
is specified without geometry; make_scene draws synthetic candidates."""
import numpy as np

TRIP = 1024                                                  # entries per trip of the walking workgroup


def candidates(n_entries, views, n_kept, kept_entry, top_idx, top_dist, max_dist):
    """cand[e] = the candidate keypoint of entry e, -1 for none (detail::best_candidate per kept query)."""
    cand = np.full(n_entries, -1, np.int32)
    for (slot, first, count), nk in zip(views, n_kept):
        for q in range(first, first + int(nk)):
            if top_idx[4 * q] >= 0 and top_dist[4 * q] <= max_dist:
                cand[kept_entry[q]] = top_idx[4 * q]
    return cand


def lists_from_candidates(rng, cand, views, mp_live=None):
    """The inverse for the scene: kept_entry / top_idx / top_dist / n_kept that give `cand` at max_dist 50.  Some entries without a candidate
    are dropped by the "gate", some are kept with an empty list, some with a best distance above 50."""
    n = len(cand)
    kept_entry = np.full(n, -7, np.int32)
    top_idx = np.full(4 * n, -1, np.int32)
    top_dist = np.full(4 * n, 256, np.uint16)
    n_kept = []
    for slot, first, count in views:
        q = first
        for e in range(first, first + count):
            how = rng.integers(0, 3)
            if cand[e] < 0 and how == 0:
                continue                                     # the gate dropped it
            kept_entry[q] = e
            if cand[e] >= 0:
                top_idx[4 * q], top_dist[4 * q] = cand[e], rng.integers(0, 51)
                top_idx[4 * q + 1], top_dist[4 * q + 1] = rng.integers(0, 8), 60
            elif how == 1:
                top_idx[4 * q], top_dist[4 * q] = rng.integers(0, 8), rng.integers(51, 257)
            q += 1
        n_kept.append(q - first)
    return kept_entry, top_idx, top_dist, np.array(n_kept, np.int32)


def observation_count(kf_mp, n_mp):
    v = kf_mp[(kf_mp >= 0) & (kf_mp < n_mp)]
    return np.bincount(v, minlength=n_mp).astype(np.int32)


def copy_tables(T):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in T.items()}


# ---- the tables form ------------------------------------------------------------------------------------------------------------------
def replace_tables(T, l, w, note=None):
    kf_mp, n_mp = T["kf_mp"], len(T["mp_live"])
    gained = []
    for s in range(kf_mp.shape[0]):
        at = np.nonzero(kf_mp[s] == l)[0]
        if not len(at):
            continue
        if (kf_mp[s] == w).any():
            kf_mp[s, at] = -1
        else:
            kf_mp[s, at] = w
            T["n_obs"][w] += len(at)
            gained.append(s)
    T["mp_live"][l] = 0
    T["mp_flags"][l] = 0
    T["n_obs"][l] = 0
    if T.get("mp_track") is not None:
        t = T["mp_track"][l]
        if t != -1:
            if T["mp_track"][w] == -1:
                T["mp_track"][w] = t
                inside = 0 <= t - T["track_base"] < len(T["track_row"])
                if inside:
                    T["track_row"][t - T["track_base"]] = w
                if note is not None:
                    note["track_transfer" if inside else "track_outside"] += 1
            elif note is not None:
                note["track_both"] += 1
    return gained


def fuse_tables(T, mp_index, views, cand, source_slot=-1):
    """The walk on copies of the tables.  Returns the tables after it and the outputs of ms_map_fuse, plus `note`: how often the scene's
    conditions occurred (read by the tests, not by the comparison)."""
    T = copy_tables(T)
    kf_mp, flags, live, n_obs = T["kf_mp"], T["mp_flags"], T["mp_live"], T["n_obs"]
    n_mp, n = len(live), len(mp_index)
    outcome, kp, other = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    erased_rows, erased_into, counts = [], [], np.zeros(8, np.int32)
    note = dict(track_transfer=0, track_both=0, track_outside=0, ties=0, gained_then_2=0, loser_later_1=0, winner_later_loses=0, unlisted_then_3=0)
    gained_k, views_done = set(), 0
    for v, (K, first, count) in enumerate(views):
        stop, killed_here, unlisted_here = False, set(), set()
        for e in range(first, first + count):
            m = int(mp_index[e])
            row = kf_mp[K]
            if not live[m]:
                c = 1
                note["loser_later_1"] += m in killed_here
            elif (row == m).any():
                c = 2
                note["gained_then_2"] += (K, m) in gained_k
            elif not flags[m] & 2:
                c = 3
                note["unlisted_then_3"] += m in unlisted_here
            elif cand[e] < 0:
                c = 0
            else:
                k = int(cand[e])
                x = int(row[k])
                kp[e] = k
                if not 0 <= x < n_mp:
                    c = 4
                    row[k] = m
                    n_obs[m] += 1
                else:
                    other[e] = x
                    if n_obs[m] < n_obs[x]:
                        if not flags[x] & 2:
                            c = 5
                            n_obs[x] -= 1
                            row[k] = m
                            n_obs[m] += 1
                            unlisted_here.add(x)
                        else:
                            c, l, w = 6, m, x
                    else:
                        note["ties"] += n_obs[m] == n_obs[x]
                        c, l, w = 7, x, m
                        killed_here.add(x)
                    if c >= 6:
                        note["winner_later_loses"] += l in erased_into
                        g = replace_tables(T, l, w, note)
                        gained_k.update((s, w) for s in g)
                        stop = stop or source_slot in g
                        erased_rows.append(l)
                        erased_into.append(w)
            outcome[e] = c
            counts[c] += 1
        views_done = v + 1
        if stop and source_slot >= 0:
            break
    T.update(outcome=outcome, kp=kp, other=other, erased_rows=np.array(erased_rows, np.int32), erased_into=np.array(erased_into, np.int32), counts=counts,
             views_done=views_done, note=note)
    return T


def pair_outcomes(pairs):
    merged, out = set(), []
    for a, b in pairs:
        if a == b:
            out.append(1)
        elif a in merged or b in merged:
            out.append(2)
        else:
            merged.add(a)
            out.append(0)
    return np.array(out, np.uint8)


def replace_pairs_tables(T, pairs):
    T = copy_tables(T)
    out = pair_outcomes(pairs)
    rows, into = [], []
    for (a, b), o in zip(pairs, out):
        if o == 0:
            replace_tables(T, int(a), int(b))
            rows.append(a)
            into.append(b)
    T.update(outcome=out, erased_rows=np.array(rows, np.int32), erased_into=np.array(into, np.int32))
    return T


# ---- the sequential form --------------------------------------------------------------------------------------------------------------
class Map:
    """mapDB as the reference holds it, built from the tables: map_points[id] = dict(obs={slot: keypoint}, flags, track); keyframes[slot] =
    the mapPoints list; track_to_mp = trackIdToMapPoint (the tracks inside the window only: the tables know no others)."""

    def __init__(self, T):
        kf_mp, n_mp = T["kf_mp"], len(T["mp_live"])
        self.n_mp = n_mp
        self.keyframes = [[int(r) if 0 <= r < n_mp else -1 for r in row] for row in kf_mp]
        self.raw = kf_mp.copy()                              # what an entry held when it was no valid row: restored by to_tables
        tr = T.get("mp_track")
        self.map_points = {r: dict(obs={}, flags=int(T["mp_flags"][r]), track=int(tr[r]) if tr is not None else -1) for r in range(n_mp) if T["mp_live"][r]}
        for s, row in enumerate(self.keyframes):
            for j, r in enumerate(row):
                if r != -1:
                    self.map_points[r]["obs"][s] = j         # the invariants: listed rows are live, a slot lists a row once
        self.has_tracks = tr is not None
        self.dead_tracks = {r: int(tr[r]) for r in range(n_mp)} if tr is not None else {}
        self.track_base = T.get("track_base", 0)
        self.track_to_mp = {}
        if tr is not None:
            for i, r in enumerate(T["track_row"]):
                self.track_to_mp[i + self.track_base] = int(r)
        self.gained = set()                                  # the slots in which a replaceWith put the winner where it was not listed

    def replace_with(self, this, other):
        if this == other:
            return
        a, b = self.map_points[this], self.map_points[other]
        if a["track"] != -1:
            if b["track"] == -1:
                if a["track"] in self.track_to_mp:
                    self.track_to_mp[a["track"]] = other
                b["track"] = a["track"]
            # else trackIdToMapPoint.erase: the window keeps the dead row, which 9.11's PRESENT rule reads as erased
        for s, j in a["obs"].items():
            if s not in b["obs"]:
                self.keyframes[s][j] = other
                b["obs"][s] = j
                self.gained.add(s)
            else:
                self.keyframes[s][j] = -1
        self.dead_tracks[this] = a["track"]
        del self.map_points[this]

    def to_tables(self):
        kf_mp = self.raw.copy()
        for s, row in enumerate(self.keyframes):
            for j, r in enumerate(row):
                if r != -1 or 0 <= kf_mp[s, j] < self.n_mp:
                    kf_mp[s, j] = r
        live = np.zeros(self.n_mp, np.uint8)
        flags = np.zeros(self.n_mp, np.uint8)
        n_obs = np.zeros(self.n_mp, np.int32)
        for r, mp in self.map_points.items():
            live[r], flags[r], n_obs[r] = 1, mp["flags"], len(mp["obs"])
        out = dict(kf_mp=kf_mp, mp_live=live, mp_flags=flags, n_obs=n_obs)
        if self.has_tracks:
            out["mp_track"] = np.array([self.map_points[r]["track"] if r in self.map_points else self.dead_tracks[r] for r in range(self.n_mp)], np.int32)
            out["track_row"] = np.array([self.track_to_mp[i + self.track_base] for i in range(len(self.track_to_mp))], np.int32)
        return out


def fuse_sequential(T, mp_index, views, cand, source_slot=-1):
    """replaceDuplication per view on a Map built from the tables.  A row that was dead before the call is skipped where the reference would
    throw (code 1).  The early stop is the caller's re-read of currentKeyframe.mapPoints, stated here as in the tables form."""
    M = Map(T)
    pre_dead = T["mp_live"] == 0
    pre_flags = T["mp_flags"].copy()
    n = len(mp_index)
    outcome, kp, other = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    erased_rows, erased_into, counts, views_done = [], [], np.zeros(8, np.int32), 0
    for v, (K, first, count) in enumerate(views):
        kf = M.keyframes[K]
        erased = set()
        M.gained.clear()
        for e in range(first, first + count):
            mp_id = int(mp_index[e])
            if mp_id in erased or mp_id not in M.map_points:                     # :429
                c = 1
            else:
                mp = M.map_points[mp_id]
                if K in mp["obs"]:                                                # :434
                    c = 2
                elif not mp["flags"] & 2:                                         # :438
                    c = 3
                elif cand[e] < 0:                                                 # the gates, :497
                    c = 0
                else:
                    best = int(cand[e])
                    kp[e] = best
                    matched = kf[best]
                    if matched == -1:                                             # :502
                        c = 4
                        mp["obs"][K] = best
                        kf[best] = mp_id
                        M.raw[K, best] = -1                                       # whatever non-row the entry held is overwritten
                    else:
                        other[e] = matched
                        mm = M.map_points[matched]
                        if len(mp["obs"]) < len(mm["obs"]):
                            if not mm["flags"] & 2:                               # the tables' reading of :511: see DESIGN 9.12
                                c = 5
                                del mm["obs"][K]
                                kf[best] = mp_id
                                mp["obs"][K] = best
                            else:
                                c = 6
                                M.replace_with(mp_id, matched)
                                erased_rows.append(mp_id)
                                erased_into.append(matched)
                            erased.add(mp_id)
                        else:
                            c = 7
                            M.replace_with(matched, mp_id)
                            erased.add(matched)
                            erased_rows.append(matched)
                            erased_into.append(mp_id)
            outcome[e] = c
            counts[c] += 1
        views_done = v + 1
        if source_slot >= 0 and source_slot in M.gained:
            break
    out = M.to_tables()
    out["mp_flags"] = np.where(out["mp_live"] != 0, out["mp_flags"], np.where(pre_dead, pre_flags, 0)).astype(np.uint8)
    out.update(outcome=outcome, kp=kp, other=other, erased_rows=np.array(erased_rows, np.int32), erased_into=np.array(erased_into, np.int32), counts=counts,
               views_done=views_done)
    return out


def replace_pairs_sequential(T, pairs):
    M = Map(T)
    pre_dead, pre_flags = T["mp_live"] == 0, T["mp_flags"].copy()
    merged, out, rows, into = set(), [], [], []
    for a, b in pairs:
        a, b = int(a), int(b)
        if a == b:
            out.append(1)
            continue
        if a in merged or b in merged:
            out.append(2)
            continue
        merged.add(a)
        M.replace_with(a, b)
        out.append(0)
        rows.append(a)
        into.append(b)
    res = M.to_tables()
    res["mp_flags"] = np.where(res["mp_live"] != 0, res["mp_flags"], np.where(pre_dead, pre_flags, 0)).astype(np.uint8)
    res.update(outcome=np.array(out, np.uint8), erased_rows=np.array(rows, np.int32), erased_into=np.array(into, np.int32))
    return res


TABLE_KEYS = ("kf_mp", "mp_live", "mp_flags", "n_obs", "mp_track", "track_row")
LIST_KEYS = ("outcome", "kp", "other", "erased_rows", "erased_into", "counts")


def same(a, b, keys):
    return [k for k in keys if (a.get(k) is None) != (b.get(k) is None) or (a.get(k) is not None and not np.array_equal(a[k], b[k]))]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def make_tables(rng, n_kf, stride, n_mp, per_slot, empty=(), tracks=True, dead=0.1):
    """Tables that keep the invariants: listed rows are live, a slot lists a row once.  Besides -1 the non-valid entries are n_mp and n_mp + 1."""
    live = (rng.random(n_mp) >= dead).astype(np.uint8)
    flags = rng.choice(np.array([0, 1, 2, 3], np.uint8), n_mp, p=[0.1, 0.15, 0.25, 0.5])
    kf_mp = np.full((n_kf, stride), -1, np.int32)
    alive = np.nonzero(live)[0]
    for s in range(n_kf):
        if s in empty:
            continue
        n = min(per_slot, stride, len(alive))
        kf_mp[s, rng.permutation(stride)[:n]] = rng.permutation(alive)[:n]
        free = np.nonzero(kf_mp[s] == -1)[0]
        junk = free[rng.random(len(free)) < 0.05]
        kf_mp[s, junk] = n_mp + rng.integers(0, 2, len(junk))
    T = dict(kf_mp=kf_mp, mp_flags=flags, mp_live=live, n_obs=observation_count(kf_mp, n_mp))
    if tracks:
        base, n_track = 100, max(n_mp // 2, 1)
        track = np.full(n_mp, -1, np.int32)
        owners = rng.permutation(n_mp)[: (3 * n_mp) // 5]
        ids = base - n_mp // 10 + rng.permutation(n_mp)[: len(owners)]          # a tenth below the window, a part above it
        track[owners] = ids
        row = np.full(n_track, -1, np.int32)
        for r, t in zip(owners, ids):
            if 0 <= t - base < n_track:
                row[t - base] = r
        T.update(mp_track=track, track_row=row, track_base=base)
    return T


def make_views(rng, T, slots, counts, with_cand=0.85):
    """Views over `slots` with `counts` distinct rows each (drawn from all rows: dead ones, rows K lists and rows of any flags included) and a
    synthetic candidate for with_cand of the entries."""
    n_mp, stride = len(T["mp_live"]), T["kf_mp"].shape[1]
    mp_index, views, first = [], [], 0
    for slot, count in zip(slots, counts):
        mp_index.append(rng.permutation(n_mp)[:count])
        views.append((int(slot), first, int(count)))
        first += count
        if count and rng.random() < 0.5:                     # a gap of entries that belong to no view
            gap = int(rng.integers(1, 4))
            mp_index.append(rng.integers(0, n_mp, gap))
            first += gap
    mp_index = np.concatenate(mp_index).astype(np.int32) if mp_index else np.zeros(0, np.int32)
    cand = np.full(len(mp_index), -1, np.int32)
    for slot, f, c in views:
        has = rng.random(c) < with_cand
        cand[f:f + c][has] = rng.integers(0, stride, int(has.sum()))
    return mp_index, views, cand


def make_scene(seed=5, n_kf=40, stride=640, n_mp=3000, empty=(7, 19, 33), counts=(2700, 300, 1100, 0, 500, 200), per_slot=320, source_slot=39):
    """The base scene: 40 slots (3 empty), stride 640, 3 000 rows, 6 views (one empty; the first with more candidates than two trips).  The
    source slot is walked by no view."""
    rng = np.random.default_rng(seed)
    T = make_tables(rng, n_kf, stride, n_mp, per_slot, empty)
    slots = [s for s in rng.permutation(n_kf) if s not in empty and s != source_slot][: len(counts)]
    mp_index, views, cand = make_views(rng, T, slots, counts)
    kept_entry, top_idx, top_dist, n_kept = lists_from_candidates(rng, cand, views)
    return dict(T=T, mp_index=mp_index, views=views, cand=cand, kept_entry=kept_entry, top_idx=top_idx, top_dist=top_dist, n_kept=n_kept, max_dist=50,
                source_slot=source_slot)


def make_pairs(rng, T, n_pairs):
    """Pairs over live rows: chains (a -> b, b -> c), equal pairs, pairs the `merged` rule skips."""
    alive = rng.permutation(np.nonzero(T["mp_live"])[0])
    pairs, i = [], 0
    while len(pairs) < n_pairs and i + 3 < len(alive):
        a, b, c = (int(x) for x in alive[i:i + 3])
        i += 3
        how = rng.integers(0, 5)
        if how == 0:
            pairs += [(a, b), (b, c)]                        # a chain
        elif how == 1:
            pairs += [(a, a)]
        elif how == 2:
            pairs += [(a, b), (a, c)]                        # the second is skipped: a was merged
        elif how == 3:
            pairs += [(a, b), (c, a)]                        # skipped too
        else:
            pairs += [(a, b)]
    return np.array(pairs[:n_pairs], np.int32).reshape(-1, 2)


# ---- the whole deduplicateMapPoints chain on real geometry ---------------------------------------------------------------------------
def make_geometry_scene(seed=21, n_pairs=220, n_kf=7, stride=256, n_kp=150, n_adjacent=4):
    """A map whose points come in near-duplicate pairs (row p and row p + n_pairs: almost the same position, normal, distances and
    descriptor) over project_gate_ref's table, seen by n_kf - 1 keyframes near the origin (the last slot stays empty).  A keyframe's keypoints
    sit near the projections of points its FUSE gates keep, carry that point's descriptor a few bits off and are bound to the point, to its
    twin or to nothing -- a pair at most once per keyframe, so a slot lists a row once.  current = slot 0, adjacent = slots 1 .. n_adjacent."""
    import project_gate_ref as G
    rng = np.random.default_rng(seed)
    n_mp = 2 * n_pairs
    sf = G.scale_factors(8, 1.2)
    half = G.make_table(rng, n_pairs)
    flip = lambda n, p: ((np.uint32(1) << rng.integers(0, 32, (n, 8)).astype(np.uint32)) * (rng.random((n, 8)) < p)).astype(np.uint32)
    table = dict(pos=np.concatenate([half["pos"], half["pos"] + rng.normal(0, 2e-3, (n_pairs, 3))]), norm=np.concatenate([half["norm"]] * 2),
                 min_dist=np.concatenate([half["min_dist"]] * 2), max_dist=np.concatenate([half["max_dist"]] * 2),
                 desc=np.concatenate([half["desc"], half["desc"] ^ flip(n_pairs, 0.3)]))
    views_of, kfs = {}, {}
    kf_mp = np.full((n_kf, stride), -1, np.int32)
    everything = np.arange(n_mp, dtype=np.int32)
    for s in range(n_kf - 1):
        R, t = G.random_pose(rng)
        views_of[s] = dict(R=R, t=t, cam=G.CAM)
        g = G.gate_view(table, dict(views_of[s], threshold=3.0, mode=G.FUSE, indices=everything), sf, 1.2)
        kept_pairs = np.unique(g["kept"] % n_pairs)
        pairs = rng.permutation(kept_pairs)[:n_kp]
        src = np.array([p if g["status"][p] == G.KEPT else p + n_pairs for p in pairs])      # a kept member of the pair
        n = len(src)
        kfs[s] = dict(x=(g["x"][src] + rng.normal(0, 0.7, n)).astype(np.float32), y=(g["y"][src] + rng.normal(0, 0.7, n)).astype(np.float32),
                      desc=table["desc"][src] ^ flip(n, 0.3), octave=rng.integers(0, 8, n).astype(np.int32))
        how = rng.random(n)
        first = pairs if s == 0 else pairs + n_pairs         # the current keyframe mostly holds the first members, the others the twins
        second = pairs + n_pairs if s == 0 else pairs
        kf_mp[s, :n] = np.where(how < 0.55, first, np.where(how < 0.75, second, -1))
    live = np.ones(n_mp, np.uint8)
    listed = np.zeros(n_mp, bool)
    listed[kf_mp[kf_mp >= 0]] = True
    live[~listed & (rng.random(n_mp) < 0.5)] = 0
    flags = rng.choice(np.array([0, 1, 2, 3], np.uint8), n_mp, p=[0.05, 0.1, 0.25, 0.6])
    track = np.full(n_mp, -1, np.int32)
    owners = rng.permutation(n_mp)[: n_mp // 2]
    track[owners] = 40 + rng.permutation(n_mp)[: len(owners)]
    track_row = np.full(300, -1, np.int32)
    for r in owners:
        if 0 <= track[r] - 50 < 300:
            track_row[track[r] - 50] = r
    T = dict(kf_mp=kf_mp, mp_flags=flags, mp_live=live, n_obs=observation_count(kf_mp, n_mp), mp_track=track, track_row=track_row, track_base=50)
    return dict(T=T, table=table, views_of=views_of, kfs=kfs, sf=sf, scale_factor=1.2, current=0, adjacent=list(range(1, 1 + n_adjacent)), margin=3.0, everything=everything)


def geometry_candidates(scene, slot, rows):
    """replaceDuplication's gates and descriptor search (:442-499) for `rows` against keyframe `slot`, by the gate and score restatements of
    project_gate_ref: per row the best keypoint inside the radius (the first of the radius query's order at the smallest distance) when its
    distance is <= 50, else -1."""
    import project_gate_ref as G
    view = dict(scene["views_of"][slot], threshold=scene["margin"], mode=G.FUSE, indices=rows)
    g = G.gate_view(scene["table"], view, scene["sf"], scene["scale_factor"])
    kf = scene["kfs"][slot]
    fs = G.FeatureSearch(kf["x"], kf["y"])
    cand = np.full(len(rows), -1, np.int32)
    for k in g["kept"]:
        mp = scene["table"]["desc"][int(rows[k])]
        best, best_idx = 256, -1
        for j in fs.around(g["x"][k], g["y"][k], g["radius"][k]):
            d = G.hamming(mp, kf["desc"][j])
            if d < best:
                best, best_idx = d, int(j)
        if best_idx != -1 and best <= 50:
            cand[k] = best_idx
    return cand, g["near_level"]


def deduplicate_sequential(scene):
    """deduplicateMapPoints (mapper_helpers.cpp:320-347): replaceDuplication per adjacent keyframe from the current keyframe's list AS IT IS
    THEN, then the ascending union of the adjacent keyframes' rows against the current keyframe.  Each replaceDuplication is fuse_sequential
    on one view.  Returns the tables, the erased rows and winners in order, the counts, `changes` = how many of the adjacent keyframes
    found the current list changed by their predecessor's replaces, and near = the near_level entries met (must be 0 for an exact test)."""
    T = copy_tables(scene["T"])
    n_mp = len(T["mp_live"])
    erased_rows, erased_into, counts, changes, near = [], [], np.zeros(8, np.int32), 0, 0

    def one(slot, rows):
        nonlocal T, near
        cand, near_level = geometry_candidates(scene, slot, rows)
        near += int(near_level.sum())
        out = fuse_sequential(T, rows, [(slot, 0, len(rows))], cand, -1)
        erased_rows.extend(out["erased_rows"].tolist()); erased_into.extend(out["erased_into"].tolist())
        counts[:] += out["counts"]
        T = {k: out.get(k, T.get(k)) for k in TABLE_KEYS + ("track_base",)}

    before = None
    for slot in scene["adjacent"]:
        row = T["kf_mp"][scene["current"]]
        rows = row[(row >= 0) & (row < n_mp)].astype(np.int32)
        gained = before is not None and len(set(rows.tolist()) - before) > 0
        changes += gained
        before = set(rows.tolist())
        one(slot, rows)
    adj = T["kf_mp"][scene["adjacent"]]
    one(scene["current"], np.unique(adj[(adj >= 0) & (adj < n_mp)]).astype(np.int32))
    T.update(erased_rows=np.array(erased_rows, np.int32), erased_into=np.array(erased_into, np.int32), counts=counts, changes=changes, near=near)
    return T
