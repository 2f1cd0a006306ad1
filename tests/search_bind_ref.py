"""The specification of ms_bound_mask and ms_search_bind, in two forms that tests/test_search_bind_ref.py holds equal:

  sequential()   the literal loop of searchByProjection (keyframe_matcher.cpp:349-389) behind its gates: per kept query the radius query, the scan
                 over the keypoints that carry no map point in a MUTABLE kf.mapPoints, the accept rule, and both addObservations
                 (kf.mapPoints[best] = m, observations[m][K] = best).
  tables()       what the device runs: the top-4 lists of ms_projection_topk scored once against the initial mask, the walk over them with a
                 `taken` mark per keypoint, the rescan of a query whose list ran out, kf_mp / n_obs updated in place, and the outcome codes
                 (0 no candidate, 1 too far, 2 ratio, 3 bound from the list, 4 bound after a rescan; a rescan that binds nothing sets bit 3).

score_lists() restates ms_projection_topk (float32 radius query, (distance, position) order).  The scenes: make_matcher_scene of
project_gate_ref never rescans, so clustered_scene() packs eight queries and eight keypoints into a few pixels, with crafted clusters that
reach the rescan codes 8, 9 and 10 and lane-settled queries (0, 1) in every trip of 1024 queries; band_scene() is one query whose y band holds
every keypoint."""
import numpy as np

import project_gate_ref as G

F = np.float32
TRIP = 1024                                                  # queries per trip of the walk, positions per pass of a rescan, keypoints per trip of the marks
THR_HIGH = 100
NO_WINDOW = G.NO_WINDOW
CODES = (0, 1, 2, 3, 4, 8, 9, 10)


def bound_mask(kf_mp, slot, n_kp, n_mp):
    """ms_bound_mask: 1 where keypoint j of the slot carries a row of the table."""
    return (kf_mp[slot, :n_kp].astype(np.uint32) < np.uint32(n_mp)).astype(np.uint8)


def popcount_rows(a):
    return np.unpackbits(np.ascontiguousarray(a, np.uint32).view(np.uint8).reshape(len(a), -1), axis=1).sum(axis=1).astype(np.int32)


def band(fs, x, y, r):
    """The radius query of k_projection_candidates: sorted positions inside the y band and the circle, float32, every operation rounded."""
    x, y, r = F(x), F(y), F(r)
    lo = int(np.searchsorted(fs.y, y - r, side="left"))
    hi = int(np.searchsorted(fs.y, y + r, side="right"))
    dx = x - fs.x[lo:hi]; dy = y - fs.y[lo:hi]
    return lo + np.flatnonzero((dx * dx + dy * dy) < r * r)


def scored(S, q, mark):
    """(keys, keypoints) of query q over the keypoints with mark == 0 inside its octave window, in (distance, position) order."""
    fs, kf = S["fs"], S["kf"]
    pos = band(fs, S["q_x"][q], S["q_y"][q], S["q_radius"][q])
    j = fs.order[pos]
    ok = (mark[j] == 0) & (kf["octave"][j] >= S["q_min_octave"][q]) & (kf["octave"][j] <= S["q_max_octave"][q])
    pos, j = pos[ok], j[ok]
    d = popcount_rows(kf["desc"][j] ^ S["q_desc"][q][None, :]) if len(j) else np.zeros(0, np.int32)
    key = d.astype(np.int64) * (1 << 20) + pos
    o = np.argsort(key, kind="stable")
    return key[o], j[o]


def score_lists(S, skip):
    """ms_projection_topk for the scene's kept queries against `skip`: top_idx, top_dist, top_octave [n, 4], n_scored [n]."""
    n = S["n_kept"]
    ti = np.full((n, 4), -1, np.int32); td = np.full((n, 4), 256, np.uint16); to = np.full((n, 4), -1, np.int32); ns = np.zeros(n, np.int32)
    for q in range(n):
        key, j = scored(S, q, skip)
        k = min(4, len(j))
        ti[q, :k] = j[:k]; td[q, :k] = key[:k] >> 20; to[q, :k] = S["kf"]["octave"][j[:k]]; ns[q] = len(j)
    return dict(top_idx=ti, top_dist=td, top_octave=to, n_scored=ns)


def decide(best, bd, bd2, bl, bl2):
    if best < 0:
        return 0
    if bd > THR_HIGH:
        return 1
    if bl == bl2 and bd > 0.8 * bd2:
        return 2
    return 3


def tables(S, lists=None, skip=None):
    """The walk on copies of the tables.  Returns kf_mp, n_obs, match_kp [count], outcome [count], usable [n_kp] (from all ones), counts [6],
    n_matched and note: stepped queries, queries with a taken list entry, rescans per trip."""
    K, first, n_kp = S["slot"], S["first"], S["n_kp"]
    kf_mp, n_obs = S["kf_mp"].copy(), S["n_obs"].copy()
    skip = bound_mask(kf_mp, K, n_kp, S["n_mp"]) if skip is None else skip
    L = score_lists(S, skip) if lists is None else lists
    ti, td, to, ns = L["top_idx"], L["top_dist"], L["top_octave"], L["n_scored"]
    oct_ = S["kf"]["octave"]
    taken = np.zeros(n_kp, np.uint8)
    match_kp = np.full(S["count"], -1, np.int32); outcome = np.zeros(S["count"], np.uint8); usable = np.ones(n_kp, np.uint8)
    counts = np.zeros(6, np.int32)
    note = dict(stepped=0, conflicts=0, rescans=0)
    for q in range(S["n_kept"]):
        e = int(S["kept_entry"][q]); m = int(S["mp_index"][e])
        if ti[q, 0] < 0 or td[q, 0] > THR_HIGH:              # settled without a step: every candidate, free or not, is at least that far
            c = 0 if ti[q, 0] < 0 else 1
            outcome[q] = c; counts[c] += 1
            continue
        note["stepped"] += 1
        listed = [k for k in range(4) if ti[q, k] >= 0]
        free = [k for k in listed if not taken[ti[q, k]]][:2]
        note["conflicts"] += any(taken[ti[q, k]] for k in listed)
        best, bd, bl = (int(ti[q, free[0]]), int(td[q, free[0]]), int(to[q, free[0]])) if free else (-1, 256, -1)
        bd2, bl2 = (int(td[q, free[1]]), int(to[q, free[1]])) if len(free) > 1 else (256, -1)
        again = len(free) < 2 and ns[q] > 4
        if again:
            note["rescans"] += 1; counts[5] += 1
            key, j = scored(S, q, skip | taken)
            best, bd, bl = (int(j[0]), int(key[0] >> 20), int(oct_[j[0]])) if len(j) else (-1, 256, -1)
            bd2, bl2 = (int(key[1] >> 20), int(oct_[j[1]])) if len(j) > 1 else (256, -1)
        c = decide(best, bd, bd2, bl, bl2)
        counts[c + (c == 3 and again)] += 1
        if c < 3:
            outcome[q] = c | 8 if again else c
            continue
        outcome[q] = 4 if again else 3
        kf_mp[K, best] = m; n_obs[m] += 1; match_kp[e - first] = best; taken[best] = 1; usable[best] = 0
    return dict(kf_mp=kf_mp, n_obs=n_obs, match_kp=match_kp, outcome=outcome, usable=usable, counts=counts, n_matched=int((match_kp >= 0).sum()), note=note,
                lists=L, skip=skip)


def sequential(S):
    """The reference's loop as it stands.  Returns (matches [(entry, keypoint)] in walk order, kf.mapPoints of K, observations {row: {K: keypoint}})."""
    K, n_kp, fs, kf = S["slot"], S["n_kp"], S["fs"], S["kf"]
    map_points = [int(r) if 0 <= r < S["n_mp"] else -1 for r in S["kf_mp"][K, :n_kp]]
    observations, matches = {}, []
    for q in range(S["n_kept"]):
        e = int(S["kept_entry"][q]); m = int(S["mp_index"][e])
        best, best2, lvl, lvl2, best_idx = 256, 256, -1, -1, -1
        for pos in band(fs, S["q_x"][q], S["q_y"][q], S["q_radius"][q]):
            j = int(fs.order[pos])
            if map_points[j] != -1:                          # :358-360
                continue
            if kf["octave"][j] < S["q_min_octave"][q] or kf["octave"][j] > S["q_max_octave"][q]:
                continue
            d = G.hamming(S["q_desc"][q], kf["desc"][j])
            if d < best:
                best2, best, lvl2, lvl, best_idx = best, d, lvl, int(kf["octave"][j]), j
            elif d < best2:
                lvl2, best2 = int(kf["octave"][j]), d
        if best_idx == -1 or best > THR_HIGH:
            continue
        if lvl == lvl2 and best > 0.8 * best2:
            continue
        map_points[best_idx] = m                             # :388
        observations.setdefault(m, {})[K] = best_idx         # :389
        matches.append((e, best_idx))
    return matches, map_points, observations


def agree(S, t, seq):
    """[] when the tables form `t` says what the sequential form `seq` says."""
    matches, map_points, observations = seq
    bad = []
    K, n_kp = S["slot"], S["n_kp"]
    want_row = np.array(map_points, np.int64)
    got_row = np.where(t["kf_mp"][K, :n_kp].astype(np.uint32) < S["n_mp"], t["kf_mp"][K, :n_kp], -1)
    if not np.array_equal(want_row, got_row):
        bad.append("kf_mp[K]")
    if [(int(e), int(t["match_kp"][e - S["first"]])) for e in S["kept_entry"][:S["n_kept"]] if t["match_kp"][e - S["first"]] >= 0] != matches:
        bad.append("matches")
    n_obs = S["n_obs"].copy()
    for m in observations:
        n_obs[m] += 1
    if not np.array_equal(n_obs, t["n_obs"]):
        bad.append("n_obs")
    other = np.arange(S["kf_mp"].shape[0]) != K
    if not np.array_equal(S["kf_mp"][other], t["kf_mp"][other]) or not np.array_equal(S["kf_mp"][K, n_kp:], t["kf_mp"][K, n_kp:]):
        bad.append("other slots")
    return bad


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def low_bits(k):
    """A descriptor mask with exactly k bits set."""
    out = np.zeros(8, np.uint32)
    for w in range(8):
        b = min(32, max(0, k - 32 * w))
        out[w] = 0xFFFFFFFF if b == 32 else (1 << b) - 1
    return out


def finish(rng, kf, qx, qy, qr, qd, stride, pre_bound, n_kf=3, slot=1, gated_out=7):
    """Tables and lists around a keyframe and its kept queries (already in walk order)."""
    n_kp, n_q = len(kf["x"]), len(qx)
    count, first = n_q + gated_out, 5
    kept_entry = first + np.sort(rng.permutation(count)[:n_q]).astype(np.int32)
    n_bound = int(pre_bound.sum())
    n_mp = count + n_bound + 40
    rows = rng.permutation(n_mp).astype(np.int32)
    mp_index = np.concatenate([rng.integers(0, n_mp, first), rows[:count], rng.integers(0, n_mp, 3)]).astype(np.int32)
    kf_mp = np.full((n_kf, stride), -1, np.int32)
    kf_mp[slot, np.flatnonzero(pre_bound)] = rows[count:count + n_bound]
    for s in range(n_kf):
        if s != slot:
            k = min(stride, n_mp) // 2
            kf_mp[s, rng.permutation(stride)[:k]] = rng.permutation(n_mp)[:k]
    kf_mp[slot, rng.permutation(np.flatnonzero(~pre_bound))[:3]] = (n_mp, n_mp + 7, -5)      # entries outside the table count as none
    mp_live = np.ones(n_mp, np.uint8)
    mp_live[rows[count + n_bound:count + n_bound + 20]] = 0
    n_obs = np.where(mp_live > 0, rng.integers(1, 6, n_mp), 0).astype(np.int32)
    S = dict(kf=kf, fs=G.FeatureSearch(kf["x"], kf["y"]), n_kp=n_kp, stride=stride, n_kf=n_kf, slot=slot, n_mp=n_mp, kf_mp=kf_mp, mp_live=mp_live, n_obs=n_obs,
             mp_index=mp_index, first=first, count=count, n_kept=n_q, kept_entry=kept_entry,
             q_x=np.asarray(qx, F), q_y=np.asarray(qy, F), q_radius=np.asarray(qr, F), q_desc=np.ascontiguousarray(qd, np.uint32),
             q_min_octave=np.full(n_q, NO_WINDOW[0], np.int32), q_max_octave=np.full(n_q, NO_WINDOW[1], np.int32))
    return S


def clustered_scene(n_clusters, seed, stride=None, n_kp=None, lead_settled=0):
    """n_clusters clusters of 8 queries and 8 keypoints (see the module text); per trip of the walk three crafted clusters (E: five keypoints
    that five queries bind, the other three rescan and find nothing, code 8; N: four bound, then the rescans find only noise, code 9; R: four
    bound, then the rescans end in the ratio test, code 10), three isolated queries (code 0) and three noise queries (code 1).  The crafted
    clusters' queries stay inside their trip; all others are shuffled over the whole walk.  lone keypoints fill up to n_kp; lead_settled queries
    that settle without a step are put in front."""
    rng = np.random.default_rng(seed)
    n_q = 8 * n_clusters
    trips = -(-(n_q + lead_settled) // TRIP)
    flip = lambda n, p: ((np.uint32(1) << rng.integers(0, 32, (n, 8)).astype(np.uint32)) * (rng.random((n, 8)) < p)).astype(np.uint32)
    rnd = lambda n: rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    kx, ky, kd, ko, free_kp = [], [], [], [], []
    qx, qy, qr, qd, qtrip = [], [], [], [], []
    special = []
    for t in range(trips):
        for kind in "ENR":
            if 8 * (len(special) + 1) <= n_q and min((t + 1) * TRIP, n_q + lead_settled) - max(t * TRIP, lead_settled) >= 40:
                special.append((t, kind))
    for c in range(n_clusters):
        base = rnd(1)[0]
        if c < len(special):
            t, kind = special[c]
            cx, cy = 560.0 + 40.0 * (c % 2), 30.0 + 36.0 * (c // 2)
            bits = dict(E=(0, 8, 16, 24, 32), N=(0, 8, 16, 24, 128, 136), R=(0, 8, 16, 24, 40, 44))[kind]
            for i, b in enumerate(bits):
                kx.append(cx + rng.uniform(-2, 2)); ky.append(cy + rng.uniform(-2, 2)); kd.append(base ^ low_bits(b)); ko.append(i % 3 if i < 4 else 1)
                free_kp.append(False)
            for _ in range(8):
                qx.append(cx); qy.append(cy); qr.append(8.0); qd.append(base); qtrip.append(t)
            continue
        cx, cy = rng.uniform(20, 520), rng.uniform(20, 460)
        ang, rad = rng.uniform(0, 2 * np.pi, 8), rng.uniform(0, 3, 8)
        kx += list(cx + rad * np.cos(ang)); ky += list(cy + rad * np.sin(ang)); kd += list(base ^ flip(8, 0.3)); ko += list(rng.integers(0, 3, 8))
        free_kp += [True] * 8
        qx += list(cx + rng.normal(0, 1, 8)); qy += list(cy + rng.normal(0, 1, 8)); qr += list(rng.uniform(6, 12, 8)); qd += list(base ^ flip(8, 0.3))
        qtrip += [-1] * 8
    for _ in range(max(0, (n_kp or 0) - len(kx))):
        kx.append(rng.uniform(20, 520)); ky.append(rng.uniform(20, 460)); kd.append(rnd(1)[0]); ko.append(int(rng.integers(0, 3))); free_kp.append(True)
    qx, qy, qr, qd, qtrip = np.array(qx), np.array(qy), np.array(qr), np.array(qd, np.uint32), np.array(qtrip)
    # the walk order: crafted queries at random places of their trip, the others shuffled over what is left
    total = n_q + lead_settled
    order = np.full(total, -1, np.int64)
    order[:lead_settled] = -2
    for t in range(trips):
        mine = np.flatnonzero(qtrip == t)
        lo, hi = max(t * TRIP, lead_settled), min((t + 1) * TRIP, total)
        order[lo + rng.permutation(hi - lo)[:len(mine)]] = rng.permutation(mine)
    order[order == -1] = rng.permutation(np.flatnonzero(qtrip == -1))
    lead = order == -2
    src = np.where(lead, 0, order)
    QX, QY, QR, QD = qx[src], qy[src], qr[src], qd[src].copy()
    ordinary = np.flatnonzero((qtrip[src] == -1) & ~lead)
    # settled queries: the leading ones, and six ordinary ones per trip -- alternately isolated (no keypoint in range) and noise (the
    # cluster's descriptor with 160 bits turned over, so every keypoint of the cluster is farther than 100)
    settle = list(np.flatnonzero(lead))
    for t in range(trips):
        inside = ordinary[(ordinary >= t * TRIP) & (ordinary < (t + 1) * TRIP)]
        settle += list(rng.permutation(inside)[:6])
    for i, p in enumerate(settle):
        if lead[p]:
            s = int(rng.permutation(np.flatnonzero(qtrip == -1))[0])
            QX[p], QY[p], QR[p], QD[p] = qx[s], qy[s], qr[s], qd[s]
        if i % 2 == 0:
            QX[p], QY[p] = 632.0, rng.uniform(20, 460)
        else:
            QD[p] = QD[p] ^ low_bits(160)
    kf = dict(x=np.array(kx, F), y=np.array(ky, F), desc=np.array(kd, np.uint32), octave=np.array(ko, np.int32))
    pre_bound = np.array(free_kp) & (rng.random(len(kx)) < 0.1)
    S = finish(rng, kf, QX, QY, QR, QD, stride or len(kx), pre_bound)
    S["lead_settled"] = lead_settled
    return S


def band_scene(seed=5, n_kp=2100):
    """One y band that holds every keypoint (sorted position = keypoint index, three passes of 1024).  Queries 0-2 bind the main query's three
    best keypoints A, B, C; the main query (3) finds one free list entry (D), has n_scored = n_kp and rescans: best D in the second pass,
    second E in the third.  Query 4 finds all four list entries taken, rescans too and binds E."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)
    x = rng.uniform(20, 620, n_kp); y = 195.0 + 10.0 * np.arange(n_kp) / n_kp
    desc = base[None, :] ^ low_bits(128)[None, :] ^ (rng.integers(0, 2 ** 32, (n_kp, 8), dtype=np.uint64).astype(np.uint32) & np.uint32(0x0F0F0000))
    octave = rng.integers(0, 3, n_kp).astype(np.int32)
    spots = dict(A=(100, 0), B=(200, 1), C=(300, 2), D=(1500, 3), E=(2090, 10), F=(50, 12))
    for name, (i, bits) in spots.items():
        desc[i] = base ^ low_bits(bits)
    octave[[100, 200, 300, 1500, 2090, 50]] = (0, 1, 2, 0, 1, 2)
    kf = dict(x=x.astype(F), y=y.astype(F), desc=desc, octave=octave)
    qx = [x[100], x[200], x[300], 320.0, 320.0]; qy = [y[100], y[200], y[300], 200.0, 200.0]; qr = [3.0, 3.0, 3.0, 400.0, 400.0]
    qd = [desc[100], desc[200], desc[300], base, base ^ low_bits(3)]
    S = finish(rng, kf, qx, qy, qr, qd, n_kp + 12, np.zeros(n_kp, bool), gated_out=2)
    S["spots"] = {k: v[0] for k, v in spots.items()}
    return S


def matcher_scene(seed=77):
    """make_matcher_scene's SEARCH view with tables around it: (scene of project_gate_ref, its keyframe, S without lists or queries -- the
    device chain makes them).  Slot K's row carries the scene's `bound` keypoints."""
    sc, kfs, bound = G.make_matcher_scene(seed)
    rng = np.random.default_rng(seed + 1000)
    kf, view = kfs[0], sc["views"][0]
    b = np.flatnonzero(bound)
    n_kp, n_mp = len(kf["x"]), len(sc["table"]["pos"]) + len(b) + 9      # the keyframe table knows more rows than the view walks
    kf_mp = np.full((3, 512), -1, np.int32)
    kf_mp[1, b] = len(sc["table"]["pos"]) + rng.permutation(len(b) + 9)[:len(b)]
    kf_mp[0, :200] = rng.permutation(n_mp)[:200]
    n_obs = rng.integers(1, 6, n_mp).astype(np.int32)
    g, idx = sc["ref"][0], np.asarray(view["indices"], np.int32)
    kept = g["kept"]
    S = dict(kf=kf, fs=G.FeatureSearch(kf["x"], kf["y"]), n_kp=n_kp, stride=512, n_kf=3, slot=1, n_mp=n_mp, kf_mp=kf_mp, mp_live=np.ones(n_mp, np.uint8), n_obs=n_obs,
             bound=bound, mp_index=idx, first=0, count=len(idx), n_kept=len(kept), kept_entry=kept.astype(np.int32), q_x=g["x"][kept], q_y=g["y"][kept],
             q_radius=g["radius"][kept], q_desc=np.ascontiguousarray(sc["table"]["desc"][idx[kept]], np.uint32), q_min_octave=g["q_min_octave"],
             q_max_octave=g["q_max_octave"])
    return sc, kf, S


_SCENES = {}


def gpu_scene(name):
    """The scenes of tests/test_gpu_search_bind.py, each built once with its tables() result under 'want'."""
    make = dict(clustered=lambda: clustered_scene(340, 11, stride=2816), kp1100=lambda: clustered_scene(137, 12, n_kp=1100),
                kp2100=lambda: clustered_scene(262, 13, n_kp=2100, stride=2100), band=band_scene, lead=lambda: clustered_scene(40, 14, lead_settled=TRIP),
                small=lambda: clustered_scene(40, 15))
    if name not in _SCENES:
        S = make[name]()
        S["want"] = tables(S)
        _SCENES[name] = S
    return _SCENES[name]


GPU_SCENES = ("clustered", "kp1100", "kp2100", "band", "lead", "small")


def codes_per_trip(S, w):
    """Per trip of the walk the set of outcome codes of its queries."""
    return [set(w["outcome"][t:min(t + TRIP, S["n_kept"])].tolist()) for t in range(0, S["n_kept"], TRIP)]
