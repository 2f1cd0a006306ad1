"""numpy restatement of the map-point gates in front of the projection-guided matchers -- the specification of ms_project_gate.

The three loops (file:line relative to the reference tree):
  SEARCH  searchByProjection        keyframe_matcher.cpp:313-345  (Keyframe::isInFrustum, keyframe.cpp:247-262: the same gates, no radius)
  FUSE    replaceDuplication        keyframe_matcher.cpp:442-471
  SIM3    findMatchesTranformedMps  keyframe_matcher.cpp:573-596
Types as the reference has them: positions, poses and the pinhole projection in float64; mpToKf, the viewing distance of SEARCH / FUSE, the
cosine, predictScaleLevel (map_point.cpp:174-183) and the radius in float32, every operation rounded on its own, sums left to right.
numpy keeps float32 arrays in float32, so each line below is one rounded operation per element.

A view is a dict: R [3, 3] and t [3] float64 (p_c = R p + t; SIM3: rotBAW / transBAW, may carry a scale), cam = (fx, fy, cx, cy, width,
height), threshold (SEARCH: threshold, FUSE / SIM3: margin), view_cos_limit (SEARCH), mode, indices (rows of the table, in walk order).
The table is a dict: pos [n, 3] float64, norm [n, 3] float32, min_dist, max_dist [n] float32, desc [n, 8] uint32.

Also here: the sequential restatement of the whole searchByProjection loop (:313-400, binding and accept rule included), of
findMatchesTranformedMps (:564-631), and the scene generator the GPU tests draw from."""
import numpy as np

SEARCH, FUSE, SIM3 = 0, 1, 2
KEPT, NOT_VISIBLE, DISTANCE, ZERO_NORMAL, ANGLE = 0, 1, 2, 3, 4
NO_WINDOW = (-0x7fffffff, 0x7fffffff)
F = np.float32
CAM = (450.0, 450.0, 320.0, 240.0, 640, 480)


def camera_centre(R, t):
    """worldToCameraMatrixCameraCenter: -R^T t in float64, summed left to right."""
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    return np.array([-((R[0, j] * t[0] + R[1, j] * t[1]) + R[2, j] * t[2]) for j in range(3)])


def predict_level(max_dist, dist, scale_factor, n_levels):
    """MapPoint::predictScaleLevel on float32 arrays: (level, q in float32, ratio).  ceil of +inf -> n_levels - 1, of NaN -> 0 (the reference's
    conversion of those to int is undefined)."""
    with np.errstate(all="ignore"):
        ratio = (max_dist / dist).astype(F)
        q = (np.log(ratio) / np.log(F(scale_factor))).astype(F)
        cq = np.ceil(q)
    top = n_levels - 1
    level = np.zeros(len(q), np.int32)
    pos = cq > 0
    hi = pos & (cq >= F(top))
    mid = pos & ~hi
    level[hi] = top
    level[mid] = cq[mid].astype(np.int32)
    return level, q, ratio


def radius_of(mode, level, threshold, cos, sf):
    """The search radius in float32, left to right (:342, :470-471, :596)."""
    sf = np.asarray(sf, F); ref = len(sf) // 2
    thr = F(threshold)
    if mode == SEARCH:
        m = np.where(cos > F(0.998), F(0.625), F(1.0)).astype(F)
        return ((m * thr) * sf[level]) / sf[ref]
    if mode == FUSE:
        return ((thr * sf[level]) / sf[ref]) * F(2.4477)
    return thr * sf[level]


def near_level_mask(ratio, scale_factor):
    """Entries whose level may differ by one between two conforming logf implementations: |q - round(q)| <= 1e-5 max(1, |q|), q in float64
    from the float32 ratio.  (Two logf results of <= 1 ulp and one float division: ~4e-7 relative; 1e-5 is that with margin.)"""
    with np.errstate(all="ignore"):
        q = np.log(ratio.astype(np.float64)) / np.log(np.float64(F(scale_factor)))
        return np.abs(q - np.round(q)) <= 1e-5 * np.maximum(1.0, np.abs(q))


def gate_view(table, view, sf, scale_factor):
    """One view's loop over view['indices'].  Returns a dict of per-entry arrays: status, x, y, dist (float32; 0 where not visible), level
    (-1 unless kept), radius (0 unless kept), cos, near_level, and kept (positions in the view, walk order), q_min_octave / q_max_octave."""
    idx = np.asarray(view["indices"], np.int64).reshape(-1)
    n, mode, n_levels = len(idx), int(view["mode"]), len(sf)
    R = np.asarray(view["R"], np.float64).reshape(3, 3); t = np.asarray(view["t"], np.float64).reshape(3)
    fx, fy, cx, cy, w, h = view["cam"]
    p = np.asarray(table["pos"], np.float64).reshape(-1, 3)[idx]
    dmin = np.asarray(table["min_dist"], F)[idx]; dmax = np.asarray(table["max_dist"], F)[idx]
    out = dict(status=np.full(n, NOT_VISIBLE, np.uint8), x=np.zeros(n, F), y=np.zeros(n, F), dist=np.zeros(n, F), level=np.full(n, -1, np.int32),
               radius=np.zeros(n, F), cos=np.ones(n, F), near_level=np.zeros(n, bool))
    with np.errstate(all="ignore"):
        pc = [((R[i, 0] * p[:, 0] + R[i, 1] * p[:, 1]) + R[i, 2] * p[:, 2]) + t[i] for i in range(3)]
        u = fx * (pc[0] / pc[2]) + cx
        v = fy * (pc[1] / pc[2]) + cy
        vis = (pc[2] > 0) & (u >= 0) & (u < float(w)) & (v >= 0) & (v < float(h))
        out["x"][vis] = u[vis].astype(F); out["y"][vis] = v[vis].astype(F)
        if mode == SIM3:
            dd = np.sqrt((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2])
            in_range = ~((dd < dmin.astype(np.float64)) | (dmax.astype(np.float64) < dd))
            dist = dd.astype(F)
            cos = np.ones(n, F)
            zero = angle = np.zeros(n, bool)
        else:
            c = camera_centre(R, t)
            d = (c[None, :] - p).astype(F)
            dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            in_range = ~((dist < dmin) | (dmax < dist))
            nrm = np.asarray(table["norm"], F).reshape(-1, 3)[idx]
            cos = ((d[:, 0] / dist) * nrm[:, 0] + (d[:, 1] / dist) * nrm[:, 1]) + (d[:, 2] / dist) * nrm[:, 2]
            zero = (nrm == 0).all(axis=1) if mode == FUSE else np.zeros(n, bool)
            angle = cos < (F(view["view_cos_limit"]) if mode == SEARCH else F(0.5))
        out["dist"][vis] = dist[vis]
        status = np.where(~vis, NOT_VISIBLE, np.where(~in_range, DISTANCE, np.where(zero, ZERO_NORMAL, np.where(angle, ANGLE, KEPT)))).astype(np.uint8)
        out["status"] = status
        out["cos"] = cos.astype(F)
        k = status == KEPT
        level, _, ratio = predict_level(dmax, dist, scale_factor, n_levels)
        out["level"][k] = level[k]
        out["radius"][k] = radius_of(mode, level[k], view["threshold"], cos[k], sf).astype(F)
        out["near_level"] = k & near_level_mask(ratio, scale_factor)
    out["kept"] = np.flatnonzero(k).astype(np.int32)
    lv = out["level"][k]
    out["q_min_octave"] = (lv - 1 if mode == SIM3 else np.full(len(lv), NO_WINDOW[0])).astype(np.int32)
    out["q_max_octave"] = (lv if mode == SIM3 else np.full(len(lv), NO_WINDOW[1])).astype(np.int32)
    return out


def gate_one(table, view, sf, scale_factor, i=0):
    """(status, x, y, dist, level, radius) of entry i as python scalars."""
    g = gate_view(table, view, sf, scale_factor)
    return int(g["status"][i]), float(g["x"][i]), float(g["y"][i]), float(g["dist"][i]), int(g["level"][i]), float(g["radius"][i])


# ---- the loops behind the gates -------------------------------------------------------------------------------------------------
def hamming(a, b):
    return int(np.unpackbits((np.asarray(a, np.uint32) ^ np.asarray(b, np.uint32)).view(np.uint8)).sum())


class FeatureSearch:
    """feature_search.cpp:22-48: keypoints sorted by y (stable, as ms_feature_search_sort), the radius query in float32."""

    def __init__(self, x, y):
        self.order = np.argsort(np.asarray(y, F), kind="stable")
        self.x = np.asarray(x, F)[self.order]; self.y = np.asarray(y, F)[self.order]

    def around(self, x, y, r):
        x, y, r = F(x), F(y), F(r)
        lo = int(np.searchsorted(self.y, y - r, side="left"))
        hi = int(np.searchsorted(self.y, y + r, side="right"))
        dx = x - self.x[lo:hi]; dy = y - self.y[lo:hi]
        return self.order[lo:hi][(dx * dx + dy * dy) < r * r]


def search_by_projection(kf, bound, table, view, sf, scale_factor):
    """searchByProjection (:313-400), one map point after the other.  kf: dict x, y [n] float32, desc [n, 8] uint32, octave [n] int32;
    bound [n] uint8 marks keypoints that carry an observed map point (:358) and is updated in place.  Returns the match list
    [(position in view['indices'], keypoint index)] in walk order."""
    g = gate_view(table, view, sf, scale_factor)
    fs = FeatureSearch(kf["x"], kf["y"])
    desc = np.asarray(table["desc"], np.uint32).reshape(-1, 8)
    matches = []
    for k in g["kept"]:
        mp = desc[int(view["indices"][k])]
        best, best2, lvl, lvl2, best_idx = 256, 256, -1, -1, -1
        for j in fs.around(g["x"][k], g["y"][k], g["radius"][k]):
            if bound[j]:
                continue
            d = hamming(mp, kf["desc"][j])
            if d < best:
                best2, best, lvl2, lvl, best_idx = best, d, lvl, int(kf["octave"][j]), int(j)
            elif d < best2:
                lvl2, best2 = int(kf["octave"][j]), d
        if best_idx == -1 or best > 100:
            continue
        if lvl == lvl2 and best > 0.8 * best2:
            continue
        bound[best_idx] = 1
        matches.append((int(k), best_idx))
    return matches


def find_matches_transformed(kf, table, view, sf, scale_factor):
    """findMatchesTranformedMps (:564-631) for the entries of a SIM3 view: per entry the best keypoint inside the radius with octave in
    [level - 1, level], accepted at <= 100, or -1."""
    g = gate_view(table, view, sf, scale_factor)
    fs = FeatureSearch(kf["x"], kf["y"])
    desc = np.asarray(table["desc"], np.uint32).reshape(-1, 8)
    out = np.full(len(view["indices"]), -1, np.int32)
    for k in g["kept"]:
        mp, lv = desc[int(view["indices"][k])], int(g["level"][k])
        best, best_idx = 256, -1
        for j in fs.around(g["x"][k], g["y"][k], g["radius"][k]):
            if kf["octave"][j] < lv - 1 or kf["octave"][j] > lv:
                continue
            d = hamming(mp, kf["desc"][j])
            if d < best:
                best, best_idx = d, int(j)
        if best <= 100:
            out[k] = best_idx
    return out


def scale_factors(n_levels, scale_factor):
    """StaticSettings::scaleFactors (static_settings.cpp:9-20): a float32 product chain."""
    sf = np.ones(n_levels, F)
    for l in range(1, n_levels):
        sf[l] = F(scale_factor) * sf[l - 1]
    return sf


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def random_pose(rng, scale=1.0):
    """A camera near the origin looking down +z: small rotation, small translation; SIM3 views carry a scale."""
    w = rng.normal(0, 0.08, 3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    return scale * R, rng.normal(0, 0.3, 3)


def make_table(rng, n_mp, n_levels=8, scale_factor=1.2):
    """Map points around a camera at the origin: most in front and inside a 640 x 480 frustum, some outside, some behind; normals near the
    direction to the origin (some far off, some zero); [min, max] viewing distances around the true distance (some beside it)."""
    z = rng.uniform(1.5, 12.0, n_mp) * np.where(rng.random(n_mp) < 0.06, -1.0, 1.0)
    pos = np.stack([rng.uniform(-0.95, 0.95, n_mp) * np.abs(z), rng.uniform(-0.7, 0.7, n_mp) * np.abs(z), z], axis=1)
    d = np.linalg.norm(pos, axis=1)
    nrm = -pos / d[:, None] + rng.normal(0, 0.45, (n_mp, 3)) * (rng.random(n_mp) < 0.5)[:, None]
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm[rng.random(n_mp) < 0.05] = 0.0
    nrm[rng.random(n_mp) < 0.1] *= -1.0
    max_dist = d * rng.uniform(0.85, float(scale_factor) ** (n_levels - 1) * 1.2, n_mp)
    min_dist = max_dist / float(scale_factor) ** rng.uniform(n_levels - 4, n_levels + 1, n_mp)
    return dict(pos=pos, norm=nrm.astype(F), min_dist=min_dist.astype(F), max_dist=max_dist.astype(F),
                desc=rng.integers(0, 2 ** 32, (n_mp, 8), dtype=np.uint64).astype(np.uint32))


def make_views(rng, counts, modes, n_mp=1500, n_levels=8, scale_factor=1.2, special=None):
    """A scene for ms_project_gate: a table of n_mp map points and len(counts) views, view v with counts[v] entries in mode modes[v].
    special: {v: 'kept' | 'rejected'} draws view v's entries from the points its gates keep / reject (an all-kept / all-rejected view).
    Returns a dict: table, views, sf, scale_factor, ref (gate_view of every view) and near_level (the per-view masks back to back)."""
    sf = scale_factors(n_levels, scale_factor)
    table = make_table(rng, n_mp, n_levels, scale_factor)
    views = []
    for v, (cnt, mode) in enumerate(zip(counts, modes)):
        R, t = random_pose(rng, rng.uniform(0.9, 1.1) if mode == SIM3 else 1.0)
        view = dict(R=R, t=t, cam=CAM, threshold=float(rng.choice([7.5, 10.0, 15.0])) if mode != FUSE else 3.0,
                    view_cos_limit=0.5, mode=mode, indices=np.arange(n_mp, dtype=np.int32))
        want = (special or {}).get(v)
        if want:
            st = gate_view(table, view, sf, scale_factor)["status"]
            pool = np.flatnonzero(st == KEPT if want == "kept" else st != KEPT)
            view["indices"] = rng.choice(pool, cnt, replace=len(pool) < cnt).astype(np.int32)
        else:
            view["indices"] = rng.choice(n_mp, cnt, replace=cnt > n_mp).astype(np.int32)
        views.append(view)
    scene = dict(table=table, views=views, sf=sf, scale_factor=float(scale_factor))
    regate(scene)
    return scene


def regate(scene):
    """(Re)compute scene['ref'] and scene['near_level'] from the scene's table, views and scale factors."""
    scene["ref"] = [gate_view(scene["table"], v, scene["sf"], scene["scale_factor"]) for v in scene["views"]]
    scene["near_level"] = np.concatenate([r["near_level"] for r in scene["ref"]] + [np.zeros(0, bool)])
    return scene


def gpu_test_draws():
    """(seed, counts, modes, special) of every generator draw the GPU tests use; test_project_gate_ref.py holds each one's near_level share
    under 0.1 % of its entries (a condition on the INPUTS: a seed that breaks it is redrawn, the bound stays)."""
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
    draws = []
    for mode in (SEARCH, FUSE, SIM3):
        for s, n in enumerate(sizes):
            draws.append((100 * mode + s, [n], [mode], None))
        draws.append((100 * mode + 50, [300, 0, 257], [mode] * 3, {0: "kept", 2: "rejected"}))
        draws.append((100 * mode + 51, [(37 * i) % 130 for i in range(21)], [mode] * 21, {3: "kept", 7: "rejected"}))
    draws.append((900, [257, 0, 64, 1000, 65, 255], [SEARCH, FUSE, SIM3, FUSE, SEARCH, SIM3], {2: "kept", 4: "rejected"}))
    return draws


LARGE_TRIP = 256 * 256                                       # entries of a view whose workgroup counts k_gate_offsets scans in one trip
LARGE_N_MP = 3000


def large_draws():
    """(seed, counts, modes, special) of the draws whose long views have more workgroups than the 256 whose counts are scanned at a time; over
    LARGE_N_MP map points.  The first has a second trip of two workgroups, a view of exactly one trip and a short view; the second has the long
    view (one entry into its second trip) behind a short one, so that its workgroups do not start the block table.
    test_project_gate_ref.py holds near_level under 0.1 % of each and the kept entries on both sides of LARGE_TRIP."""
    return [(3, [LARGE_TRIP + 300, LARGE_TRIP, 700], [SEARCH, SIM3, FUSE], None),
            (7, [700, LARGE_TRIP + 1], [FUSE, SEARCH], None)]        # seeds 4 .. 6 reject the one entry of the second trip


def large_scene(draw):
    seed, counts, modes, special = draw
    return make_views(np.random.default_rng(seed), counts, modes, n_mp=LARGE_N_MP, special=special)


def make_matcher_scene(seed=77):
    """The end-to-end scene of the GPU tests: 300 map points under a SEARCH and a SIM3 view, and per view a keyframe of 500 keypoints.  The
    map points' descriptors come in 60 clusters of five and each keypoint sits near the projection of a kept map point with that point's
    descriptor a few bits off, so several queries compete for a keypoint; about 30 % of the keypoints are bound beforehand.
    Returns (scene, [keyframe dict per view], bound).  test_project_gate_ref.py holds its near_level mask empty."""
    rng = np.random.default_rng(seed)
    sc = make_views(rng, [300, 300], [SEARCH, SIM3], n_mp=300)
    t = sc["table"]
    base = rng.integers(0, 2 ** 32, (60, 8), dtype=np.uint64).astype(np.uint32)
    flip = lambda n, p: ((np.uint32(1) << rng.integers(0, 32, (n, 8)).astype(np.uint32)) * (rng.random((n, 8)) < p)).astype(np.uint32)
    t["desc"] = base[np.arange(300) % 60] ^ flip(300, 0.3)
    regate(sc)
    kfs = []
    for v in range(2):
        g = sc["ref"][v]
        src = g["kept"][rng.integers(0, len(g["kept"]), 500)]
        mp = np.asarray(sc["views"][v]["indices"])[src]
        kfs.append(dict(x=(g["x"][src] + rng.normal(0, 2.0, 500)).astype(F), y=(g["y"][src] + rng.normal(0, 2.0, 500)).astype(F), desc=t["desc"][mp] ^ flip(500, 0.4),
                        octave=np.where(rng.random(500) < 0.7, g["level"][src] - rng.integers(0, 2, 500), rng.integers(0, 8, 500)).astype(np.int32)))
    bound = (rng.random(500) < 0.3).astype(np.uint8)
    return sc, kfs, bound
