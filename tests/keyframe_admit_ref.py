"""The specification of ms_keyframe_admit in numpy: Keyframe::addFullFeatures / processKeyPoints (keyframe.cpp:34-116) from a
keypoint view onto the map tables, FeatureSearch::create's order and the FeatureVector of BowIndex::transform as node lists.  Everything
is integers, copied floats and float64 arithmetic that numpy rounds step by step: a comparison with this file is bit for bit.

A frame, a dict: x, y, angle [n] float32, octave, track_id [n] int32, desc [n, 8] uint32, and -- the result of the descent, which
tests/bow_synth.py restates -- word, node [n] int32, weight [n] float64 (absent: no vocabulary).
Tables, a dict: kf_mp [n_kf, stride] int32, kp_x, kp_y, kp_depth [n_kf, stride] float32, kp_octave [n_kf, stride] int32, desc_pool
[n_pool, 8] uint32, kf_pose [n_kf, 12] float64; n_mp is the number of map-point rows.
Frame arrays of capacity cap, a dict: desc [cap, 8], angle, octave, bearing [cap, 3], usable, sorted_x, sorted_y, sorted_idx, node_id,
kp_idx [cap], node_start [cap + 1]."""
import numpy as np

OK, INVALID, CAPACITY = 0, -1, -4
TABLES = ("kf_mp", "kp_x", "kp_y", "kp_octave", "kp_depth", "desc_pool", "kf_pose")
FRAME = ("desc", "angle", "octave", "bearing", "usable", "sorted_x", "sorted_y", "sorted_idx", "node_id", "node_start", "kp_idx")
FRAME_TYPES = dict(desc=np.uint32, angle=np.float32, octave=np.int32, bearing=np.float64, usable=np.uint8, sorted_x=np.float32, sorted_y=np.float32,
                   sorted_idx=np.int32, node_id=np.int32, node_start=np.int32, kp_idx=np.int32)


def frame_arrays(cap, fill=0):
    """The arrays of an ms_admit_frame of capacity cap, every byte `fill`."""
    shape = lambda k: (cap, 8) if k == "desc" else (cap, 3) if k == "bearing" else (cap + 1,) if k == "node_start" else (cap,)
    out = {k: np.zeros(shape(k), FRAME_TYPES[k]) for k in FRAME}
    for a in out.values():
        a.view(np.uint8)[...] = fill
    return out


def bearing(cam, x, y):
    """the unit vector of ((x - cx) / fx, (y - cy) / fy, 1) in float64, every step rounded on its own"""
    xn = (np.asarray(x, np.float32).astype(np.float64) - cam["cx"]) / cam["fx"]
    yn = (np.asarray(y, np.float32).astype(np.float64) - cam["cy"]) / cam["fy"]
    nrm = np.sqrt(xn * xn + yn * yn + 1.0)
    return np.stack([xn / nrm, yn / nrm, 1.0 / nrm], axis=-1)


def sort_positions(y):
    """FeatureSearch::create by ms_feature_search_sort's rule: pos[j] = #{k : y[k] < y[j] or (y[k] == y[j] and k < j)}."""
    y = np.asarray(y, np.float32)
    k = np.arange(len(y))
    return ((y[None, :] < y[:, None]) | ((y[None, :] == y[:, None]) & (k[None, :] < k[:, None]))).sum(axis=1).astype(np.int64)


def track_indices(track_id, track_ids):
    """Per keypoint the LAST index of its id in track_ids (trackIdToIndex[id] = idx overwrites), -1 without a track or without lists, -2 for
    a tracked keypoint whose id is not listed."""
    tid = np.asarray(track_id, np.int64)
    at = np.full(len(tid), -1, np.int64)
    if track_ids is None:
        return at
    ids = np.asarray(track_ids, np.int64)
    eq = ids[None, :] == tid[:, None]
    last = np.where(eq.any(axis=1), eq.shape[1] - 1 - np.argmax(eq[:, ::-1], axis=1), -2) if eq.shape[1] else np.full(len(tid), -2, np.int64)
    return np.where(tid >= 0, last, at)


def rint_i32(v):
    """__float2int_rn: round to nearest even, saturating"""
    return np.clip(np.rint(np.asarray(v, np.float32).astype(np.float64)), -2**31, 2**31 - 1).astype(np.int64)


def depths(x, y, at, track_depth, image):
    """keyframe.cpp:57-63 with the depth image standing in for frame->getDepth"""
    n = len(x)
    d = np.full(n, -1, np.float32)
    if track_depth is not None and n:
        has = at >= 0
        d[has] = np.asarray(track_depth, np.float32)[at[has]]
    sample = np.full(n, -1, np.float32)
    if image is not None and n:
        ix, iy = rint_i32(x), rint_i32(y)
        inside = (ix >= 0) & (ix < image.shape[1]) & (iy >= 0) & (iy < image.shape[0])
        sample[inside] = image[iy[inside], ix[inside]]
    with np.errstate(invalid="ignore"):
        return np.where(d < 0, sample, d).astype(np.float32)  # a NaN stays


def node_lists(frame):
    """The FeatureVector as the ms_bow of an ms_match_frame: keypoints with weight > 0 by (node, index)."""
    n = len(frame["x"])
    if "word" not in frame:
        return np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32)
    kept = np.flatnonzero(np.asarray(frame["weight"], np.float64) > 0)
    node = np.asarray(frame["node"], np.int64)[kept]
    order = kept[np.argsort(node, kind="stable")]
    ids, counts = np.unique(node, return_counts=True)
    start = np.zeros(len(ids) + 1, np.int32)
    start[1:] = np.cumsum(counts)
    assert n == 0 or len(order) <= n
    return ids.astype(np.int32), start, order.astype(np.int32)


def admit(tables, n_mp, frame, slot, desc_base, pose, cam, cap_kp, view_capacity=None, track_ids=None, track_depth=None, depth_image=None, before=None):
    """ms_keyframe_admit.  `before` = the frame arrays as they are (default: zeros).  Returns dict(rc, counts [3], the tables and the frame
    arrays as they are afterwards, and the host outputs kp_track, word, weight, h_sorted_x, h_sorted_y, h_sorted_idx, h_octave, h_desc)."""
    n = len(frame["x"])
    stride, n_pool = tables["kf_mp"].shape[1], len(tables["desc_pool"])
    out = {k: np.array(tables[k], copy=True) for k in TABLES}
    fr = frame_arrays(cap_kp) if before is None else {k: np.array(before[k], copy=True) for k in FRAME}
    out.update(fr)
    out.update(rc=OK, counts=np.array([n, 0, 0], np.int32))
    x, y = np.asarray(frame["x"], np.float32), np.asarray(frame["y"], np.float32)
    if view_capacity is not None and n > view_capacity:
        return dict(out, rc=INVALID)
    if n > stride or n > cap_kp or desc_base + n > n_pool:
        return dict(out, rc=CAPACITY)
    row = np.asarray(tables["kf_mp"][slot], np.int64)
    at = track_indices(frame["track_id"], track_ids)
    if not (np.isfinite(x).all() and np.isfinite(y).all()) or ((row >= 0) & (row < n_mp)).any() or (at == -2).any():
        return dict(out, rc=INVALID)                         # every verdict before any write
    out["kf_mp"][slot] = -1
    out["kf_pose"][slot] = np.asarray(pose, np.float64).reshape(12)
    out["kp_x"][slot, :n], out["kp_y"][slot, :n], out["kp_octave"][slot, :n] = x, y, frame["octave"]
    out["kp_depth"][slot, :n] = depths(x, y, at, track_depth, depth_image)
    out["desc_pool"][desc_base:desc_base + n] = frame["desc"]
    out["desc"][:n], out["angle"][:n], out["octave"][:n] = frame["desc"], frame["angle"], frame["octave"]
    out["bearing"][:n] = bearing(cam, x, y).reshape(n, 3)
    out["usable"][:n] = 1
    pos = sort_positions(y)
    out["sorted_x"][pos], out["sorted_y"][pos], out["sorted_idx"][pos] = x, y, np.arange(n, dtype=np.int32)
    ids, start, order = node_lists(frame)
    out["node_id"][:len(ids)], out["node_start"][:len(start)], out["kp_idx"][:len(order)] = ids, start, order
    out["counts"] = np.array([n, len(ids), len(order)], np.int32)
    has = "word" in frame
    out.update(kp_track=np.asarray(frame["track_id"], np.int32).copy(), word=np.asarray(frame["word"], np.int32) if has else np.full(n, -1, np.int32),
               weight=np.asarray(frame["weight"], np.float64) if has else np.zeros(n, np.float64), h_sorted_x=out["sorted_x"][:n].copy(),
               h_sorted_y=out["sorted_y"][:n].copy(), h_sorted_idx=out["sorted_idx"][:n].copy(), h_octave=np.asarray(frame["octave"], np.int32).copy(),
               h_desc=np.asarray(frame["desc"], np.uint32).reshape(n, 8).copy())
    return out


def bow_vector(word, weight):
    """BowIndex::assembleVector: v[word] += weight in feature order for weight > 0, then L1 normalisation.  Returns (words ascending, values)."""
    v = {}
    for w, wt in zip(np.asarray(word).tolist(), np.asarray(weight, np.float64).tolist()):
        if wt > 0:
            v[w] = v.get(w, 0.0) + wt
    keys = sorted(v)
    norm = 0.0
    for k in keys:
        norm += abs(v[k])
    vals = [v[k] / norm if norm > 0 else v[k] for k in keys]
    return np.array(keys, np.int64), np.array(vals, np.float64)


def empty_tables(n_kf, stride, n_pool, seed=0):
    """Tables whose bytes are recognisable: random keypoint entries, pool and poses, every row empty."""
    rng = np.random.default_rng(seed)
    return dict(kf_mp=np.full((n_kf, stride), -1, np.int32), kp_x=rng.random((n_kf, stride)).astype(np.float32), kp_y=rng.random((n_kf, stride)).astype(np.float32),
                kp_octave=rng.integers(0, 8, (n_kf, stride)).astype(np.int32), kp_depth=rng.random((n_kf, stride)).astype(np.float32),
                desc_pool=rng.integers(0, 2**32, (n_pool, 8), dtype=np.uint64).astype(np.uint32), kf_pose=rng.random((n_kf, 12)))


def synth_frame(n, seed, width=640, height=480, n_tracked=0, y_step=None):
    """n keypoints; the first n_tracked carry track ids 100, 101, ...; y_step quantises y so that many are equal."""
    rng = np.random.default_rng(seed)
    y = (rng.random(n) * (height - 1)).astype(np.float32)
    if y_step:
        y = (np.floor(y / y_step) * y_step).astype(np.float32)
    tid = np.full(n, -1, np.int32)
    tid[:n_tracked] = 100 + np.arange(n_tracked)
    return dict(x=(rng.random(n) * (width - 1)).astype(np.float32), y=y, angle=(rng.random(n) * 360).astype(np.float32), octave=rng.integers(0, 8, n).astype(np.int32),
                track_id=tid, desc=rng.integers(0, 2**32, (n, 8), dtype=np.uint64).astype(np.uint32))
