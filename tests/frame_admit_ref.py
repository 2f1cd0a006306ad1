"""The specification of ms_frame_admit in numpy, and beside it a literal walk of Keyframe::addTrackerFeatures /
processKeyPoints (keyframe.cpp:34-69, :118-133) over dictionaries.  Everything is integers and copied floats: a comparison with this
file is bit for bit.

Features, a dict: x, y, depth [n] float32, id [n] int32, keep [n] uint8 or None (the host's camera.isValidPixel per feature).
Tables, a dict: kf_mp [n_kf, stride] int32, kp_x, kp_y, kp_depth [n_kf, stride] float32, kp_octave [n_kf, stride] int32, kf_pose
[n_kf, 12] float64; n_mp is the number of map-point rows.
image: [h, w] float32 or None, the stand-in for frame->getDepth; mask: [h, w] uint8 or None, the raster stand-in for isValidPixel."""
import numpy as np

OK, INVALID, CAPACITY = 0, -1, -4
TABLES = ("kf_mp", "kp_x", "kp_y", "kp_octave", "kp_depth", "kf_pose")


def rint_i32(v):
    """__float2int_rn: round to nearest even, saturating"""
    return np.clip(np.rint(np.asarray(v, np.float32).astype(np.float64)), -2**31, 2**31 - 1).astype(np.int64)


def inside(x, y, raster):
    """(inside the raster, column, row) of the rounded positions"""
    ix, iy = rint_i32(x), rint_i32(y)
    return (ix >= 0) & (ix < raster.shape[1]) & (iy >= 0) & (iy < raster.shape[0]), ix, iy


def kept_mask(feat, mask):
    """(kept, dropped by keep, dropped by the mask alone) per feature"""
    n = len(feat["x"])
    by_keep = np.zeros(n, bool) if feat.get("keep") is None else np.asarray(feat["keep"], np.uint8) == 0
    ok = np.ones(n, bool)
    if mask is not None and n:
        ins, ix, iy = inside(feat["x"], feat["y"], mask)
        ok = ins.copy()
        ok[ins] = mask[iy[ins], ix[ins]] != 0
    return ~by_keep & ok, by_keep, ~by_keep & ~ok


def depth_of(x, y, depth, image):
    """keyframe.cpp:57-63: the feature's own depth, or iff that is < 0 as written (a NaN stays) the image's sample at the rounded position, -1
    outside the image or with no image.  Returns (depths, taken from the image)."""
    d = np.asarray(depth, np.float32)
    sample, taken = np.full(len(d), -1, np.float32), np.zeros(len(d), bool)
    with np.errstate(invalid="ignore"):
        neg = d < 0
    if image is not None and len(d):
        ins, ix, iy = inside(x, y, image)
        sample[ins] = image[iy[ins], ix[ins]]
        taken = neg & ins
    return np.where(neg, sample, d).astype(np.float32), taken


def validate(feat, slot, n_kf, pose):
    """What ms_frame_admit_validate refuses of the features, the slot and the pose: INVALID or OK."""
    x, y, ids = np.asarray(feat["x"], np.float32), np.asarray(feat["y"], np.float32), np.asarray(feat["id"], np.int32)
    if not 0 <= slot < n_kf or not np.isfinite(np.asarray(pose, np.float64)).all():
        return INVALID
    if not (np.isfinite(x).all() and np.isfinite(y).all()) or (ids < 0).any() or len(np.unique(ids)) != len(ids):
        return INVALID
    return OK


def frame_admit(tables, n_mp, feat, slot, pose, image=None, mask=None, cap_kp=None):
    """ms_frame_admit.  Returns (rc, new tables, dict(kp_track, kp_feature, counts [4])); on a refusal the tables are the incoming ones and,
    for the two verdicts of the device, counts holds the call's numbers (counts[0] the needed n_kp)."""
    stride = tables["kf_mp"].shape[1]
    if validate(feat, slot, len(tables["kf_mp"]), pose):
        return INVALID, tables, dict(kp_track=np.zeros(0, np.int32), kp_feature=np.zeros(0, np.int32), counts=np.zeros(4, np.int32))
    x, y = np.asarray(feat["x"], np.float32), np.asarray(feat["y"], np.float32)
    ids = np.asarray(feat["id"], np.int32)
    cap_kp = len(x) if cap_kp is None else cap_kp
    kept, by_keep, by_mask = kept_mask(feat, mask)
    idx = np.flatnonzero(kept)                               # keypoint k is the k-th kept feature in ascending i
    n_kp = len(idx)
    depth, taken = depth_of(x[idx], y[idx], np.asarray(feat["depth"], np.float32)[idx], image)
    counts = np.array([n_kp, by_keep.sum(), by_mask.sum(), taken.sum()], np.int32)
    out = dict(kp_track=np.zeros(0, np.int32), kp_feature=np.zeros(0, np.int32), counts=counts)
    if n_kp > stride or n_kp > cap_kp:
        return CAPACITY, tables, out
    if (tables["kf_mp"][slot].view(np.uint32) < np.uint32(n_mp)).any():      # a VALID entry, keyframe.cpp:275
        return INVALID, tables, out
    T = {k: tables[k].copy() for k in TABLES}
    T["kf_mp"][slot, :] = -1
    T["kf_pose"][slot] = np.asarray(pose, np.float64).reshape(12)
    T["kp_x"][slot, :n_kp] = x[idx]; T["kp_y"][slot, :n_kp] = y[idx]
    T["kp_octave"][slot, :n_kp] = 0                          # keyframe.cpp:127
    T["kp_depth"][slot, :n_kp] = depth
    out.update(kp_track=ids[idx].copy(), kp_feature=idx.astype(np.int32))
    return OK, T, out


def literal_walk(feat, image=None, mask=None):
    """Keyframe::addTrackerFeatures (keyframe.cpp:118-133) and processKeyPoints (:49-64) statement by statement.  Returns keyPoints (a list of
    (x, y, octave)), keyPointToTrackId (a dict KpId -> TrackId, keyed as the reference keys it), mapPoints and keyPointDepth."""
    def is_valid_pixel(i):
        if feat.get("keep") is not None and not feat["keep"][i]:
            return False
        if mask is None:
            return True
        ins, ix, iy = inside(feat["x"][i:i + 1], feat["y"][i:i + 1], mask)
        return bool(ins[0]) and mask[iy[0], ix[0]] != 0

    def get_depth(px, py):
        if image is None:
            return np.float32(-1)
        ins, ix, iy = inside(np.float32([px]), np.float32([py]), image)
        return image[iy[0], ix[0]] if ins[0] else np.float32(-1)

    key_points, kp_to_track = [], {}
    for i in range(len(feat["x"])):                          # :119
        if not is_valid_pixel(i):                            # :122
            continue
        key_points.append((np.float32(feat["x"][i]), np.float32(feat["y"][i]), 0))     # :123-128
        kp_to_track.setdefault(i, int(feat["id"][i]))        # :129 emplace(KpId(i), track.id): the FEATURE index
    map_points = [-1] * len(key_points)                      # :49
    track_id_to_index = {}
    for idx in range(len(feat["x"])):                        # :51-53: the last feature with an id wins
        track_id_to_index[int(feat["id"][idx])] = idx
    depths = []
    for kp_idx, (px, py, _) in enumerate(key_points):        # :55-64
        depth = np.float32(-1)
        if kp_idx in kp_to_track:
            depth = np.float32(feat["depth"][track_id_to_index[kp_to_track[kp_idx]]])
        if depth < 0:
            depth = get_depth(px, py)
        depths.append(np.float32(depth))
    return key_points, kp_to_track, map_points, depths


def empty_tables(n_kf, stride, seed=0):
    """Tables whose rows are cleared and whose keypoint table and poses hold a pattern (so that bytes that must stay are seen to stay)."""
    rng = np.random.default_rng(seed)
    f = lambda: rng.uniform(-50, 700, (n_kf, stride)).astype(np.float32)
    return dict(kf_mp=np.full((n_kf, stride), -1, np.int32), kp_x=f(), kp_y=f(), kp_octave=rng.integers(0, 8, (n_kf, stride)).astype(np.int32), kp_depth=f(),
                kf_pose=rng.uniform(-2, 2, (n_kf, 12)))
