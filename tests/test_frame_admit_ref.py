"""tests/frame_admit_ref.py, the specification of ms_frame_admit, against its own literal walk of Keyframe::addTrackerFeatures /
processKeyPoints (keyframe.cpp:34-69, :118-133): equal on every scene without a dropped feature; different in exactly the entries DESIGN
section 3 names on a scene with one drop; the duplicate-id refusal against the reference's "the last feature wins"; the depth rule case by
case; the capacity rule, the occupied row and n_tracks == 0."""
import numpy as np
import pytest

import frame_admit_ref as R

F = np.float32
POSE = np.arange(12, dtype=np.float64) * 0.5 - 2.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def features(n, seed, w=40, h=30):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.5, 9, n).astype(F)
    depth[rng.random(n) < 0.4] = -1                          # the tracker has no depth: the image decides
    return dict(x=rng.uniform(-3, w + 2, n).astype(F), y=rng.uniform(-3, h + 2, n).astype(F), id=rng.permutation(5 * n + 7)[:n].astype(np.int32) + 100, depth=depth, keep=None)


def image(w=40, h=30):
    return (np.arange(w * h, dtype=F).reshape(h, w) * F(0.25) + F(1))


def admit(feat, stride=None, img=None, mask=None, n_mp=50, slot=1, cap_kp=None, tables=None):
    stride = max(len(feat["x"]), 1) if stride is None else stride
    tables = R.empty_tables(3, stride, seed=stride) if tables is None else tables
    return (tables,) + R.frame_admit(tables, n_mp, feat, slot, POSE, img, mask, cap_kp)


@pytest.mark.parametrize("n, with_image", [(0, True), (1, False), (7, True), (300, True), (300, False)])
def test_the_restatement_equals_the_literal_walk_when_nothing_is_dropped(n, with_image):
    feat, img = features(n, 3 + n), image() if with_image else None
    tables, rc, T, out = admit(feat, img=img)
    key_points, kp_to_track, map_points, depths = R.literal_walk(feat, img)
    assert rc == R.OK and out["counts"][0] == n == len(key_points) and out["counts"][1] == out["counts"][2] == 0
    assert same_bits(T["kp_x"][1, :n], np.array([p[0] for p in key_points], F)) and same_bits(T["kp_y"][1, :n], np.array([p[1] for p in key_points], F))
    assert (T["kp_octave"][1, :n] == 0).all() and all(p[2] == 0 for p in key_points)
    assert same_bits(T["kp_depth"][1, :n], np.array(depths, F))
    assert kp_to_track == {k: int(t) for k, t in enumerate(out["kp_track"])}       # keyPointToTrackId, which ms_match_tracked takes as kp_track
    assert (T["kf_mp"][1] == -1).all() and map_points == [-1] * n and same_bits(T["kf_pose"][1], POSE)
    assert (out["kp_feature"] == np.arange(n)).all()
    if with_image and n >= 300:
        assert 0 < out["counts"][3] < n                      # some depths came from the image, some positions lie outside it
    for k in R.TABLES:                                       # every other slot keeps its bytes
        assert same_bits(T[k][[0, 2]], tables[k][[0, 2]]), k


def test_one_dropped_feature_shifts_the_references_ids_and_depths_and_not_ours():
    n, d = 6, 2
    feat = dict(x=np.array([1, 2, 3, 4, 5, 6], F), y=np.array([1, 1, 2, 2, 3, 3], F), id=np.array([10, 11, 12, 13, 14, 15], np.int32),
                depth=np.array([0.5, 1.5, 2.5, -1, 4.5, 5.5], F), keep=np.array([1, 1, 0, 1, 1, 1], np.uint8))
    img = image()
    _, rc, T, out = admit(feat, img=img)
    key_points, kp_to_track, _, depths = R.literal_walk(feat, img)
    assert rc == R.OK and list(out["counts"]) == [5, 1, 0, 1] and len(key_points) == 5
    # ours: keypoint k carries the id and the depth of the k-th KEPT feature
    assert list(out["kp_feature"]) == [0, 1, 3, 4, 5] and list(out["kp_track"]) == [10, 11, 13, 14, 15]
    assert same_bits(T["kp_depth"][1, :5], np.array([0.5, 1.5, img[2, 4], 4.5, 5.5], F))
    # the reference: keyPointToTrackId is keyed by the FEATURE index, so keypoint d has no track, keypoints behind it carry the id of the feature
    # before theirs, and the last id sits on a keypoint that does not exist
    assert kp_to_track == {0: 10, 1: 11, 3: 13, 4: 14, 5: 15}
    ours = {k: int(t) for k, t in enumerate(out["kp_track"])}
    assert {k for k in range(n) if ours.get(k) != kp_to_track.get(k)} == {d, 3, 4, 5}      # exactly the keypoints from the drop on, and the phantom keypoint 5
    assert all(ours[k] == kp_to_track[k] for k in range(d))
    # its depths: keypoint 2 (feature 3) has no id and so takes the image; keypoint 3 (feature 4) takes feature 3's depth -1 -> the image at ITS OWN
    # position; keypoint 4 (feature 5) takes feature 4's depth
    assert same_bits(np.array(depths, F), np.array([0.5, 1.5, img[2, 4], img[3, 5], 4.5], F))
    differ = [k for k in range(5) if not same_bits(T["kp_depth"][1, k], depths[k])]
    assert differ == [3, 4]
    # positions and octaves agree: the drop changes which id and depth a keypoint gets, not the keypoints
    assert same_bits(T["kp_x"][1, :5], np.array([p[0] for p in key_points], F)) and same_bits(T["kp_y"][1, :5], np.array([p[1] for p in key_points], F))


def test_a_duplicate_id_is_refused_where_the_reference_lets_the_last_feature_win():
    feat = dict(x=np.array([1, 2, 3], F), y=np.array([1, 2, 3], F), id=np.array([7, 8, 7], np.int32), depth=np.array([1.0, 2.0, 3.0], F), keep=None)
    tables, rc, T, out = admit(feat)
    assert rc == R.INVALID and T is tables
    _, kp_to_track, _, depths = R.literal_walk(feat)
    assert kp_to_track == {0: 7, 1: 8, 2: 7} and depths == [F(3.0), F(2.0), F(3.0)]      # :51-53: keypoint 0 gets the depth of feature 2
    feat["id"][2] = 9
    assert admit(feat)[1] == R.OK


def test_other_refusals_of_the_validation():
    good = features(5, 1)
    for change in (dict(id=np.array([1, 2, -1, 4, 5], np.int32)), dict(x=np.array([1, np.nan, 3, 4, 5], F)), dict(y=np.array([1, 2, 3, np.inf, 5], F))):
        assert admit(dict(good, **change))[1] == R.INVALID, list(change)
    t = R.empty_tables(3, 5)
    assert R.frame_admit(t, 9, good, 3, POSE)[0] == R.INVALID and R.frame_admit(t, 9, good, -1, POSE)[0] == R.INVALID
    bad_pose = POSE.copy(); bad_pose[4] = np.nan
    assert R.frame_admit(t, 9, good, 1, bad_pose)[0] == R.INVALID and R.frame_admit(t, 9, good, 1, POSE)[0] == R.OK


def test_the_depth_rule_case_by_case():
    img = image(6, 4)
    feat = dict(x=np.array([1.0, 2.5, 5.5, 3.0, 0.0, 3.5, 1.0], F), y=np.array([2.0, 1.0, 1.0, 3.0, 0.0, 0.5, -0.6], F), id=np.arange(7, dtype=np.int32),
                depth=np.array([0.75, -1.0, -2.0, -0.0, np.nan, -0.5, -1.0], F), keep=None)
    _, rc, T, out = admit(feat, img=img)
    assert rc == R.OK
    d = T["kp_depth"][1, :7]
    assert d[0] == F(0.75)                                   # a depth >= 0 is kept
    assert d[1] == img[1, 2]                                 # negative, with an image: round(2.5) = 2, to even
    assert d[2] == -1                                        # negative, outside the image: round(5.5) = 6 is no column of a 6-wide image
    assert d[3] == 0 and np.signbit(d[3])                    # -0.0 is not < 0: it stays as written
    assert np.isnan(d[4])                                    # a NaN stays
    assert d[5] == img[0, 4]                                 # round(3.5) = 4, round(0.5) = 0
    assert d[6] == -1                                        # round(-0.6) = -1: above the image
    assert out["counts"][3] == 2                             # features 1 and 5
    _, rc, T, out = admit(feat, img=None)
    assert rc == R.OK and list(T["kp_depth"][1, [1, 2, 5, 6]]) == [-1, -1, -1, -1] and T["kp_depth"][1, 0] == F(0.75) and np.isnan(T["kp_depth"][1, 4]) and out["counts"][3] == 0


def test_the_mask_drops_by_the_rounded_position_and_outside_the_raster():
    mask = np.ones((4, 6), np.uint8)
    mask[1, 2] = 0
    feat = dict(x=np.array([2.5, 1.5, 5.5, 0.0, 3.0], F), y=np.array([1.0, 1.0, 1.0, 3.6, 2.0], F), id=np.arange(5, dtype=np.int32), depth=np.ones(5, F),
                keep=np.array([1, 1, 1, 1, 0], np.uint8))
    _, rc, T, out = admit(feat, mask=mask)
    # 2.5 and 1.5 both round to column 2 (to even): masked; 5.5 -> column 6 and 3.6 -> row 4 lie outside the raster; the last one falls to keep
    assert rc == R.OK and list(out["counts"]) == [0, 1, 4, 0] and len(out["kp_track"]) == 0
    feat["x"][1] = 0.5
    _, rc, T, out = admit(feat, mask=mask)
    assert list(out["counts"][:3]) == [1, 1, 3] and list(out["kp_feature"]) == [1]
    key_points, _, _, _ = R.literal_walk(feat, None, mask)
    assert len(key_points) == 1 and key_points[0][0] == F(0.5)


def test_capacity_and_the_occupied_row_leave_every_table():
    feat = features(9, 5)
    tables, rc, T, out = admit(feat, stride=9)
    assert rc == R.OK and out["counts"][0] == 9
    tables, rc, T, out = admit(feat, stride=8)
    assert rc == R.CAPACITY and T is tables and out["counts"][0] == 9 and len(out["kp_track"]) == 0
    tables, rc, T, out = admit(feat, stride=9, cap_kp=8)
    assert rc == R.CAPACITY and T is tables and out["counts"][0] == 9
    feat["keep"] = np.ones(9, np.uint8); feat["keep"][4] = 0
    assert admit(feat, stride=8)[1] == R.OK                  # n_kp, not n_tracks, is what must fit
    t = R.empty_tables(3, 9)
    t["kf_mp"][1, 8] = 49                                    # behind every keypoint, and still an observation somebody holds
    assert R.frame_admit(t, 50, feat, 1, POSE)[0] == R.INVALID
    t["kf_mp"][1, 8] = 50                                    # out of range: stale
    t["kf_mp"][1, 0] = -7
    rc, T, _ = R.frame_admit(t, 50, feat, 1, POSE)
    assert rc == R.OK and (T["kf_mp"][1] == -1).all()
    assert R.frame_admit(t, 0, feat, 1, POSE)[0] == R.OK     # no map point: no entry is valid


def test_no_features_clears_the_row_and_writes_the_pose():
    feat = dict(x=np.zeros(0, F), y=np.zeros(0, F), id=np.zeros(0, np.int32), depth=np.zeros(0, F), keep=None)
    t = R.empty_tables(3, 4)
    t["kf_mp"][1] = [-1, 99, -5, 1 << 30]
    rc, T, out = R.frame_admit(t, 50, feat, 1, POSE)
    assert rc == R.OK and list(out["counts"]) == [0, 0, 0, 0] and (T["kf_mp"][1] == -1).all() and same_bits(T["kf_pose"][1], POSE)
    for k in ("kp_x", "kp_y", "kp_octave", "kp_depth"):
        assert same_bits(T[k], t[k]), k
