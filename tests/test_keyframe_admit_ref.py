"""tests/keyframe_admit_ref.py, the numpy specification of ms_keyframe_admit, against a literal walk of the reference:
processKeyPoints with a dict for trackIdToIndex (keyframe.cpp:51-64), FeatureSearch::create as Python's stable sort by y and as
ms_feature_search_sort through the library, and the FeatureVector as a dict of lists filled in feature order (BowIndex::assemble).  No GPU."""
import math
import struct

import numpy as np
import pytest

import bow_synth
import keyframe_admit_ref as ref
import mi355slam

CAM = dict(fx=520.25, fy=519.5, cx=318.75, cy=241.125)
POSE = np.arange(12, dtype=np.float64) * 0.25 - 1.0


def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def with_descent(frame, seed, stop_words=0.3):
    """word / weight / node of a small ragged vocabulary with many stop words, by the plain restatement of DBoW2's transform"""
    vocab = bow_synth.make_vocab(seed, k=4, depth=3, ragged=0.3, stop_words=stop_words)
    frame["desc"] = bow_synth.make_queries(seed + 1, vocab, len(frame["x"])) if len(frame["x"]) else frame["desc"]
    t = bow_synth.transform_py(vocab, frame["desc"], 2)
    frame.update(word=np.array([a for a, _, _ in t], np.int32), weight=np.array([b for _, b, _ in t], np.float64), node=np.array([c for _, _, c in t], np.int32))
    return frame


def walk(tables, n_mp, frame, slot, desc_base, cap, track_ids, track_depth, image):
    """The reference, keypoint by keypoint, on Python scalars.  Returns what ref.admit returns for a call that is accepted."""
    n = len(frame["x"])
    out = {k: np.array(tables[k], copy=True) for k in ref.TABLES}
    out.update(ref.frame_arrays(cap))
    track_to_index = {}                                      # :51-53
    if track_ids is not None:
        for idx, tid in enumerate(track_ids):
            track_to_index[int(tid)] = idx
    out["kf_mp"][slot, :] = -1                               # :49, and the row is the slot's
    out["kf_pose"][slot] = POSE
    for j in range(n):
        x, y = float(frame["x"][j]), float(frame["y"][j])
        depth = -1.0                                         # :57
        tid = int(frame["track_id"][j])
        if tid >= 0 and track_ids is not None:
            depth = float(track_depth[track_to_index[tid]])  # :59, .at
        if depth < 0:                                        # :61
            depth = -1.0
            if image is not None:
                ix, iy = round(x), round(y)                  # Python rounds half to even, like __float2int_rn
                if 0 <= ix < image.shape[1] and 0 <= iy < image.shape[0]:
                    depth = float(image[iy, ix])
        out["kp_depth"][slot, j] = depth
        out["kp_x"][slot, j], out["kp_y"][slot, j], out["kp_octave"][slot, j] = frame["x"][j], frame["y"][j], frame["octave"][j]
        out["desc_pool"][desc_base + j] = frame["desc"][j]
        out["desc"][j], out["angle"][j], out["octave"][j], out["usable"][j] = frame["desc"][j], frame["angle"][j], frame["octave"][j], 1
        xn, yn = (x - CAM["cx"]) / CAM["fx"], (y - CAM["cy"]) / CAM["fy"]
        nrm = math.sqrt(xn * xn + yn * yn + 1.0)
        out["bearing"][j] = (xn / nrm, yn / nrm, 1.0 / nrm)
    order = sorted(range(n), key=lambda j: float(frame["y"][j]))      # FeatureSearch::create: stable by y
    for pos, j in enumerate(order):
        out["sorted_x"][pos], out["sorted_y"][pos], out["sorted_idx"][pos] = frame["x"][j], frame["y"][j], j
    fv = {}                                                  # DBoW2::FeatureVector
    if "word" in frame:
        for j in range(n):
            if frame["weight"][j] > 0:
                fv.setdefault(int(frame["node"][j]), []).append(j)
    at = 0
    for k, node in enumerate(sorted(fv)):
        out["node_id"][k], out["node_start"][k] = node, at
        out["kp_idx"][at:at + len(fv[node])] = fv[node]
        at += len(fv[node])
    out["node_start"][len(fv)] = at
    out["counts"] = np.array([n, len(fv), at], np.int32)
    return out


def same(a, b, names):
    for k in names:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def case(n, seed, n_tracked=0, y_step=None, descent=True, stride=None, cap=None):
    frame = ref.synth_frame(n, seed, n_tracked=n_tracked, y_step=y_step)
    if descent:
        with_descent(frame, seed)
    stride = stride or max(n, 1) + 3
    return frame, ref.empty_tables(3, stride, 2 * stride + 5, seed), cap or max(n, 1) + 2


@pytest.mark.parametrize("n, n_tracked, y_step", [(0, 0, None), (1, 1, None), (97, 20, None), (300, 40, 16.0), (64, 0, 1000.0)])
def test_the_restatement_is_the_literal_walk(n, n_tracked, y_step):
    frame, tables, cap = case(n, 11 + n, n_tracked, y_step)
    rng = np.random.default_rng(n)
    # the tracker's lists: every id of the frame, some twice (the LAST one counts), some ids no keypoint has; depths of every kind
    ids = np.concatenate([100 + np.arange(n_tracked), 100 + rng.integers(0, max(n_tracked, 1), n_tracked // 2), [7, 9]]).astype(np.int32)
    rng.shuffle(ids)
    depth = rng.choice(np.array([-1.0, -0.5, 0.0, 2.5, 7.25, np.nan], np.float32), len(ids))
    image = (rng.random((480, 640)) * 10).astype(np.float32)
    image[rng.random((480, 640)) < 0.3] = -1
    if n > 2:
        frame["x"][2], frame["y"][2] = 639.5, 10.0            # rounds to column 640: outside
        frame["x"][1], frame["y"][1] = 100.5, 479.49          # row 479: inside; column 100 (half to even)
    got = ref.admit(tables, 50, frame, 1, 4, POSE, CAM, cap, track_ids=ids, track_depth=depth, depth_image=image)
    want = walk(tables, 50, frame, 1, 4, cap, ids, depth, image)
    assert got["rc"] == ref.OK
    same(got, want, ref.TABLES + ref.FRAME + ("counts",))
    assert (got["kf_mp"][1] == -1).all() and np.array_equal(got["kf_mp"][[0, 2]], tables["kf_mp"][[0, 2]])
    assert np.array_equal(got["kp_track"], frame["track_id"]) and np.array_equal(got["h_sorted_idx"], got["sorted_idx"][:n])
    if n_tracked:
        d = got["kp_depth"][1, :n_tracked]
        assert np.isnan(d).any() or n_tracked < 10            # a NaN depth of a track stays a NaN


def test_the_sort_is_the_librarys_host_sort_and_pythons_stable_sort():
    for n, step in ((0, None), (1, None), (513, None), (700, 32.0), (50, 1e6)):
        f = ref.synth_frame(n, 5 + n, y_step=step)
        if n > 3:
            f["y"][3] = -0.0                                  # equal to +0
            f["y"][0] = 0.0
        pos = ref.sort_positions(f["y"])
        assert sorted(pos.tolist()) == list(range(n))
        idx = np.zeros(n, np.int32)
        idx[pos] = np.arange(n)
        sx, sy, si = mi355slam.feature_search_sort(f["x"], f["y"])
        assert np.array_equal(si, idx) and sx.tobytes() == f["x"][idx].tobytes() and sy.tobytes() == f["y"][idx].tobytes()
        assert idx.tolist() == sorted(range(n), key=lambda j: float(f["y"][j]))


def test_the_node_lists_are_the_feature_vector_and_the_bow_vector_is_assembled_in_feature_order():
    frame = with_descent(ref.synth_frame(400, 3), 3, stop_words=0.4)
    assert (frame["weight"] == 0).sum() > 20 and (frame["weight"] > 0).sum() > 100
    ids, start, order = ref.node_lists(frame)
    fv, v = {}, {}
    for j in range(400):                                     # BowIndex::assemble
        if frame["weight"][j] > 0:
            fv.setdefault(int(frame["node"][j]), []).append(j)
            v[int(frame["word"][j])] = v.get(int(frame["word"][j]), 0.0) + float(frame["weight"][j])
    assert ids.tolist() == sorted(fv) and start[-1] == len(order) == sum(len(l) for l in fv.values())
    for k, node in enumerate(ids.tolist()):
        assert order[start[k]:start[k + 1]].tolist() == fv[node]
    norm = 0.0
    for w in sorted(v):
        norm += abs(v[w])
    words, vals = ref.bow_vector(frame["word"], frame["weight"])
    assert words.tolist() == sorted(v) and vals.tolist() == [v[w] / norm for w in sorted(v)]
    # all keypoints in one node; no keypoint in any
    one = dict(frame, node=np.full(400, 17, np.int32), weight=np.ones(400))
    ids, start, order = ref.node_lists(one)
    assert ids.tolist() == [17] and start.tolist() == [0, 400] and order.tolist() == list(range(400))
    none = dict(frame, weight=np.zeros(400))
    assert [len(a) for a in ref.node_lists(none)] == [0, 1, 0] and ref.admit(ref.empty_tables(1, 400, 400), 0, none, 0, 0, POSE, CAM, 400)["counts"].tolist() == [400, 0, 0]
    plain = {k: frame[k] for k in ("x", "y", "angle", "octave", "track_id", "desc")}
    got = ref.admit(ref.empty_tables(1, 400, 400), 0, plain, 0, 0, POSE, CAM, 400)
    assert got["counts"].tolist() == [400, 0, 0] and (got["word"] == -1).all() and (got["weight"] == 0).all() and got["node_start"][0] == 0


def test_duplicate_track_ids_take_the_last_and_a_missing_id_is_refused():
    frame, tables, cap = case(6, 1, n_tracked=3, descent=False)
    ids, depth = np.array([101, 100, 101, 102, 101], np.int32), np.array([1, 2, 3, 4, 5], np.float32)
    assert ref.track_indices(frame["track_id"], ids).tolist() == [1, 4, 3, -1, -1, -1]
    got = ref.admit(tables, 9, frame, 0, 0, POSE, CAM, cap, track_ids=ids, track_depth=depth)
    assert got["rc"] == ref.OK and got["kp_depth"][0, :6].tolist() == [2.0, 5.0, 4.0, -1.0, -1.0, -1.0]
    got = ref.admit(tables, 9, frame, 0, 0, POSE, CAM, cap, track_ids=ids[:3], track_depth=depth[:3])      # 102 is not listed: .at throws
    assert got["rc"] == ref.INVALID
    same(got, dict(tables, **ref.frame_arrays(cap)), ref.TABLES + ref.FRAME)
    got = ref.admit(tables, 9, frame, 0, 0, POSE, CAM, cap)                                               # no lists: nobody is looked up
    assert got["rc"] == ref.OK and (got["kp_depth"][0, :6] == -1).all()
    assert ref.track_indices(frame["track_id"], np.zeros(0, np.int32)).tolist() == [-2, -2, -2, -1, -1, -1]


def test_every_refusal_leaves_every_byte():
    frame, tables, cap = case(10, 2, stride=10, cap=10)
    before = ref.frame_arrays(10, fill=0xA5)
    untouched = dict(tables, **before)
    ok = ref.admit(tables, 20, frame, 2, 15, POSE, CAM, 10, before=before)
    assert ok["rc"] == ref.OK and ok["counts"][0] == 10 and ok["node_start"][ok["counts"][1]] == ok["counts"][2]
    assert ok["sorted_x"].tobytes() != before["sorted_x"].tobytes()
    for kw, rc in ((dict(cap_kp=9), ref.CAPACITY), (dict(desc_base=16), ref.CAPACITY), (dict(view_capacity=9), ref.INVALID)):
        args = dict(slot=2, desc_base=15, cap_kp=10)
        args.update(kw)
        got = ref.admit(tables, 20, frame, args["slot"], args["desc_base"], POSE, CAM, args["cap_kp"], view_capacity=args.get("view_capacity"),
                        before=ref.frame_arrays(args["cap_kp"], fill=0xA5))
        assert got["rc"] == rc and got["counts"].tolist() == [10, 0, 0], kw
        same(got, dict(tables, **ref.frame_arrays(args["cap_kp"], fill=0xA5)), ref.TABLES + ref.FRAME)
    short = {k: v[:, :9] if k != "desc_pool" and k != "kf_pose" else v for k, v in tables.items()}
    assert ref.admit(short, 20, frame, 2, 15, POSE, CAM, 10)["rc"] == ref.CAPACITY                         # n = stride + 1
    for name, value in (("x", np.nan), ("y", np.inf), ("y", -np.inf)):
        bad = dict(frame)
        bad[name] = frame[name].copy()
        bad[name][7] = value
        got = ref.admit(tables, 20, bad, 2, 15, POSE, CAM, 10, before=before)
        assert got["rc"] == ref.INVALID
        same(got, untouched, ref.TABLES + ref.FRAME)
    bound = {k: v.copy() for k, v in tables.items()}
    bound["kf_mp"][2, 9] = 19                                # a valid entry beyond... inside the row, whatever n is
    got = ref.admit(bound, 20, frame, 2, 15, POSE, CAM, 10, before=before)
    assert got["rc"] == ref.INVALID
    same(got, dict(bound, **before), ref.TABLES + ref.FRAME)
    bound["kf_mp"][2, 9] = 20                                # not valid: (uint32)r < n_mp does not hold
    bound["kf_mp"][2, 3] = -7
    assert ref.admit(bound, 20, frame, 2, 15, POSE, CAM, 10)["rc"] == ref.OK


def test_depth_comes_from_the_track_then_the_image_then_nothing_and_a_nan_stays():
    frame, tables, cap = case(5, 4, n_tracked=4, descent=False)
    frame["x"][:], frame["y"][:] = [3.0, 3.4, 2.5, 3.5, 640.2], [1.0, 1.0, 0.5, 1.5, 2.0]
    image = np.arange(480 * 640, dtype=np.float32).reshape(480, 640)
    ids, depth = np.array([100, 101, 102, 103], np.int32), np.array([4.5, -2.0, np.nan, -0.0], np.float32)
    got = ref.admit(tables, 0, frame, 0, 0, POSE, CAM, cap, track_ids=ids, track_depth=depth, depth_image=image)["kp_depth"][0, :5]
    # from the track | track depth < 0: the image at (3, 1) | NaN stays | -0.0 is not < 0 | no track, column 640 is outside
    assert got[0] == 4.5 and got[1] == image[1, 3] and np.isnan(got[2]) and got[3] == 0 and np.signbit(got[3]) and got[4] == -1
    got = ref.admit(tables, 0, frame, 0, 0, POSE, CAM, cap, depth_image=image)["kp_depth"][0, :5]
    assert got.tolist() == [image[1, 3], image[1, 3], image[0, 2], image[2, 4], -1.0]                       # 2.5 -> 2, 3.5 -> 4, 0.5 -> 0, 1.5 -> 2
    got = ref.admit(tables, 0, frame, 0, 0, POSE, CAM, cap, track_ids=ids, track_depth=depth)["kp_depth"][0, :5]
    assert got[0] == 4.5 and got[1] == -1 and np.isnan(got[2]) and got[4] == -1
    assert ref.rint_i32(np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3e9, -3e9], np.float32)).tolist() == [0, 2, 2, 0, -2, 2**31 - 1, -2**31]


def test_the_bearing_is_float64_step_by_step():
    x, y = np.array([0.0, 318.75, 639.0, 17.3], np.float32), np.array([0.0, 241.125, 479.0, 400.9], np.float32)
    b = ref.bearing(CAM, x, y)
    for j in range(4):
        xn, yn = (float(x[j]) - CAM["cx"]) / CAM["fx"], (float(y[j]) - CAM["cy"]) / CAM["fy"]
        nrm = math.sqrt(xn * xn + yn * yn + 1.0)
        assert b[j].tolist() == [xn / nrm, yn / nrm, 1.0 / nrm]
    assert b[1].tolist() == [0.0, 0.0, 1.0] and f32(17.3) == float(x[3])
