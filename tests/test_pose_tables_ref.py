"""tests/pose_tables_ref.py, the specification of ms_pose_tables_solve, against a literal per-keypoint walk written straight
from bundle_adjuster.cpp:403-480, on the scenes of the GPU tests; and the restated problem through the CPU oracle's solver."""
import numpy as np
import pytest

import ba_synth
import pose_tables_ref as R


def literal_gather(sc, frame):
    """poseBundleAdjust's two loops over keyframe.mapPoints with a dictionary of map points: the count of :403-407, then vertices and
    edges in keypoint order (:453-480), the measurement of setMapPointMeasurement (:43-57)."""
    n_mp, s = sc["n_mp"], frame["slot"]
    mapPoints = {r: dict(status=int(sc["mp_flags"][r]), position=[float(v) for v in sc["mp_pos"][r]]) for r in range(n_mp) if sc["mp_live"][r]}
    keyframe_mapPoints = [int(r) if (0 <= r < n_mp and int(r) in mapPoints) else -1 for r in sc["kf_mp"][s, :frame["n_kp"]]]
    triangulated = 0
    for mp in keyframe_mapPoints:                            # :403-407
        if mp != -1 and mapPoints[mp]["status"] & 1:
            triangulated += 1
    fx, fy, cx, cy = (float(v) for v in frame["cam"][:4])
    point, uv, info = [], [], []
    for i, mp in enumerate(keyframe_mapPoints):              # :453-480
        if mp == -1:
            continue
        if not mapPoints[mp]["status"] & 1:
            continue
        point.append(mapPoints[mp]["position"])
        uv.append([(float(sc["kp"]["x"][s, i]) - cx) / fx, (float(sc["kp"]["y"][s, i]) - cy) / fy])
        f = float(int(frame["focal"]))
        info.append(f * f / float(sc["sigma"][int(sc["kp"]["octave"][s, i])]))
    pose = [R.pose_of_matrix(sc["poses"][s]), R.pose_of_matrix(sc["poses"][frame["prev_slot"]])]
    return dict(n=triangulated, pose=np.array(pose).reshape(2, 7), point=np.array(point).reshape(-1, 3), obs_uv=np.array(uv).reshape(-1, 2), obs_info=np.array(info, np.float64))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_gather_equals_the_literal_walk(name):
    sc, frame, g = R.cached(name)
    R.scene_conditions(name, sc, frame, g)
    want = literal_gather(sc, frame)
    assert g["n"] == want["n"] == len(g["kept"])
    for k in ("pose", "point", "obs_uv", "obs_info"):
        assert same_bits(g[k], want[k]), k
    assert same_bits(g["obs_point"], np.arange(g["n"], dtype=np.int32)) and not g["obs_pose"].any()


def test_a_bad_octave_counts_only_on_a_kept_keypoint():
    sc, frame, g = R.cached("base")
    sc = dict(sc, kp={k: v.copy() for k, v in sc["kp"].items()})
    dropped = np.setdiff1d(np.arange(frame["n_kp"]), g["kept"])
    sc["kp"]["octave"][R.FRAME, dropped[3]] = R.N_LEVELS
    assert R.gather(sc, frame)["bad_octaves"] == 0
    sc["kp"]["octave"][R.FRAME, g["kept"][3]] = -1
    assert R.gather(sc, frame)["bad_octaves"] == 1


def test_the_restated_problem_moves_the_pose(oracle):
    sc, frame, g = R.cached("base")
    prob = R.problem(frame, g)
    res = oracle.ba_solve(prob, frame["max_iters"], False)
    st = res["stats"]
    print("base scene: %d points, chi2 %.2f -> %.2f in %d iterations" % (g["n"], st["chi2_init"], st["chi2_final"], st["iters"]))
    assert st["chi2_final"] < 0.8 * st["chi2_init"] and st["iters"] >= 1
    assert same_bits(res["pose"][1], prob["pose"][1]) and same_bits(res["point"], prob["point"])             # the fixed vertices
    after, ran = R.apply(sc["poses"], frame, g, res["pose"][0])
    assert ran and not same_bits(after[R.FRAME], sc["poses"][R.FRAME])
    others = [s for s in range(sc["n_kf"]) if s != R.FRAME]
    assert same_bits(after[others], sc["poses"][others])
    # the solved pose is nearer the truth than the table's
    t = sc["true"]
    true = np.concatenate([t["R"][R.FRAME], (-t["R"][R.FRAME] @ t["c"][R.FRAME])[:, None]], 1).reshape(12)
    assert np.abs(after[R.FRAME] - true).max() < np.abs(sc["poses"][R.FRAME] - true).max()


def test_below_the_threshold_nothing_moves():
    sc, frame, g = R.cached("base")
    solved = g["pose"][0] + 0.01
    for min_visible, want_ran in ((g["n"] + 1, False), (g["n"], True)):
        after, ran = R.apply(sc["poses"], dict(frame, min_visible=min_visible), g, solved)
        assert ran == want_ran and same_bits(after, sc["poses"]) != want_ran
    after, ran = R.apply(sc["poses"], frame, g, solved, finite=False)
    assert not ran and same_bits(after, sc["poses"])
    after, ran = R.apply(sc["poses"], dict(frame, prev_slot=-1), g, solved)
    assert not ran and same_bits(after, sc["poses"])
