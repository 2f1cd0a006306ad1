"""The restatement tests/map_refresh_ref.py (the specification of ms_map_refresh / ms_loop_correct) against hand-computed cases, its
medoid against the oracle's, and the measurement of the tolerance the GPU tests hold the interpolated poses to."""
import math

import numpy as np
import pytest

import map_refresh_ref as R

F = np.float32
IDENTITY_POSE = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def one_row_table(pos):
    return dict(pos=np.array([pos], np.float64), norm=np.full((1, 3), 9, F), min_dist=np.zeros(1, F), max_dist=np.zeros(1, F), desc=np.zeros((1, 8), np.uint32))


def problem(obs_kf, octave, obs_desc=None):
    return dict(rows=np.array([0], np.int32), obs_start=np.array([0, len(obs_kf)], np.int32), obs_kf=np.array(obs_kf, np.int32),
                obs_desc=None if obs_desc is None else np.array(obs_desc, np.int32), first_octave=np.array([octave], np.int32))


def test_one_observation():
    """Identity rotation, t = (0, 0, -2): the camera centre is (0, 0, 2).  The point at the origin: normal (0, 0, 1), distance 2."""
    sf = R.scale_factors()
    pose = IDENTITY_POSE.copy(); pose[11] = -2
    pool = np.arange(16, dtype=np.uint32).reshape(2, 8)
    out, med = R.refresh(one_row_table((0, 0, 0)), [pose], pool, problem([0], 1, [1]), sf)
    assert np.array_equal(out["norm"][0], F([0, 0, 1]))
    assert out["max_dist"][0] == F(2) * sf[1] and out["min_dist"][0] == (F(2) * sf[1]) / sf[7]
    assert med[0] == 0 and np.array_equal(out["desc"][0], pool[1])


def test_two_observations_and_a_zero_term():
    """Centres (0, 0, 2) and (3, 0, 0), the point at (3, 0, 0): the second term is the zero vector and stays one (no division by zero), so the
    sum is the first unit vector alone and the normal is half of it; the distances come from the first observation."""
    sf = R.scale_factors()
    a = IDENTITY_POSE.copy(); a[11] = -2
    b = IDENTITY_POSE.copy(); b[3] = -3
    out, med = R.refresh(one_row_table((3, 0, 0)), [a, b], None, problem([0, 1], 0), sf)
    d = math.sqrt(13.0)
    want = (np.array([-3 / d, 0 / d, 2 / d]) + 0.0).astype(F) / F(2)
    assert np.array_equal(out["norm"][0], want) and np.isfinite(out["norm"]).all()
    assert out["max_dist"][0] == F(d) * sf[0] and out["min_dist"][0] == F(d) / sf[7]
    assert med[0] == -1 and not out["desc"].any()
    # the same observations the other way round: the distances now come from the zero vector
    out, _ = R.refresh(one_row_table((3, 0, 0)), [a, b], None, problem([1, 0], 3), sf)
    assert np.array_equal(out["norm"][0], want) and out["max_dist"][0] == 0 and out["min_dist"][0] == 0


def test_rows_without_descriptors_and_beyond_the_cap_keep_theirs():
    sf = R.scale_factors()
    pool = np.arange(8 * 300, dtype=np.uint32).reshape(300, 8)
    t = one_row_table((1, 2, 3)); t["desc"][0] = 77
    out, med = R.refresh(t, [IDENTITY_POSE], pool, problem([0, 0], 2, [-1, -1]), sf)
    assert med[0] == -1 and (out["desc"][0] == 77).all()
    out, med = R.refresh(t, [IDENTITY_POSE], pool, problem([0] * 257, 2, list(range(257))), sf)
    assert med[0] == -2 and (out["desc"][0] == 77).all() and out["max_dist"][0] > 0
    out, med = R.refresh(t, [IDENTITY_POSE], pool, problem([0] * 257, 2, [-1] + list(range(256))), sf)
    assert med[0] >= 1                                           # 256 descriptors fit; the position counts the observation without one


def test_medoid_equals_the_oracles(oracle):
    sc = R.make_refresh_scene()
    prob, pool = sc["prob"], sc["pool"]
    checked = 0
    for r in range(len(prob["rows"])):
        od = prob["obs_desc"][prob["obs_start"][r]:prob["obs_start"][r + 1]]
        od = od[od != -1]
        if 0 < len(od) <= R.MEDOID_MAX_OBS:
            assert R.medoid_of(pool[od]) == oracle.descriptor_medoid(pool[od]), r
            checked += 1
    assert checked > 290


def test_scene_has_the_lengths_and_special_rows():
    sc = R.make_refresh_scene()
    assert tuple(sc["lengths"][:8]) == R.REFRESH_LENGTHS == (1, 2, 3, 63, 64, 65, 256, 257)
    assert len(sc["kf_pose"]) == 40 and len(sc["prob"]["rows"]) == 300 == len(set(sc["prob"]["rows"].tolist()))
    out, med = R.refresh(sc["table"], sc["kf_pose"], sc["pool"], sc["prob"], sc["sf"])
    assert med[7] == -2 and med[12] == -1 and (med[:7] >= 0).all() and med[13] % 2 == 1
    prob = sc["prob"]
    s9 = prob["obs_start"][9]
    term = R.pose_centre(sc["kf_pose"][prob["obs_kf"][s9 + 1]]) - sc["table"]["pos"][prob["rows"][9]]
    assert not term.any()                                        # the zero term
    assert prob["first_octave"][10] == 0 and prob["first_octave"][11] == 7
    untouched = np.setdiff1d(np.arange(400), prob["rows"])
    for k in ("norm", "min_dist", "max_dist", "desc"):
        assert np.array_equal(out[k][untouched], sc["table"][k][untouched])
        assert not np.array_equal(out[k][prob["rows"]], sc["table"][k][prob["rows"]])


@pytest.mark.parametrize("n_rows,longest_last", R.SCAN_CASES)
def test_scan_scenes_put_the_special_lists_where_the_trips_of_the_descriptor_scan_meet(n_rows, longest_last):
    # what tests/test_gpu_scan_trips.py relies on: equal neighbouring offsets across the first trip's end, and the longest list (which sizes
    # the medoid pass) in the first trip for one order and in the last trip for the other, every other trip far below it
    sc = R.make_scan_scene(n_rows, longest_last)
    prob = sc["prob"]
    assert len(prob["rows"]) == n_rows == len(set(prob["rows"].tolist())) and len(sc["kf_pose"]) == 42 and len(sc["table"]["pos"]) == 2600
    n_obs, n_desc = np.diff(prob["obs_start"]), R.descriptor_counts(prob)
    assert np.array_equal(prob["obs_desc"] == -1, prob["obs_kf"] >= 40)      # no descriptor: one of the two added slots, and only then
    for a, b in zip(prob["obs_start"][:-1], prob["obs_start"][1:]):
        assert (np.diff(prob["obs_kf"][a:b]) >= 0).all()                    # slot order, as device-built lists are
    assert n_desc[R.SCAN_TRIP - 1] == 0 and n_desc[R.SCAN_TRIP - 2] > 0
    if n_rows > R.SCAN_TRIP:
        assert 0 < n_desc[R.SCAN_TRIP] < n_obs[R.SCAN_TRIP]
    trips = [n_desc[a:a + R.SCAN_TRIP] for a in range(0, n_rows, R.SCAN_TRIP)]
    assert len(trips) == {1024: 1, 1025: 2, 2100: 3}[n_rows]
    at = len(trips) - 1 if longest_last else 0
    assert sorted(trips[at])[-2:] == [256, 257] and all(t.max() <= 65 for i, t in enumerate(trips) if i != at)
    print(n_rows, longest_last, "observations", int(prob["obs_start"][-1]), "descriptors per trip", [int(t.sum()) for t in trips], "longest per trip",
          [int(t.max()) for t in trips])
    _, med = R.refresh(sc["table"], sc["kf_pose"], sc["pool"], prob, sc["sf"])
    where = np.flatnonzero(n_desc >= 256)
    assert med[where].tolist() == [int(med[where[0]]), -2] and med[where[0]] >= 0 and med[R.SCAN_TRIP - 1] == -1
    assert (med[n_desc > 0] != -1).all() and (med[R.SCAN_TRIP:] >= 0).sum() >= min(n_rows - R.SCAN_TRIP, 1)


def test_lambda_zero_returns_the_pose_and_identity_changes_nothing():
    sc = R.make_loop_scene()
    T = R.loop_transforms()
    prob = dict(sc["prob"]); prob["kf_rigid"] = np.zeros_like(prob["kf_rigid"]); prob["kf_lambda"] = np.zeros_like(prob["kf_lambda"])
    pose, pos = R.loop_correct(sc["kf_pose"], sc["pos"], T["usual"], prob)
    # lambda = 0 is the identity Sim3 exactly (scale0 = sin(theta) / sin(theta) = 1, scale1 = 0); the pose goes through matrix -> quaternion ->
    # matrix once, which is not the identity map on doubles: it comes back to rounding
    assert np.abs(pose - sc["kf_pose"]).max() < 1e-14 and np.abs(pos - sc["pos"]).max() < 1e-13
    assert R.s3_interpolate(R.as_s3(T["usual"]), 0.0) == ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0)
    assert R.s3_interpolate(R.as_s3(T["near_identity"]), 0.0) == ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0)
    pose, pos = R.loop_correct(sc["kf_pose"], sc["pos"], T["identity"], sc["prob"])
    assert np.abs(pose - sc["kf_pose"]).max() < 1e-14 and np.abs(pos - sc["pos"]).max() < 1e-13
    listed = np.zeros(len(sc["kf_pose"]), bool); listed[sc["prob"]["kf_slot"]] = True
    assert np.array_equal(pose[~listed], sc["kf_pose"][~listed])
    moved = np.zeros(len(sc["pos"]), bool); moved[sc["prob"]["mp_row"]] = True
    assert np.array_equal(pos[~moved], sc["pos"][~moved])


def test_lambda_one_is_the_rigid_correction_and_points_keep_their_camera_coordinates():
    sc = R.make_loop_scene()
    for name, T in R.loop_transforms().items():
        q, t, s = R.s3_interpolate(R.as_s3(T), 1.0)
        sign = -1.0 if T[0] < 0 else 1.0                         # slerp ends on the representative in identity's hemisphere
        assert np.allclose(q, sign * np.array(T[:4]), atol=1e-15) and t == tuple(T[4:7]) and s == T[7], name
        pose, pos = R.loop_correct(sc["kf_pose"], sc["pos"], T, sc["prob"])
        # :503 moves a point so that it keeps its coordinates in its reference keyframe's camera
        prob = sc["prob"]
        for j in range(0, len(prob["mp_row"]), 25):
            row, slot = prob["mp_row"][j], prob["kf_slot"][prob["mp_ref"][j]]
            before = sc["kf_pose"][slot].reshape(3, 4) @ np.append(sc["pos"][row], 1.0)
            after = pose[slot].reshape(3, 4) @ np.append(pos[row], 1.0)
            assert np.abs(before - after).max() < 1e-12, name


def test_branches_of_the_scenes():
    """The scenes reach slerp's linear branch, its sign flip and a 179 degree rotation."""
    T = R.loop_transforms()
    assert abs(T["near_identity"][0]) >= 1.0 - R.EPS and max(abs(v) for v in T["near_identity"][1:4]) > 0
    assert T["negative_w"][0] < 0 and abs(2 * math.degrees(math.acos(T["rot179"][0])) - 179.0) < 1e-9
    sc = R.make_loop_scene()
    assert tuple(sc["prob"]["kf_lambda"][6:10]) == R.LOOP_LAMBDAS == (0.0, 1e-9, 0.5, 1.0) and sc["prob"]["kf_rigid"][:6].all() and not sc["prob"]["kf_rigid"][6:].any()


def test_interpolation_tolerance_is_measured_and_recorded():
    """Every acos / sin result of the slerp moved by -2, 0 or +2 ulp (the bound the ROCm device library documents for the float64 functions), all 80
    combinations, over every transform of the loop scene; 4 x the largest change of any pose entry / point coordinate.  Measured here:
    poses 4.44e-15, points 6.57e-14 (translations up to 5, point coordinates up to 8); the recorded values are these rounded up."""
    sc = R.make_loop_scene()
    tol_pose, tol_point = R.interpolation_tolerance(sc, list(R.loop_transforms().values()))
    print("measured tolerance: poses %.3g points %.3g" % (tol_pose, tol_point))
    assert 0 < tol_pose <= R.TOL_POSE and 0 < tol_point <= R.TOL_POINT
    assert R.TOL_POSE < 4 * tol_pose and R.TOL_POINT < 4 * tol_point          # the recorded values are the measurement, not a loose stand-in
