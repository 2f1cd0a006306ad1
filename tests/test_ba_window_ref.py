"""tests/ba_window_ref.py, the specification of ms_ba_window_lists and ms_ba_window_apply, against itself on the CPU: the
vectorised restatement equals a literal dictionary walk written like bundle_adjuster.cpp:214-290 and :376-390, the pose conversion meets
every branch of Eigen's and returns through the rotation matrix, and the scenes of the GPU tests hold what those tests rely on."""
import numpy as np
import pytest

import ba_window_ref as R

GATHERED = ("pose", "point", "obs_point", "obs_pose", "obs_uv", "obs_info", "edge_slot", "edge_kp", "edge_point", "rows")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def twice_scene():
    """4 slots x 6: row 2 is bound twice in slot 1 and once in slot 3, slot 0 is not local."""
    rng = np.random.default_rng(3)
    sc = dict(n_kf=4, stride=6, n_mp=5, kf_id=np.array([7, 9, -1, 2], np.int32), mp_flags=np.array([3, 2, 3, 3, 0], np.uint8))
    return R.finish(sc, rng, [[0, 2, 3], [2, 0, 2, 1], [2, 3], [3, 2, 4]])


def test_gather_equals_the_literal_walk_on_the_base_scene():
    sc, w = R.cached("base")
    lit = R.literal_gather(sc, R.BASE_LOCAL, 0)
    for k in GATHERED:
        assert same_bits(w[k], lit[k]), k
    assert (w["n_edge"], w["n_current"]) == (lit["n_edge"], lit["n_current"])
    # the current keyframe's count is not a property of position 0
    for cur in (3, 7):
        assert R.gather(sc, R.BASE_LOCAL, cur)["n_current"] == R.literal_gather(sc, R.BASE_LOCAL, cur)["n_current"] > 0


def test_gather_equals_the_literal_walk_with_a_row_bound_twice_in_a_slot():
    sc = twice_scene()
    local = (1, 3)
    w, lit = R.gather(sc, local, 0), R.literal_gather(sc, local, 0)
    for k in GATHERED:
        assert same_bits(w[k], lit[k]), k
    assert (w["n_edge"], w["n_current"]) == (lit["n_edge"], lit["n_current"])
    assert list(w["rows"]) == [0, 2, 3] and w["n_current"] == 3
    two = np.nonzero((w["edge_slot"] == 1) & (w["rows"][w["edge_point"]] == 2))[0]
    assert len(two) == 2 and two[1] == two[0] + 1 and w["edge_kp"][two[0]] < w["edge_kp"][two[1]]       # both kept, ascending keypoint


def test_base_scene_conditions():
    sc, w = R.cached("base")
    R.base_conditions(sc, w)


def test_big_scene_conditions():
    sc, w = R.cached("big")
    carry = R.big_conditions(sc, w)
    print("72 000 listed observations, %d kept, %d of them in the first trip of the offsets scan" % (w["n_edge"], carry))
    chi2 = R.big_chi2(w)
    _, erased, _ = R.apply(R.state_of(sc), w, w["pose"], w["point"], chi2, R.LOCAL)
    assert w["n_edge"] > R.APPLY_TRIP and (erased < R.APPLY_TRIP).any() and (erased >= R.APPLY_TRIP).any() and (np.diff(erased) > 0).all()


@pytest.mark.parametrize("mode", [R.LOCAL, R.NEIGHBOR])
def test_apply_equals_the_literal_loop(mode):
    sc, w = R.cached("base")
    rng = np.random.default_rng(11)
    chi2 = R.base_chi2(sc, w)
    pose = w["pose"] + rng.normal(0, 1e-3, w["pose"].shape)
    point = w["point"] + rng.normal(0, 1e-2, w["point"].shape)
    got, erased, n_stale = R.apply(R.state_of(sc), w, pose, point, chi2, mode)
    want, erased_lit, _ = R.literal_apply(R.state_of(sc), w, pose, point, chi2, mode)
    for k in want:
        assert same_bits(got[k], want[k]), k
    assert n_stale == 0 and same_bits(erased, erased_lit)
    if mode == R.LOCAL:
        R.apply_conditions(sc, w, chi2, got)
        assert len(erased) == sum(len(g) for _, _, g in R.BASE_APPLY.values())
    else:
        before = R.state_of(sc)
        assert len(erased) == 0 and all(same_bits(got[k], before[k]) for k in ("kf_mp", "n_obs", "mp_flags"))
        others = [s for s in range(sc["n_kf"]) if s != R.BASE_LOCAL[0]]
        assert same_bits(got["poses"][others], before["poses"][others]) and not same_bits(got["poses"][R.BASE_LOCAL[0]], before["poses"][R.BASE_LOCAL[0]])


def test_a_stale_edge_is_skipped_and_counted():
    sc, w = R.cached("base")
    chi2 = np.full(w["n_edge"], np.inf)
    st = R.state_of(sc)
    e = 17
    st["kf_mp"][w["edge_slot"][e], w["edge_kp"][e]] = 399
    got, erased, n_stale = R.apply(st, w, w["pose"], w["point"], chi2, R.LOCAL)
    assert n_stale == 1 and e not in erased and len(erased) == w["n_edge"] - 1 and got["kf_mp"][w["edge_slot"][e], w["edge_kp"][e]] == 399


# ---- the pose conversion
def rotations():
    """Rotations about axes and by angles that reach each branch of Eigen's conversion and both signs of w before normalizeRotation."""
    rng = np.random.default_rng(2)
    out = []
    for axis in (np.array([1.0, 0.2, 0.1]), np.array([0.1, 1.0, 0.2]), np.array([0.2, 0.1, 1.0]), np.array([1.0, 1.0, 1.0])):
        for angle in (0.3, -0.3, 2.0, 3.0, -3.0, 3.1, -3.1):
            a = axis / np.linalg.norm(axis) * angle
            th = np.linalg.norm(a)
            K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) / th
            out.append(np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K)
    out += [R.rotation(rng, rng.uniform(0, np.pi)) for _ in range(40)]
    return out


def test_quaternion_branches_and_round_trip():
    Rs = rotations()
    seen = set()
    worst = 0.0
    margin = 0.0
    for M in Rs:
        q, branch, flipped = R.quat_of_matrix(M.reshape(9))
        seen.add((branch, flipped))
        assert q[3] >= 0.0 and abs(sum(v * v for v in q) - 1.0) < 4e-16
        back = np.array(R.matrix_of_pose(q + [0.0, 0.0, 0.0])).reshape(3, 4)[:, :3]
        worst = max(worst, float(np.abs(back - M).max()))
        # the restatement's own error: the same trip on the same pose after a re-orthonormalisation (the nearest rotation, by SVD)
        U, _, Vt = np.linalg.svd(M)
        O = U @ Vt
        q2, _, _ = R.quat_of_matrix(O.reshape(9))
        back2 = np.array(R.matrix_of_pose(q2 + [0.0, 0.0, 0.0])).reshape(3, 4)[:, :3]
        margin = max(margin, float(np.abs(back2 - O).max()))
    print("round trip through the quaternion: largest element-wise difference %.3e, the restatement's own on re-orthonormalised input %.3e" % (worst, margin))
    assert {b for b, _ in seen} == {0, 1, 2, 3}, seen
    assert {f for b, f in seen if b != 3} == {False, True}, seen         # trace > 0 gives w > 0 always
    assert worst <= margin


def test_pose_written_back_reproduces_the_table_rotation():
    sc, w = R.cached("base")
    margin = R.round_trip_margin()
    got, _, _ = R.apply(R.state_of(sc), w, w["pose"], w["point"], np.zeros(w["n_edge"]), R.LOCAL)
    diff = float(np.abs(got["poses"][list(R.BASE_LOCAL)] - sc["poses"][list(R.BASE_LOCAL)]).max())
    print("pose -> quaternion -> pose on the base scene: %.3e, margin %.3e" % (diff, margin))
    assert diff <= margin
    assert same_bits(got["poses"].reshape(-1, 3, 4)[:, :, 3], sc["poses"].reshape(-1, 3, 4)[:, :, 3])          # t is copied
