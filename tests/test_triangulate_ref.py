"""CPU checks of tests/triangulate_ref.py, the specification of ms_triangulate: the pinned solvers against their defining
properties and against LAPACK, every reason code and every failure-path position write on constructed cases, and the fixtures of the GPU
test (tests/test_gpu_triangulate.py): no decision of theirs lies within a relative 1e-6 of its threshold, they produce every reason code,
and POSITION_REL_DIFF is what the fixtures measure."""
import numpy as np
import pytest

import triangulate_ref as R

D = np.float64


def scene(n_kf=20, seed=5):
    rng = np.random.default_rng(seed)
    poses, cams, focal = R.make_keyframes(rng, n_kf, special=False)
    return rng, poses, cams, focal


def exact_observations(poses, cams, ks, X):
    """The observations of X from the keyframes ks with normalized points that no pixel grid has rounded."""
    P = poses[ks]
    pc = [P[:, 4 * r] * X[0] + P[:, 4 * r + 1] * X[1] + P[:, 4 * r + 2] * X[2] + P[:, 4 * r + 3] for r in range(3)]
    return R.observe_normalized(P, cams[ks], pc[0] / pc[2], pc[1] / pc[2])


def point_in_front(rng):
    return np.array([rng.uniform(0.0, 2.0), rng.uniform(-1.0, 1.0), rng.uniform(3.0, 9.0)])


def test_lindstrom_meets_the_epipolar_constraint_and_the_dlt_point_reprojects_onto_the_corrected_points():
    rng, poses, cams, _ = scene()
    worst_epipolar = worst_reprojection = 0.0
    for _ in range(2000):
        ks = np.sort(rng.choice(20, 2, replace=False))
        o = exact_observations(poses, cams, ks, point_in_front(rng))
        o["xn"] = o["xn"] + rng.normal(0.0, 2e-3, 2)                                                 # a pixel at f = 500
        o["yn"] = o["yn"] + rng.normal(0.0, 2e-3, 2)
        parts = {}
        ok, h = R.triangulate_two_view(o, 0, 1, parts=parts)
        assert ok
        E = np.array(parts["E"], D)
        x1, x2 = np.array(parts["x1"] + [1.0], D), np.array(parts["x2"] + [1.0], D)
        worst_epipolar = max(worst_epipolar, abs(x2 @ E @ x1))
        p = np.array(h[:3], D) / h[3]
        for P, x in ((o["P"][0], x1), (o["P"][1], x2)):
            pc = P.reshape(3, 4) @ np.append(p, 1.0)
            worst_reprojection = max(worst_reprojection, np.abs(pc[:2] / pc[2] - x[:2]).max())
    print("epipolar residual %.3e, reprojection onto the corrected points %.3e" % (worst_epipolar, worst_reprojection))
    assert worst_epipolar <= 3.3e-13
    assert worst_reprojection <= 1e-9


@pytest.mark.parametrize("solver", ["nview", "two_view", "midpoint"])
def test_solvers_recover_noise_free_points(solver):
    rng, poses, cams, _ = scene(seed=6)
    worst = 0.0
    for _ in range(300):
        n = 2 if solver == "two_view" else int(rng.integers(3, 40)) if solver == "nview" else int(rng.integers(2, 40))
        ks = np.sort(rng.choice(20, n, replace=n > 20))
        if len(set(ks.tolist())) < 2:
            continue
        X = point_in_front(rng)
        o = exact_observations(poses, cams, ks, X)
        ok, h = (R.triangulate_nview(o) if solver == "nview" else R.triangulate_two_view(o, 0, 1) if solver == "two_view" else R.triangulate_midpoint(o))
        assert ok
        worst = max(worst, np.abs(np.array(h[:3], D) / h[3] - X).max() / np.abs(X).max())
    print("%s: %.3e" % (solver, worst))
    assert worst <= 1e-9


@pytest.mark.parametrize("n", [3, 4])
def test_jacobi_agrees_with_lapack(n):
    rng = np.random.default_rng(7)
    for _ in range(200):
        B = rng.normal(size=(n + 2, n)) * 10.0 ** rng.uniform(-3, 3, n)                               # badly scaled columns, as the fourth column of A is
        A = B.T @ B
        A = (A + A.T) / 2
        w, V = R.jacobi(A.tolist())
        V = np.array(V, D)
        assert np.abs(V.T @ V - np.eye(n)).max() < 1e-14
        assert np.allclose(np.sort(np.array(w, D)), np.linalg.eigvalsh(A), rtol=1e-10, atol=1e-13 * np.abs(A).max())
        assert np.abs(V @ np.diag(w) @ V.T - A).max() <= 1e-13 * np.abs(A).max()


def test_tree_sum_is_the_stated_tree():
    v = np.random.default_rng(8).normal(size=37)
    rounds = []
    for base in (0, 16, 32):
        w = [v[base + i] if base + i < 37 else 0.0 for i in range(16)]
        a = [w[i] + w[i + 8] for i in range(8)]
        a = [a[i] + a[i + 4] for i in range(4)]
        a = [a[i] + a[i + 2] for i in range(2)]
        rounds.append(a[0] + a[1])
    assert R.tree_sum(v) == ((0.0 + rounds[0]) + rounds[1]) + rounds[2]
    assert R.tree_sum(np.zeros(0)) == 0.0


# ---------------------------------------------------------------------------------------------------- constructed cases
S = R.settings()
ENTRY = np.array([7.0, -8.0, 9.0])                           # the position a point holds on entry


class Case:
    """One map point seen from the keyframes ks of a small corridor, pixels rounded to float32."""

    def __init__(self, ks, X=(0.7, 0.2, 6.0), seed=11):
        _, self.poses, self.cams, self.focal = scene(12, seed)
        self.kf = np.array(ks, np.int64)
        uvz = [R.project(self.poses, self.cams, k, np.array(X, D)) for k in ks]
        self.x = np.array([u for u, v, z in uvz], np.float32)
        self.y = np.array([v for u, v, z in uvz], np.float32)
        self.z = [z for u, v, z in uvz]
        self.octave = np.full(len(ks), 4, np.int64)
        self.depth = None
        self.X = np.array(X, D)

    def run(self, mode, was=False, settings=S, quantities=None):
        pos, status, reason, n_pass = R.triangulate_point(ENTRY, was, self.kf, self.x, self.y, self.octave, self.depth, self.poses, self.cams, self.focal,
                                                          settings, mode, quantities=quantities)
        return np.array(pos, D), status, reason, n_pass


ALL_MODES = (R.TME, R.MIDPOINT, R.FIRST_LAST)


@pytest.mark.parametrize("mode", ALL_MODES)
def test_success_and_its_status(mode):
    for ks, status in (((0, 11), R.UNSURE), ((0, 5, 11), R.TRIANGULATED), ((4, 5, 6), R.TRIANGULATED if mode == R.FIRST_LAST else R.UNSURE)):
        pos, st, reason, n_pass = Case(ks).run(mode)         # 4, 5, 6: 0.2 apart at 6 m is 1.9 degrees, between the two angles
        assert (st, reason) == (status, R.R_NONE)
        assert np.abs(pos - Case(ks).X).max() < 0.05
        assert n_pass == (len(ks) if mode == R.FIRST_LAST else 0)


@pytest.mark.parametrize("mode", ALL_MODES)
def test_reason_1_fewer_than_two_observations(mode):
    for ks in ((), (3,)):
        pos, st, reason, n_pass = Case(ks).run(mode, was=True)
        assert (st, reason, n_pass) == (R.NOT_TRIANGULATED, R.R_FEW_OBSERVATIONS, 0) and np.array_equal(pos, ENTRY)


@pytest.mark.parametrize("mode", ALL_MODES)
def test_reason_2_triangulation_angle(mode):
    for ks in ((5, 6), (5, 6, 6) if mode != R.FIRST_LAST else (5, 0, 6)):                             # 0.1 apart at 6 m: 0.95 degrees
        pos, st, reason, _ = Case(ks).run(mode)
        assert (st, reason) == (R.NOT_TRIANGULATED, R.R_ANGLE) and np.array_equal(pos, ENTRY)


def test_reason_3_solver_failure():
    c = Case((0, 11))
    c.poses[11, 3::4] = 1e200                                # the rays do not see the translation, the solvers overflow
    for mode in (R.TME, R.FIRST_LAST):
        pos, st, reason, _ = c.run(mode)
        assert (st, reason) == (R.NOT_TRIANGULATED, R.R_SOLVER) and np.array_equal(pos, ENTRY)
    c = Case((0, 5, 11))
    c.poses[5, 0] = np.nan                                   # a NaN ray: the pair (0, 11) still passes the angle check
    for mode in (R.TME, R.MIDPOINT):
        pos, st, reason, _ = c.run(mode)
        assert (st, reason) == (R.NOT_TRIANGULATED, R.R_SOLVER) and np.array_equal(pos, ENTRY)
    q = []
    c.run(R.MIDPOINT, quantities=q)
    assert [name for name, _, _ in q] == ["angle", "pivot"] and np.isnan(q[1][1])


@pytest.mark.parametrize("mode", (R.TME, R.MIDPOINT))
def test_reason_4_negative_depth(mode):
    pos, st, reason, _ = Case((0, 11), X=(0.7, 0.2, -6.0)).run(mode)                                  # the lines meet behind the cameras
    assert (st, reason) == (R.NOT_TRIANGULATED, R.R_DEPTH) and np.array_equal(pos, ENTRY)


@pytest.mark.parametrize("mode", (R.TME, R.MIDPOINT))
def test_reason_5_reprojection_error(mode):
    c = Case((0, 5, 11))
    c.y[1] += 30.0
    pos, st, reason, _ = c.run(mode)
    assert (st, reason) == (R.NOT_TRIANGULATED, R.R_REPROJECTION) and np.array_equal(pos, ENTRY)
    c = Case((0, 5, 11))
    c.octave[:] = (7, 0, 7)                                  # the limit follows the octave (2.4 px at octave 0, 8.5 px at octave 7)
    c.y[1] += 5.0
    assert c.run(mode)[2] == R.R_REPROJECTION
    c.octave[:] = 7
    assert c.run(mode)[2] == R.R_NONE


def test_reason_6_and_the_position_written_before_the_checks():
    c = Case((0, 11))
    c.y[1] += 40.0
    pos, st, reason, n_pass = c.run(R.FIRST_LAST)
    assert (st, reason, n_pass) == (R.NOT_TRIANGULATED, R.R_FEW_PASSING, 0)
    assert np.all(np.isfinite(pos)) and not np.array_equal(pos, ENTRY)                                # :776
    c = Case((0, 3, 11))
    c.y[1] += 40.0                                           # the middle observation fails, the two the point came from pass
    assert c.run(R.FIRST_LAST)[1:] == (R.TRIANGULATED, R.R_NONE, 2)
    c.y[2] += 40.0
    pos, st, reason, n_pass = c.run(R.FIRST_LAST)
    assert (st, reason) == (R.NOT_TRIANGULATED, R.R_FEW_PASSING) and n_pass < 2 and not np.array_equal(pos, ENTRY)


def test_first_last_has_no_positive_depth_test():
    c = Case((0, 11), X=(0.7, 0.2, -6.0))
    pos, st, reason, n_pass = c.run(R.FIRST_LAST)            # behind both cameras: reproject says invisible, so no observation passes
    assert (st, reason, n_pass) == (R.NOT_TRIANGULATED, R.R_FEW_PASSING, 0) and pos[2] < 0.0


def test_reason_7_dense_stereo_skip():
    dense = R.settings(dense_stereo_depth=True)
    c = Case((0, 5, 11))
    pos, st, reason, _ = c.run(R.FIRST_LAST, settings=dense)
    assert (st, reason) == (R.NOT_TRIANGULATED, R.R_DENSE_SKIP) and np.array_equal(pos, ENTRY)
    c.depth = np.array([0.0, 0.0, c.z[2]], np.float32)                                               # with a depth on the last observation the flag is not read
    assert c.run(R.FIRST_LAST, settings=dense)[1:] == (R.TRIANGULATED, R.R_NONE, 3)
    for mode in (R.TME, R.MIDPOINT):
        assert Case((0, 5, 11)).run(mode, settings=dense)[1] == R.TRIANGULATED                        # a FIRST_LAST flag


@pytest.mark.parametrize("mode", (R.TME, R.MIDPOINT))
@pytest.mark.parametrize("at", (0, 1, 2))
def test_depth_branch_writes_the_position_inside_the_loop(mode, at):
    c = Case((0, 5, 11))
    c.depth = np.array([-1.0, 0.0, -1.0], np.float32)
    c.depth[at] = c.z[at]
    o = R.observe(c.poses, c.cams, c.kf, c.x, c.y)
    from_depth = np.array(R.depth_position(o, at, c.depth[at]), D)
    pos, st, reason, _ = c.run(mode)
    assert (st, reason) == (R.UNSURE, R.R_NONE) and np.array_equal(pos, from_depth) and np.abs(pos - c.X).max() < 1e-3
    assert c.run(mode, was=True)[1] == R.TRIANGULATED        # a point that was triangulated ignores the depths (:621)
    c.x[2 if at != 2 else 0] += 30.0                         # a later (or earlier) check fails: the position stays written (:622)
    pos, st, reason, _ = c.run(mode)
    assert (st, reason) == (R.NOT_TRIANGULATED, R.R_REPROJECTION) and np.array_equal(pos, from_depth)
    pos, st, reason, _ = c.run(mode, was=True)
    assert (st, reason) == (R.NOT_TRIANGULATED, R.R_REPROJECTION) and np.array_equal(pos, ENTRY)


def test_first_last_depth_on_the_last_observation():
    c = Case((0, 5, 11))
    c.depth = np.array([c.z[0], c.z[1], 0.0], np.float32)                                            # only the last observation's depth counts
    o = R.observe(c.poses, c.cams, c.kf, c.x, c.y)
    pos, st, reason, n_pass = c.run(R.FIRST_LAST, was=True)
    assert (st, reason, n_pass) == (R.TRIANGULATED, R.R_NONE, 3) and not np.array_equal(pos, ENTRY)
    c.depth[2] = 2.0 * c.z[2]                                # a wrong depth: written (:746), then too few observations pass
    pos, st, reason, n_pass = c.run(R.FIRST_LAST, was=True)
    assert (st, reason, n_pass) == (R.NOT_TRIANGULATED, R.R_FEW_PASSING, 1)
    assert np.array_equal(pos, np.array(R.depth_position(o, 2, c.depth[2]), D))


def test_triangulate_touches_listed_rows_only_and_resets_every_listed_flag():
    c = Case((0, 5, 11))
    mp_pos = np.arange(15, dtype=D).reshape(5, 3)
    mp_flags = np.array([1, 1, 3, 3, 1], np.uint8)
    prob = dict(rows=[3, 1, 2], was_triangulated=[1, 0, 1], obs_start=[0, 3, 3, 4], obs_kf=[0, 5, 11, 2], obs_x=list(c.x) + [5.0], obs_y=list(c.y) + [6.0],
                obs_octave=[4, 4, 4, 0], obs_depth=None)
    pos, flags, status, reason, n_pass = R.triangulate(mp_pos, mp_flags, c.poses, c.cams, c.focal, prob, S, R.TME)
    assert status.tolist() == [R.TRIANGULATED, 0, 0] and reason.tolist() == [0, 1, 1] and flags.tolist() == [1, 0, 0, 3, 1]
    assert np.array_equal(pos[[0, 1, 2, 4]], mp_pos[[0, 1, 2, 4]]) and np.abs(pos[3] - c.X).max() < 0.05
    assert R.triangulate(mp_pos, None, c.poses, c.cams, c.focal, prob, S, R.TME)[1] is None


# ---------------------------------------------------------------------------------------------------- the fixtures of the GPU test
def test_fixtures_hold_every_observation_count_reason_and_status():
    sc = R.make_scene()
    counts = np.diff(sc["prob"]["obs_start"])
    assert set(R.OBS_COUNTS) <= set(counts.tolist()) and len(sc["prob"]["rows"]) == R.POINTS_PER_CALL[-1]
    assert len(set(sc["prob"]["rows"].tolist())) == len(sc["prob"]["rows"]) and sc["poses"].shape == (70, 12)
    assert set(counts[:65].tolist()) >= set(R.OBS_COUNTS)                                           # the small calls hold the long lists too
    reasons, statuses = set(), set()
    for mode, with_depth, dense in R.FIXTURES:
        f = R.fixture(mode, with_depth, dense)
        reasons |= set((mode, int(r)) for r in f["reason"])
        statuses |= set((mode, int(s)) for s in f["status"])
        assert f["n_pass"].max() == (300 if mode == R.FIRST_LAST else 0)
    for mode in (R.TME, R.MIDPOINT):
        assert {r for m, r in reasons if m == mode} == {0, 1, 2, 3, 4, 5}
    assert {r for m, r in reasons if m == R.FIRST_LAST} == {0, 1, 2, 3, 6, 7}
    assert statuses == {(m, s) for m in ALL_MODES for s in (0, 1, 2)}
    # depth on the first, a middle and the last observation, with was_triangulated both ways
    f = R.fixture(R.TME, True)
    start, depth, was = f["prob"]["obs_start"], f["prob"]["obs_depth"], f["prob"]["was_triangulated"]
    seen = set()
    for r in range(len(was)):
        d = np.flatnonzero(depth[start[r]:start[r + 1]] > 0)
        n = start[r + 1] - start[r]
        if len(d) and n >= 3:
            seen.add(("first" if d[0] == 0 else "last" if d[0] == n - 1 else "middle", int(was[r])))
    assert seen == {(w, b) for w in ("first", "middle", "last") for b in (0, 1)}


def test_no_fixture_decision_lies_within_1e_6_of_its_threshold():
    near, total = [], 0
    for mode, with_depth, dense in R.FIXTURES:
        f = R.fixture(mode, with_depth, dense)
        for entry, quantities in enumerate(f["quantities"]):
            for name, value, threshold in quantities:
                total += 1
                if R.margin(name, value, threshold) < 1e-6:
                    near.append((mode, with_depth, dense, entry, name, float(value), float(threshold)))
    print("%d decisions" % total)
    assert total > 50000 and near == []                      # zero near cases: the GPU test leaves out nothing


def test_position_rel_diff_is_the_fixtures_measurement():
    measured = R.measure_position_difference()
    print("measured %.3e" % measured)
    # LAPACK's own rounding differs from build to build, so the constant is held to the measurement within a factor of four either way
    assert 0.25 * R.POSITION_REL_DIFF <= measured <= 4.0 * R.POSITION_REL_DIFF
    assert R.GPU_POSITION_TOLERANCE == 100.0 * R.POSITION_REL_DIFF
