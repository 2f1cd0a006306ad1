"""CPU checks of tests/project_gate_ref.py, the specification of ms_project_gate: hand-computed cases for every gate and mode, and the
condition on the generator's draws that the GPU tests rely on (near_level covers at most 0.1 % of a draw's entries)."""
import numpy as np
import pytest

import project_gate_ref as R

F = np.float32
SF = R.scale_factors(8, 1.2)


def table(pos, norm=(0, 0, -1), dmin=1.0, dmax=8.0):
    return dict(pos=np.array([pos], np.float64), norm=np.array([norm], F), min_dist=np.array([dmin], F), max_dist=np.array([dmax], F),
                desc=np.zeros((1, 8), np.uint32))


def view(mode, threshold=10.0, R_=np.eye(3), t=(0, 0, 0), cos_limit=0.5):
    return dict(R=R_, t=np.array(t, np.float64), cam=R.CAM, threshold=threshold, view_cos_limit=cos_limit, mode=mode, indices=[0])


def test_scale_factors_are_the_float32_product_chain():
    assert SF[0] == 1 and SF[3] == F(1.2) * (F(1.2) * F(1.2)) and SF.dtype == F


@pytest.mark.parametrize("mode,thr,radius", [(R.SEARCH, 10.0, F(0.625) * F(10) * SF[3] / SF[4]), (R.FUSE, 3.0, F(3) * SF[3] / SF[4] * F(2.4477)),
                                             (R.SIM3, 7.5, F(7.5) * SF[3])])
def test_point_on_the_axis_is_kept_with_the_modes_radius(mode, thr, radius):
    # identity pose, depth 4, normal towards the camera: pixel (cx, cy), dist 4, cos 1 (> 0.998: the small-angle factor), ratio 1.2^2.5 -> level 3
    st, x, y, dist, level, rad = R.gate_one(table((0, 0, 4), dmax=float(F(4) * F(1.2) ** F(2.5))), view(mode, thr), SF, 1.2)
    assert (st, x, y, dist, level) == (R.KEPT, 320.0, 240.0, 4.0, 3) and F(rad) == radius


def test_a_wide_angle_takes_the_full_threshold():
    # normal 36.87 deg off the viewing ray: cos 0.8 <= 0.998 -> factor 1
    g = R.gate_view(table((0, 0, 4), norm=(0.6, 0, -0.8), dmax=4.0), view(R.SEARCH, 10.0), SF, 1.2)
    assert g["status"][0] == R.KEPT and g["cos"][0] == F(0.8) and g["level"][0] == 0 and g["radius"][0] == F(10) * SF[0] / SF[4]


@pytest.mark.parametrize("mode", [R.SEARCH, R.FUSE, R.SIM3])
def test_visibility(mode):
    for pos, want in (((0, 0, 0), 1), ((0, 0, -4), 1), ((-320 / 450 * 4, 0, 4), 0), ((320 / 450 * 4, 0, 4), 1), ((0, 1e9, 4), 1), ((np.nan, 0, 4), 1),
                      ((0, 0, np.inf), 1)):
        st, x, y, dist, level, rad = R.gate_one(table(pos, dmin=0.5, dmax=80.0), view(mode), SF, 1.2)
        assert (st == R.NOT_VISIBLE) == bool(want), (pos, st)
        if want:
            assert (x, y, dist, level, rad) == (0, 0, 0, -1, 0)


@pytest.mark.parametrize("mode", [R.SEARCH, R.FUSE, R.SIM3])
def test_distance_bounds_are_inclusive(mode):
    for dmin, dmax, want in ((4.0, 9.0, R.KEPT), (1.0, 4.0, R.KEPT), (np.nextafter(F(4), F(5)), 9.0, R.DISTANCE), (1.0, np.nextafter(F(4), F(0)), R.DISTANCE)):
        st, _, _, dist, level, _ = R.gate_one(table((0, 0, 4), dmin=dmin, dmax=dmax), view(mode), SF, 1.2)
        assert st == want and dist == 4.0 and (level >= 0) == (want == R.KEPT)


def test_sim3_distance_is_the_scaled_camera_frame_norm():
    # rotBAW = 2 I, transBAW = (0, 0, 1): p_c = (0, 0, 9), distance 9 (the world distance 4 would pass [3, 5]; 9 does not)
    assert R.gate_one(table((0, 0, 4), dmin=3.0, dmax=5.0), view(R.SIM3, 7.5, 2 * np.eye(3), (0, 0, 1)), SF, 1.2)[0] == R.DISTANCE
    st, x, y, dist, level, rad = R.gate_one(table((0, 0, 4), dmin=3.0, dmax=9.0), view(R.SIM3, 7.5, 2 * np.eye(3), (0, 0, 1)), SF, 1.2)
    assert (st, x, y, dist, level) == (R.KEPT, 320.0, 240.0, 9.0, 0) and F(rad) == F(7.5)


def test_angle_gate_and_zero_normal():
    half = (np.sqrt(0.75), 0, -0.5)                        # cos exactly 0.5 in float32: kept at the limit, rejected just below
    assert R.gate_one(table((0, 0, 4), norm=half), view(R.SEARCH), SF, 1.2)[0] == R.KEPT
    assert R.gate_one(table((0, 0, 4), norm=half), view(R.FUSE, 3.0), SF, 1.2)[0] == R.KEPT
    below = (np.sqrt(0.75), 0, float(np.nextafter(F(-0.5), F(0))))
    assert R.gate_one(table((0, 0, 4), norm=below), view(R.SEARCH), SF, 1.2)[0] == R.ANGLE
    assert R.gate_one(table((0, 0, 4), norm=below), view(R.FUSE, 3.0), SF, 1.2)[0] == R.ANGLE
    assert R.gate_one(table((0, 0, 4), norm=below), view(R.SEARCH, cos_limit=0.25), SF, 1.2)[0] == R.KEPT       # isInFrustum's own limit
    assert R.gate_one(table((0, 0, 4), norm=below), view(R.SIM3, 7.5), SF, 1.2)[0] == R.KEPT                    # no angle gate
    assert R.gate_one(table((0, 0, 4), norm=(0, 0, 0)), view(R.SEARCH), SF, 1.2)[0] == R.ANGLE                  # cos 0 < 0.5
    assert R.gate_one(table((0, 0, 4), norm=(0, 0, 0)), view(R.FUSE, 3.0), SF, 1.2)[0] == R.ZERO_NORMAL          # :460 comes first
    # the distance gate comes before both
    assert R.gate_one(table((0, 0, 4), norm=(0, 0, 0), dmax=3.0), view(R.FUSE, 3.0), SF, 1.2)[0] == R.DISTANCE


def test_camera_centre_is_minus_rt_t():
    a = 0.3
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    c = np.array([0.5, -0.25, 1.0])
    assert np.allclose(R.camera_centre(Rz, -Rz @ c), c, atol=1e-15)
    # a point 4 in front of that camera along its axis: distance 4 to rounding, pixel (cx, cy)
    p = c + Rz.T @ np.array([0, 0, 4.0])
    st, x, y, dist, _, _ = R.gate_one(table(p, norm=tuple(-(Rz.T @ np.array([0, 0, 1.0])))), view(R.SEARCH, R_=Rz, t=-Rz @ c), SF, 1.2)
    assert st == R.KEPT and abs(x - 320) < 1e-4 and abs(y - 240) < 1e-4 and abs(dist - 4) < 1e-6


def test_level_is_clamped_at_both_ends_and_pinned_for_inf_and_nan():
    lv = lambda dmax, dist: int(R.predict_level(np.array([dmax], F), np.array([dist], F), 1.2, 8)[0][0])
    assert lv(4.0, 4.0) == 0 and lv(3.0, 4.0) == 0                   # ratio <= 1: log <= 0
    assert lv(4.0 * 1.2 ** 6.5, 4.0) == 7 and lv(4.0 * 1.2 ** 30, 4.0) == 7
    assert lv(4.0, 0.0) == 7                                         # ratio +inf
    assert lv(0.0, 0.0) == 0 and lv(np.nan, 4.0) == 0                # ratio NaN
    assert lv(4.0 * 1.2 ** 2.5, 4.0) == 3


def test_near_level_marks_integer_quotients_only():
    r = np.array([1.2 ** 2, 1.2 ** 2.5, F(1.2) * F(1.2), 1.0], F)
    assert R.near_level_mask(r, 1.2).tolist() == [True, False, True, True]


def test_walk_order_and_octave_window():
    rng = np.random.default_rng(5)
    sc = R.make_views(rng, [200, 200], [R.SEARCH, R.SIM3])
    for g, v in zip(sc["ref"], sc["views"]):
        assert np.array_equal(g["kept"], np.flatnonzero(g["status"] == 0)) and 20 < len(g["kept"]) < 200
        lv = g["level"][g["kept"]]
        if v["mode"] == R.SIM3:
            assert np.array_equal(g["q_min_octave"], lv - 1) and np.array_equal(g["q_max_octave"], lv)
        else:
            assert (g["q_min_octave"] == -0x7fffffff).all() and (g["q_max_octave"] == 0x7fffffff).all()


def test_generator_draws_cover_every_status_and_stay_clear_of_level_boundaries():
    seen = np.zeros(5, int)
    for seed, counts, modes, special in R.gpu_test_draws():
        sc = R.make_views(np.random.default_rng(seed), counts, modes, special=special)
        n = sum(counts)
        assert len(sc["near_level"]) == n and sc["near_level"].sum() <= 1e-3 * n, (seed, int(sc["near_level"].sum()), n)
        for g in sc["ref"]:
            seen += np.bincount(g["status"], minlength=5)
        for v, want in (special or {}).items():
            st = sc["ref"][v]["status"]
            assert (st == 0).all() if want == "kept" else (st != 0).all()
    assert (seen > 50).all(), seen


def test_large_draws_stay_clear_of_level_boundaries_and_keep_entries_on_both_sides_of_the_second_scan_trip():
    for draw in R.large_draws():
        seed, counts, modes, special = draw
        sc = R.large_scene(draw)
        n = sum(counts)
        assert len(sc["table"]["pos"]) == 3000 and [len(v["indices"]) for v in sc["views"]] == counts and [v["mode"] for v in sc["views"]] == modes
        print(seed, "near_level", int(sc["near_level"].sum()), "of", n)
        assert len(sc["near_level"]) == n and sc["near_level"].sum() <= 1e-3 * n, (seed, int(sc["near_level"].sum()), n)
        long_views = 0
        for cnt, g in zip(counts, sc["ref"]):
            if cnt <= R.LARGE_TRIP:
                continue
            long_views += 1
            past = int((g["kept"] >= R.LARGE_TRIP).sum())
            print(seed, "a view of", cnt, "keeps", len(g["kept"]), "entries,", past, "of them in the second trip")
            assert len(g["kept"]) - past >= 1000             # the carry into the second trip is not zero ...
            if cnt >= R.LARGE_TRIP + 300:                    # ... and is used: by at least 50 kept entries,
                assert past >= 50
            else:                                            # or, in a second trip of one entry, by that entry
                assert cnt == R.LARGE_TRIP + 1 and past == 1 and g["kept"][-1] == R.LARGE_TRIP
        assert long_views == 1
    assert R.large_draws()[1][1][0] > 0                      # the second draw's long view does not start the block table


def test_sequential_search_binds_each_keypoint_once():
    rng = np.random.default_rng(9)
    sc = R.make_views(rng, [120], [R.SEARCH], n_mp=120)
    g = sc["ref"][0]
    k = g["kept"]
    # two keypoints per kept map point, both with its exact descriptor, the first already bound: the second one is taken
    kf = dict(x=np.repeat(g["x"][k], 2), y=np.repeat(g["y"][k], 2), desc=np.repeat(sc["table"]["desc"][sc["views"][0]["indices"][k]], 2, axis=0),
              octave=np.zeros(2 * len(k), np.int32))
    bound = np.zeros(2 * len(k), np.uint8); bound[0::2] = 1
    m = R.search_by_projection(kf, bound, sc["table"], sc["views"][0], sc["sf"], 1.2)
    assert len(m) > 10 and all(j % 2 == 1 for _, j in m) and len({j for _, j in m}) == len(m) and bound.sum() == len(k) + len(m)


def test_matcher_scene_has_competition_and_no_entry_near_a_level_boundary():
    sc, kfs, bound = R.make_matcher_scene()
    assert not sc["near_level"].any()                       # a condition on the input: redraw the seed if it breaks
    assert 120 < bound.sum() < 180 and all(len(k["x"]) == 500 for k in kfs)
    m = R.search_by_projection(kfs[0], bound.copy(), sc["table"], sc["views"][0], sc["sf"], 1.2)
    assert len(m) > 40 and (R.find_matches_transformed(kfs[1], sc["table"], sc["views"][1], sc["sf"], 1.2) >= 0).sum() > 40
