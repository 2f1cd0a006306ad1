"""ms_map_refresh and ms_loop_correct on the device against tests/map_refresh_ref.py, their specification.

The refresh is +, x, / and square roots in one stated order, so normal, min / max distance, descriptor row and medoid are bit-equal to the
restatement, whatever the order of the rows and however many share a call.  In the loop correction the rigid members and the point stage are
bit-equal too (the point stage fed the device's own poses); the interpolated poses pass through acos and sin, which differ between math
libraries, and are held to the tolerance tests/test_map_refresh_ref.py measures: 4 x the largest change of any output when every acos / sin
result moves by up to 2 ulp -- poses 5e-15 (measured 4.44e-15), points 7e-14 (measured 6.57e-14)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import map_refresh_ref as R
import mi355slam
import project_gate_ref as G

pytestmark = pytest.mark.gpu
F = np.float32
FIELDS = (("norm", F, 3), ("min_dist", F, 1), ("max_dist", F, 1), ("desc", np.uint32, 8))

SCENE = R.make_refresh_scene()
WANT, WANT_MEDOID = R.refresh(SCENE["table"], SCENE["kf_pose"], SCENE["pool"], SCENE["prob"], SCENE["sf"])
LOOP = R.make_loop_scene()
TRANSFORMS = R.loop_transforms()


def upload(ctx, t):
    return mi355slam.MapPointTable(ctx, t["pos"], t["norm"], t["min_dist"], t["max_dist"], t["desc"])


def download(table):
    out = {name: getattr(table, name).download(dt, (table.n, w) if w > 1 else (table.n,)) for name, dt, w in FIELDS}
    out["pos"] = table.pos.download(np.float64, (table.n, 3))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same_table(got, want):
    for k in ("pos", "norm", "min_dist", "max_dist", "desc"):
        g, w = bits(got[k]).reshape(len(want[k]), -1), bits(want[k]).reshape(len(want[k]), -1)
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert len(bad) == 0, "%s differs in rows %s" % (k, bad[:8])


@pytest.fixture(scope="module")
def device_scene(ctx):
    return mi355slam.KeyframePoseTable(ctx, SCENE["kf_pose"]), ctx.upload(SCENE["pool"])


def test_refresh_equals_the_restatement(ctx, device_scene):
    """40 keyframes, 300 of 400 rows, lists of 1, 2, 3, 63, 64, 65, 256 and 257 observations (257 -> -2), a repeated keyframe, a zero term, octave
    0 and the last level, a row without descriptors; the 100 rows that are not listed keep their bytes."""
    poses, pool = device_scene
    table = upload(ctx, SCENE["table"])
    medoid = mi355slam.map_refresh(ctx, table, poses, SCENE["prob"], SCENE["sf"], pool)
    assert np.array_equal(medoid, WANT_MEDOID)
    assert medoid[7] == -2 and medoid[12] == -1
    assert_same_table(download(table), WANT)


def test_refresh_without_a_pool_leaves_the_descriptors(ctx, device_scene):
    poses, _ = device_scene
    table = upload(ctx, SCENE["table"])
    medoid = mi355slam.map_refresh(ctx, table, poses, SCENE["prob"], SCENE["sf"], None)
    want = dict(WANT); want["desc"] = SCENE["table"]["desc"]
    assert (medoid == -1).all()
    assert_same_table(download(table), want)


def test_same_bits_in_another_order_and_alone(ctx, device_scene):
    poses, pool = device_scene
    n = len(SCENE["prob"]["rows"])
    order = np.random.default_rng(1).permutation(n)
    table = upload(ctx, SCENE["table"])
    medoid = mi355slam.map_refresh(ctx, table, poses, R.sub_problem(SCENE["prob"], order), SCENE["sf"], pool)
    assert np.array_equal(medoid, WANT_MEDOID[order])
    assert_same_table(download(table), WANT)
    table = upload(ctx, SCENE["table"])
    alone = list(range(14)) + [n - 1]                          # the constructed lengths and special rows, each in a call of its own
    for e in alone:
        medoid = mi355slam.map_refresh(ctx, table, poses, R.sub_problem(SCENE["prob"], np.array([e])), SCENE["sf"], pool)
        assert medoid[0] == WANT_MEDOID[e], e
    got, rows = download(table), SCENE["prob"]["rows"][alone]
    for k in ("norm", "min_dist", "max_dist", "desc"):
        assert np.array_equal(bits(got[k][rows]), bits(WANT[k][rows])), k
    others = np.setdiff1d(np.arange(table.n), rows)
    for k in ("norm", "min_dist", "max_dist", "desc"):
        assert np.array_equal(bits(got[k][others]), bits(SCENE["table"][k][others])), k


def test_zero_rows_are_accepted(ctx, device_scene):
    poses, pool = device_scene
    table = upload(ctx, SCENE["table"])
    empty = dict(rows=np.zeros(0, np.int32), obs_start=np.zeros(1, np.int32), obs_kf=np.zeros(0, np.int32), obs_desc=np.zeros(0, np.int32),
                 first_octave=np.zeros(0, np.int32))
    assert len(mi355slam.map_refresh(ctx, table, poses, empty, SCENE["sf"], pool)) == 0
    assert_same_table(download(table), SCENE["table"])


def test_invalid_lists_are_rejected_and_write_nothing(ctx, device_scene):
    poses, pool = device_scene
    table = upload(ctx, SCENE["table"])
    prob = R.sub_problem(SCENE["prob"], np.arange(20))
    for change in (dict(rows=np.r_[prob["rows"][:19], prob["rows"][0]]), dict(obs_kf=np.r_[prob["obs_kf"][:-1], 40]), dict(first_octave=np.r_[prob["first_octave"][:19], 8])):
        with pytest.raises(mi355slam.MsError):
            mi355slam.map_refresh(ctx, table, poses, {**prob, **change}, SCENE["sf"], pool)
    assert_same_table(download(table), SCENE["table"])


def test_allocations_stay_flat_over_50_calls(ctx, device_scene):
    poses, pool = device_scene
    table = upload(ctx, SCENE["table"])
    allocs = mi355slam.lib().ms_debug_host_allocs
    allocs.restype = C.c_longlong
    pose_table = mi355slam.KeyframePoseTable(ctx, LOOP["kf_pose"])
    points = upload(ctx, dict(SCENE["table"], pos=SCENE["table"]["pos"]))
    mi355slam.map_refresh(ctx, table, poses, SCENE["prob"], SCENE["sf"], pool)                        # warm-up: the largest call
    mi355slam.loop_correct(ctx, points, pose_table, TRANSFORMS["usual"], small_loop_problem())
    before = allocs()
    rng = np.random.default_rng(2)
    for i in range(50):
        prob = R.sub_problem(SCENE["prob"], rng.permutation(300)[:1 + 6 * i])
        mi355slam.map_refresh(ctx, table, poses, prob, SCENE["sf"], pool if i % 2 else None)
        if i % 10 == 0:
            mi355slam.loop_correct(ctx, points, pose_table, TRANSFORMS["usual"], small_loop_problem())
    assert allocs() == before


def small_loop_problem():
    p = LOOP["prob"]
    keep = p["mp_row"] < 400
    return dict(p, mp_row=p["mp_row"][keep], mp_ref=p["mp_ref"][keep])


def run_loop(ctx, T):
    poses = mi355slam.KeyframePoseTable(ctx, LOOP["kf_pose"])
    n = len(LOOP["pos"])
    table = mi355slam.MapPointTable(ctx, LOOP["pos"], np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F), np.zeros((n, 8), np.uint32))
    mi355slam.loop_correct(ctx, table, poses, T, LOOP["prob"])
    return poses.download(), table.pos.download(np.float64, (n, 3))


@pytest.mark.parametrize("name", list(TRANSFORMS))
def test_loop_correction_rigid_members_and_point_stage_are_exact(ctx, name):
    T, prob = TRANSFORMS[name], LOOP["prob"]
    pose, pos = run_loop(ctx, T)
    want_pose, prev = R.correct_poses(LOOP["kf_pose"], T, prob)
    rigid = prob["kf_slot"][prob["kf_rigid"] != 0]
    assert len(rigid) == 6 and np.array_equal(bits(pose[rigid]), bits(want_pose[rigid]))
    listed = np.zeros(len(pose), bool); listed[prob["kf_slot"]] = True
    assert np.array_equal(bits(pose[~listed]), bits(LOOP["kf_pose"][~listed]))
    assert np.array_equal(prev, LOOP["kf_pose"][prob["kf_slot"]])
    want_pos = R.move_points(LOOP["pos"], pose, prev, prob)   # the point stage on the device's own poses
    assert np.array_equal(bits(pos), bits(want_pos))


@pytest.mark.parametrize("name", list(TRANSFORMS))
def test_loop_correction_interpolated_poses_and_end_to_end(ctx, name):
    """lambda in {0, 1e-9, 0.5, 1} and random ones; T usual, within 1e-9 of identity (slerp's linear branch), a 179 degree rotation, w < 0."""
    T = TRANSFORMS[name]
    pose, pos = run_loop(ctx, T)
    want_pose, want_pos = R.loop_correct(LOOP["kf_pose"], LOOP["pos"], T, LOOP["prob"])
    d_pose, d_pos = np.abs(pose - want_pose).max(), np.abs(pos - want_pos).max()
    print("%s: poses %.3g (tolerance %.3g), points %.3g (tolerance %.3g)" % (name, d_pose, R.TOL_POSE, d_pos, R.TOL_POINT))
    assert d_pose <= R.TOL_POSE and d_pos <= R.TOL_POINT


def test_invalid_corrections_are_rejected_and_write_nothing(ctx):
    poses = mi355slam.KeyframePoseTable(ctx, LOOP["kf_pose"])
    n = len(LOOP["pos"])
    table = mi355slam.MapPointTable(ctx, LOOP["pos"], np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F), np.zeros((n, 8), np.uint32))
    p = LOOP["prob"]
    lam = p["kf_lambda"].copy(); lam[7] = np.nan
    for T, change in ((TRANSFORMS["usual"], dict(kf_slot=np.r_[p["kf_slot"][:-1], p["kf_slot"][0]])), (TRANSFORMS["usual"], dict(mp_row=np.r_[p["mp_row"][:-1], n])),
                      (TRANSFORMS["usual"], dict(kf_lambda=lam)), (TRANSFORMS["usual"][:7] + (np.inf,), {})):
        with pytest.raises(mi355slam.MsError):
            mi355slam.loop_correct(ctx, table, poses, T, {**p, **change})
    assert np.array_equal(poses.download(), LOOP["kf_pose"]) and np.array_equal(table.pos.download(np.float64, (n, 3)), LOOP["pos"])


def test_correct_loop_through_the_mirror_equals_the_two_calls():
    import test_map_refresh_abi
    out = subprocess.run([test_map_refresh_abi.build_smoke(), "--gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "gpu ok chained" in out.stdout


def test_gates_after_refresh_equal_the_gates_on_a_host_built_table(ctx, device_scene):
    """searchByProjection's gates over the refreshed rows, from the keyframe that keeps most of them: the table refreshed on the device against a
    table whose rows the host computed and uploaded (the path before this call existed)."""
    poses, pool = device_scene
    sf, rows = SCENE["sf"], SCENE["prob"]["rows"]
    views = []
    for P in SCENE["kf_pose"]:
        P = P.reshape(3, 4)
        views.append(dict(R=P[:, :3].copy(), t=P[:, 3].copy(), cam=G.CAM, threshold=10.0, view_cos_limit=0.5, mode=G.SEARCH, indices=rows))
    view = max(views, key=lambda v: len(G.gate_view(WANT, v, sf, 1.2)["kept"]))
    assert len(G.gate_view(WANT, view, sf, 1.2)["kept"]) >= 3
    dev = upload(ctx, SCENE["table"])
    mi355slam.map_refresh(ctx, dev, poses, SCENE["prob"], sf, pool)
    host = upload(ctx, SCENE["table"])
    for row in rows:
        host.update(int(row), 1, norm=WANT["norm"][row], min_dist=WANT["min_dist"][row], max_dist=WANT["max_dist"][row], desc=WANT["desc"][row])
    e_dev, v_dev = mi355slam.project_gate(ctx, dev, [view], sf, 1.2)
    e_host, v_host = mi355slam.project_gate(ctx, host, [view], sf, 1.2)
    assert int((e_dev["status"] == 0).sum()) >= 3
    for k in e_dev:
        assert np.array_equal(bits(e_dev[k]), bits(e_host[k])), k
    for k in v_dev[0]:
        assert np.array_equal(bits(v_dev[0][k]), bits(v_host[0][k])), k
