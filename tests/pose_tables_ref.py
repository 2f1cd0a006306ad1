"""The specification of ms_pose_tables_solve, restated in numpy: poseBundleAdjust (bundle_adjuster.cpp:396-491) on the map
tables -- the gather of the frame's pose-only problem from its kf_mp row, and the apply of the solver's pose.

A scene is a dict of the tables of tests/ba_window_ref.py (kf_mp, mp_flags, mp_pos, poses, kp, cams, focal, sigma, ...) plus mp_live [n_mp]
uint8; a frame is the dict mi355slam.pose_tables_frame takes (slot, prev_slot, n_kp, cam, focal, edge_meas, edge_info, min_visible, max_iters,
huber_delta).  A row r is PRESENT iff 0 <= r < n_mp as an unsigned test and mp_live[r] != 0; bit 0 of mp_flags is TRIANGULATED.

Operation order: the poses by ba_window_ref.pose_of_matrix, obs_uv = ((double)x - cx) / fx, obs_info = (double)focal * (double)focal /
(double)sigma[octave] -- the expressions of ms_ba_window_lists, each float64 operation a single IEEE operation, so the device arrays equal
these bit for bit."""
import numpy as np

import ba_synth
import ba_window_ref as W
from ba_window_ref import matrix_of_pose, pose_of_matrix

N_LEVELS = W.N_LEVELS
FRAME, PREV = 1, 2                                           # the scenes' slots: the frame, its previous keyframe (slot 0 is a bystander)
INT32_MIN = -2 ** 31
# what a keypoint's kf_mp entry is: a TRIANGULATED live row | -1 | n_mp | INT32_MIN | a TRIANGULATED row that is not live | an UNSURE live row
K, NONE, HIGH, LOW, DEAD, UNSURE = "K", "N", "H", "M", "D", "U"
DROPPED = (NONE, HIGH, LOW, DEAD, UNSURE)
# minVisibleMapPointsInCurrentFrameBA and poseBAIterations of the tests.  Three iterations, as the pose-only tests of tests/test_gpu_ba_small_kernels.py
# run: ten reach rounding, where rho = 0 / 0 decides between accept and reject and the LM trajectory is no longer comparable with the oracle's
MIN_VISIBLE, MAX_ITERS = 10, 3


# ---- gather
def present(sc, r):
    r = np.asarray(r, np.int64)
    ok = (r >= 0) & (r < sc["n_mp"])
    live = sc.get("mp_live")
    if live is not None:
        ok[ok] = np.asarray(live)[r[ok]] != 0
    return ok


def gather(sc, frame):
    """The problem the gather kernel writes: pose [2, 7], point [n, 3], obs_point, obs_pose [n] int32, obs_uv [n, 2], obs_info [n], n =
    n_triangulated, kept = the kept keypoints, bad_octaves = the kept keypoints whose octave lies outside [0, N_LEVELS)."""
    s, n_kp = int(frame["slot"]), int(frame["n_kp"])
    r = np.asarray(sc["kf_mp"], np.int64)[s, :n_kp]
    keep = present(sc, r)
    keep[keep] = (np.asarray(sc["mp_flags"])[r[keep]] & 1) != 0
    kept = np.nonzero(keep)[0]                               # ascending keypoint order
    rows = r[kept]
    fx, fy, cx, cy = (float(v) for v in frame["cam"][:4])
    x, y = sc["kp"]["x"][s, kept].astype(np.float64), sc["kp"]["y"][s, kept].astype(np.float64)
    octave = sc["kp"]["octave"][s, kept].astype(np.int64)
    bad = (octave < 0) | (octave >= N_LEVELS)
    focal = float(int(frame["focal"]))
    info = focal * focal / np.asarray(sc["sigma"], np.float32).astype(np.float64)[np.clip(octave, 0, N_LEVELS - 1)]
    n = len(kept)
    return dict(pose=np.array([pose_of_matrix(sc["poses"][s]), pose_of_matrix(sc["poses"][int(frame["prev_slot"])])], np.float64).reshape(2, 7),
                point=np.asarray(sc["mp_pos"], np.float64)[rows].reshape(-1, 3), obs_point=np.arange(n, dtype=np.int32), obs_pose=np.zeros(n, np.int32),
                obs_uv=np.stack([(x - cx) / fx, (y - cy) / fy], 1) if n else np.zeros((0, 2)), obs_info=info, n=n, kept=kept, bad_octaves=int(bad.sum()))


def problem(frame, g):
    """The ms_ba_problem of a gathered frame, as tests/ba_synth.py lays a problem out: pose 0 free, pose 1 fixed, every point fixed, the
    odometry edge from vertex 0 = the frame to vertex 1 = the previous keyframe."""
    return dict(pose=g["pose"].copy(), pose_fixed=np.array([0, 1], np.uint8), point=g["point"].copy(), point_fixed=np.ones(g["n"], np.uint8),
                obs_pose=g["obs_pose"].copy(), obs_point=g["obs_point"].copy(), obs_uv=g["obs_uv"].copy(), obs_info=g["obs_info"].copy(),
                huber_delta=float(frame["huber_delta"]), edge_i=np.array([0], np.int32), edge_j=np.array([1], np.int32),
                edge_meas=np.asarray(frame["edge_meas"], np.float64).reshape(1, 7), edge_info=np.asarray(frame["edge_info"], np.float64).reshape(1, 36))


# ---- apply
def apply(poses, frame, g, solved_pose, finite=True):
    """(poses after the call, ran): the frame's slot becomes the matrix of the solver's pose 0 iff the frame has at least min_visible
    triangulated points and the solve ended in a finite state; nothing else changes."""
    out = np.array(poses, np.float64)
    ran = g["n"] >= int(frame["min_visible"]) and bool(finite) and int(frame["prev_slot"]) != -1
    if ran:
        out[int(frame["slot"])] = matrix_of_pose(solved_pose)
    return out, ran


# ---- scenes
def odometry_edge(sc, rng=None):
    """makeOdometryEdge(frame, previous): the measurement poseDifference(previous, frame) of the true poses with a little noise, and the
    information of the reference's prior (rotation, translation order)."""
    t = sc["true"]
    true = [ba_synth._pose(t["R"][s], -t["R"][s] @ t["c"][s]) for s in (FRAME, PREV)]
    M = ba_synth._compose(true[1], ba_synth._inverse(true[0]))
    if rng is not None:
        M = ba_synth._compose(ba_synth._pose(ba_synth._rotvec(rng.normal(0, 0.001, 3)), rng.normal(0, 0.002, 3)), M)
    info = np.diag([100.0 ** 2] * 3 + [50.0 ** 2] * 3) * (0.26667 / 0.1)
    return M, info.reshape(36)


def make_scene(kinds, stride=640, seed=71, beyond=5):
    """3 slots x stride.  kinds[j] says what keypoint j of the frame (slot FRAME) is bound to; `beyond` more keypoints behind n_kp = len(kinds)
    are bound to TRIANGULATED live rows and must not be read.  The rows are dealt out in a shuffled order, so kept rows do not ascend with
    the keypoint.  Returns (scene, frame)."""
    rng = np.random.default_rng(seed)
    kinds = list(kinds)
    n_kp = len(kinds)
    assert n_kp + beyond <= stride
    n_rows = sum(k in (K, DEAD, UNSURE) for k in kinds) + beyond
    n_mp = n_rows + 7                                        # a few rows nobody observes
    sc = dict(n_kf=3, stride=stride, n_mp=n_mp, kf_id=np.array([4, 9, 7], np.int32))
    deal = list(rng.permutation(n_mp)[:n_rows])
    flags, live = np.full(n_mp, 3, np.uint8), np.ones(n_mp, np.uint8)
    want = np.zeros(n_kp + beyond, np.int64)
    for j, k in enumerate(kinds + [K] * beyond):
        if k in (K, DEAD, UNSURE):
            want[j] = deal.pop()
            if k == DEAD:
                live[want[j]] = 0
            if k == UNSURE:
                flags[want[j]] = 2
        else:
            want[j] = {NONE: -1, HIGH: n_mp, LOW: INT32_MIN}[k]
    valid = (want >= 0) & (want < n_mp)
    rows = [int(r) for r in want[valid]]
    sc["mp_flags"] = flags
    sc = W.finish(sc, rng, [rows[::3], rows, rows[1::2]])    # the bystander and the previous keyframe see some of the same rows
    sc["mp_live"] = live
    # finish() shuffles a slot's keypoints: put the frame's into the order asked for (the valid rows' keypoints keep their pixels)
    col_of = {int(r): j for j, r in enumerate(sc["kf_mp"][FRAME]) if 0 <= r < n_mp}
    used = [col_of[int(r)] for r in want[valid]]
    taken = set(used)
    rest = [j for j in range(stride) if j not in taken]
    order = np.zeros(stride, np.int64)
    order[np.nonzero(valid)[0]] = used
    order[np.nonzero(~valid)[0]] = rest[:int((~valid).sum())]
    order[n_kp + beyond:] = rest[int((~valid).sum()):]
    assert sorted(order.tolist()) == list(range(stride))
    sc["kf_mp"][FRAME] = sc["kf_mp"][FRAME][order]
    for k in sc["kp"]:
        sc["kp"][k][FRAME] = sc["kp"][k][FRAME][order]
    sc["kf_mp"][FRAME, :n_kp + beyond] = want.astype(np.int32)
    sc["kf_mp"][FRAME, n_kp + beyond:] = -1
    # the frame's table pose lies far off the truth (about 9 degrees and 0.4 m a coordinate): three LM iterations do not converge from there, so the oracle's
    # accept / reject decisions stand away from rounding and the trajectories can be compared step for step
    P = sc["poses"][FRAME].reshape(3, 4)
    sc["poses"][FRAME] = np.concatenate([W.rotation(rng, 0.15) @ P[:, :3], (P[:, 3] + rng.normal(0, 0.4, 3))[:, None]], 1).reshape(12)
    meas, info = odometry_edge(sc, rng)
    frame = dict(slot=FRAME, prev_slot=PREV, n_kp=n_kp, cam=sc["cams"][FRAME], focal=int(sc["focal"][FRAME]), edge_meas=meas, edge_info=info, min_visible=MIN_VISIBLE,
                 max_iters=MAX_ITERS, huber_delta=ba_synth.HUBER_DELTA)
    return sc, frame


def mixed(n_kp, n_kept, seed, kept_at=(), none_before=0):
    """n_kp kinds with exactly n_kept kept keypoints: those of kept_at, the rest drawn at or behind `none_before`; the dropped ones cycle
    through every kind of dropped entry."""
    rng = np.random.default_rng(seed)
    kept = set(int(j) for j in kept_at)
    free = [j for j in range(none_before, n_kp) if j not in kept]
    kept |= set(int(j) for j in rng.permutation(free)[:n_kept - len(kept)])
    assert len(kept) == n_kept, (len(kept), n_kept)
    out, d = [], 0
    for j in range(n_kp):
        if j in kept:
            out.append(K)
        else:
            out.append(DROPPED[d % len(DROPPED)])
            d += 1
    return out


TRIP = 256                                                   # keypoints per trip of the gather's workgroup
# name -> (kinds, stride): the smallest shapes at which each mechanism of the gather and of k_ba_pose_only can fail
SCENES = {
    "base": lambda: (mixed(600, 150, 1, kept_at=(0, 255, 256, 257, 511, 512, 599)), 640),            # kept on both sides of both trip boundaries
    "kp0": lambda: ([], 640),
    "kp1": lambda: ([K], 640),
    "kp255": lambda: (mixed(255, 90, 2, kept_at=(254,)), 640),
    "kp256": lambda: (mixed(256, 90, 3, kept_at=(255,)), 640),
    "kp257": lambda: (mixed(257, 90, 4, kept_at=(255, 256)), 640),
    "second_trip_only": lambda: (mixed(512, 40, 5, none_before=256) + [NONE, UNSURE] * 44, 640),      # nothing kept in the first trip or the third
    "tri0": lambda: (mixed(300, 0, 6), 640),
    "tri192": lambda: (mixed(600, 192, 7, kept_at=(255, 256)), 640),
    "tri193": lambda: (mixed(600, 193, 8, kept_at=(255, 256)), 640),                               # the second register slot of k_ba_pose_only
    "overflow": lambda: (mixed(1600, 1537, 9), 2048),                                              # beyond PO_OT * PO_K = 1536 observations
}
_CACHE = {}


def cached(name):
    """(scene, frame, gathered) of a named scene, computed once and shared; callers must not change them."""
    if name not in _CACHE:
        kinds, stride = SCENES[name]()
        sc, frame = make_scene(kinds, stride=stride, seed=100 + sorted(SCENES).index(name))
        _CACHE[name] = (sc, frame, gather(sc, frame))
    return _CACHE[name]


def scene_conditions(name, sc, frame, g):
    """What the named scenes promise."""
    n_kp, kept = frame["n_kp"], g["kept"]
    trip = kept // TRIP
    want_n = dict(kp0=0, kp1=1, tri0=0, tri192=192, tri193=193, overflow=1537, base=150, second_trip_only=40).get(name)
    assert want_n is None or g["n"] == want_n, (name, g["n"])
    assert n_kp == dict(kp0=0, kp1=1, kp255=255, kp256=256, kp257=257, overflow=1600, tri0=300).get(name, 600)
    if name in ("base", "tri192", "tri193"):
        assert {255, 256} <= set(kept.tolist()) and set(trip.tolist()) == {0, 1, 2}
    if name == "base":
        assert {0, 511, 512, 599} <= set(kept.tolist())
        r = sc["kf_mp"][FRAME, :n_kp].astype(np.int64)
        dropped = np.setdiff1d(np.arange(n_kp), kept)
        assert (r[dropped] == -1).any() and (r[dropped] == sc["n_mp"]).any() and (r[dropped] == INT32_MIN).any()
        inside = dropped[(r[dropped] >= 0) & (r[dropped] < sc["n_mp"])]
        assert (sc["mp_live"][r[inside]] == 0).any() and (sc["mp_flags"][r[inside]] == 2).any()
        assert (np.diff(r[kept]) < 0).any() and (np.diff(r[kept]) > 0).any()                       # the rows do not ascend with the keypoint
        assert set(sc["kp"]["octave"][FRAME, kept].tolist()) == set(range(N_LEVELS))
    if name == "second_trip_only":
        assert set(trip.tolist()) == {1}
    if name == "kp257":
        assert kept[-1] == 256
    beyond = sc["kf_mp"][FRAME, n_kp:n_kp + 5].astype(np.int64)
    assert present(sc, beyond).all() and (sc["mp_flags"][beyond] == 3).all()                       # bound behind n_kp: must not be gathered
    assert g["bad_octaves"] == 0
