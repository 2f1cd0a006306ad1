"""tests/map_publish_ref.py, the numpy specification of ms_map_publish, against a literal walk of publishMapForViewer
(mapper_helpers.cpp:823-839) and updatePointCloudRecording (:881-909) over Python dicts and sets: six map states, the point vector and the
accumulated records compared after every state; and the pose rule against float32(numpy.linalg.inv(P)).  No GPU, no library."""
import numpy as np

import map_publish_ref as R

F = np.float32
TRIANGULATED, NOT_TRIANGULATED, UNSURE = 0, 1, 2            # MapPointStatus as int(mp.status) prints it
FLAGS = {TRIANGULATED: 3, UNSURE: 2, NOT_TRIANGULATED: 0}
N_ROWS, STRIDE = 16, 6


class Mp:
    def __init__(self, id_, position, status, observations, seed):
        rng = np.random.default_rng(seed)
        self.id, self.position, self.status = id_, np.array(position, np.float64), status
        self.observations = dict(observations)               # KfId -> KpId
        self.norm = rng.normal(size=3).astype(F)
        self.color = rng.integers(0, 256, 3).astype(np.uint8)


def f32(v):
    """cast<float>(): a value beyond float becomes an infinity, silently"""
    with np.errstate(over="ignore"):
        return v.astype(F)


# ---- the reference, statement by statement
def publish_walk(map_points, current_map_points, local_mp_ids):
    visible_ids = set()
    for mp_id in current_map_points:
        if mp_id != -1:
            visible_ids.add(mp_id)
    mps = []
    for mp_id in sorted(map_points):
        mp = map_points[mp_id]
        if mp.status == NOT_TRIANGULATED:
            continue
        mps.append(dict(position=f32(mp.position), normal=mp.norm, color=np.array([mp.color[0], mp.color[1], mp.color[2]], F) / F(255.0), status=int(mp.status),
                        localMap=local_mp_ids is not None and mp.id in local_mp_ids, nowVisible=mp.id in visible_ids))
    return mps


def record_walk(t, records, map_points):
    for mp_id in sorted(map_points):
        mp = map_points[mp_id]
        if len(mp.observations) < 4:
            continue
        p = f32(mp.position)
        if mp.id not in records:
            records[mp.id] = dict(positions=[(t, p)], normal=mp.norm, removed=False)
        elif (records[mp.id]["positions"][-1][1] != p).any():
            records[mp.id]["positions"].append((t, p))
            records[mp.id]["normal"] = mp.norm
    p0 = np.zeros(3, F)
    for mp_id in sorted(records):
        if not records[mp_id]["removed"] and mp_id not in map_points:
            records[mp_id]["removed"] = True
            records[mp_id]["positions"].append((t, p0))


# ---- the tables of a map state: row = MpId (ids are never reused), slot = the keyframe's rank
def tables_of(map_points, keyframes):
    t = dict(mp_pos=np.full((N_ROWS, 3), 7.5), mp_norm=np.full((N_ROWS, 3), F(-3)), mp_flags=np.zeros(N_ROWS, np.uint8), mp_live=np.zeros(N_ROWS, np.uint8),
             n_obs=np.zeros(N_ROWS, np.int32), mp_color=np.zeros((N_ROWS, 3), np.uint8), kf_mp=np.full((len(keyframes), STRIDE), -1, np.int32),
             kf_pose=np.zeros((len(keyframes), 12)))
    for mp in map_points.values():
        t["mp_pos"][mp.id], t["mp_norm"][mp.id], t["mp_color"][mp.id] = mp.position, mp.norm, mp.color
        t["mp_flags"][mp.id], t["mp_live"][mp.id], t["n_obs"][mp.id] = FLAGS[mp.status], 1, len(mp.observations)
    for slot, kf_id in enumerate(sorted(keyframes)):
        t["kf_mp"][slot, :len(keyframes[kf_id])] = keyframes[kf_id]
    t["mp_flags"][15] = 3                                    # a stale flag on a free row
    return t


def apply_events(t, records, out):
    """what the mirror's updatePointCloudRecording does with the event stream"""
    for r, kind, p, n in zip(out["ev_row"], out["ev_kind"], out["ev_pos"], out["ev_norm"]):
        if kind == R.NEW:
            assert int(r) not in records
            records[int(r)] = dict(positions=[(t, p)], normal=n, removed=False)
        elif kind == R.MOVED:
            records[int(r)]["positions"].append((t, p))
            records[int(r)]["normal"] = n
        else:
            assert kind == R.REMOVED and (p == 0).all()
            records[int(r)]["removed"] = True
            records[int(r)]["positions"].append((t, p))


def same_records(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k]["removed"] == b[k]["removed"] and a[k]["normal"].tobytes() == b[k]["normal"].tobytes(), k
        assert [x[0] for x in a[k]["positions"]] == [x[0] for x in b[k]["positions"]], k
        assert all(x[1].astype(F).tobytes() == y[1].astype(F).tobytes() for x, y in zip(a[k]["positions"], b[k]["positions"])), k


def states():
    """six map states, each (map points, keyframes, localMpIds): created; reaching 4 observations; moved; below 4 again; removed; a NaN"""
    obs = lambda n: {kf: 0 for kf in range(10, 10 + n)}
    mps = {i: Mp(i, [i + 0.1, -i * 0.3, 1e-3 * i + 1 / 3], (TRIANGULATED, UNSURE, NOT_TRIANGULATED)[i % 3], obs(2 + i % 2), i) for i in range(10)}
    kfs = {10: [0, 1, -1, 2], 11: [3, -1, 4], 12: [5, 6, -1, 9, 2]}
    yield mps, kfs, {1, 5, 8}
    for i in (0, 1, 2, 4, 6, 7):                             # six points reach 4 or 5 observations; 2 is NOT_TRIANGULATED and is recorded all the same
        mps[i].observations = obs(4 + i % 2)
    mps[3].status = TRIANGULATED
    kfs[13] = [7, 7, -1, 0]
    yield mps, kfs, {0, 7}
    for i in (0, 2, 3, 6):                                   # moved: 3 has too few observations and gives nothing
        mps[i].position = mps[i].position + [0.25, 0.0, -1e-9]
    mps[7].position = mps[7].position * (1 + 2.0 ** -40)     # a move below float resolution: no change of the record
    mps[10] = Mp(10, [1, 2, 3], UNSURE, obs(6), 10)
    yield mps, kfs, None
    for i in (0, 4):                                         # below 4 again, and moved: nothing
        mps[i].observations = obs(3)
        mps[i].position = mps[i].position + 5.0
    yield mps, kfs, {10}
    for i in (0, 1, 3, 6):                                   # removed: 0 and 1 and 6 are recorded (0 with few observations now), 3 never was
        del mps[i]
    kfs[14] = [10, 2]
    yield mps, kfs, {2, 10, 11}
    mps[2].position = np.array([np.nan, 1.0, 2.0])
    mps[7].position = np.array([1e39, -1e39, 1e-46])         # beyond float: +-inf and 0
    yield mps, kfs, {2}
    yield mps, kfs, {2}                                      # the same state again: the NaN moves again, nothing else does


def test_the_restatement_follows_the_literal_walk_through_six_map_states():
    records_walk, records_ref = {}, {}
    rec_pos, rec_state = R.empty_record(N_ROWS)
    events = []
    for step, (mps, kfs, local) in enumerate(states()):
        t = tables_of(mps, kfs)
        current = len(kfs) - 1                               # mapDB.keyframes.rbegin()
        rc, out, rec_pos, rec_state = R.map_publish(t, rec_pos, rec_state, R.VIEW | R.RECORD, current, 4, sorted(local or ()) + [-1, N_ROWS, 1 << 30], kf_list=range(len(kfs)))
        assert rc == 0
        want = publish_walk(mps, kfs[max(kfs)], local)
        assert out["counts"][0] == len(want) == len(out["pub_row"])
        for k, w in enumerate(want):
            assert out["pub_pos"][k].tobytes() == w["position"].tobytes() and out["pub_norm"][k].tobytes() == w["normal"].tobytes()
            assert out["pub_color"][k].tobytes() == w["color"].tobytes() and out["pub_status"][k] == w["status"]
            assert out["pub_bits"][k] == int(w["localMap"]) + 2 * int(w["nowVisible"]), (step, k)
        assert out["counts"][5] == sum(w["localMap"] for w in want) and out["counts"][6] == sum(w["nowVisible"] for w in want)
        assert out["counts"][7] == sum(mp.status == NOT_TRIANGULATED for mp in mps.values())
        record_walk(float(step), records_walk, mps)
        apply_events(float(step), records_ref, out)
        same_records(records_walk, records_ref)
        assert (np.diff(out["ev_row"]) > 0).all() and out["counts"][1] == len(out["ev_row"]) == out["counts"][2:5].sum()
        events.append(out["ev_kind"].tolist())
        # the record state is the walk's records: state 1 = recorded and not removed, 2 = removed
        assert {int(r) for r in np.flatnonzero(rec_state == 1)} == {k for k, v in records_walk.items() if not v["removed"]}
        assert {int(r) for r in np.flatnonzero(rec_state == 2)} == {k for k, v in records_walk.items() if v["removed"]}
    assert events[0] == [] and events[1] == [R.NEW] * 6 and events[2] == [R.MOVED] * 3 + [R.NEW] and events[3] == []
    assert events[4] == [R.REMOVED] * 3 and events[5] == [R.MOVED, R.MOVED] and events[6] == [R.MOVED]
    assert records_walk[7]["positions"][-1][1].tolist() == [np.inf, -np.inf, 0.0]


def test_a_present_row_with_state_removed_is_new_and_a_refusal_changes_nothing():
    mps = {i: Mp(i, [i, i, i], TRIANGULATED, {k: 0 for k in range(4)}, i) for i in range(4)}
    t = tables_of(mps, {1: [0]})
    pos, state = R.empty_record(N_ROWS)
    state[2] = 2
    rc, out, pos2, state2 = R.map_publish(t, pos, state, R.RECORD)
    assert rc == 0 and out["ev_kind"].tolist() == [R.NEW] * 4 and state2[:4].tolist() == [1, 1, 1, 1] and out["counts"][0] == 0 and len(out["pub_row"]) == 0
    rc, out, pos3, state3 = R.map_publish(t, pos, state, R.VIEW | R.RECORD, cap_ev=3)
    assert rc == R.CAPACITY and out["counts"][:2].tolist() == [4, 4] and "ev_row" not in out and pos3 is pos and state3 is state
    rc, out, _, _ = R.map_publish(t, pos2, state2, R.VIEW | R.RECORD, cap_pub=4, cap_ev=0)
    assert rc == 0 and out["counts"][:2].tolist() == [4, 0]
    # -0.0 against a recorded 0.0 is no move
    t["mp_pos"][0] = [-0.0, 0.0, -0.0]
    assert pos2[0].tolist() == [0, 0, 0] and R.map_publish(t, pos2, state2, R.RECORD)[1]["counts"][1] == 0


def test_the_pose_rule_is_within_one_float_step_of_the_general_inverse():
    """Both sides carry double rounding error near 1e-16 relative before a single cast to float, so they can land on neighbouring floats and
    no further apart."""
    rng = np.random.default_rng(2023)
    worst = 0.0
    for _ in range(50):
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        tv = rng.uniform(-1e3, 1e3, 3)
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = Rm, tv
        got, want = R.pose_wc(P[:3].reshape(12)), np.linalg.inv(P).astype(F)
        assert got[3].tolist() == [0, 0, 0, 1]
        step = np.spacing(np.abs(want[:3]))
        assert (np.abs(got[:3].astype(np.float64) - want[:3].astype(np.float64)) <= step).all()
        worst = max(worst, float((np.abs(got[:3].astype(np.float64) - want[:3]) / step).max()))
    assert worst <= 1.0
