"""tests/map_extract_ref.py, the specification of ms_map_extract, against a literal walk of MapDB(mapDB, activeKeyframes)
(mapdb.cpp:116-159) and MapPoint(mp, activeKeyframes) (map_point.cpp:22-43) over dictionaries and sets, on every scene the GPU test uses; and the
properties the restatement must have by itself."""
import numpy as np
import pytest

import mi355slam
import map_extract_ref as R


def test_the_feature_is_there():
    assert hasattr(mi355slam.lib(), "ms_map_extract") and hasattr(mi355slam.KeyframeTable, "map_extract")


def walk(t, active):
    """The reference's containers built from the tables, then the constructor, literally.  A map point is its row (MpId = row, which is the
    order the tables keep); a keyframe is its slot, walked in the order given; the observations are the transpose of kf_mp over the occupied
    slots.  Returns (surviving MpIds, observations per MpId as {slot: [keypoints]}, the filtered track map, the cut links per active slot)."""
    n_kf, stride = t["kf_mp"].shape
    n_mp = len(t["mp_flags"])
    live = lambda r: 0 <= r < n_mp and (t["mp_live"] is None or t["mp_live"][r] != 0)
    map_points = {}                                          # mapDB.mapPoints: MpId -> observations
    for r in range(n_mp):
        if live(r):
            map_points[r] = {}
    for s in range(n_kf):
        if t["kf_id"][s] < 0:
            continue
        for j in range(stride):
            r = int(t["kf_mp"][s, j])
            if r in map_points:
                map_points[r].setdefault(s, []).append(j)
    track_to_mp = {}
    if t["track_row"] is not None:
        for i, r in enumerate(t["track_row"]):
            r = int(r)
            if r in map_points and t["mp_track"][r] == t["track_base"] + i:      # the presence rule of 9.11
                track_to_mp[t["track_base"] + i] = r
    active_kf = set(int(s) for s in active)
    active_mp, links = set(), {}
    for s in active:                                         # :119-135
        nxt, prv = int(t["next"][s]), int(t["previous"][s])
        links[int(s)] = (prv if prv in active_kf else -1, nxt if nxt in active_kf else -1)
        for r in t["kf_mp"][s]:
            if int(r) in map_points:                         # mpId.v >= 0; an entry with no map point behind it is dropped (the .at would throw)
                active_mp.add(int(r))
    new_points = {}
    for r in sorted(active_mp):                              # :137-139, map_point.cpp:32-36
        new_points[r] = {s: kps for s, kps in map_points[r].items() if s in active_kf}
    new_tracks = {tid: r for tid, r in track_to_mp.items() if r in active_mp}      # :141-145
    return sorted(active_mp), new_points, new_tracks, links


@pytest.mark.parametrize("name", list(R.SCENES))
def test_the_restatement_equals_the_literal_walk(name):
    sc, z, want = R.cached(name)
    R.scene_conditions(name, sc, z, want)
    t, active = sc["t"], sc["active"]
    got = R.extract(t, active, z, R.fresh_dst(t, z))         # with every optional output, whatever the scene asks for
    mp_ids, points, tracks, links = walk(t, active)
    n = int(got["counts"][0])
    assert got["rc"] == R.OK and got["row_src"][:n].tolist() == mp_ids
    # each point's surviving observations: the transpose of the destination table, translated back
    obs = {}
    for i, s in enumerate(active):
        for j, d in enumerate(got["kf_mp"][i]):
            if d >= 0:
                obs.setdefault(int(got["row_src"][d]), {}).setdefault(int(s), []).append(j)
    assert obs == points
    assert got["n_obs"][:n].tolist() == [sum(len(k) for k in points[r].values()) for r in mp_ids]
    if t["track_row"] is not None:
        kept = {z["track_base"] + i: int(got["row_src"][d]) for i, d in enumerate(got["track_row"]) if d >= 0}
        assert kept == tracks and got["counts"][3] == len(tracks)
    where = {int(s): i for i, s in enumerate(active)}
    assert R.cut_links(t, active) == [tuple(where.get(x, -1) for x in links[int(s)]) for s in active]


def test_links_of_the_first_scene_by_hand():
    sc, z, want = R.cached("every_kind")
    # KfIds 31 (slot 1), 37 (4), 40 (0), 52 (2), 60 (5): the chain in slots is 1 - 4 - 0 - 2 - 5; active 4, 0, 2 -> destination slots 0, 1, 2
    assert R.cut_links(sc["t"], sc["active"]) == [(-1, 1), (0, 2), (1, -1)]
    assert R.cut_links(sc["t"], [2, 4]) == [(-1, -1), (-1, -1)]                                            # 0 lies between them and is not active


@pytest.mark.parametrize("name", list(R.SCENES))
def test_properties(name):
    sc, z, _ = R.cached(name)
    t = sc["t"]
    got = R.extract(t, sc["active"], z, R.fresh_dst(t, z))
    n, rs, rd = int(got["counts"][0]), got["row_src"], got["row_dst"]
    assert (np.diff(rs[:n]) > 0).all() and (rd[rs[:n]] == np.arange(n)).all() and (rd >= 0).sum() == n
    e = got["kf_mp"].reshape(-1)
    assert np.array_equal(np.bincount(e[e >= 0], minlength=z["n_mp_dst"]), got["n_obs"]) and got["counts"][1] == (e >= 0).sum()
    assert (got["mp_live"][:n] == 1).all() and not got["mp_live"][n:].any() and not got["mp_flags"][n:].any()


@pytest.mark.parametrize("name", list(R.SCENES))
def test_the_full_copy_keeps_every_live_row_that_a_keyframe_lists_and_a_second_extraction_is_the_identity(name):
    sc, _, _ = R.cached(name)
    t = sc["t"]
    active = R.occupied(t)
    n_kf, stride = t["kf_mp"].shape
    e = np.asarray(t["kf_mp"], np.int64)[active].reshape(-1)
    listed = np.unique(e[R.present(t, e)])
    pool = 0 if t["desc_pool"] is None else len(t["desc_pool"])
    z = R.sizes(t, len(active), len(listed), pool)
    got = R.extract(t, active, z)
    assert got["rc"] == R.OK and np.array_equal(got["row_src"], listed) and len(listed) > 5
    # the extraction as a source of its own, all slots active: the identity on the row fields and on the table
    t2 = {k: got.get(k) for k in R.DST}
    t2.update(kf_id=t["kf_id"][active], track_base=z["track_base"], desc_base=got["dst_desc_base"], n_kp=t["n_kp"][active])
    for k in ("mp_track", "track_row", "kf_pose", "desc_pool") + R.KP_FIELDS:
        t2.setdefault(k, None)
    z2 = R.sizes(t2, len(active), len(listed), pool)
    again = R.extract(t2, list(range(len(active))), z2)
    for k in R.ROW_FIELDS + R.KP_FIELDS + ("kf_mp", "mp_live", "n_obs", "track_row", "kf_pose"):
        if got.get(k) is not None:
            assert again[k].tobytes() == got[k].tobytes(), k
    assert np.array_equal(again["row_src"], np.arange(len(listed))) and again["counts"][2] == 0


def test_capacity_and_no_active_slots():
    sc, z, want = R.cached("every_kind")
    t, n = sc["t"], int(want["counts"][0])
    zs = dict(z, n_mp_dst=n - 1)
    before = R.fresh_dst(t, zs, 0x5A)
    short = R.extract(t, sc["active"], zs, before)
    assert short["rc"] == R.CAPACITY and short["counts"].tolist() == want["counts"].tolist()
    assert all(short[k].tobytes() == before[k].tobytes() for k in before)                                 # nothing of the destination is written
    exact = R.extract(t, sc["active"], dict(z, n_mp_dst=n), R.fresh_dst(t, dict(z, n_mp_dst=n), 0x5A))
    assert exact["rc"] == R.OK and exact["mp_live"].all()
    empty = R.extract(t, [], z, R.fresh_dst(t, z, 0x5A))
    assert empty["rc"] == R.OK and empty["counts"].tolist() == [0] * 5 and (empty["kf_mp"] == -1).all() and not empty["mp_live"].any()
    assert (empty["track_row"] == -1).all() and (empty["row_dst"] == -1).all() and (empty["mp_track"] == -1).all() and not empty["kp_x"].any()
    assert empty["mp_pos"].tobytes() == R.fresh_dst(t, z, 0x5A)["mp_pos"].tobytes()                       # the other fields are left alone
