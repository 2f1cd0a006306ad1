"""The specification of ms_frame_finish in numpy: setPointCloudOutput (mapper_helpers.cpp:484-497) and the table part of
removeKeyframe (:375-431) on the map tables, and the scenes the GPU tests run.  Everything is integers and copied doubles: a comparison
with this file is bit for bit.

Tables, a dict: kf_mp [n_kf, stride] int32, kf_id [n_kf] int32 (-1: an empty slot), mp_flags [n_mp] uint8 (bit 0 TRIANGULATED), mp_live
[n_mp] uint8 or None (every row live), mp_pos [n_mp, 3] float64, mp_track [n_mp] int32 or None, n_obs [n_mp] int32 or None."""
import numpy as np

OK, CAPACITY = 0, -4
TABLES = ("kf_mp", "mp_flags", "mp_live", "n_obs")          # what a call may write


def valid(t, r):
    """(uint32)r < n_mp, the rule of DESIGN 9.6"""
    return (r >= 0) & (r < len(t["mp_flags"]))


def cloud(t, slot, n_kp):
    """:484-497 for the keyframe in `slot`: the keypoints in order whose map point is PRESENT and TRIANGULATED."""
    e = np.asarray(t["kf_mp"][slot, :n_kp], np.int64) if slot >= 0 else np.zeros(0, np.int64)
    ok = valid(t, e)
    r = np.where(ok, e, 0)
    n_mp = len(t["mp_flags"])
    flags = t["mp_flags"] if n_mp else np.zeros(1, np.uint8)
    live = np.ones(max(n_mp, 1), np.uint8) if t["mp_live"] is None or not n_mp else t["mp_live"]
    kept = ok & (live[r] != 0) & ((flags[r] & 1) != 0)
    rows = e[kept].astype(np.int32)
    track = t["mp_track"][rows] if t["mp_track"] is not None else np.full(len(rows), -1, np.int32)
    return dict(cloud_row=rows, cloud_kp=np.nonzero(kept)[0].astype(np.int32), cloud_track=track.astype(np.int32),
                cloud_pos=np.asarray(t["mp_pos"], np.float64).reshape(-1, 3)[rows].copy())


def remain_counts(t, remove):
    """Per row the valid entries of the remaining slots (kf_id >= 0, not in the list), with multiplicity."""
    keep = np.asarray(t["kf_id"]) >= 0
    keep[np.asarray(remove, np.int64)] = False
    e = np.asarray(t["kf_mp"], np.int64)[keep].reshape(-1)
    return np.bincount(e[valid(t, e)], minlength=len(t["mp_flags"])).astype(np.int32)


def finish(t, remove, cloud_slot, n_kp, cap_removed=None):
    """ms_frame_finish.  Returns dict(rc, the cloud, removed_rows, counts [3], and the four tables a call may write as they are afterwards)."""
    remove = [int(s) for s in remove]
    out = cloud(t, cloud_slot, n_kp)
    after = {k: (None if t[k] is None else np.array(t[k], copy=True)) for k in TABLES}
    e = np.asarray(t["kf_mp"], np.int64)[remove].reshape(-1) if remove else np.zeros(0, np.int64)      # list order, then keypoint index
    ok = valid(t, e)
    listed, at = np.unique(e[ok], return_index=True)
    listed = listed[np.argsort(at, kind="stable")]           # each listed row once, in first-claim order
    remain = remain_counts(t, remove) if remove else None
    removed = np.array([r for r in listed if t["mp_live"][r] and remain[r] == 0], np.int32)
    out.update(removed_rows=removed, counts=np.array([len(out["cloud_row"]), len(removed), int(ok.sum())], np.int32))
    if cap_removed is not None and len(removed) > cap_removed:
        out.update(rc=CAPACITY, removed_rows=np.zeros(0, np.int32), **after)       # every verdict before any write
        return out
    if remove:
        after["kf_mp"][remove] = -1
        after["mp_live"][removed] = 0
        after["mp_flags"][removed] = 0
        if after["n_obs"] is not None:
            after["n_obs"][listed] = remain[listed]
    out.update(rc=OK, **after)
    return out


# ---------------------------------------------------------------------------------------------------------------------------- scenes
def _tables(kf_mp, kf_id, n_mp, seed, live=True, track=True, tri=0.6):
    rng = np.random.default_rng(seed)
    return dict(kf_mp=np.array(kf_mp, np.int32), kf_id=np.asarray(kf_id, np.int32), mp_flags=(rng.random(n_mp) < tri).astype(np.uint8) * 3,
                mp_live=np.ones(n_mp, np.uint8) if live else None, mp_pos=rng.standard_normal((n_mp, 3)),
                mp_track=(1000 + rng.permutation(n_mp)).astype(np.int32) if track else None, n_obs=np.full(n_mp, 77, np.int32))      # n_obs comes in stale


def per_frame():
    """Scene 1: 4 slots x 70 on 90 rows; slot 1 is empty with stale entries, slot 3 is the frame (60 keypoints) and is removed."""
    rng = np.random.default_rng(11)
    kf = np.full((4, 70), -1, np.int32)
    shared = np.arange(30, 60)                               # rows the keyframes in slots 0 and 2 see
    kf[0, :25] = np.r_[5, 5, rng.choice(shared, 23, replace=False)]
    kf[2, :20] = np.r_[5, 25, 27, rng.choice(shared, 17, replace=False)]
    kf[1, :6] = [22, 41, 88, -3, 22, 5]                      # stale: the slot's kf_id is -1
    kf[3, :10] = [-1, 95, -7, 5, 20, 21, 22, 23, 24, 25]
    kf[3, 10:50] = np.where(rng.random(40) < 0.7, rng.choice(np.r_[shared, np.arange(60, 88)], 40, replace=False), -1)
    kf[3, 30] = 24                                           # listed twice
    kf[3, 62], kf[3, 65] = 26, 27                            # behind n_kp: not in the cloud, still erased
    t = _tables(kf, [10, -1, 12, 13], 90, 1)
    t["mp_flags"][[20, 23, 24, 25, 26, 5]] = 3
    t["mp_flags"][[21, 22]] = 2
    t["mp_live"][[23, 70, 45]] = 0                           # 23 seen only here; 70 maybe here; 45 by the others too
    return dict(t=t, remove=[3], cloud_slot=3, n_kp=60)


def two_removed():
    """Scene 2: 5 slots x 40 on 60 rows; slots 3 and 1 are removed, in that order; the cloud is slot 0's, which remains."""
    rng = np.random.default_rng(12)
    kf = np.where(rng.random((5, 40)) < 0.75, rng.integers(0, 50, (5, 40)), -1).astype(np.int32)
    kf[3, 4], kf[1, 2] = 57, 57                              # seen by the two removed slots alone: removed once, claimed by slot 3
    kf[1, 9], kf[2, 9] = 58, 58                              # removed and remaining: stays
    kf[1, 0] = 59                                            # claimed by slot 1 only
    kf[4] = -1
    t = _tables(kf, [3, 8, 5, 9, -1], 60, 2)
    return dict(t=t, remove=[3, 1], cloud_slot=0, n_kp=40)


def cloud_trips():
    """Scene 3: three trips of the cloud walk, kept keypoints on both sides of each trip's edge; no live bytes, no tracks, nothing removed."""
    rng = np.random.default_rng(13)
    kf = np.full((2, 600), -1, np.int32)
    kf[1] = rng.permutation(700)[:600]
    t = _tables(kf, [4, 6], 700, 3, live=False, track=False, tri=0.0)
    kept = np.unique(np.r_[255, 256, 511, 512, 599, rng.choice(600, 150, replace=False)])
    kept = kept[~np.isin(kept, [254, 257, 510, 513, 598])]
    t["mp_flags"][kf[1, kept]] = 1
    t["kf_mp"][1, 100], t["kf_mp"][1, 300] = 700, -2     # invalid entries inside the walk
    return dict(t=t, remove=[], cloud_slot=1, n_kp=600, kept=kept[~np.isin(kept, [100, 300])])


def second_offsets_trip():
    """Scene 4: 9 removed slots x 8192 = 288 workgroups of 256 entries, more than one trip of block_offsets; 80 000 rows."""
    rng = np.random.default_rng(14)
    n_mp = 80000
    kf = np.where(rng.random((11, 8192)) < 0.8, rng.integers(0, n_mp, (11, 8192)), -1).astype(np.int32)
    t = _tables(kf, [20, 3, 4, 5, 6, 7, 8, 9, 10, 11, 21], n_mp, 4)
    t["mp_live"][rng.choice(n_mp, 4000, replace=False)] = 0
    return dict(t=t, remove=[5, 1, 2, 3, 9, 4, 6, 7, 8], cloud_slot=0, n_kp=8192)


SCENES = dict(per_frame=per_frame, two_removed=two_removed, cloud_trips=cloud_trips, second_offsets_trip=second_offsets_trip)
_cache = {}


def cached(name):
    """(scene, finish(scene)), computed once and shared; neither is to be changed."""
    if name not in _cache:
        sc = SCENES[name]()
        _cache[name] = (sc, finish(sc["t"], sc["remove"], sc["cloud_slot"], sc["n_kp"]))
    return _cache[name]


def scene_conditions(name, sc, want):
    """What each scene is there to hit."""
    t, kf = sc["t"], sc["t"]["kf_mp"]
    if name == "per_frame":
        row, n_kp = kf[3], sc["n_kp"]
        assert (row == -1).any() and (row >= 90).any() and (row < -1).any() and t["kf_id"][1] < 0 and valid(t, kf[1]).any()
        removed, cl = set(want["removed_rows"].tolist()), want["cloud_row"].tolist()
        assert 5 not in removed and want["n_obs"][5] == 3 and t["n_obs"][5] == 77                      # also seen by remaining slots, twice by one
        assert 20 in removed and 20 in cl and 21 in removed and 21 not in cl
        assert 22 in removed and 22 in kf[1] and 22 not in kf[[0, 2]]                                  # only the stale entry besides
        assert 23 not in removed and 23 not in cl and want["mp_live"][23] == 0 and t["mp_flags"][23] & 1
        assert cl.count(24) == 2 and want["removed_rows"].tolist().count(24) == 1
        assert 25 in cl and 25 not in removed
        assert 26 in removed and 26 not in cl and t["mp_flags"][26] & 1 and 27 not in removed and list(row[n_kp:]).count(-1) == 70 - n_kp - 2
        assert want["removed_rows"].tolist() != sorted(want["removed_rows"].tolist())                  # first-claim order is not row order
        assert (want["n_obs"] != 77).sum() == len(np.unique(row[valid(t, row)]))
    elif name == "two_removed":
        assert want["removed_rows"].tolist().count(57) == 1 and 58 not in want["removed_rows"] and want["n_obs"][58] == 1 and 59 in want["removed_rows"]
        order = want["removed_rows"].tolist()
        assert order.index(57) < order.index(59) and sc["cloud_slot"] not in sc["remove"] and len(want["cloud_row"]) > 3
    elif name == "cloud_trips":
        assert {255, 256, 511, 512, 599} <= set(want["cloud_kp"].tolist()) and np.array_equal(want["cloud_kp"], sc["kept"])
        assert not {254, 257, 510, 513, 598} & set(want["cloud_kp"].tolist()) and (want["cloud_track"] == -1).all() and want["counts"][1] == 0
    elif name == "second_offsets_trip":
        assert len(sc["remove"]) * kf.shape[1] > 256 * 256
        first = {}
        for i, s in enumerate(sc["remove"]):
            for j, r in enumerate(kf[s]):
                first.setdefault(int(r), i * kf.shape[1] + j)
        blocks = {first[int(r)] // 256 for r in want["removed_rows"]}
        assert max(blocks) >= 256 and min(blocks) < 256 and len(want["removed_rows"]) > 10000           # owners on both sides of the scan's trip edge
