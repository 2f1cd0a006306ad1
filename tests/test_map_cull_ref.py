"""tests/map_cull_ref.py (the specification of ms_observation_count and ms_map_cull) against a dictionary model written the way the reference
writes it: MapPoint::observations per point, MapDB::removeMapPoint, cullMapPoints over the whole map and cullKeyframes / removeKeyframe in
sorted order (mapper_helpers.cpp:349-482, mapdb.cpp:161-174, map_point.cpp:45-63).  Where the table breaks the reference's invariant (a row
twice in one slot) an observation carries its multiplicity and observations.size() is their sum.  Then: the fixed scene of the GPU tests
exercises every rule, so a kernel cannot pass on an empty case."""
import numpy as np

import map_cull_ref as R


class Model:
    def __init__(self, kf_mp, mp_flags, mp_live, n_mp, kf_id, kf_t):
        self.n_mp = n_mp
        self.slots = [[int(e) for e in row] for row in kf_mp]                      # Keyframe::mapPoints per slot
        self.kf_id, self.kf_t = [int(i) for i in kf_id], [float(t) for t in kf_t]
        self.slot_of = {i: k for k, i in enumerate(self.kf_id) if i >= 0}            # mapDB.keyframes
        self.flags, self.live = [int(f) for f in mp_flags], [int(l) for l in mp_live]
        self.observations = [dict() for _ in range(n_mp)]                           # per row: KfId -> multiplicity
        for k, row in enumerate(self.slots):
            if self.kf_id[k] >= 0:
                for e in row:
                    if 0 <= e < n_mp:
                        self.observations[e][self.kf_id[k]] = self.observations[e].get(self.kf_id[k], 0) + 1
        self.removed = {}

    def size(self, r):
        return sum(self.observations[r].values())

    def remove_map_point(self, r, why):                                              # mapdb.cpp:161-174
        for row in self.slots:                                                       # eraseObservation in every keyframe; stale entries too
            for j, e in enumerate(row):
                if e == r:
                    row[j] = -1
        self.observations[r] = {}
        self.live[r], self.flags[r] = 0, 0
        self.removed[r] = why

    def cull_map_points(self, current, min_age):                                     # :349-373
        for r in range(self.n_mp):
            if not self.live[r]:
                continue
            obs = self.observations[r]
            if not obs:
                self.remove_map_point(r, R.EMPTY)
                continue
            obs_age = int(self.kf_t[current] - self.kf_t[self.slot_of[min(obs)]])    # int(): toward zero
            if self.kf_id[current] not in obs and obs_age > min_age and not self.flags[r] & 1:
                self.remove_map_point(r, R.AGED)

    def remove_keyframe(self, k):                                                    # :375-431
        to_erase = set()
        for e in self.slots[k]:
            if 0 <= e < self.n_mp:
                obs = self.observations[e]
                obs[self.kf_id[k]] -= 1
                if obs[self.kf_id[k]] == 0:
                    del obs[self.kf_id[k]]
                if not obs and self.live[e]:
                    to_erase.add(e)
        for r in sorted(to_erase):
            self.remove_map_point(r, R.ORPHANED)
        self.slots[k] = [-1] * len(self.slots[k])

    def cull_keyframes(self, cand, keep, s):                                         # :433-482
        removed = [0] * len(cand)
        for i in sorted(range(len(cand)), key=lambda i: -self.kf_id[cand[i]]):
            if keep[i]:
                continue
            k = cand[i]
            n_map_points = n_critical = 0
            for e in self.slots[k]:
                if not 0 <= e < self.n_mp:
                    continue
                n_map_points += 1
                if self.size(e) <= s["min_obs_for_ba"]:
                    n_critical += 1
            if R.ratio_test(n_critical, n_map_points, s["max_critical_ratio"], s["ratio_float32"]):
                self.remove_keyframe(k)
                removed[i] = 1
        return removed


def random_case(rng):
    n_kf, stride, n_mp = int(rng.integers(1, 13)), int(rng.integers(1, 10)), int(rng.integers(0, 41))
    kf_mp = rng.integers(-1, n_mp + 2, (n_kf, stride)).astype(np.int32)              # rows may repeat within a slot
    kf_mp[rng.random((n_kf, stride)) < 0.3] = -1
    ids = rng.permutation(40)[:n_kf].astype(np.int32)
    ids[rng.random(n_kf) < 0.15] = -1
    current = int(rng.integers(0, n_kf))
    if ids[current] < 0:
        ids[current] = 41
    kf_t = np.round(rng.normal(0, 6, n_kf), int(rng.integers(0, 3)))                # negative ages, ages that truncate to 0
    others = [k for k in range(n_kf) if k != current and ids[k] >= 0]
    cand = rng.permutation(others)[:int(rng.integers(0, len(others) + 1))].astype(np.int32)
    keep = (rng.random(len(cand)) < 0.2).astype(np.uint8)
    s = R.settings(current, cull_points=int(rng.random() < 0.8), min_age=float(rng.integers(-3, 6)), min_obs_for_ba=int(rng.integers(0, 4)),
                   max_critical_ratio=float(rng.choice([0.0, 0.1, 0.25, 0.5, 0.7, 1.0, 1.5, -0.5])), ratio_float32=int(rng.integers(0, 2)))
    flags = rng.integers(0, 4, n_mp).astype(np.uint8)
    live = (rng.random(n_mp) < 0.8).astype(np.uint8) * rng.integers(1, 256, n_mp).astype(np.uint8)
    return kf_mp, flags, live, n_mp, ids, kf_t, cand, keep, s


def test_restatement_equals_the_dictionary_model_on_random_small_maps():
    rng = np.random.default_rng(2024)
    seen = {R.EMPTY: 0, R.AGED: 0, R.ORPHANED: 0, "kf": 0, "f32": 0}
    for case in range(2500):
        kf_mp, flags, live, n_mp, ids, kf_t, cand, keep, s = random_case(rng)
        n_obs, first, last = R.observation_count(kf_mp, n_mp, ids)
        M = Model(kf_mp, flags, live, n_mp, ids, kf_t)
        for r in range(n_mp):
            assert n_obs[r] == M.size(r), (case, r)
            obs = M.observations[r]
            assert first[r] == (M.slot_of[min(obs)] if obs else -1) and last[r] == (M.slot_of[max(obs)] if obs else -1), (case, r)
        got = R.map_cull(kf_mp, flags, live, n_mp, ids, kf_t, cand, keep, s)
        if s["cull_points"]:
            M.cull_map_points(s["current_slot"], s["min_age"])
        removed = M.cull_keyframes([int(c) for c in cand], keep, s)
        assert np.array_equal(got["kf_mp"], np.array(M.slots, np.int32).reshape(kf_mp.shape)), case
        assert np.array_equal(got["mp_live"] != 0, np.array(M.live, np.uint8) != 0) and np.array_equal(got["mp_flags"], np.array(M.flags, np.uint8)), case
        assert np.array_equal(got["mp_live"][got["mp_live"] != 0], live[got["mp_live"] != 0]), case      # a surviving byte keeps its value
        assert [int(x) for x in got["n_obs"]] == [M.size(r) for r in range(n_mp)], case
        assert [int(r) for r in got["removed_rows"]] == sorted(M.removed), case
        assert [int(w) for w in got["removed_why"]] == [M.removed[r] for r in sorted(M.removed)], case
        assert [int(x) for x in got["cand_removed"]] == removed and got["n_removed_kf"] == sum(removed), case
        for w in got["removed_why"]:
            seen[int(w)] += 1
        seen["kf"] += sum(removed)
        seen["f32"] += s["ratio_float32"]
    assert min(seen.values()) > 100, seen


def test_age_truncates_toward_zero():
    t = np.array([0.0, 2.75, -2.75])
    assert R.age_of(t, 1, 0) == 2 and R.age_of(t, 2, 0) == -2 and R.age_of(t, 0, 1) == -2 and R.age_of(t, 1, 2) == 5


def test_the_fixed_scene_exercises_every_rule():
    scene, s = R.make_scene(), R.scene_settings()
    assert scene["kf_mp"].shape == (70, 100) and scene["n_mp"] == 1003
    kf_mp, flags, live, n_mp, cur = scene["kf_mp"], scene["mp_flags"], scene["mp_live"], scene["n_mp"], s["current_slot"]
    out = R.run_scene(scene, s)
    why = np.zeros(n_mp, np.uint8)
    why[out["removed_rows"]] = out["removed_why"]
    for reason in (R.EMPTY, R.AGED, R.ORPHANED):
        assert (why == reason).sum() >= 5, reason
    # a live row spared by each single clause of the age rule, the other two clauses holding
    n_obs, first, last = R.observation_count(kf_mp, n_mp, scene["kf_id"])
    assert (first != last).any() and first[kf_mp[5][R.valid(kf_mp[5], n_mp)]].tolist().count(5) > 0        # slot 5 holds the oldest id
    in_cur = np.zeros(n_mp, bool)
    in_cur[kf_mp[cur][R.valid(kf_mp[cur], n_mp)]] = True
    seen = live.astype(bool) & (n_obs > 0)
    old = np.array([seen[r] and R.age_of(scene["kf_t"], cur, first[r]) > s["min_age"] for r in range(n_mp)])
    tri = (flags & 1) != 0
    assert (seen & in_cur & old & ~tri).any() and (seen & ~in_cur & ~old & ~tri).any() and (seen & ~in_cur & old & tri).any()
    assert not why[seen & (in_cur | ~old | tri)].tolist().count(R.AGED)
    # free rows are never removed; observed rows that hold no map point stay as they are
    assert not why[live == 0].any() and (n_obs[live == 0] > 0).any() and (n_obs[live == 0] == 0).any()
    # candidates: kept by cand_keep, removed and kept on the ratio, and a decision that the initial counts alone would not give
    assert scene["cand_keep"].sum() >= 1 and len(out["trace"]) == len(scene["cand"]) - scene["cand_keep"].sum()
    decisions = [t[3] for t in out["trace"]]
    assert any(decisions) and not all(decisions)
    assert out["n_removed_kf"] == sum(decisions) and all(out["cand_removed"][scene["cand_keep"] != 0] == 0)
    after1 = R.run_scene(scene, s, n_cand=0)                 # pass 1 alone
    differs = 0
    for k, n_map_points, n_critical, removed in out["trace"]:
        rows = after1["kf_mp"][k][R.valid(after1["kf_mp"][k], n_mp)]
        static = R.ratio_test(int((after1["n_obs"][rows] <= s["min_obs_for_ba"]).sum()), len(rows), s["max_critical_ratio"], s["ratio_float32"])
        differs += static != removed
    assert differs >= 1
    ids = scene["kf_id"][[t[0] for t in out["trace"]]]
    assert (np.diff(ids) < 0).all() and not (np.diff([t[0] for t in out["trace"]]) < 0).all()               # id order is not slot order
    # one pair of settings for which ratio_float32 changes a decision
    pair = R.find_ratio_pair(scene, s)
    assert pair is not None and pair[0]["ratio_float32"] == 0 and pair[1]["ratio_float32"] == 1
    # without the point pass nothing is removed for reasons 1 and 2
    out0 = R.run_scene(scene, R.scene_settings(cull_points=0))
    assert set(out0["removed_why"].tolist()) <= {R.ORPHANED} and np.array_equal(R.run_scene(scene, s, n_cand=0)["cand_removed"], np.zeros(0, np.uint8))


def test_the_large_scenes_remove_rows_on_both_sides_of_the_second_scan_trip():
    # what tests/test_gpu_scan_trips.py relies on: the offsets of the blocks past 65 536 rows are a carry (non-zero, and used)
    for n_mp in R.LARGE_N_MP:
        sc = R.large_scene(n_mp)
        assert sc["kf_mp"].shape == (12, 2048) and len(sc["cand"]) == 11 and sc["current"] not in sc["cand"]
        assert {-1, n_mp, n_mp + 1} <= set(np.unique(sc["kf_mp"]).tolist())
        for ratio_float32 in (0, 1):
            out = R.run_scene(sc, R.large_settings(sc, ratio_float32))
            rows, why = out["removed_rows"], out["removed_why"]
            past = rows >= R.LARGE_TRIP
            print(n_mp, ratio_float32, "removed", len(rows), "past the trip", int(past.sum()), "reasons there", np.bincount(why[past], minlength=4)[1:].tolist(),
                  "keyframes", out["n_removed_kf"])
            assert (~past).sum() >= 1000 and set(why.tolist()) == {R.EMPTY, R.AGED, R.ORPHANED} and 1 <= out["n_removed_kf"] < len(sc["cand"])
            if n_mp == R.LARGE_TRIP + 300:                   # a second trip of two blocks: every reason occurs in it
                assert past.sum() >= 50 and set(why[past].tolist()) == {R.EMPTY, R.AGED, R.ORPHANED}
            elif n_mp == R.LARGE_TRIP + 1:                   # a second trip of one row: that row is removed
                assert rows[-1] == R.LARGE_TRIP and past.sum() == 1
            else:
                assert past.sum() == 0


def test_the_fill_scene_removes_candidates_behind_the_rows_one_workgroup():
    sc, s = R.fill_scene()
    assert sc["n_mp"] <= 256 and len(sc["cand"]) == 300 == len(set(sc["cand"].tolist())) and 2 + len(sc["cand"]) > 256 * ((sc["n_mp"] + 255) // 256)
    first = R.run_scene(sc, s)
    assert first["cand_removed"][R.FILL_FIRST:].sum() >= 5 and 0 < first["cand_removed"][:R.FILL_FIRST].sum() < R.FILL_FIRST
    again = R.fill_second_call(sc, first)
    kept = again["cand_keep"] != 0
    assert np.array_equal(kept[R.FILL_FIRST:], first["cand_removed"][R.FILL_FIRST:] != 0) and not kept[:R.FILL_FIRST].any()
    second = R.run_scene(again, s)
    assert not second["cand_removed"][kept].any()            # where the first call left a 1, the second call's answer is 0
    print("first call removes", int(first["cand_removed"][R.FILL_FIRST:].sum()), "of", 300 - R.FILL_FIRST, "candidates behind position", R.FILL_FIRST,
          "and", int(first["cand_removed"].sum()), "in all; the second", int(second["cand_removed"].sum()))
