"""tests/obs_lists_ref.py (the specification of ms_observation_lists) against a dictionary model written the way the reference
keeps its observations -- `std::map<KfId, KpId> observations` per map point, filled by walking the keyframes (map_point.hpp,
MapPoint::addObservation) -- on random small maps, and the properties of the fixed scenes the GPU test relies on."""
import numpy as np

import obs_lists_ref as R


def model(kf_mp, n_mp, kf_id, mp_flags, kp, desc_base, sel, n_levels):
    """Sequential, with dictionaries.  A keyframe lists a map point at most once here (the reference's invariant), so a KfId is a key."""
    observations = {}                                        # MpId -> {KfId: (slot, KpId)}
    for slot in range(len(kf_id)):                           # any order: the map sorts by key
        if kf_id[slot] < 0:
            continue
        for j, r in enumerate(kf_mp[slot]):
            if 0 <= r < n_mp:
                obs = observations.setdefault(int(r), {})
                assert int(kf_id[slot]) not in obs
                obs[int(kf_id[slot])] = (slot, j)
    source = kf_mp[sel["slot"]] if sel["source"] == R.FROM_SLOT else sel["rows_in"]
    out = {k: [] for k in R.ROW_ARRAYS + R.OBS_ARRAYS}
    out["obs_start"].append(0)
    seen, violations = set(), 0
    for r in source:
        r = int(r)
        if not 0 <= r < n_mp or r in seen:
            continue
        seen.add(r)
        obs = observations.get(r, {})
        if sel["filter"] == R.REFRESH and not mp_flags[r] & 2:                          # NOT_TRIANGULATED or BAD, :1066
            continue
        if sel["filter"] == R.RETRIANGULATE and not ((mp_flags[r] & 1) == 0 or len(obs) >= 2):      # :1088
            continue
        if sel["drop_empty"] and not obs:
            continue
        out["rows"].append(r)
        out["n_obs_row"].append(len(obs))
        out["was_triangulated"].append(int((mp_flags[r] & 2) != 0))
        first = 0
        for i, kid in enumerate(sorted(obs)):                # std::map iteration: ascending KfId
            slot, j = obs[kid]
            octave = int(kp["octave"][slot, j])
            if n_levels > 0 and not 0 <= octave < n_levels:
                violations += 1
                octave = min(max(octave, 0), n_levels - 1)
            if i == 0:
                first = octave
            out["obs_kf"].append(slot); out["obs_kp"].append(j); out["obs_octave"].append(octave)
            out["obs_x"].append(kp["x"][slot, j]); out["obs_y"].append(kp["y"][slot, j]); out["obs_depth"].append(kp["depth"][slot, j])
            out["obs_desc"].append(-1 if desc_base[slot] < 0 else int(desc_base[slot]) + j)
        out["first_octave"].append(first)
        out["obs_start"].append(len(out["obs_kf"]))
    return out, violations


def random_map(rng):
    n_kf, stride, n_mp = int(rng.integers(1, 7)), int(rng.integers(1, 9)), int(rng.integers(0, 13))
    kf_mp = np.full((n_kf, stride), -1, np.int32)
    for k in range(n_kf):
        n = int(rng.integers(0, min(stride, n_mp) + 1))
        row = np.full(stride, -1, np.int64)
        row[:n] = rng.permutation(n_mp)[:n]                  # distinct inside a slot
        junk = rng.random(stride) < 0.15
        row[n:][junk[n:]] = rng.choice([n_mp, n_mp + 3, R.INT32_MIN, -7], int(junk[n:].sum()))
        kf_mp[k] = rng.permutation(row)
    kf_id = rng.permutation(20)[:n_kf].astype(np.int32)
    kf_id[rng.random(n_kf) < 0.25] = -1
    kp, base = R.keypoint_table(rng, n_kf, stride)
    kp["octave"][rng.random((n_kf, stride)) < 0.05] = rng.choice([-1, R.N_LEVELS, 40])
    return kf_mp, n_mp, kf_id, rng.integers(0, 4, max(n_mp, 1)).astype(np.uint8), kp, base


def test_restatement_equals_the_dictionary_model_on_random_maps():
    rng = np.random.default_rng(2027)
    n_checked = n_nonempty = 0
    for _ in range(2400):
        kf_mp, n_mp, kf_id, flags, kp, base = random_map(rng)
        live = np.nonzero(kf_id >= 0)[0]
        if rng.integers(0, 2) and len(live):
            sel = R.select(R.FROM_SLOT, int(rng.integers(0, 3)), int(rng.integers(0, 2)), int(rng.choice(live)))
        else:
            rows_in = rng.integers(-2, n_mp + 2, int(rng.integers(0, 2 * n_mp + 3)))
            sel = R.select(R.FROM_ROWS, int(rng.integers(0, 3)), int(rng.integers(0, 2)), rows_in=rows_in)
        n_levels = int(rng.choice([0, R.N_LEVELS]))
        got = R.observation_lists(kf_mp, n_mp, kf_id, flags, kp, base, sel, n_levels)
        want, violations = model(kf_mp, n_mp, kf_id, flags, kp, base, sel, n_levels)
        for name in R.ROW_ARRAYS + R.OBS_ARRAYS:
            assert got[name].tolist() == [x.item() if hasattr(x, "item") else x for x in want[name]], name
        assert (got["n_rows"], got["n_obs"], got["violations"]) == (len(want["rows"]), len(want["obs_kf"]), violations)
        n_checked += 1
        n_nonempty += got["n_obs"] > 0
    assert n_checked >= 2000 and n_nonempty >= 500


def test_multiplicity_follows_observation_count():
    """Entries of one slot that name the same row are all kept, in ascending j: the lengths are ms_observation_count's."""
    import map_cull_ref
    s = R.scene_a()
    out = R.run_scene(s, R.select(R.FROM_ROWS, rows_in=np.arange(s["n_mp"])))
    assert np.array_equal(out["n_obs_row"], map_cull_ref.observation_count(s["kf_mp"], s["n_mp"], s["kf_id"])[0])
    slot, row = R.A_TWICE
    a, b = out["obs_start"][row], out["obs_start"][row + 1]
    mine = out["obs_kp"][a:b][out["obs_kf"][a:b] == slot]
    assert len(mine) == 2 and mine[0] < mine[1]
    once = R.run_scene(s, R.select(R.FROM_SLOT, slot=slot))
    assert (once["rows"] == row).sum() == 1 and (s["kf_mp"][slot] == row).sum() == 2       # selected at its first occurrence only


def test_scene_a_exercises_every_rule():
    s = R.scene_a()
    n_mp, kf_mp, kf_id = s["n_mp"], s["kf_mp"], s["kf_id"]
    whole = R.select(R.FROM_ROWS, rows_in=np.arange(n_mp))
    out = R.run_scene(s, whole)
    assert kf_mp.shape == (R.A_KF, R.A_STRIDE) and all(out["n_obs_row"][r] == n for r, n in s["lengths"].items())
    assert {0, 1, 2, 63, 64, 65} <= set(out["n_obs_row"].tolist())
    live = np.nonzero(kf_id >= 0)[0]
    assert (np.diff(kf_id[live]) < 0).any() and len(set(kf_id[live].tolist())) == len(live)          # not monotone in the slot, distinct
    for r in np.nonzero(out["n_obs_row"] > 1)[0]:            # and every list IS in KfId order, which is not slot order for some
        ids = kf_id[out["obs_kf"][out["obs_start"][r]:out["obs_start"][r + 1]]]
        assert (np.diff(ids) >= 0).all()
    assert any((np.diff(out["obs_kf"][out["obs_start"][r]:out["obs_start"][r + 1]]) < 0).any() for r in range(n_mp))
    empty = np.nonzero(kf_id < 0)[0]
    assert len(empty) >= 3 and not np.isin(out["obs_kf"], empty).any()
    stale = kf_mp[empty]
    assert ((stale >= 0) & (stale < n_mp)).sum() >= 6        # the stale entries would count if the empty slots were read ...
    counted = R.observation_lists(kf_mp, n_mp, np.where(kf_id < 0, 1000 + np.arange(len(kf_id)), kf_id), s["mp_flags"], s["kp"], s["desc_base"], whole)
    assert counted["n_obs"] > out["n_obs"]                   # ... and the result would differ
    for v in (-1, n_mp, n_mp + 1, R.INT32_MIN):
        assert (kf_mp[live] == v).any()
    assert (out["obs_desc"] == -1).any() and (out["obs_desc"] >= 0).any()
    assert out["was_triangulated"].min() == 0 and out["was_triangulated"].max() == 1
    for source, kw in ((R.FROM_ROWS, dict(rows_in=np.arange(n_mp))), (R.FROM_SLOT, dict(slot=R.A_CURRENT))):
        everything = R.run_scene(s, R.select(source, **kw))
        for flt in (R.REFRESH, R.RETRIANGULATE):             # each filter drops rows and keeps rows
            part = R.run_scene(s, R.select(source, flt, **kw))
            assert 0 < part["n_rows"] < everything["n_rows"]
    assert R.run_scene(s, R.select(R.FROM_ROWS, R.ALL, 1, rows_in=np.arange(n_mp)))["n_rows"] == int((out["n_obs_row"] > 0).sum()) < n_mp
    retri = R.run_scene(s, R.select(R.FROM_ROWS, R.RETRIANGULATE, rows_in=np.arange(n_mp)))
    kept = np.zeros(n_mp, bool)
    kept[retri["rows"]] = True
    tri = (s["mp_flags"] & 1) != 0
    assert (kept & tri & (out["n_obs_row"] >= 2)).any() and (~kept & tri & (out["n_obs_row"] < 2)).any() and kept[~tri].all()


def test_scene_b_has_the_long_lists_and_two_scan_trips():
    s = R.scene_b()
    out = R.run_scene(s, R.select(R.FROM_ROWS, rows_in=np.arange(s["n_mp"])))
    assert s["kf_mp"].shape == (1100, 8) and all(out["n_obs_row"][r] == n for r, n in s["lengths"].items())
    assert out["n_obs_row"][6] == 1100 and out["n_obs_row"][5] == 1025
    assert -(-s["n_mp"] // 256) > 256                        # more block totals than one trip of the offsets scan takes


def test_scene_c_has_more_long_lists_than_the_long_sort_has_workgroups():
    s = R.scene_c()
    out = R.run_scene(s, R.select(R.FROM_ROWS, rows_in=np.arange(s["n_mp"])))
    assert s["kf_mp"].shape == (66, 1040) and all(out["n_obs_row"][r] == n for r, n in s["lengths"].items())
    n_long = int((out["n_obs_row"] > 64).sum())              # the lists a wave does not sort on its own
    assert n_long == 1030 > 1024 and out["n_obs_row"].max() == 65 and {0, 1} <= set(out["n_obs_row"].tolist())
    a, b = out["obs_start"][7], out["obs_start"][8]          # a list is in id order, which is not slot order, and its keypoints are not in order either
    assert (np.diff(s["kf_id"][out["obs_kf"][a:b]]) > 0).all() and (np.diff(out["obs_kf"][a:b]) < 0).any() and (np.diff(out["obs_kp"][a:b]) < 0).any()
