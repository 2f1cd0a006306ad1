"""The map kernels at the sizes where their one-workgroup scans take a second trip and carry a running sum into it: k_cull_offsets past
65 536 rows, k_gate_offsets with a view past 65 536 entries (9.4), k_refresh_dscan past 1 024 rows (9.5, 9.9); k_obs_fill
when ms_map_cull's result block is longer than the rows; and k_ol_sort_long with more long lists than workgroups.  Everything is compared for exact equality with the features' restatements, through
the helpers of the features' own tests.  The scenes come from the *_ref modules, whose CPU tests hold the conditions that make these runs
bite: a non-zero carry, results on both sides of every trip boundary, the longest descriptor list in the first trip and in the last."""
import numpy as np
import pytest

import map_cull_ref as CR
import map_refresh_ref as MR
import mi355slam
import obs_lists_ref as OR
import project_gate_ref as GR
import test_gpu_map_cull as TC
import test_gpu_obs_lists as TO
import test_gpu_project_gate as TG

pytestmark = pytest.mark.gpu


# ---- ms_map_cull ----

def cull(ctx, sc, s):
    return TC.run(ctx, sc["kf_mp"], sc["mp_flags"], sc["mp_live"], sc["n_mp"], sc["kf_id"], sc["kf_t"], sc["cand"], sc["cand_keep"], s)


@pytest.mark.parametrize("n_mp", CR.LARGE_N_MP)
def test_cull_packs_the_removed_rows_past_one_trip_of_block_offsets(ctx, n_mp):
    sc = CR.large_scene(n_mp)
    kf_mp, flags, live, cand = sc["kf_mp"], sc["mp_flags"], sc["mp_live"], sc["cand"]
    for ratio_float32 in (0, 1):
        s = CR.large_settings(sc, ratio_float32)
        w = CR.run_scene(sc, s)
        got = cull(ctx, sc, s)
        print(n_mp, ratio_float32, "removed rows", len(got["removed_rows"]), "of them past the first trip", int((got["removed_rows"] >= CR.LARGE_TRIP).sum()), "want",
              len(w["removed_rows"]), int((w["removed_rows"] >= CR.LARGE_TRIP).sum()))
        TC.assert_same_cull(got, w)
        # rows and slots not named by the result are byte-identical to the input
        rows = np.zeros(n_mp, bool)
        rows[got["removed_rows"]] = True
        assert np.array_equal(got["mp_live"][~rows], live[~rows]) and np.array_equal(got["mp_flags"][~rows], flags[~rows])
        slots = np.zeros(len(kf_mp), bool)
        slots[cand[got["cand_removed"] != 0]] = True
        untouched = ~np.append(rows, [False, False])[np.where(kf_mp >= 0, kf_mp, n_mp)] & ~slots[:, None]
        assert np.array_equal(got["kf_mp"][untouched], kf_mp[untouched])
    # two slots, five rows, on the workspace the large call left: its block offsets must not show
    kf_mp = np.array([[0, 1, 4], [1, -1, 5]], np.int32)
    flags, live = np.array([0, 0, 1, 0, 0], np.uint8), np.array([1, 1, 1, 1, 0], np.uint8)
    kf_id, kf_t = np.array([7, 3], np.int32), np.array([10.0, 2.0])
    s2 = CR.settings(0, 1, min_age=1.0, min_obs_for_ba=1, max_critical_ratio=0.75)
    w = CR.map_cull(kf_mp, flags, live, 5, kf_id, kf_t, [1], None, s2)
    assert len(w["removed_rows"]) >= 1
    TC.assert_same_cull(TC.run(ctx, kf_mp, flags, live, 5, kf_id, kf_t, [1], None, s2), w)


def test_cull_zeroes_a_result_block_longer_than_the_rows(ctx):
    sc, s = CR.fill_scene()
    w1 = CR.run_scene(sc, s)
    assert w1["cand_removed"][CR.FILL_FIRST:].any()
    first = cull(ctx, sc, s)
    TC.assert_same_cull(first, w1)
    again = CR.fill_second_call(sc, w1)                      # the same shapes, so the same place in the workspace
    w2 = CR.run_scene(again, s)
    second = cull(ctx, again, s)
    print("cand_removed behind position", CR.FILL_FIRST, "first call", first["cand_removed"][CR.FILL_FIRST:].tolist(), "second call",
          second["cand_removed"][CR.FILL_FIRST:].tolist(), "want", w2["cand_removed"][CR.FILL_FIRST:].tolist())
    TC.assert_same_cull(second, w2)
    assert not second["cand_removed"][again["cand_keep"] != 0].any()


# ---- ms_project_gate ----

LARGE_DRAWS = GR.large_draws()


@pytest.mark.parametrize("draw", LARGE_DRAWS, ids=["seed%d" % d[0] for d in LARGE_DRAWS])
def test_gate_packs_a_view_past_one_trip_of_workgroup_counts(ctx, draw):
    sc = GR.large_scene(draw)
    assert np.array_equal(sc["sf"], mi355slam.scale_factors(8, 1.2))
    table = TG.upload(ctx, sc["table"])
    entries, per_view = mi355slam.project_gate(ctx, table, sc["views"], sc["sf"], 1.2)
    counts = [len(v["indices"]) for v in sc["views"]]
    print(draw[0], "n_kept", [len(p["kept"]) for p in per_view], "want", [len(r["kept"]) for r in sc["ref"]], "of", counts)
    TG.check(sc, entries, per_view)
    # the long view alone: the same bytes as inside the batch
    v = int(np.argmax(counts))
    at, n = sum(counts[:v]), counts[v]
    assert n > GR.LARGE_TRIP
    alone_e, alone_v = mi355slam.project_gate(ctx, table, [sc["views"][v]], sc["sf"], 1.2)
    for k in entries:
        assert np.array_equal(alone_e[k].view(np.uint8), entries[k][at:at + n].view(np.uint8)), k
    for k in per_view[v]:
        assert np.array_equal(alone_v[0][k].view(np.uint8), per_view[v][k].view(np.uint8)), k


# ---- ms_observation_lists ----

def test_observation_lists_sort_more_long_lists_than_the_long_sort_has_workgroups(ctx):
    """k_ol_sort_long strides its 1024 workgroups over the lists longer than 64 and ranks each through one LDS array: with 1030 such lists a
    workgroup takes a second one."""
    scene = TO.Scene(ctx, OR.scene_c())
    try:
        rows_in = np.random.default_rng(6).permutation(scene.s["n_mp"]).astype(np.int32)
        want = TO.check(scene, OR.select(OR.FROM_ROWS, rows_in=rows_in))
        assert (want["n_obs_row"] > 64).sum() > 1024
        TO.check(scene, OR.select(OR.FROM_ROWS, OR.RETRIANGULATE, 1, rows_in=rows_in[::-1]))
    finally:
        scene.free()


# ---- ms_map_refresh_lists ----

def scan_setup(ctx, n_rows, longest_last):
    """A scan scene as device tables (descriptors: a pool laid out slot by slot) and its lists built on the device, the way
    test_gpu_obs_lists.refresh_setup builds them."""
    sc = MR.make_scan_scene(n_rows, longest_last)
    prob = sc["prob"]
    rng = np.random.default_rng(77)
    n_kf, n_mp, n_obs = len(sc["kf_pose"]), len(sc["table"]["pos"]), int(prob["obs_start"][-1])
    octave = rng.integers(0, len(sc["sf"]), n_obs).astype(np.int32)
    octave[prob["obs_start"][:-1]] = prob["first_octave"]    # a row's first observation carries the fixture's octave
    kf_mp, tables, js = TO.as_tables(prob, n_kf, dict(octave=octave), dict(octave=0))
    stride = kf_mp.shape[1]
    base = (np.arange(n_kf) * stride).astype(np.int32)
    base[n_kf - 2:] = -1                                     # the two slots without descriptors
    pool = rng.integers(0, 2 ** 32, (n_kf * stride, 8), dtype=np.uint64).astype(np.uint32)
    src, okf = prob["obs_desc"].astype(np.int64), prob["obs_kf"].astype(np.int64)
    has = src >= 0                                           # the fixture's descriptors: near-duplicates, so medoids are contested
    pool[okf[has] * stride + js[has]] = sc["pool"][src[has]]
    table = mi355slam.KeyframeTable(ctx, kf_mp)
    zeros = np.zeros((n_kf, stride), np.float32)
    kp = mi355slam.KeypointTable(ctx, zeros, zeros, tables["octave"], zeros)
    flags_in = rng.integers(0, 4, n_mp).astype(np.uint8)
    lists, n_rows_dev, n_obs_dev = table.observation_lists(np.arange(n_kf, dtype=np.int32), n_mp, OR.select(OR.FROM_ROWS, OR.ALL, 1, rows_in=prob["rows"]), kp, base,
                                                           flags_in, len(sc["sf"]))
    table.kf_mp.free(); kp.free()
    assert (n_rows_dev, n_obs_dev) == (n_rows, n_obs)
    got = lists.download(n_rows_dev, n_obs_dev)
    for name in ("rows", "obs_start", "obs_kf", "first_octave"):             # the device lists ARE the scene's lists
        assert TO.bits(got[name]) == TO.bits(np.ascontiguousarray(prob[name])), name
    assert np.array_equal(got["obs_desc"], np.where(has, okf * stride + js, -1))
    return dict(sc=sc, lists=lists, n_rows=n_rows_dev, n_obs=n_obs_dev, got=got, pool=pool, flags_in=flags_in, n_mp=n_mp, prob=prob)


@pytest.mark.parametrize("n_rows,longest_last", MR.SCAN_CASES)
def test_refresh_lists_scans_the_descriptor_counts_past_one_trip(ctx, n_rows, longest_last):
    T = scan_setup(ctx, n_rows, longest_last)
    try:
        sc, got = T["sc"], T["got"]
        n_desc = MR.descriptor_counts(got)
        assert n_desc[MR.SCAN_TRIP - 1] == 0 and n_desc.max() == 257 and (int(np.argmax(n_desc)) >= MR.SCAN_TRIP) == longest_last
        lists_prob = {k: got[k] for k in ("rows", "obs_start", "obs_kf", "obs_desc", "first_octave")}
        other = np.setdiff1d(np.arange(T["n_mp"]), got["rows"])
        for with_desc in (True, False):
            want, want_medoid = MR.refresh(sc["table"], sc["kf_pose"], T["pool"] if with_desc else None, lists_prob, sc["sf"])
            host, device = TO._refresh_state(ctx, T, with_desc, "host"), TO._refresh_state(ctx, T, with_desc, "device")
            print(n_rows, longest_last, with_desc, "medoids device / host twin / restatement that differ:", int((device["medoid"] != host["medoid"]).sum()),
                  int((device["medoid"] != want_medoid).sum()), "descriptor rows that differ:", int((device["desc"] != want["desc"]).any(axis=1).sum()))
            for name in host:                                # the twin on the downloaded lists
                assert host[name].dtype == device[name].dtype and TO.bits(host[name]) == TO.bits(device[name]), name
            assert device["medoid"].dtype == want_medoid.dtype and np.array_equal(device["medoid"], want_medoid)      # the restatement
            for name in ("norm", "min_dist", "max_dist", "desc"):
                assert TO.bits(device[name]) == TO.bits(np.ascontiguousarray(want[name])), name
                assert len(other) and TO.bits(device[name][other]) == TO.bits(np.ascontiguousarray(sc["table"][name])[other]), name
            assert TO.bits(device["pos"]) == TO.bits(np.ascontiguousarray(sc["table"]["pos"])) and TO.bits(device["flags"]) == TO.bits(T["flags_in"])
            if with_desc:
                assert {-2, -1} <= set(device["medoid"].tolist()) and (device["medoid"][MR.SCAN_TRIP:] >= 0).sum() >= min(n_rows - MR.SCAN_TRIP, 1)
                assert device["medoid"][MR.SCAN_TRIP - 1] == -1
            else:
                assert (device["medoid"] == -1).all()
    finally:
        T["lists"].free()
