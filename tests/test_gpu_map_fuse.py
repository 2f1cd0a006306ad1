"""ms_map_fuse and ms_map_replace_pairs on the device against tests/map_fuse_ref.py, their specification.  Integer work: every
comparison is exact equality.  tests/test_map_fuse_ref.py asserts on the restatement that the base scene holds the conditions relied on
here (every code in every trip of a three-trip view, chains, ties, the track cases, the early stop)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import map_fuse_ref as R
import mi355slam

pytestmark = pytest.mark.gpu

SCENE = R.make_scene()
WANT = {}                                                    # source_slot -> the restatement on the scene, computed once
PER_ENTRY = ("outcome", "kp", "other", "erased_rows", "erased_into")


def want(source_slot):
    if source_slot not in WANT:
        WANT[source_slot] = R.fuse_tables(SCENE["T"], SCENE["mp_index"], SCENE["views"], SCENE["cand"], source_slot)
    return WANT[source_slot]


def fuse(ctx, S, source_slot=-1, T=None, table=None, **kw):
    T = S["T"] if T is None else T
    t = mi355slam.KeyframeTable(ctx, T["kf_mp"]) if table is None else table
    try:
        return t.fuse(T, S["mp_index"], S["views"], S["n_kept"], S["kept_entry"], S["top_idx"], S["top_dist"], S["max_dist"], source_slot, **kw)
    finally:
        if table is None:
            t.kf_mp.free()


def assert_same(got, w, lists=PER_ENTRY):
    assert R.same(got, w, R.TABLE_KEYS + tuple(lists) + ("counts",)) == []
    assert got["views_done"] == w["views_done"] and got["n_erased"] == len(w["erased_rows"])


def test_scene_walks_every_view(ctx):
    got = fuse(ctx, SCENE)
    assert_same(got, want(-1))
    assert got["views_done"] == 6 and (got["counts"] > 0).all() and got["n_erased"] > 100


def test_scene_stops_early_for_the_source_slot(ctx):
    got = fuse(ctx, SCENE, SCENE["source_slot"])
    w = want(SCENE["source_slot"])
    assert_same(got, w)
    assert 1 <= got["views_done"] < 6


@pytest.mark.parametrize("left_out", PER_ENTRY)
def test_each_optional_output_left_out_once(ctx, left_out):
    keep = tuple(k for k in PER_ENTRY if k != left_out)
    got = fuse(ctx, SCENE, want=keep)
    assert left_out not in got
    assert_same(got, want(-1), keep)


def test_without_track_tables(ctx):
    T = {k: v for k, v in SCENE["T"].items() if k not in ("mp_track", "track_row", "track_base")}
    w = R.fuse_tables(T, SCENE["mp_index"], SCENE["views"], SCENE["cand"], -1)
    got = fuse(ctx, SCENE, T=T)
    assert "mp_track" not in got and "track_row" not in got
    assert_same(got, w)
    assert np.array_equal(w["outcome"], want(-1)["outcome"])                     # the tracks decide nothing


def violated(which):
    S = dict(SCENE, T=R.copy_tables(SCENE["T"]))
    slot, first, count = S["views"][2]
    if which == "dead row listed":
        j = int(np.argmax((S["T"]["kf_mp"][slot] >= 0) & (S["T"]["kf_mp"][slot] < 3000)))
        S["T"]["mp_live"][S["T"]["kf_mp"][slot, j]] = 0
    elif which == "kept_entry outside its slice":
        S["kept_entry"] = S["kept_entry"].copy()
        S["kept_entry"][first + 1] = first + count           # the first entry behind the slice
    elif which == "kept_entry negative":
        S["kept_entry"] = S["kept_entry"].copy()
        S["kept_entry"][first] = -1
    elif which == "top_idx at stride":
        S["top_idx"] = S["top_idx"].copy()
        S["top_idx"][4 * (first + 2)] = 640
    elif which == "top_idx below -1":
        S["top_idx"] = S["top_idx"].copy()
        S["top_idx"][4 * first] = -2
    return S


@pytest.mark.parametrize("which", ("dead row listed", "kept_entry outside its slice", "kept_entry negative", "top_idx at stride", "top_idx below -1"))
def test_each_pre_pass_violation_leaves_the_tables_as_they_were(ctx, which):
    S = violated(which)
    t = mi355slam.KeyframeTable(ctx, S["T"]["kf_mp"])
    with pytest.raises(mi355slam.MsError, match="violations on the device"):
        fuse(ctx, S, table=t)
    after = t._fuse_last
    assert R.same(after, S["T"], R.TABLE_KEYS) == []
    assert (after["outcome"] == 0).all() and (after["kp"] == -1).all() and (after["other"] == -1).all()
    t.kf_mp.free()


def test_host_validation_runs_in_front_of_the_device(ctx):
    S = dict(SCENE, mp_index=SCENE["mp_index"].copy())
    slot, first, count = S["views"][1]
    S["mp_index"][first + 1] = S["mp_index"][first]
    t = mi355slam.KeyframeTable(ctx, S["T"]["kf_mp"])
    with pytest.raises(mi355slam.MsError, match="view 1 lists row %d twice" % S["mp_index"][first]):
        fuse(ctx, S, table=t)
    assert R.same(t._fuse_last, S["T"], R.TABLE_KEYS) == []
    t.kf_mp.free()


def test_two_calls_give_the_same_bits_and_the_workspace_only_grows(ctx):
    allocs = mi355slam.lib().ms_debug_host_allocs
    allocs.restype = C.c_longlong
    rng = np.random.default_rng(2)
    pairs = R.make_pairs(rng, SCENE["T"], 40)
    t = mi355slam.KeyframeTable(ctx, SCENE["T"]["kf_mp"])
    a = fuse(ctx, SCENE)
    pa = t.replace_pairs(SCENE["T"], pairs)
    before = allocs()
    b = fuse(ctx, SCENE)
    t.kf_mp.free()
    t = mi355slam.KeyframeTable(ctx, SCENE["T"]["kf_mp"])
    pb = t.replace_pairs(SCENE["T"], pairs)
    fuse(ctx, SCENE, SCENE["source_slot"], want=())          # and a smaller one
    assert allocs() == before
    assert R.same(a, b, R.TABLE_KEYS + PER_ENTRY + ("counts",)) == []
    assert R.same(pa, pb, R.TABLE_KEYS + ("outcome", "erased_rows", "erased_into")) == []
    t.kf_mp.free()


def small_scene(seed, n_kf, stride, n_mp, per_slot, counts):
    rng = np.random.default_rng(seed)
    T = R.make_tables(rng, n_kf, stride, n_mp, per_slot, dead=0.15)
    slots = rng.permutation(n_kf)[: len(counts)]
    mp_index, views, cand = R.make_views(rng, T, slots, counts)
    kept_entry, top_idx, top_dist, n_kept = R.lists_from_candidates(rng, cand, views)
    return dict(T=T, mp_index=mp_index, views=views, cand=cand, kept_entry=kept_entry, top_idx=top_idx, top_dist=top_dist, n_kept=n_kept, max_dist=50)


# the loops of the walk past their first trip: a replace strides 16 waves over the slots (second trip from 17 slots, fifth from
# 65) and scans a row 64 entries at a time; the marks of K and the pre-pass go over a row in steps of 1 024 and 256; a view's slice is read
# in trips of 1 024 entries (the base scene's first view takes three)
@pytest.mark.parametrize("n_kf, stride, n_mp, per_slot, counts", [
    (70, 33, 400, 20, (300, 150, 90)),                       # more than 64 slots, a stride below one wave
    (17, 64, 300, 40, (200, 100)),                           # the second trip over the slots holds one slot; a row is exactly one scan
    (5, 1100, 1500, 700, (1100, 400)),                       # a stride above 1 024; a slice of two trips
    (3, 2100, 900, 500, (800, 1)),                           # three trips over a row for the marks
])
def test_tables_past_each_loops_first_trip(ctx, n_kf, stride, n_mp, per_slot, counts):
    S = small_scene(n_kf * 1000 + stride, n_kf, stride, n_mp, per_slot, counts)
    w = R.fuse_tables(S["T"], S["mp_index"], S["views"], S["cand"], -1)
    assert len(w["erased_rows"]) >= 10 and (w["counts"][4:] > 0).all()
    if counts[0] > R.TRIP:                                   # replaces in the last trip
        assert (w["outcome"][S["views"][0][1] + R.TRIP:S["views"][0][1] + counts[0]] >= 6).sum() >= 3
    assert_same(fuse(ctx, S), w)


def test_candidates_follow_max_dist(ctx):
    S = dict(SCENE, max_dist=25)
    cand = R.candidates(len(S["mp_index"]), S["views"], S["n_kept"], S["kept_entry"], S["top_idx"], S["top_dist"], 25)
    assert 0 < (cand >= 0).sum() < (SCENE["cand"] >= 0).sum()
    assert_same(fuse(ctx, S), R.fuse_tables(S["T"], S["mp_index"], S["views"], cand, -1))


def test_replace_pairs_with_chains_and_every_outcome(ctx):
    rng = np.random.default_rng(3)
    pairs = R.make_pairs(rng, SCENE["T"], 60)
    w = R.replace_pairs_tables(SCENE["T"], pairs)
    assert set(w["outcome"].tolist()) == {0, 1, 2} and set(w["erased_into"].tolist()) & set(w["erased_rows"].tolist())
    t = mi355slam.KeyframeTable(ctx, SCENE["T"]["kf_mp"])
    got = t.replace_pairs(SCENE["T"], pairs)
    assert R.same(got, w, R.TABLE_KEYS + ("outcome", "erased_rows", "erased_into")) == [] and got["n_erased"] == len(w["erased_rows"])
    t.kf_mp.free()
    T = {k: v for k, v in SCENE["T"].items() if k not in ("mp_track", "track_row", "track_base")}                # without tracks, without lists
    t = mi355slam.KeyframeTable(ctx, T["kf_mp"])
    got = t.replace_pairs(T, pairs, want=())
    assert R.same(got, R.replace_pairs_tables(T, pairs), R.TABLE_KEYS + ("outcome",)) == [] and "erased_rows" not in got
    assert t.replace_pairs(got, np.zeros((0, 2), np.int32))["n_erased"] == 0
    t.kf_mp.free()


def test_replace_pairs_turns_a_dead_row_away_untouched(ctx):
    dead = int(np.argmin(SCENE["T"]["mp_live"]))
    alive = np.nonzero(SCENE["T"]["mp_live"])[0]
    pairs = np.array([[alive[0], alive[1]], [alive[2], dead]], np.int32)
    t = mi355slam.KeyframeTable(ctx, SCENE["T"]["kf_mp"])
    with pytest.raises(mi355slam.MsError, match="1 listed rows are not live"):
        t.replace_pairs(SCENE["T"], pairs)
    assert R.same(t._fuse_last, SCENE["T"], R.TABLE_KEYS) == []
    t.kf_mp.free()


def test_the_whole_deduplicate_chain_on_real_geometry(ctx):
    """ms_project_gate -> ms_projection_topk -> ms_map_fuse with the lists staying on the device, direction 1 re-gated after every early stop,
    then ms_map_point_union and direction 2, against replaceDuplication per keyframe fed by the gate and score restatements."""
    S = R.make_geometry_scene()
    w = R.deduplicate_sequential(S)
    assert w["near"] == 0 and w["changes"] >= 1
    t = S["table"]
    table = mi355slam.MapPointTable(ctx, t["pos"], t["norm"], t["min_dist"], t["max_dist"], t["desc"])
    kfs = {s: mi355slam.ProjectionKeyframe(ctx, k["x"], k["y"], k["desc"], k["octave"]) for s, k in S["kfs"].items()}
    kt = mi355slam.KeyframeTable(ctx, S["T"]["kf_mp"])
    got = kt.deduplicate(table, kfs, S["views_of"], S["T"], S["current"], S["adjacent"], S["margin"], S["sf"], S["scale_factor"])
    assert R.same(got, w, R.TABLE_KEYS + ("erased_rows", "erased_into")) == []
    # a batch gates the list as it was at its start: a row that an earlier view of the batch erased is still an entry of the later ones and
    # ends as code 1 there, where the reference's list no longer holds it.  Every other code counts the same entries.
    keep = [0, 2, 3, 4, 5, 6, 7]
    assert np.array_equal(got["counts"][keep], w["counts"][keep]) and got["counts"][1] >= w["counts"][1]
    assert got["regates"] >= 1                               # the walk stopped early at least once and the rest was gated again
    kt.kf_mp.free()


def test_mirror_smoke_on_the_device():
    import test_map_fuse_abi
    out = subprocess.check_output([test_map_fuse_abi.build_smoke(), "--gpu"], text=True)
    for line in ("deduplicateMapPoints ok", "searchAndDeduplicate ok", "mergeMatchedMapPoints ok"):
        assert line in out, out
