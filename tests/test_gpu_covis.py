"""ms_covisibility and ms_map_point_union on the device against tests/covis_ref.py, their specification.  Integer work:
every comparison is exact equality.  Out-of-range entries here are n_mp and n_mp + 1 only (besides -1); the rest of the range is covered
on the host by tests/test_covis_ref.py and by the mirror's update() in tests/covis_smoke.cpp."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import covis_ref as R
import mi355slam

pytestmark = pytest.mark.gpu

N_KF, STRIDE, N_MP = 70, 100, 1003
KF_MP, FLAGS = R.make_scene()
WANT = {}                                                    # (min_covis, require, forced) -> the restatement, computed once


def want(min_covis, require, forced):
    key = (min_covis, require, forced)
    if key not in WANT:
        WANT[key] = R.covisibility(KF_MP, N_MP, FLAGS, R.scene_queries(N_KF, min_covis, require, forced))
    return WANT[key]


@pytest.fixture(scope="module")
def table(ctx):
    return mi355slam.KeyframeTable(ctx, KF_MP)


@pytest.fixture(scope="module")
def flags(ctx):
    return ctx.upload(FLAGS)


def assert_same_covis(got, wanted):
    count, neighbours, n_nb = got
    w_count, w_neighbours, w_n = wanted
    assert np.array_equal(n_nb, w_n)
    assert count.dtype == np.int32 and np.array_equal(count, w_count)
    for q in range(len(w_neighbours)):
        assert np.array_equal(neighbours[q], w_neighbours[q]), q


@pytest.mark.parametrize("forced", R.FORCED)
@pytest.mark.parametrize("require", R.REQUIRE)
def test_scene_all_queries_in_one_call(table, flags, require, forced):
    lengths = set()
    for min_covis in R.MIN_COVIS:
        got = table.covisibility(R.scene_queries(N_KF, min_covis, require, forced), N_MP, flags)
        assert_same_covis(got, want(min_covis, require, forced))
        lengths |= set(int(n) for n in got[2])
    assert max(lengths) >= 10 and (forced != "none" or 0 in lengths)


def test_count_output_is_optional(table, flags):
    queries = R.scene_queries(N_KF, 5, 1, "chain")
    count, neighbours, n_nb = table.covisibility(queries, N_MP, flags, want_count=False)
    assert count is None
    w = want(5, 1, "chain")
    assert np.array_equal(n_nb, w[2]) and all(np.array_equal(a, b) for a, b in zip(neighbours, w[1]))


def test_same_bits_alone_first_last_and_on_a_second_call(table, flags):
    probe = (31, 30, 32, 5, 1)
    others = [q for q in R.scene_queries(N_KF, 1, 0, "chain") if q[0] != 31]
    w_count, w_nb, _ = R.covisibility(KF_MP, N_MP, FLAGS, [probe])
    for queries, at in (([probe], 0), ([probe] + others, 0), (others + [probe], 69), (others + [probe], 69)):
        assert len(queries) in (1, 70)
        count, neighbours, n_nb = table.covisibility(queries, N_MP, flags)
        assert np.array_equal(count[at], w_count[0]) and np.array_equal(neighbours[at], w_nb[0]) and n_nb[at] == len(w_nb[0])


def test_small_call_after_a_large_one_sees_no_stale_marks(table, flags):
    big = R.scene_queries(N_KF, 1, 0, "none")
    assert_same_covis(table.covisibility(big, N_MP, flags), want(1, 0, "none"))
    small = [(50, -1, -1, 1, 0), (3, -1, 4, 5, 1)]          # positions 0 and 1 held slots 0 and 1 in the large call
    assert_same_covis(table.covisibility(small, N_MP, flags), R.covisibility(KF_MP, N_MP, FLAGS, small))


def random_table(rng, n_kf, stride, n_mp):
    """Entries drawn from -1, the valid rows and the two out-of-range values n_mp, n_mp + 1; rows may repeat within a slot."""
    kf_mp = rng.integers(-1, n_mp + 2, (n_kf, stride)).astype(np.int32)
    kf_mp[rng.random((n_kf, stride)) < 0.3] = -1
    return kf_mp, rng.integers(0, 4, max(n_mp, 1)).astype(np.uint8)[:n_mp]


def random_queries(rng, n_kf, n_q):
    return [(int(rng.integers(0, n_kf)), int(rng.integers(-1, n_kf)), int(rng.integers(-1, n_kf)), int(rng.integers(-1, 4)), int(rng.integers(0, 4)))
            for _ in range(n_q)]


# strides around the wave and the workgroup, and every stride at which the count kernel changes the number of registers per lane or
# between dwordx4 and dword loads; n_mp around the bitmap word; n_kf around the wave of the neighbour walk
SHAPES = ([(5, s, 1003) for s in (1, 63, 64, 65, 257, 1024, 1028, 2048, 2049, 4096, 4100, 8192)] +
          [(9, 40, m) for m in (1, 31, 32, 33, 1003, 0)] +
          [(k, 36, 300) for k in (1, 63, 64, 65, 130)])


@pytest.mark.parametrize("n_kf,stride,n_mp", SHAPES)
def test_shapes_where_lanes_and_words_run_out(ctx, n_kf, stride, n_mp):
    rng = np.random.default_rng(1000 * n_kf + stride + n_mp)
    kf_mp, fl = random_table(rng, n_kf, stride, n_mp)
    t = mi355slam.KeyframeTable(ctx, kf_mp)
    queries = random_queries(rng, n_kf, 7)
    got = t.covisibility(queries, n_mp, fl)
    assert_same_covis(got, R.covisibility(kf_mp, n_mp, fl, queries))
    if n_mp >= 31 and stride >= 36:
        assert got[0].max() >= 1
    lists = rng.integers(0, n_kf, 6).astype(np.int32)
    problems = [(0, 6, -1, 0), (1, 4, int(lists[0]), 1), (6, 0, -1, 0)]
    rows, owner, n_rows = t.map_point_union(lists, problems, n_mp, fl)
    w_rows, w_owner, w_n = R.map_point_union(kf_mp, n_mp, fl, lists, problems)
    assert np.array_equal(n_rows, w_n)
    for u in range(len(problems)):
        assert np.array_equal(rows[u], w_rows[u]) and np.array_equal(owner[u], w_owner[u]), u
    t.kf_mp.free()


def test_no_queries_and_no_problems(table, flags):
    count, neighbours, n_nb = table.covisibility([], N_MP, flags)
    assert count.shape == (0, N_KF) and neighbours == [] and len(n_nb) == 0
    rows, owner, n_rows = table.map_point_union([], [], N_MP, flags)
    assert rows == [] and owner == [] and len(n_rows) == 0


UNION_LIST = np.array([30, 31, 32, 33, 34, 35, 20, 13] + [44, 43, 42, 44, 41] + list(range(N_KF)), np.int32)
UNION_PROBLEMS = [(0, 8, 33, 2),             # a list with an exclude slot and require = 2; it holds the slot with out-of-range entries and the empty one
                  (13, N_KF, -1, 0),         # no filter: the whole map
                  (8, 5, -1, 0),             # descending slots with a repeated slot: owner is the list position
                  (8, 0, 31, 1)]             # an empty list


def assert_same_union(got, wanted):
    rows, owner, n_rows = got
    w_rows, w_owner, w_n = wanted
    assert np.array_equal(n_rows, w_n)
    for u in range(len(w_rows)):
        assert np.array_equal(rows[u], w_rows[u]) and np.array_equal(owner[u], w_owner[u]), u


def test_unions_four_problems_in_one_call(table, flags):
    wanted = R.map_point_union(KF_MP, N_MP, FLAGS, UNION_LIST, UNION_PROBLEMS)
    got = table.map_point_union(UNION_LIST, UNION_PROBLEMS, N_MP, flags)
    assert_same_union(got, wanted)
    assert_same_union(table.map_point_union(UNION_LIST, UNION_PROBLEMS, N_MP, flags), wanted)      # a second call: the same bits
    rows, owner, n_rows = got
    assert n_rows[3] == 0 and 0 < n_rows[0] < n_rows[1] and n_rows[1] > 900
    assert set(owner[2].tolist()) == {0, 1, 2, 4}            # positions in the list 44, 43, 42, 44, 41; position 3 repeats slot 44
    no_owner = table.map_point_union(UNION_LIST, UNION_PROBLEMS, N_MP, flags, want_owner=False)
    assert no_owner[1] is None and all(np.array_equal(a, b) for a, b in zip(no_owner[0], wanted[0]))
    # a one-problem call after the four-problem call: the marks of problem 0 are overwritten
    one = [(8, 5, -1, 0)]
    assert_same_union(table.map_point_union(UNION_LIST, one, N_MP, flags), R.map_point_union(KF_MP, N_MP, FLAGS, UNION_LIST, one))


def test_large_union_whose_offsets_scan_loops(ctx):
    n_mp, n_kf, stride = 76805, 8, 2048                     # 301 blocks of 256 rows: the offsets scan takes two rounds
    rng = np.random.default_rng(8)
    kf_mp = rng.integers(0, n_mp + 2, (n_kf, stride)).astype(np.int32)
    kf_mp[rng.random((n_kf, stride)) < 0.1] = -1
    kf_mp[0, :4] = (0, n_mp - 1, 255, 256)
    fl = rng.integers(0, 4, n_mp).astype(np.uint8)
    t = mi355slam.KeyframeTable(ctx, kf_mp)
    lists = np.array([7, 6, 5, 4, 3, 2, 1, 0, 5], np.int32)
    problems = [(0, 8, -1, 0), (0, 9, 4, 2)]
    wanted = R.map_point_union(kf_mp, n_mp, fl, lists, problems)
    got = t.map_point_union(lists, problems, n_mp, fl)
    assert_same_union(got, wanted)
    assert_same_union(t.map_point_union(lists, problems, n_mp, fl), wanted)
    assert got[2][0] > 12000 and got[0][0][0] == 0 and got[0][0][-1] == n_mp - 1
    t.kf_mp.free()


def test_update_of_one_slot(ctx):
    kf_mp = KF_MP.copy()
    t = mi355slam.KeyframeTable(ctx, kf_mp)
    kf_mp[13, :5] = (7, 8, 500, 501, 1002)
    kf_mp[40] = -1
    t.update(13, kf_mp[13, :5])
    t.update(40, [])
    assert np.array_equal(t.download(), kf_mp)
    queries = R.scene_queries(N_KF, 1, 0, "none")
    assert_same_covis(t.covisibility(queries, N_MP, None), R.covisibility(kf_mp, N_MP, None, queries))
    t.kf_mp.free()


def test_invalid_and_capacity_are_errors(table, flags):
    for queries in ([(N_KF, -1, -1, 1, 0)], [(0, N_KF, -1, 1, 0)], [(0, -1, -2, 1, 0)]):
        with pytest.raises(mi355slam.MsError, match="covisibility"):
            table.covisibility(queries, N_MP, flags)
    with pytest.raises(mi355slam.MsError, match="no mp_flags"):
        table.covisibility([(0, -1, -1, 1, 1)], N_MP, None)
    with pytest.raises(mi355slam.MsError, match="slice"):
        table.map_point_union(UNION_LIST, [(80, 10, -1, 0)], N_MP, flags)
    with pytest.raises(mi355slam.MsError, match="caps"):
        table.covisibility_device([(0, -1, -1, 1, 0)] * 4097, N_MP, flags, None, table.kf_mp)      # rejected before anything is written


def test_allocations_stay_flat(table, flags):
    allocs = mi355slam.lib().ms_debug_host_allocs
    allocs.restype = C.c_longlong
    table.covisibility(R.scene_queries(N_KF, 1, 0, "chain"), N_MP, flags, want_count=False)        # warm-up: the largest calls (counts in the workspace)
    table.map_point_union(UNION_LIST, UNION_PROBLEMS, N_MP, flags)
    before = allocs()
    for i in range(20):
        table.covisibility(R.scene_queries(N_KF, i % 7, i % 2, "chain")[:1 + 3 * i], N_MP, flags, want_count=i % 3 > 0)
        table.map_point_union(UNION_LIST, UNION_PROBLEMS[:1 + i % 4], N_MP, flags)
    assert allocs() == before


def test_mirror_smoke_on_the_device():
    import test_covis_abi
    out = subprocess.check_output([test_covis_abi.build_smoke(), "--gpu"], text=True)
    for line in ("getNeighbors ok", "computeAdjacentKeyframes ok", "localMapPoints ok", "update ok"):
        assert line in out, out
