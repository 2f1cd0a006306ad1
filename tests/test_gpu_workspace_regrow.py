"""The grow-only workspaces of the map-side entry points (ms_grow, one per feature on the context) on a context of its own, so that they
start empty: a small call, a call that outgrows the small call's device block, and the small call again.  Every answer is compared with
the restatement as the feature's own GPU test compares it; ms_debug_host_allocs rises across the large call (the block was freed and
allocated again) and not at all across the repeated small one.  Every call is a valid call."""
import ctypes as C

import numpy as np
import pytest

import covis_ref
import mi355slam
import test_gpu_covis as TC
import test_gpu_triangulate as TT
import triangulate_ref

pytestmark = pytest.mark.gpu


@pytest.fixture()
def own_ctx():
    c = mi355slam.Context(0)
    yield c
    c.close()


def _allocs():
    f = mi355slam.lib().ms_debug_host_allocs
    f.restype = C.c_longlong
    return f()


def test_covisibility_block_regrows_once(own_ctx):
    rng = np.random.default_rng(41)
    calls = []
    # 1 query: queries, neighbour counts and a 12-byte bitmap, 256 bytes each -> the first device block is 4096 bytes;
    # 64 queries on 2048 map points: the bitmaps alone are 4 * 64 * (64 + 1) = 16640 bytes
    for n_kf, stride, n_mp, n_q in ((5, 40, 33, 1), (9, 40, 2048, 64)):
        kf_mp, fl = TC.random_table(rng, n_kf, stride, n_mp)
        queries = TC.random_queries(rng, n_kf, n_q)
        calls.append((mi355slam.KeyframeTable(own_ctx, kf_mp), queries, n_mp, fl, covis_ref.covisibility(kf_mp, n_mp, fl, queries)))
    rose = []
    for table, queries, n_mp, fl, wanted in (calls[0], calls[1], calls[0]):
        before = _allocs()
        got = table.covisibility(queries, n_mp, fl)
        rose.append(_allocs() - before)
        TC.assert_same_covis(got, wanted)
    print("allocations per call:", rose)
    assert rose[0] >= 1 and rose[1] >= 1 and rose[2] == 0
    for table, *_ in calls:
        table.kf_mp.free()


def test_triangulate_block_regrows_once(own_ctx):
    want = triangulate_ref.fixture(triangulate_ref.TME, True)
    dev = TT.Device(own_ctx)
    small, large = range(4), range(65)                       # 65 rows: sixteen times the rows, and their rays alone outgrow the first block
    rose = []
    for entries in (small, large, small):
        prob = triangulate_ref.sub_problem(want["prob"], entries)
        before = _allocs()
        got, pos, flags = dev.run(prob, want["settings"], triangulate_ref.TME)
        rose.append(_allocs() - before)
        TT.assert_matches(got, pos, flags, want, entries)
    print("allocations per call:", rose)
    assert rose[0] >= 1 and rose[1] >= 1 and rose[2] == 0
    del dev                                                  # its device buffers go before the context does
