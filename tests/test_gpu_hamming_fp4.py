"""k_hamming_mfma on FP4 operands (four v_mfma_scale_f32_32x32x64_f8f6f4 per 32 x 32 tile): the matrix-core search against the CPU oracle and
against the popcount kernel (set_hamming_path(1)), equal array by array.  Nothing here has a tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NT = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300]      # tile (32), stage (128 and 256) and workgroup (256 queries) edges
NQ = [1, 63, 64, 65, 255, 256, 257]


def _rand(rng, n):
    return rng.integers(0, 2**32, (n, 8), dtype=np.uint64).astype(np.uint32)


def _both_paths(ctx, q, t):
    """(matrix-core result, popcount result) of one search."""
    import mi355slam
    got = mi355slam.hamming_best2(ctx, q, t)
    ctx.set_hamming_path(1)
    try:
        pop = mi355slam.hamming_best2(ctx, q, t)
    finally:
        ctx.set_hamming_path(0)
    return got, pop


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def pool():
    rng = np.random.default_rng(404)
    q, t = _rand(rng, max(NQ)), _rand(rng, max(NT))
    near = rng.permutation(max(NT))[:200]                       # some targets are noisy copies of queries, so best and second differ widely
    noise = np.packbits(rng.random((200, 256)) < 0.06, axis=1, bitorder="little").view(np.uint32)
    t[near] = q[near % max(NQ)] ^ noise
    q.setflags(write=False); t.setflags(write=False)
    return q, t


@pytest.mark.parametrize("nt", NT)
def test_sizes(oracle, ctx, pool, nt):
    for nq in NQ:
        q, t = pool[0][:nq], pool[1][:nt]
        got, pop = _both_paths(ctx, q, t)
        want = oracle.hamming_best2(q, t)
        assert _same(got, want), (nq, nt)
        assert _same(got, pop), (nq, nt)


def test_one_hot_every_bit_position(oracle, ctx):
    """Query i and target i have only bit i set: distance 0 on the diagonal, 2 elsewhere.  A query bit and a target bit that
    do not share their k slot show here and nowhere else."""
    eye = np.zeros((256, 8), np.uint32)
    for i in range(256):
        eye[i, i >> 5] = np.uint32(1) << np.uint32(i & 31)
    got, pop = _both_paths(ctx, eye, eye)
    assert np.array_equal(got[0], np.arange(256, dtype=np.int32))
    assert (got[1] == 0).all() and (got[2] == 2).all()
    assert _same(got, pop) and _same(got, oracle.hamming_best2(eye, eye))
    # against a rolled target set the match must follow the bit, whatever row it sits in
    rolled = np.roll(eye, 37, axis=0)
    got, pop = _both_paths(ctx, eye, rolled)
    assert np.array_equal(got[0], (np.arange(256, dtype=np.int32) + 37) % 256) and (got[1] == 0).all() and (got[2] == 2).all()
    assert _same(got, pop)


def test_extremes(oracle, ctx):
    zero, ones = np.zeros((70, 8), np.uint32), np.full((70, 8), 0xFFFFFFFF, np.uint32)
    for q, t, d in [(zero, zero, 0), (ones, ones, 0), (zero, ones, 256), (ones, zero, 256)]:
        got, pop = _both_paths(ctx, q, t[:45])
        assert (got[0] == 0).all() and (got[1] == d).all() and (got[2] == d).all()
        assert _same(got, pop)
        want = oracle.hamming_best2(q, t[:45])
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        if d < 256:         # at distance 256 the reference's scan keeps no index (-1) while both device kernels name row 0, as test_gpu_match.py pins it
            assert np.array_equal(got[0], want[0])


def test_ties_lowest_index_wins(oracle, ctx):
    """Copies of one descriptor at two rows that differ in the register (low and high index bits), the lane half, the tile and the stage
    (for stages of 128 and of 256 targets): the lower row must win and second must equal best."""
    rng = np.random.default_rng(77)
    # a lane's rows of a tile are (reg & 3) + 8 * (reg >> 2) + 4 * (lane half); no row is used twice
    pairs = [(5, 6), (1, 9), (2, 4), (7, 39), (40, 100), (11, 139), (12, 268), (130, 261), (31, 32), (127, 128), (255, 256), (299, 298)]
    assert len({r for ab in pairs for r in ab}) == 2 * len(pairs)
    for flips in (0, 3):
        q, t = _rand(rng, len(pairs)), _rand(rng, 300)
        for k, (a, b) in enumerate(pairs):                           # every pair gets a query of its own, `flips` bits away from both copies
            c = q[k].copy()
            c[k % 8] ^= np.uint32((1 << flips) - 1)
            t[a] = c; t[b] = c
        got, pop = _both_paths(ctx, q, t)
        assert _same(got, oracle.hamming_best2(q, t)) and _same(got, pop)
        assert np.array_equal(got[0], np.array([min(ab) for ab in pairs], np.int32))
        assert (got[1] == flips).all() and (got[2] == flips).all()


def test_sets_ragged_counts(oracle, ctx):
    import mi355slam
    rng = np.random.default_rng(12)
    stride, counts = 300, np.array([300, 0, 129], np.int32)
    pool = _rand(rng, 3 * stride)
    pool[2 * stride:2 * stride + 100] = pool[:100] ^ np.uint32(5)   # set 2 holds near copies of set 0
    pq, pt = np.array([0, 0, 2, 1, 0, 2], np.int32), np.array([0, 2, 0, 0, 1, 2], np.int32)
    n = len(pq)
    dp, dc, dq, dt = ctx.upload(pool), ctx.upload(counts), ctx.upload(pq), ctx.upload(pt)
    out = []
    for path in (0, 1):
        obi, obd, osd = ctx.alloc(4 * n * stride), ctx.alloc(2 * n * stride), ctx.alloc(2 * n * stride)
        ctx.set_hamming_path(path)
        try:
            mi355slam.hamming_best2_sets(ctx, dp, stride, dc, dp, stride, dc, dq, dt, n, obi, obd, osd)
            ctx.sync()
        finally:
            ctx.set_hamming_path(0)
        out.append((obi.download(np.int32, (n, stride)), obd.download(np.uint16, (n, stride)), osd.download(np.uint16, (n, stride))))
    assert _same(out[0], out[1])
    bi, bd, sd = out[0]
    for k in range(n):
        a, b = pq[k], pt[k]
        m = counts[a]
        wi, wd, ws = oracle.hamming_best2(pool[a * stride:a * stride + m], pool[b * stride:b * stride + counts[b]])
        assert np.array_equal(bi[k, :m], wi) and np.array_equal(bd[k, :m], wd) and np.array_equal(sd[k, :m], ws), k
        assert (bi[k, m:] == -1).all() and (bd[k, m:] == 256).all() and (sd[k, m:] == 256).all(), k
    assert (bi[4] == -1).all() and (bd[4] == 256).all()             # a set matched against the empty one


def test_repeat_is_identical(ctx, pool):
    import mi355slam
    first = mi355slam.hamming_best2(ctx, pool[0], pool[1])
    again = mi355slam.hamming_best2(ctx, pool[0], pool[1])
    assert _same(first, again)
