"""CPU: the raised threshold of k_fast (tests/fast_prune_ref.py) never changes what the selection sees.

For every case the K smallest keys of the pruned candidate list equal those of the unpruned one exactly, over random tile orders and 1 .. 64 tiles
in flight.  The frames are the bench's synthetic ones (dense and sparse) at 320 x 240 and 512 x 256 with 4 and 8 pyramid levels, max_kpts 100 (the
quota cuts far above the threshold) and 2000 (the small levels hold fewer candidates than their quota: nothing may be pruned there), without and
with a minimum distance (K = 4 quota), and two constructed frames: identical corner stamps -- all scores equal, quota below their number, the
bound must stay below them -- and the same with exactly K stronger corners."""
import numpy as np
import pytest

import fast_prune_ref as fp

THR = 20
_pyr = {}


def _pyramid_scores(oracle, w, h, sparse):
    """Score maps of the 8-level pyramid of one synthetic frame (levels 0 .. 3 of it are the 4-level pyramid: the sizes depend on the scale factor alone)."""
    import synth
    key = (w, h, sparse)
    if key not in _pyr:
        img = synth.synth_frame(w, h, 1000, 2, 1, sparse=sparse)
        levels, _ = oracle.build_pyramid(oracle.cfg(levels=8), img)
        _pyr[key] = [fp.score_map(l) for l in levels]
    return _pyr[key]


def test_numpy_score_map_equals_the_oracles(oracle):
    import synth
    rng = np.random.default_rng(3)
    for img in (synth.synth_frame(97, 61, 7), rng.integers(0, 256, (40, 53), dtype=np.uint8), fp.stamp_frame(90, 70, 2)[0]):
        assert np.array_equal(fp.score_map(img), oracle.fast_score_map(img, 0))


def test_bound_is_the_largest_score_k_candidates_exceed():
    h = np.zeros(256, np.int64)
    assert fp.bound(h, 20, 5) == 20
    h[60] = 7
    assert fp.bound(h, 20, 5) == 59 and fp.bound(h, 20, 7) == 59 and fp.bound(h, 20, 8) == 20       # ties: only STRICTLY greater scores count
    h[90] = 5
    assert fp.bound(h, 20, 5) == 89 and fp.bound(h, 20, 6) == 59 and fp.bound(h, 20, 12) == 59 and fp.bound(h, 20, 13) == 20
    h[255] = 5
    assert fp.bound(h, 20, 5) == 254
    assert fp.bound(h, 20, 0) == 20 and fp.bound(h, 100, 6) == 100


def _check_level(scores, K, rng, tile=(64, 30)):
    h, w = scores.shape
    full = fp.nms_keys(scores, THR)
    want = fp.select(full, K)
    tiles = fp.tiles_of(w, h, *tile)
    assert np.array_equal(np.sort(np.concatenate([fp.nms_keys(scores, THR, *t) for t in tiles])), np.sort(full))     # the tiling itself loses nothing
    pruned_any = False
    for in_flight in (1, 2, 4, 7, 64):
        order = rng.permutation(len(tiles))
        got, used = fp.pruned_keys(scores, THR, K, tiles, order, in_flight)
        assert np.array_equal(fp.select(got, K), want), (w, h, K, in_flight)
        assert len(got) <= len(full) and np.isin(got, full).all()
        pruned_any |= len(got) < len(full)
    return len(full), pruned_any


@pytest.mark.parametrize("min_distance", [0.0, 12.0])
@pytest.mark.parametrize("max_kpts", [100, 2000])
@pytest.mark.parametrize("levels", [4, 8])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("w,h", [(320, 240), (512, 256)])
def test_selection_is_unchanged(oracle, w, h, sparse, levels, max_kpts, min_distance):
    maps = _pyramid_scores(oracle, w, h, sparse)[:levels]
    quotas = oracle.level_quotas(levels, 1.2, max_kpts)
    rng = np.random.default_rng(w + levels + max_kpts)
    short = pruned = 0
    for l, s in enumerate(maps):
        K = fp.select_count(int(quotas[l]), oracle.level_min_dist(min_distance, s.shape[1], s.shape[0]))
        n, p = _check_level(s, K, rng)
        short += n < K
        pruned += p
        assert not (n <= K and p)                                       # fewer candidates than the selection looks at: all of them are needed
    if max_kpts == 2000 and min_distance > 0 and sparse:
        assert short > 0                                                # the case max_kpts = 2000 is there for (the sparse frames have 600 .. 800 candidates a level)
    if max_kpts == 100 and not sparse and min_distance == 0.0:
        assert pruned > 0                                               # and here the rule does remove work


def test_equal_scores_are_never_pruned_away(oracle):
    """All corners score 60 and the quota is below their number: the bound stops at 59 and every later tile still finds its stamps."""
    img, n = fp.stamp_frame(320, 240)
    s = fp.score_map(img)
    full = fp.nms_keys(s, THR)
    assert len(full) == n and (fp.key_scores(full) == 60).all()
    tiles = fp.tiles_of(320, 240, 64, 30)
    rng = np.random.default_rng(1)
    for K in (1, 100, n - 1, n, n + 1):
        for in_flight in (1, 3, 64):
            got, used = fp.pruned_keys(s, THR, K, tiles, rng.permutation(len(tiles)), in_flight)
            assert max(used) <= 59 and (K > 100 or in_flight == 64 or max(used) == 59)       # (with K <= 100 of 368 the bound does get there)
            assert np.array_equal(np.sort(got), np.sort(full))          # nothing is lost at all: every tile works below the stamps' score
            assert np.array_equal(fp.select(got, K), fp.select(full, K))


def test_exactly_k_stronger_corners(oracle):
    """The same frame with exactly K corners of score 90: once all K are known the bound is 89 and the stamps go, the K stay; one fewer and it must not."""
    K = 100
    img, n = fp.stamp_frame(320, 240, n_strong=K)
    s = fp.score_map(img)
    full = fp.nms_keys(s, THR)
    sc = fp.key_scores(full)
    assert (sc == 90).sum() == K and (sc == 60).sum() == n and len(full) == n + K
    tiles = fp.tiles_of(320, 240, 64, 30)
    rng = np.random.default_rng(2)
    for k_sel, top in ((K, 89), (K + 1, 59), (K - 1, 89)):
        for in_flight in (1, 3, 64):
            got, used = fp.pruned_keys(s, THR, k_sel, tiles, rng.permutation(len(tiles)), in_flight)
            assert max(used) <= top
            assert np.array_equal(fp.select(got, k_sel), fp.select(full, k_sel))
            assert (fp.key_scores(got) == 90).sum() == K                # the strong ones are found whatever the bound
