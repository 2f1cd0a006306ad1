"""k_fast's raised threshold on the device: within a batch a tile skips corners that cannot reach their level's quota, and the
extractor's full output stays what the oracle computes, frame by frame, bit for bit.

The batch is 256 frames of 512 x 256 with 4 levels and max_kpts = 100: 62 tiles per frame, ~16 k workgroups of which about a thousand are
resident, so the tiles of a frame do run at different times and the pruning is live -- asserted through ms_orb_last_candidate_counts.  The 256
frames are 16 different synthetic frames (4 sequences of 4), each at 16 places of the batch: the oracle and the unpruned candidate counts
(tests/fast_prune_ref.py on the oracle's pyramid) are computed once per different frame and shared by the tests."""
import numpy as np
import pytest

import fast_prune_ref as fp

pytestmark = pytest.mark.gpu

W, H, LEVELS, KP, THR, DISTINCT, BATCH = 512, 256, 4, 100, 20, 16, 256
_memo = {}


def _distinct():
    import synth
    if "frames" not in _memo:
        _memo["frames"] = synth.synth_sequences(DISTINCT, W, H, 1000, n_seq=4)
    return _memo["frames"]


def _batch(n=BATCH):
    return np.ascontiguousarray(_distinct()[np.arange(n) % DISTINCT])


def _want(oracle, key, imgs, mask=None, **kw):
    """The oracle's output for every frame of `imgs`, once per key."""
    if key not in _memo:
        ocfg = oracle.cfg(levels=kw.get("levels", LEVELS), scale_factor=1.2, max_kpts=kw.get("max_kpts", KP), fast_threshold=THR, min_distance=kw.get("min_distance", 0.0))
        _memo[key] = [oracle.orb_extract(ocfg, img, valid_mask=mask) for img in imgs]
    return _memo[key]


def _unpruned(oracle, key, imgs, levels=LEVELS):
    """NMS maxima above the threshold per (frame, level): what a detector that prunes nothing hands to the selection."""
    if key not in _memo:
        ocfg = oracle.cfg(levels=levels, scale_factor=1.2, max_kpts=KP, fast_threshold=THR)
        _memo[key] = np.array([[len(fp.nms_keys(fp.score_map(l), THR)) for l in oracle.build_pyramid(ocfg, img)[0]] for img in imgs])
    return _memo[key]


def _same(got, want, what):
    assert len(got["x"]) == len(want["x"]), what
    for k in ("x", "y", "angle"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k)
    assert np.array_equal(got["octave"], want["octave"]) and np.array_equal(got["desc"], want["desc"]), what


def _check_frames(ex, want, n, what):
    for f in range(n):
        _same(ex.download(f), want[f % len(want)], "%s frame %d" % (what, f))


@pytest.fixture(scope="module")
def big(ctx):
    import mi355slam
    ex = mi355slam.OrbExtractor(ctx, W, H, levels=LEVELS, scale_factor=1.2, max_kpts=KP, fast_threshold=THR, max_batch=BATCH)
    dev = ctx.upload(_batch())
    yield ex, dev
    ex.close()
    dev.free()


def test_batch_is_exact_and_prunes(oracle, ctx, big):
    ex, dev = big
    want, full = _want(oracle, "plain", _distinct()), _unpruned(oracle, "full", _distinct())
    assert min(len(k["x"]) for k in want) > 50
    ex.extract(dev, n_frames=BATCH, frame_stride=W * H, row_stride=W)
    _check_frames(ex, want, BATCH, "batch")
    counts = ex.last_candidate_counts()
    ref = full[np.arange(BATCH) % DISTINCT]
    print("candidates: %d of %d unpruned" % (counts.sum(), ref.sum()))
    assert counts.shape == ref.shape and (counts <= ref).all() and (counts > 0).all()
    assert counts.sum() < ref.sum()                                        # the pruning is live under this test
    # a one-frame call on the same extractor: all of its tiles start together, nothing is known, nothing is pruned
    ex.extract(dev, n_frames=1, frame_stride=W * H, row_stride=W)
    _same(ex.download(0), want[0], "single frame")
    assert np.array_equal(ex.last_candidate_counts(), full[:1])


def test_fewer_frames_than_max_batch(oracle, ctx, big):
    ex, dev = big
    want, full = _want(oracle, "plain", _distinct()), _unpruned(oracle, "full", _distinct())
    n = 100
    ex.extract(dev, n_frames=n, frame_stride=W * H, row_stride=W)
    _check_frames(ex, want, n, "100 of 256")
    counts = ex.last_candidate_counts()
    assert counts.shape == (n, LEVELS) and (counts <= full[np.arange(n) % DISTINCT]).all()


def test_host_frames_in_four_pieces(oracle, ctx, big):
    """Host frames of a batch go in as four pieces, each with its own launches on offset pointers: the score bins follow the frame offset."""
    ex, _ = big
    want, full = _want(oracle, "plain", _distinct()), _unpruned(oracle, "full", _distinct())
    ex.extract(_batch())
    _check_frames(ex, want, BATCH, "host batch")
    counts = ex.last_candidate_counts()
    ref = full[np.arange(BATCH) % DISTINCT]
    assert (counts <= ref).all() and (counts > 0).all() and counts.sum() < ref.sum()


def _mask():
    rng = np.random.default_rng(11)
    return (rng.random((H // 32, W // 32)) < 0.7).astype(np.uint8).repeat(32, 0).repeat(32, 1)


@pytest.mark.parametrize("case", ["min_distance", "valid_mask", "both"])
def test_minimum_distance_and_valid_mask(oracle, ctx, case):
    """With a minimum distance the selection looks at 4 x quota candidates, and the bound counts that many; the camera mask acts after the selection.  Each
    on its own, so that a failure names its cause, and both together."""
    import mi355slam
    md = 0.0 if case == "valid_mask" else 12.0
    mask = None if case == "min_distance" else _mask()
    assert oracle.level_min_dist(12.0, W, H) >= 2
    want = _want(oracle, ("variant", case), _distinct(), mask=mask, min_distance=md)
    loose = _want(oracle, "plain", _distinct())
    assert any(len(a["x"]) != len(b["x"]) or not np.array_equal(a["x"], b["x"]) for a, b in zip(want, loose))       # the variant does change the output
    full = _unpruned(oracle, "full", _distinct())
    ex = mi355slam.OrbExtractor(ctx, W, H, levels=LEVELS, scale_factor=1.2, max_kpts=KP, fast_threshold=THR, max_batch=BATCH, min_distance=md)
    if mask is not None:
        ex.set_valid_mask(mask)
    dev = ctx.upload(_batch())
    ex.extract(dev, n_frames=BATCH, frame_stride=W * H, row_stride=W)
    _check_frames(ex, want, BATCH, case)
    counts = ex.last_candidate_counts()
    ref = full[np.arange(BATCH) % DISTINCT]
    print("%s: %d candidates of %d unpruned" % (case, counts.sum(), ref.sum()))
    assert (counts <= ref).all() and (counts > 0).all() and counts.sum() < ref.sum()
    if case == "min_distance":                                             # the bound counts 4 x quota: no level may have fewer candidates than the selection looks at
        quotas = oracle.level_quotas(LEVELS, 1.2, KP)
        K = np.array([fp.select_count(int(quotas[l]), 2) for l in range(LEVELS)])
        assert (counts >= np.minimum(K, ref)).all()
    ex.close()
    dev.free()


@pytest.mark.parametrize("n_strong", [0, 100])
def test_equal_score_stamps(oracle, ctx, n_strong):
    """1800 corners of score exactly 60 and a quota of 100: the bound must stop at 59, so every tile of every frame still finds all of its stamps.  With
    exactly 100 corners of score 90 added the bound may reach 89 once all of them are known -- and they are all found, in every frame."""
    import mi355slam
    w, h, n_frames, K = 640, 480, 64, 100
    img, n = fp.stamp_frame(w, h, n_strong=n_strong)
    want = _want(oracle, ("stamps", n_strong), [img], levels=1, max_kpts=K)
    assert len(want[0]["x"]) == K
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=1, scale_factor=1.2, max_kpts=K, fast_threshold=THR, max_batch=n_frames)
    dev = ctx.upload(np.ascontiguousarray(np.broadcast_to(img, (n_frames, h, w))))
    ex.extract(dev, n_frames=n_frames, frame_stride=w * h, row_stride=w)
    _check_frames(ex, want, n_frames, "stamps")
    counts = ex.last_candidate_counts()
    if n_strong == 0:
        assert (counts == n).all()
    else:
        assert (counts >= K).all() and (counts <= n + K).all()
    ex.close()
    dev.free()


def test_nothing_is_carried_between_calls(oracle, ctx):
    """Dense frames, then dim sparse ones whose corners are all weaker than the cut of the dense ones, then dense again: score bins left over from the
    first call would raise the second call's threshold above everything it has."""
    import mi355slam
    import synth
    n = 128
    dense = _distinct()
    dim = np.ascontiguousarray(synth.synth_sequences(4, W, H, 2000, n_seq=4, sparse=True) >> 1)
    want_dense, want_dim = _want(oracle, "plain", dense), _want(oracle, "dim", dim)
    # the premise, for every dense frame, every dim frame and every level: more than the level's quota of dense corners beat every dim corner of that
    # level, so the bound the first call ends with lies above everything the second call has
    ocfg = oracle.cfg(levels=LEVELS, scale_factor=1.2, max_kpts=KP, fast_threshold=THR)
    quotas = oracle.level_quotas(LEVELS, 1.2, KP)
    dim_maps = [[fp.score_map(l) for l in oracle.build_pyramid(ocfg, f)[0]] for f in dim]
    for l in range(LEVELS):
        strongest_dim = max(int(m[l].max()) for m in dim_maps)
        for f in dense:
            sc = np.sort(fp.key_scores(fp.nms_keys(fp.score_map(oracle.build_pyramid(ocfg, f)[0][l]), THR)))[::-1]
            assert strongest_dim < int(sc[int(quotas[l])]), (l, strongest_dim)
    assert 0 < min(len(k["x"]) for k in want_dim)
    ex = mi355slam.OrbExtractor(ctx, W, H, levels=LEVELS, scale_factor=1.2, max_kpts=KP, fast_threshold=THR, max_batch=n)
    d_dense, d_dim = ctx.upload(_batch(n)), ctx.upload(np.ascontiguousarray(dim[np.arange(n) % 4]))
    for dev, want, what in ((d_dense, want_dense, "dense"), (d_dim, want_dim, "dim"), (d_dense, want_dense, "dense again")):
        ex.extract(dev, n_frames=n, frame_stride=W * H, row_stride=W)
        _check_frames(ex, want, n, what)
    ex.close()
    d_dense.free()
    d_dim.free()
