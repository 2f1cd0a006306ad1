"""The extractor's one device block (orb_geom.h: ORB_BLOCK_*) behaves like the separate allocations it replaces: every per-frame array is reached
at the right offset for every frame of a batch, the arrays of two extractors and of an extractor made after another was destroyed do not meet, and
the valid mask -- the one allocation left outside the block -- comes and goes.  Frames are 160 x 120 at 3 levels of factor 1.2 (the last level is
111 x 83) unless a case says otherwise; every comparison is exact, against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, LEVELS, KPTS = 160, 120, 3, 300
KW = dict(levels=LEVELS, scale_factor=1.2, max_kpts=KPTS)


def _same(got, want):
    assert len(got["x"]) == len(want["x"])                                               # the count
    for k in ("x", "y", "angle"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k      # float32 bit patterns
    assert np.array_equal(got["octave"], want["octave"])
    assert np.array_equal(got["track_id"], want["track_id"])
    assert np.array_equal(got["desc"], want["desc"])


@pytest.fixture(scope="module")
def scene(oracle):
    """Three frames and what the oracle makes of each, computed once."""
    frames = np.stack([oracle.synth_frame(W, H, 700 + i, 3 * i, i) for i in (0, 1, 0)])       # frame 2 = frame 0
    want = [oracle.orb_extract(oracle.cfg(**KW), f) for f in frames]
    assert all(len(w["x"]) > 50 for w in want) and (want[0]["octave"] == LEVELS - 1).any()
    assert not np.array_equal(want[0]["desc"][:20], want[1]["desc"][:20])
    return frames, want


def test_batch_position(scene, ctx):
    """The same frame alone, and as frame 0 and frame 2 of a batch of three."""
    import mi355slam
    frames, want = scene
    one = mi355slam.OrbExtractor(ctx, W, H, max_batch=1, **KW)
    three = mi355slam.OrbExtractor(ctx, W, H, max_batch=3, **KW)
    one.extract(frames[:1])
    three.extract(frames)
    _same(one.download(0), want[0])
    for f in range(3):
        _same(three.download(f), want[f])


def test_tracks(scene, oracle, ctx):
    """No room for tracks (the track arrays still have an element), and room for five with three given."""
    import mi355slam
    frames, want = scene
    ex = mi355slam.OrbExtractor(ctx, W, H, max_tracks=0, max_batch=2, **KW)
    assert ex.capacity == KPTS
    ex.extract(frames[:2])
    _same(ex.download(0), want[0]); _same(ex.download(1), want[1])
    tracks = [[(40.5, 30.25), (100.0, 90.0), (5.0, 5.0)], [(80.0, 60.0), (120.25, 33.5), (70.0, 99.0)]]      # (5, 5) lies inside the 19 px border
    ids = [[11, 12, 13], [21, 22, 23]]
    ex = mi355slam.OrbExtractor(ctx, W, H, max_tracks=5, max_batch=2, **KW)
    assert ex.capacity == KPTS + 5
    ex.extract(frames[:2], track_xy=tracks, track_id=ids)
    for f in range(2):
        w = oracle.orb_extract(oracle.cfg(**KW), frames[f], track_xy=np.asarray(tracks[f], np.float32), track_id=ids[f])
        assert (w["track_id"] >= 0).sum() == (2, 3)[f]
        _same(ex.download(f), w)


def test_quota_overflow(oracle, ctx):
    """15 levels / 160 keypoints at factor 1.2: the quotas add up to 161, so the per-frame stride of the detection and output arrays is 161
    (tests/golden/orb_geom_cases.txt holds the same configuration); 560 x 520 keeps the last level at 44 x 41."""
    import mi355slam
    def multiscale(r, w, h, blocks):      # random blocks of three sizes: corners on every level
        img = np.zeros((h, w), np.int64) + 20
        for s, amp in zip(blocks, (110, 70, 40)):
            img += np.kron(r.integers(0, 2, (h // s + 1, w // s + 1)), np.ones((s, s), np.int64))[:h, :w] * amp
        return np.clip(img + r.integers(0, 12, (h, w)), 0, 255).astype(np.uint8)
    r = np.random.default_rng(0)
    frames = np.stack([multiscale(r, 560, 520, (192, 48, 16)) for _ in range(2)])
    ex = mi355slam.OrbExtractor(ctx, 560, 520, levels=15, scale_factor=1.2, max_kpts=160, max_batch=2)
    assert ex.capacity == 161 and ex.level_size(14) == (44, 41)
    ex.extract(frames)
    for f in range(2):
        w = oracle.orb_extract(oracle.cfg(levels=15, scale_factor=1.2, max_kpts=160), frames[f])
        assert len(w["x"]) > 140
        _same(ex.download(f), w)
    assert (w["octave"] >= 12).any()
    # 8 levels / 7 keypoints (also in the record): quotas 2 1 1 1 1 1 1 0 = 8, and both frames fill all eight, so level 6 of frame 0 sits in slot 7 --
    # with a stride of max_kpts that is frame 1's slot 0
    r = np.random.default_rng(9)
    frames = np.stack([multiscale(r, 240, 200, (64, 24, 8)) for _ in range(2)])
    ex = mi355slam.OrbExtractor(ctx, 240, 200, levels=8, scale_factor=1.2, max_kpts=7, max_tracks=3, max_batch=2)
    assert ex.capacity == 8 + 3
    ex.extract(frames)
    for f in range(2):
        w = oracle.orb_extract(oracle.cfg(levels=8, scale_factor=1.2, max_kpts=7), frames[f])
        assert len(w["x"]) == 8 and (w["octave"] == 6).any()
        _same(ex.download(f), w)


def test_two_extractors_at_once(scene, oracle, ctx):
    """Two extractors of different configurations alive on one context, their calls interleaved; then one is destroyed and the other goes on."""
    import mi355slam
    frames, want = scene
    kw_b = dict(levels=2, scale_factor=1.5, max_kpts=500, fast_threshold=12, max_tracks=2)
    other = np.stack([oracle.synth_frame(200, 136, 900 + i) for i in range(2)])
    want_b = [oracle.orb_extract(oracle.cfg(levels=2, scale_factor=1.5, max_kpts=500, fast_threshold=12), f) for f in other]
    assert all(len(w["x"]) > 50 for w in want_b)
    a = mi355slam.OrbExtractor(ctx, W, H, max_batch=3, **KW)
    b = mi355slam.OrbExtractor(ctx, 200, 136, max_batch=2, **kw_b)
    a.extract(frames)
    b.extract(other)
    got_a = [a.download(f) for f in range(3)]
    got_b = [b.download(f) for f in range(2)]
    for f in range(3): _same(got_a[f], want[f])
    for f in range(2): _same(got_b[f], want_b[f])
    a.close()
    b.extract(other[::-1].copy())
    _same(b.download(0), want_b[1]); _same(b.download(1), want_b[0])


def test_valid_mask_set_and_cleared(scene, oracle, ctx):
    import mi355slam
    frames, want = scene
    mask = np.ones((H, W), np.uint8)
    mask[:, :50] = 0
    mask[90:, :] = 0
    masked = oracle.orb_extract(oracle.cfg(**KW), frames[0], valid_mask=mask)
    assert 10 < len(masked["x"]) < len(want[0]["x"])
    ex = mi355slam.OrbExtractor(ctx, W, H, max_batch=1, **KW)
    ex.extract(frames[:1]); _same(ex.download(0), want[0])
    ex.set_valid_mask(mask)
    ex.extract(frames[:1]); _same(ex.download(0), masked)
    ex.set_valid_mask(None)
    ex.extract(frames[:1]); _same(ex.download(0), want[0])


def test_downloads_from_the_last_frame(scene, oracle, ctx):
    """The blurred plane (k_blur on demand) and the detections of the last level of the last frame of a batch: the far end of the slab and of the
    detection arrays."""
    import mi355slam
    frames, _ = scene
    ex = mi355slam.OrbExtractor(ctx, W, H, max_batch=3, **KW)
    ex.extract(frames)
    quotas = oracle.level_quotas(LEVELS, 1.2, KPTS)
    for f in (2, 1):
        levels, blurs = oracle.build_pyramid(oracle.cfg(**KW), frames[f])
        l = LEVELS - 1
        assert ex.level_size(l) == (111, 83) == (levels[l].shape[1], levels[l].shape[0])
        assert np.array_equal(ex.download_level(f, l, blurred=True), blurs[l])
        assert np.array_equal(ex.download_level(f, l, blurred=False), levels[l])
        xs, ys, sc = oracle.detect_level(levels[l], 20, int(quotas[l]))
        gx, gy, gs = ex.download_detections(f, l)
        assert len(xs) > 5 and np.array_equal(gx, xs) and np.array_equal(gy, ys) and np.array_equal(gs, sc)


def test_create_again_with_a_larger_batch(scene, ctx):
    import mi355slam
    frames, want = scene
    ex = mi355slam.OrbExtractor(ctx, W, H, max_batch=1, **KW)
    ex.extract(frames[1:2])
    first = ex.download(0)
    ex.close()
    ex = mi355slam.OrbExtractor(ctx, W, H, max_batch=3, **KW)
    ex.extract(frames)
    _same(first, want[1])
    for f in range(3): _same(ex.download(f), want[f])
    _same(ex.download(1), first)
