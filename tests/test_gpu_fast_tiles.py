"""k_fast's three lane layouts (fast_tiles.h): the wide 248 x 30 tile and the tall 120 x 62 / 56 x 126 tiles of a level's narrow remainder
column, against the CPU oracle.

Single-level shapes sit on each layout's edges (r = (w - 3) mod 248 is the width the last column has to cover):
    252 x 150   r = 1     56 x 126 tiles, seam at y = 126
    307 x 150   r = 56    56 x 126 tiles at their widest
    308 x 150   r = 57    120 x 62 tiles at their narrowest, seams at y = 62 and 124
    371 x 80    r = 120   120 x 62 tiles at their widest
    372 x 80    r = 121   a wide tile beside a full column
    251 x 40    r = 0     one full column, no remainder
    300 x 63    h - 3 = 60: two tile rows, a third would hold no position
and 640 x 480 with 8 levels holds all three layouts in one extractor.  Frames are uniform noise (corners on every seam) and one structured
frame, in one batch (blockIdx.y).  A top-quota comparison can hide a missing or doubled seam corner when the quota cuts the list, so every
single-level shape has a parametrisation in which ALL of the oracle's corners fit the quota -- asserted on the oracle's side."""
import numpy as np
import pytest

SHAPES = [(252, 150), (307, 150), (308, 150), (371, 80), (372, 80), (251, 40), (300, 63)]
# (threshold, max_kpts).  The level quota of a 1-level extractor is max_kpts, at most 4096 (the selection's capacity).  Uniform noise is dense in
# corners: the oracle counts 4.6 k of them on 308 x 150 at threshold 7, 4.4 k at 20 and 3.5 k at 40.  So (7, 500) is the usual cut list, (20, 4096) is
# uncut on all shapes but the two largest, and (40, 4096) cuts nothing anywhere -- the case the quota condition asks for (the threshold is raised for it)
PARAMS = [(7, 500), (20, 4096), (40, 4096)]
UNCUT = (40, 4096)

_cache = {}


def _frames(oracle, w, h):
    key = (w, h)
    if key not in _cache:
        rng = np.random.default_rng(1000 * w + h)
        _cache[key] = np.stack([rng.integers(0, 256, (h, w), dtype=np.uint8), oracle.synth_frame(w, h, 77, 3, 1), rng.integers(0, 256, (h, w), dtype=np.uint8)])
    return _cache[key]


def _corner_count(oracle, img, thr):
    """All 3x3 strict maxima of the FAST score above the threshold (what k_fast hands to the selection, before any quota or border filter)."""
    s = oracle.fast_score_map(img, thr)
    c = s[1:-1, 1:-1]
    keep = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                keep &= c > s[1 + dy:s.shape[0] - 1 + dy, 1 + dx:s.shape[1] - 1 + dx]
    return int(keep.sum())


def _compare(oracle, ex, imgs, levels, max_kpts, thr):
    ocfg = oracle.cfg(levels=levels, scale_factor=1.2, max_kpts=max_kpts, fast_threshold=thr)
    quotas = oracle.level_quotas(levels, 1.2, max_kpts)
    for f in range(len(imgs)):
        pyr, _ = oracle.build_pyramid(ocfg, imgs[f])
        for l in range(levels):
            xs, ys, sc = oracle.detect_level(pyr[l], thr, int(quotas[l]))
            gx, gy, gs = ex.download_detections(f, l)
            assert np.array_equal(gx, xs) and np.array_equal(gy, ys) and np.array_equal(gs, sc), "frame %d level %d" % (f, l)
        got, want = ex.download(f), oracle.orb_extract(ocfg, imgs[f])
        assert len(got["x"]) == len(want["x"])
        for k in ("x", "y", "angle"):
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
        assert np.array_equal(got["octave"], want["octave"]) and np.array_equal(got["desc"], want["desc"])
    return quotas


@pytest.mark.parametrize("w,h", SHAPES)
def test_uncut_parametrisation_is_uncut(oracle, w, h):
    """CPU: with UNCUT every corner of every frame fits the level quota, so the GPU comparison below sees each seam corner."""
    thr, max_kpts = UNCUT
    quota = int(oracle.level_quotas(1, 1.2, max_kpts)[0])
    counts = [_corner_count(oracle, img, thr) for img in _frames(oracle, w, h)]
    print(w, h, counts, quota)
    assert max(counts) < quota and min(counts[0], counts[2]) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("thr,max_kpts", PARAMS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_single_level_shapes_bit_exact(oracle, ctx, w, h, thr, max_kpts):
    import mi355slam
    imgs = _frames(oracle, w, h)
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=1, scale_factor=1.2, max_kpts=max_kpts, fast_threshold=thr, max_batch=len(imgs))
    ex.extract(imgs)
    quotas = _compare(oracle, ex, imgs, 1, max_kpts, thr)
    if (thr, max_kpts) == UNCUT:
        assert max(_corner_count(oracle, img, thr) for img in imgs) < int(quotas[0])
    ex.close()


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [7, 20])
def test_vga_pyramid_all_layouts_bit_exact(oracle, ctx, thr):
    import mi355slam
    imgs = _frames(oracle, 640, 480)[:2]
    ex = mi355slam.OrbExtractor(ctx, 640, 480, levels=8, scale_factor=1.2, max_kpts=2000, fast_threshold=thr, max_batch=len(imgs))
    ex.extract(imgs)
    _compare(oracle, ex, imgs, 8, 2000, thr)
    ex.close()
