"""One-sided FAST scoring in k_fast.

A survivor of the compass pre-test is scored only on the side(s) whose pre-test it passed: with t >= 1 a ring cannot score
above t on both sides (two arcs of 9 on a ring of 16 overlap), and a side scores above t only where its pre-test holds.
The CPU part checks that lemma, and the kernel's formulation of it, in numpy; the GPU part runs frames built so that many
survivors pass BOTH pre-tests and compares the detector against the oracle bit for bit.
"""
import numpy as np
import pytest

# ring offsets in k_fast's order: index k and k + 8 are opposite; 0 / 8 = (0, +-3), 4 / 12 = (+-3, 0)
RDX = np.array([0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1])
RDY = np.array([3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3])
ARCS = (np.arange(16)[:, None] + np.arange(9)[None, :]) % 16          # the 16 arcs of 9


def _side_score(v):
    """max over the 16 arcs of 9 of min(v): v is (n, 16)."""
    return v[:, ARCS].min(axis=2).max(axis=1)


def _rings(rng, n):
    """Centres, rings and thresholds that hit every case: arcs brighter and darker than the centre at once, ties, extremes."""
    c = rng.integers(0, 256, n)
    thr = rng.integers(1, 255, n)
    ring = rng.integers(0, 256, (n, 16))
    # half of the rings: one bright arc and one dark arc of random lengths and starts around the centre
    k = n // 2
    for sign in (1, -1):
        start = rng.integers(0, 16, k)
        length = rng.integers(3, 17, k)
        amp = rng.integers(0, 256, k)
        idx = (start[:, None] + np.arange(16)[None, :]) % 16
        on = np.arange(16)[None, :] < length[:, None]
        vals = np.clip(c[:k, None] + sign * (amp[:, None] + rng.integers(-3, 4, (k, 16))), 0, 255)
        rows = np.repeat(np.arange(k)[:, None], 16, axis=1)
        ring[rows[on], idx[on]] = vals[on]
    return c, ring, thr


def _pretest(c, ring, thr):
    """Phase A1's compass test per side: (ring darker than c - t on both opposite pairs, ring brighter than c + t on both)."""
    d = c[:, None] - ring
    dark = np.minimum(np.maximum(d[:, 0], d[:, 8]), np.maximum(d[:, 4], d[:, 12])) > thr
    bright = np.maximum(np.minimum(d[:, 0], d[:, 8]), np.minimum(d[:, 4], d[:, 12])) < -thr
    return dark, bright


def test_one_sided_lemma_random_rings():
    rng = np.random.default_rng(20261016)
    for _ in range(8):
        c, ring, thr = _rings(rng, 40000)
        d = c[:, None] - ring
        s_dark, s_bright = _side_score(d), _side_score(-d)
        two_sided = np.maximum(s_dark, s_bright)
        pre_dark, pre_bright = _pretest(c, ring, thr)
        corner = two_sided > thr
        assert corner.sum() > 1000 and (corner & pre_dark & pre_bright).sum() > 0
        assert not np.any(corner & (s_dark > thr) & (s_bright > thr))            # never a corner on both sides
        passed = np.where(pre_dark, s_dark, -1000)
        passed = np.maximum(passed, np.where(pre_bright, s_bright, -1000))
        assert np.array_equal(passed[corner], two_sided[corner])                  # the passed side(s) give the exact score
        assert not np.any(passed[~corner] > thr[~corner])                        # and never invent a corner


def test_kernel_formulation_matches_two_sided_score():
    """The kernel's arithmetic: one ladder on d (ring darker) or on ~d = -d - 1 (ring brighter, +1 afterwards), and a second
    ladder on ~d only for lanes that passed both pre-tests and are not corners on the darker-ring side."""
    rng = np.random.default_rng(7)
    c, ring, thr = _rings(rng, 200000)
    d = (c[:, None] - ring).astype(np.int16)
    two_sided = np.maximum(_side_score(d.astype(np.int32)), _side_score(-d.astype(np.int32)))
    pre_dark, pre_bright = _pretest(c, ring, thr)
    survivor = pre_dark | pre_bright
    # P = sgn * r + k modulo 2^16 with (sgn, k) = (-1, c) or (1, ~c)
    sgn = np.where(pre_dark, 0xFFFF, 1).astype(np.uint16)[:, None]
    k = np.where(pre_dark, c, ~c & 0xFFFF).astype(np.uint16)[:, None]
    p = (sgn * ring.astype(np.uint16) + k).astype(np.uint16).view(np.int16).astype(np.int32)
    best = _side_score(p) + np.where(pre_dark, 0, 1)
    again = pre_dark & pre_bright & (best <= thr)
    second = _side_score((ring - c[:, None] - 1).astype(np.int32)) + 1
    best = np.where(again, np.maximum(best, second), best)
    corner = two_sided > thr
    assert np.array_equal(survivor & (best > thr), corner)                       # the same corners ...
    assert np.array_equal(best[corner], two_sided[corner])                       # ... with the same scores


def _both_sides_frame(w, h, seed):
    """Wedges, thin bright bars crossing dark bars and steep cones: beside the crossings and on every slanted slope the ring
    has a brighter pixel AND a darker one in each opposite pair, so both pre-tests pass, while only one side (or none) is a
    corner."""
    rng = np.random.default_rng(seed)
    img = 128 + rng.integers(0, 6, (h, w))
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(40):                                          # wedges: half-planes through a random point, cut by a second one
        y0, x0 = rng.integers(0, h), rng.integers(0, w)
        a1, a2 = rng.uniform(0, 2 * np.pi, 2)
        inside = ((xx - x0) * np.cos(a1) + (yy - y0) * np.sin(a1) > 0) & ((xx - x0) * np.cos(a2) + (yy - y0) * np.sin(a2) > 0)
        inside &= (np.abs(xx - x0) < 60) & (np.abs(yy - y0) < 60)
        img[inside] = rng.integers(0, 256)
    for _ in range(30):                                          # a dark bar crossed by a bright one, and the other way round
        y0, x0, th = int(rng.integers(4, h - 4)), int(rng.integers(4, w - 4)), int(rng.integers(1, 4))
        lo, hi = (int(rng.integers(0, 40)), int(rng.integers(215, 256)))[::1 if rng.integers(0, 2) else -1]
        img[y0:y0 + th, max(0, x0 - 80):x0 + 80] = lo
        img[max(0, y0 - 80):y0 + 80, x0:x0 + th] = hi
    for _ in range(24):                                          # steep cones: on a slanted slope both pre-tests hold, the curvature makes one side a corner
        y0, x0 = rng.integers(0, h), rng.integers(0, w)
        k = rng.uniform(8, 45)
        r = np.hypot(xx - x0, yy - y0)
        v = (k * r) % 510
        img = np.where(r < 50, np.minimum(v, 510 - v), img)      # a triangle wave of the radius
    return img.clip(0, 255).astype(np.uint8)


def test_frames_pass_both_pre_tests():
    """The GPU frames below really exercise the second ladder: many pre-test survivors pass both sides."""
    img = _both_sides_frame(640, 480, 1).astype(np.int32)
    ys, xs = np.mgrid[3:477, 3:637]
    c = img[ys, xs].ravel()
    ring = np.stack([img[ys + RDY[k], xs + RDX[k]].ravel() for k in range(16)], axis=1)
    pre_dark, pre_bright = _pretest(c, ring, np.full(c.shape, 20))
    assert (pre_dark & pre_bright).sum() > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [1, 7, 20, 60, 120])
def test_both_sides_frames_bit_exact(oracle, ctx, thr):
    import mi355slam
    imgs = np.stack([_both_sides_frame(640, 480, s) for s in (1, 2)])
    n, h, w = imgs.shape
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=4, scale_factor=1.2, max_kpts=3000, fast_threshold=thr, max_batch=n)
    ex.extract(imgs)
    ocfg = oracle.cfg(levels=4, scale_factor=1.2, max_kpts=3000, fast_threshold=thr)
    quotas = oracle.level_quotas(4, 1.2, 3000)
    for f in range(n):
        levels, _ = oracle.build_pyramid(ocfg, imgs[f])
        for l in range(4):
            xs, ys, sc = oracle.detect_level(levels[l], thr, int(quotas[l]))
            gx, gy, gs = ex.download_detections(f, l)
            assert np.array_equal(gx, xs) and np.array_equal(gy, ys) and np.array_equal(gs, sc), "frame %d level %d" % (f, l)
        got, want = ex.download(f), oracle.orb_extract(ocfg, imgs[f])
        assert len(got["x"]) == len(want["x"]) > 0
        for k in ("x", "y", "angle"):
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
        assert np.array_equal(got["octave"], want["octave"]) and np.array_equal(got["desc"], want["desc"])
