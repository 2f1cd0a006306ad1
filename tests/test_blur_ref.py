"""CPU only: the oracle's blur against a third statement of the operation (blur_ref.py: plain integers in numpy), and the distance of both
from the real-valued Gaussian.  This pins oracle/frontend.c before any GPU test compares k_blur with it."""
import numpy as np
import pytest

import blur_ref

CASES = blur_ref.cases()


@pytest.fixture(scope="module")
def pyramids(oracle):
    """name -> (levels, blurs) of the oracle."""
    return {c[0]: blur_ref.case_pyramid(oracle, c) for c in CASES}


def test_cases_cover_the_shapes_they_name():
    ws, hs = {c[1] for c in CASES}, {c[2] for c in CASES}
    assert ws >= {40, 41, 42, 43, 244, 245, 247, 248, 249, 251, 252, 253, 496, 497, 500}
    assert hs >= {40, 41, 53, 54, 55, 69, 71, 72, 73, 75, 90}
    assert len({c[0] for c in CASES}) == len(CASES)
    l1 = [blur_ref.level_sizes(w, h, 2, 1.2)[1] for _, w, h, _ in CASES if blur_ref.levels_for(w, h) == 2]
    assert {40, 41, 42, 43} <= {w for w, _ in l1} and {40, 41} <= {h for _, h in l1}          # the minimum sizes also behind the resize
    for _, w, h, img in CASES:
        assert img.shape == (h, w) and img.dtype == np.uint8 and not img.flags.writeable
    for kind in ("zeros", "full", "checker", "stripes"):
        assert sum(c[0].startswith(kind) for c in CASES) == 3


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_oracle_blur_is_the_integer_filter(oracle, pyramids, case):
    name, w, h, img = case
    levels, blurs = pyramids[name]
    assert [(a.shape[1], a.shape[0]) for a in levels] == blur_ref.level_sizes(w, h, blur_ref.levels_for(w, h), 1.2)
    assert np.array_equal(levels[0], img)
    for l, (lvl, blur) in enumerate(zip(levels, blurs)):
        want = blur_ref.blur_u8(lvl)
        bad = np.argwhere(want != blur)
        assert len(bad) == 0, "level %d: %d pixels differ, first at (y, x) = %s" % (l, len(bad), tuple(bad[0]))


def test_taps_are_the_quantised_gaussian(oracle):
    """Plain rounding of 256 g gives 18 34 49 55 49 34 18 = 257; the fixed-point kernel has to sum to 256 and carries the rounding error
    inwards, so a tap may be off by up to one unit, no more."""
    g = np.exp(-(np.arange(7) - 3.0) ** 2 / 8.0)
    g = g / g.sum() * 256
    assert blur_ref.TAPS.sum() == 256 and np.array_equal(blur_ref.TAPS, blur_ref.TAPS[::-1])
    assert np.abs(blur_ref.TAPS - g).max() < 1.0
    assert np.array_equal(oracle.gauss7_taps()[1], blur_ref.TAPS)


def test_distance_to_the_real_gaussian(pyramids):
    """max |blur_u8 - round(gaussian_f64)| over both levels of the noise cases is 2 grey levels (measured: 2, reached at one pixel of the
    49 x 50 frame; 1 everywhere else; the unrounded distance |blur_u8 - gaussian_f64| peaks at 1.514).

    Where it comes from: the taps times 256 are 17.961 33.555 48.822 55.323, stored as 18 34 48 56, so the 1-D tap errors are
    (+0.039 +0.445 -0.822 +0.677 -0.822 +0.445 +0.039) / 256.  They sum to zero (no error on flat images: the all-0 and all-255 cases
    give 0), and they alternate in sign, so the worst input alternates too: 0 / 255 stripes of period 2 collect 255 * 1.567 / 256 = 1.56,
    plus 0.5 of the final rounding = 2.04 (measured on the stripes cases: 2.045, integer distance 2).  Noise correlates with that pattern
    only in part: up to 1.01 of filter error + 0.5.  An adversarial image could reach 255 * sum |q (x) q / 65536 - g (x) g| + 1 = 5.08; no
    case here is one.  A value above 3 on noise would mean wrong taps or a wrong normalisation."""
    worst, worst_real = 0, 0.0
    for name, w, h, img in CASES:
        for lvl in pyramids[name][0]:
            b, g = blur_ref.blur_u8(lvl), blur_ref.gaussian_f64(lvl)
            d = int(np.abs(b.astype(np.int64) - np.rint(g).astype(np.int64)).max())
            if name.startswith("noise"):
                worst, worst_real = max(worst, d), max(worst_real, float(np.abs(b - g).max()))
            elif name.startswith(("zeros", "full")):
                assert d == 0, name
            else:
                assert d <= 2, name
    print("integer blur vs rounded Gaussian on noise: %d grey levels (unrounded %.4f)" % (worst, worst_real))
    assert worst <= 2
