"""The blur of the pyramid (image_pyramid.cpp:84: GaussianBlur 7 x 7, sigma 2, BORDER_REFLECT_101 on 8-bit pixels) in plain numpy, and the
shapes at which k_blur's tiles, border waves and row reflection change behaviour (shared by two test files).

blur_u8 is OpenCV's 8-bit fixed-point path written as integers: the Gaussian taps in 8.8 fixed point, 18 34 48 56 48 34 18 (sum 256), applied
along rows and columns without an intermediate rounding, then (acc + 32768) >> 16.  gaussian_f64 is the real-valued filter the taps stand
for.  Neither shares code with oracle/frontend.c or with the kernel.
"""
import numpy as np

TAPS = np.array([18, 34, 48, 56, 48, 34, 18], np.int64)
SEED = 20261


def _separable(p, taps, h, w):
    rows = sum(taps[i] * p[:, i:i + w] for i in range(7))            # (h + 6, w)
    return sum(taps[j] * rows[j:j + h, :] for j in range(7))         # (h, w)


def blur_u8(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2 and min(img.shape) >= 4
    h, w = img.shape
    p = np.pad(img, 3, mode="reflect").astype(np.int64)              # numpy's "reflect" leaves the edge pixel out: BORDER_REFLECT_101
    out = (_separable(p, TAPS, h, w) + 32768) >> 16
    assert TAPS.sum() == 256 and 0 <= out.min() and out.max() <= 255  # 255 * 256 * 256 + 32768 < 256 << 16: nothing to clamp
    return out.astype(np.uint8)


def gaussian_f64(img):
    img = np.asarray(img)
    h, w = img.shape
    g = np.exp(-(np.arange(7) - 3.0) ** 2 / 8.0)                     # cv::getGaussianKernel(7, 2)
    g /= g.sum()
    return _separable(np.pad(img, 3, mode="reflect").astype(np.float64), g, h, w)


def level_sizes(w, h, levels, f):
    """round(size / scale) with the float32 product chain of the scale factors (static_settings.cpp)."""
    s, out = np.float32(1.0), []
    for _ in range(levels):
        out.append((int(np.round(w / float(s))), int(np.round(h / float(s)))))
        s = np.float32(f) * s
    return out


def levels_for(w, h):
    """Two levels at 1.2 wherever level 1 is still 40 x 40 (the smallest level an extractor takes), else the frame alone."""
    return 2 if min(level_sizes(w, h, 2, 1.2)[1]) >= 40 else 1


# Widths: the minimum and all four w % 4; one 248 px segment with a second tile column of 1 .. 5 pixels, and just under it; two segments.
# Heights: the minimum; 53 .. 55 (the third wave's first rows: 18 rows per wave); the 72-row tile +- 3, where the halo rows of the last wave
# reflect; 90.  Level 1 (w / 1.2, h / 1.2) adds 203 .. 211, 413 .. 417 x 45 .. 75.  A frame under 48 px has no level 1 of 40 px, so those go
# in alone, and the last four sizes put the same minimum widths and heights (40 .. 43) on level 1 instead, behind the resize.
SIZES = [(40, 40), (41, 41), (42, 53), (43, 54), (244, 55), (245, 69), (247, 71), (248, 72), (249, 73), (251, 75), (252, 90), (253, 40),
         (496, 41), (497, 72), (500, 73), (252, 75), (249, 54), (496, 90),
         (48, 48), (49, 50), (50, 52), (52, 49)]
SATURATED = [(43, 54), (249, 73), (497, 72)]       # narrow; a second tile column of one pixel; two segments and a third column of one pixel

_cases = None


def cases():
    """[(name, w, h, image)]: uniform noise at every size of SIZES; all 0, all 255, a one-pixel 0 / 255 checkerboard and 0 / 255 vertical
    stripes of period 2 at the sizes of SATURATED (the packed 16-bit column sums at their largest value, 255 * 256).  Built once, read-only."""
    global _cases
    if _cases is None:
        out = []
        for i, (w, h) in enumerate(SIZES):
            out.append(("noise-%dx%d" % (w, h), w, h, np.random.default_rng(SEED + i).integers(0, 256, (h, w), dtype=np.uint8)))
        for (w, h) in SATURATED:
            y, x = np.mgrid[0:h, 0:w]
            out.append(("zeros-%dx%d" % (w, h), w, h, np.zeros((h, w), np.uint8)))
            out.append(("full-%dx%d" % (w, h), w, h, np.full((h, w), 255, np.uint8)))
            out.append(("checker-%dx%d" % (w, h), w, h, (((x + y) & 1) * 255).astype(np.uint8)))
            out.append(("stripes-%dx%d" % (w, h), w, h, ((x & 1) * 255).astype(np.uint8)))
        for c in out:
            c[3].flags.writeable = False
        _cases = out
    return _cases


_pyramids = {}


def case_pyramid(oracle, case):
    """(levels, blurs) of the oracle for one of cases(), built once per process, read-only."""
    name, w, h, img = case
    if name not in _pyramids:
        levels, blurs = oracle.build_pyramid(oracle.cfg(levels=levels_for(w, h), scale_factor=1.2), img)
        for a in levels + blurs:
            a.flags.writeable = False
        _pyramids[name] = (levels, blurs)
    return _pyramids[name]
