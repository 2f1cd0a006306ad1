"""GPU: the blurred pyramid that ImagePyramid::getBlurredLevel hands out (ms_orb_download_level(..., blurred = 1)), produced on demand by
k_blur since k_describe blurs its own patches.  Every blurred level is compared bit for bit with blur_ref.blur_u8 (plain integers in
numpy) of the level the CPU oracle built; the unblurred device level is compared with that oracle level too, so that a blur failure is
not a resize failure in disguise.

Shapes: blur_ref.cases() (tile columns and rows, border waves, reflected halo rows, saturated contents).  State: frames after the first,
the blurred planes after another extract, level 0 in place / copied on the device / uploaded in pieces.
"""
import numpy as np
import pytest

import blur_ref

pytestmark = pytest.mark.gpu

CASES = blur_ref.cases()
W, H = 252, 75             # one 248 px segment + a tile column of 4 pixels; 72 rows + 3: the second tile row reflects into the first


def _noise(seed, w=W, h=H, n=None):
    shape = (h, w) if n is None else (n, h, w)
    return np.random.default_rng(blur_ref.SEED + 1000 + seed).integers(0, 256, shape, dtype=np.uint8)


def _extractor(ctx, w, h, levels=2, scale_factor=1.2, max_batch=1):
    import mi355slam
    return mi355slam.OrbExtractor(ctx, w, h, levels=levels, scale_factor=scale_factor, max_kpts=300, max_batch=max_batch)


def _levels(oracle, img, levels=2, scale_factor=1.2):
    return oracle.build_pyramid(oracle.cfg(levels=levels, scale_factor=scale_factor), img)[0]


def _same(got, want, what):
    assert got.shape == want.shape, "%s: %s against %s" % (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        y, x = bad[0]
        raise AssertionError("%s: %d of %d pixels differ (rows %d..%d, columns %d..%d), first at (y %d, x %d): %d, want %d" % (
            what, len(bad), got.size, bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max(), y, x, got[y, x], want[y, x]))


def _check_plain(ex, f, want, what=""):
    for l, lvl in enumerate(want):
        _same(ex.download_level(f, l, False), lvl, "%s frame %d level %d" % (what, f, l))


def _check_blurred(ex, f, want, what=""):
    for l, lvl in enumerate(want):
        _same(ex.download_level(f, l, True), blur_ref.blur_u8(lvl), "%s frame %d blurred level %d" % (what, f, l))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_tile_edge_shapes_bit_exact(oracle, ctx, case):
    name, w, h, img = case
    want = blur_ref.case_pyramid(oracle, case)[0]
    ex = _extractor(ctx, w, h, levels=len(want))
    ex.extract(img)
    for l in range(len(want)):
        assert ex.level_size(l) == (want[l].shape[1], want[l].shape[0])
    _check_plain(ex, 0, want, name)
    _check_blurred(ex, 0, want, name)
    ex.close()


def test_every_frame_of_a_batch(oracle, ctx):
    """Frames f > 0 live one slab stride further: the blur must read and write there, and the download must look there."""
    frames = _noise(1, n=3)
    ex = _extractor(ctx, W, H, max_batch=3)
    ex.extract(frames)
    for f in (2, 0, 1):
        want = _levels(oracle, frames[f])
        _check_blurred(ex, f, want)
        _check_plain(ex, f, want)
    ex.close()


def test_blurred_levels_follow_the_last_extract(oracle, ctx):
    """The blurred planes are filled when somebody asks; an extract in between makes them stale, whatever was asked for before."""
    import mi355slam
    a, b, c, d = _noise(10), _noise(11), _noise(12), _noise(13)
    batch = _noise(14, n=3)
    ex = _extractor(ctx, W, H, max_batch=3)
    ex.extract(a)
    _check_blurred(ex, 0, _levels(oracle, a), "A")
    ex.extract(b)
    _check_blurred(ex, 0, _levels(oracle, b), "B after A")
    _check_plain(ex, 0, _levels(oracle, b), "B after A")
    ex.extract(c)
    _check_plain(ex, 0, _levels(oracle, c), "C")                    # unblurred first: that download must not pass for a blur
    _check_blurred(ex, 0, _levels(oracle, c), "C")
    ex.extract(batch)
    for f in (1, 2):
        _check_blurred(ex, f, _levels(oracle, batch[f]), "batch of 3")
    ex.extract(d)                                                    # the batch shrinks: frame 0 is new, frames 1 and 2 are gone
    _check_blurred(ex, 0, _levels(oracle, d), "batch of 1 after 3")
    _check_plain(ex, 0, _levels(oracle, d), "batch of 1 after 3")
    for blurred in (True, False):
        with pytest.raises(mi355slam.MsError, match="bad frame/level"):
            ex.download_level(1, 0, blurred)
    ex.close()
    fresh = _extractor(ctx, W, H, max_batch=3)                       # nothing extracted: there is no level of either kind
    for blurred in (True, False):
        with pytest.raises(mi355slam.MsError, match="bad frame/level"):
            fresh.download_level(0, 0, blurred)
    fresh.close()


def _padded(frames, row_stride, rows):
    """frames [n, H, W] inside [n, rows, row_stride] of 255: whatever is read from the padding as a pixel shows against the dark right edge."""
    out = np.full((frames.shape[0], rows, row_stride), 255, np.uint8)
    out[:, :H, :W] = frames
    return out


def test_level0_in_place_and_copied(oracle, ctx):
    """Aligned device frames are level 0 where they lie, with the caller's pitch and frame stride (256 is also the slab's pitch for this
    width, 272 is not); any other stride goes through the device-side copy into the slab."""
    frames = _noise(20, n=2)
    frames[:, :, W - 8:] //= 8                                       # a dark right edge (<= 31) beside padding of 255
    frames[:, H - 4:, :] //= 8                                       # and a dark last rows above the padding rows of the two-frame buffer
    want = [_levels(oracle, f) for f in frames]
    for what, row_stride, rows, n in (("in place, pitch 256", 256, H, 1), ("in place, pitch 272", 272, H, 1), ("copied, pitch w + 5", W + 5, H, 1),
                                      ("two frames in place", 272, H + 3, 2), ("two frames copied", W + 5, H + 3, 2)):
        host = _padded(frames[:n], row_stride, rows)
        buf = ctx.upload(host)
        assert buf.ptr % 16 == 0
        ex = _extractor(ctx, W, H, max_batch=2)
        ex.extract(buf, n_frames=n, frame_stride=rows * row_stride, row_stride=row_stride)
        for f in reversed(range(n)):
            _check_blurred(ex, f, want[f], what)
            _check_plain(ex, f, want[f], what)
        assert np.array_equal(buf.download(), host)                  # the caller's frames are read, never written
        ex.close()
        buf.free()


def test_after_a_chunked_host_batch(oracle, ctx):
    """32 or more host frames go up in four pieces of ceil(n / 4) on a copy stream, each piece's kernels enqueued on its own: 33 frames are
    pieces 0..8, 9..17, 18..26, 27..32.  The one k_blur launch afterwards covers the whole batch."""
    n, w, h = 33, 64, 48
    frames = _noise(30, w, h, n)
    ex = _extractor(ctx, w, h, levels=1, max_batch=n)
    ex.extract(frames)
    for f in (0, 8, 9, 16, 17, 18, 26, 27, 32):
        _check_blurred(ex, f, [frames[f]], "33 host frames")
        _check_plain(ex, f, [frames[f]], "33 host frames")
    ex.close()


def test_random_sizes(oracle, ctx):
    """30 random (size, levels, scale factor) draws, noise or the synthetic scene; blurred levels only."""
    rng = np.random.default_rng(blur_ref.SEED + 40)
    done = 0
    while done < 30:
        w, h = int(rng.integers(40, 701)), int(rng.integers(40, 301))
        levels, sf = int(rng.integers(1, 4)), float(rng.choice([1.1, 1.2, 1.5, 2.0]))
        ws, hs = oracle.level_sizes(levels, sf, w, h)
        if min(ws[-1], hs[-1]) < 40:
            continue
        img = rng.integers(0, 256, (h, w), dtype=np.uint8) if done % 2 == 0 else oracle.synth_frame(w, h, int(rng.integers(0, 1000)))
        ex = _extractor(ctx, w, h, levels=levels, scale_factor=sf)
        ex.extract(img)
        _check_blurred(ex, 0, _levels(oracle, img, levels, sf), "%dx%d, %d levels at %.1f" % (w, h, levels, sf))
        ex.close()
        done += 1
