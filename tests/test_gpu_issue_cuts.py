"""GPU parity of k_resize's scalar row bases and three-instruction vertical pass (csrc/resize_vpass.h) and of k_describe's folded BRIEF index
(csrc/describe_brief_index.h), bit-exact against the CPU oracle.

  333 x 119, 3 levels x 1.2, 3 device frames with a row stride of 352 and a frame stride of 120 rows, used in place as level 0: frame and row
      bases that are real 64-bit sums (plane + frame * stride + row * pitch, pitch != width), 278 px = a full wave beside an edge wave,
      short last groups whose loaded rows clamp at the source's last row
  150 x 200, 4 levels x 1.5, 1 frame: the general path's loads and stores, and levels narrow enough (100, 67, 44 px) that the single wave of a
      row is an edge wave whose 12-byte fetch starts left of its window
  200 x 150, 3 levels, 2 frames: descriptors and angles array by array; the oracle's keypoints must cover all four quadrants of the steering
      angle, the reflect path (a window that leaves its level) and at least 200 keypoints, or the case shows nothing
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _assert_levels(oracle, ex, imgs, levels, f):
    ocfg = oracle.cfg(levels=levels, scale_factor=f, max_kpts=500)
    for i in range(len(imgs)):
        want, _ = oracle.build_pyramid(ocfg, imgs[i])
        for l in range(levels):
            assert ex.level_size(l) == (want[l].shape[1], want[l].shape[0])
            got = ex.download_level(i, l, False)
            bad = np.argwhere(got != want[l])
            assert len(bad) == 0, "frame %d level %d: %d pixels differ, first at (row, col) %s" % (i, l, len(bad), bad[0])


def test_resize_levels_bit_exact_with_a_padded_row_stride(oracle, ctx):
    import mi355slam
    w, h, levels, f, n, stride, rows = 333, 119, 3, 1.2, 3, 352, 120
    imgs = np.stack([oracle.synth_frame(w, h, 4100 + 7 * i, 3 * i, i) for i in range(n)])
    padded = np.full((n, rows, stride), 0xA5, np.uint8)           # bytes past a row's end must not reach a pixel
    padded[:, :h, :w] = imgs
    buf = ctx.upload(padded)
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=levels, scale_factor=f, max_kpts=500, max_batch=n)
    ex.extract(buf, n_frames=n, frame_stride=rows * stride, row_stride=stride)      # 16-byte aligned strides: level 0 is the caller's buffer
    _assert_levels(oracle, ex, imgs, levels, f)


def test_resize_levels_bit_exact_general_path_narrow_levels(oracle, ctx):
    import mi355slam
    w, h, levels, f = 150, 200, 4, 1.5
    imgs = oracle.synth_frame(w, h, 4200)[None]
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=levels, scale_factor=f, max_kpts=500, max_batch=1)
    ex.extract(imgs)
    assert [ex.level_size(l)[0] for l in range(levels)] == [150, 100, 67, 44]
    _assert_levels(oracle, ex, imgs, levels, f)


DESC = dict(w=200, h=150, levels=3, scale_factor=1.2, fast_threshold=15, max_kpts=500, lk_track_level=0, min_distance=0.0, seeds=(4, 21))


def describe_case(oracle):
    """The frames of the descriptor case and the oracle's keypoints for them, with what the case must show (also run on the CPU, without a device)."""
    d = DESC
    imgs = np.stack([oracle.synth_frame(d["w"], d["h"], s) for s in d["seeds"]])
    ocfg = oracle.cfg(levels=d["levels"], scale_factor=d["scale_factor"], fast_threshold=d["fast_threshold"], max_kpts=d["max_kpts"],
                      lk_track_level=0, min_distance=0.0)
    want = [oracle.orb_extract(ocfg, img) for img in imgs]
    angle = np.concatenate([k["angle"] for k in want])
    quadrants = {int(a // 90) % 4 for a in angle}
    # keypoints whose 45 x 48-byte window leaves their level (k_describe's own test): the byte-by-byte REFLECT_101 fetch
    quotas = oracle.level_quotas(d["levels"], d["scale_factor"], d["max_kpts"])
    border = 0
    for img in imgs:
        levels, _ = oracle.build_pyramid(ocfg, img)
        for l in range(d["levels"]):
            lh, lw = levels[l].shape
            xs, ys, _ = oracle.detect_level(levels[l], d["fast_threshold"], int(quotas[l]))
            border += int((~((xs >= 23) & (xs + 24 < lw) & (ys >= 22) & (ys + 22 < lh))).sum())
    return imgs, ocfg, want, quadrants, border, len(angle)


def test_descriptors_and_angles_equal_the_oracle(oracle, ctx):
    import mi355slam
    d = DESC
    imgs, ocfg, want, quadrants, border, total = describe_case(oracle)
    print("descriptor case: %d keypoints, angle quadrants %s, %d within 24 px of a border" % (total, sorted(quadrants), border))
    assert quadrants == {0, 1, 2, 3}
    assert border >= 1
    assert total >= 200
    ex = mi355slam.OrbExtractor(ctx, d["w"], d["h"], levels=d["levels"], scale_factor=d["scale_factor"], max_kpts=d["max_kpts"], lk_track_level=0,
                                fast_threshold=d["fast_threshold"], max_tracks=0, max_batch=len(imgs), min_distance=0.0)
    ex.extract(imgs)
    for f in range(len(imgs)):
        got = ex.download(f)
        assert len(got["x"]) == len(want[f]["x"])
        for k in ("x", "y", "angle"):
            assert np.array_equal(got[k].view(np.uint32), want[f][k].view(np.uint32)), (f, k)
        assert np.array_equal(got["octave"], want[f]["octave"])
        assert got["desc"].shape == (len(want[f]["x"]), 8) and np.array_equal(got["desc"], want[f]["desc"])
