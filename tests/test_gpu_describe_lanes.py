"""GPU parity of k_describe's lane maps (csrc/describe_lanes.h): single small frames and a 3-frame batch, bit-exact against the CPU oracle in
x, y, angle, octave and all 8 descriptor words.

The sizes are chosen so that both window-fetch paths run in every case: a keypoint whose 45 x 48-byte window lies inside its level takes the
table-driven dword fetch (nine pieces, all three dword-column wraps), one within 24 px of a border the byte-by-byte REFLECT_101 path.  Each
case asserts that both kinds are present (from the oracle's per-level detections), and the keypoint totals cover counts that are and are not
a multiple of the four keypoints of a workgroup.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_BASE = dict(scale_factor=1.2, lk_track_level=0, min_distance=0.0)


def _frame(oracle, kind, w, h, seed):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    return oracle.synth_frame(w, h, seed)


def _inner_and_border(oracle, ocfg, d, img):
    """How many of the frame's detections have their whole window inside their level (k_describe's test), and how many do not."""
    levels, _ = oracle.build_pyramid(ocfg, img)
    quotas = oracle.level_quotas(d["levels"], d["scale_factor"], d["max_kpts"])
    ni = nb = 0
    for l in range(d["levels"]):
        h, w = levels[l].shape
        xs, ys, _ = oracle.detect_level(levels[l], d["fast_threshold"], int(quotas[l]))
        inner = (xs >= 23) & (xs + 24 < w) & (ys >= 22) & (ys + 22 < h)
        ni += int(inner.sum())
        nb += int((~inner).sum())
    return ni, nb


def _check(oracle, ctx, imgs, **kw):
    import mi355slam
    d = dict(_BASE, **kw)
    ocfg = oracle.cfg(**d)
    n, h, w = imgs.shape
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=d["levels"], scale_factor=d["scale_factor"], max_kpts=d["max_kpts"], lk_track_level=0,
                                fast_threshold=d["fast_threshold"], max_tracks=0, max_batch=n, min_distance=0.0)
    ex.extract(imgs)
    totals = []
    for f in range(n):
        got, want = ex.download(f), oracle.orb_extract(ocfg, imgs[f])
        ni, nb = _inner_and_border(oracle, ocfg, d, imgs[f])
        print("%dx%d frame %d: %d keypoints, %d with the window inside the level, %d on the reflect path" % (w, h, f, len(want["x"]), ni, nb))
        assert ni > 0 and nb > 0 and ni + nb == len(want["x"])
        assert len(got["x"]) == len(want["x"])
        for k in ("x", "y", "angle"):
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
        assert np.array_equal(got["octave"], want["octave"])
        assert got["desc"].shape == (len(want["x"]), 8) and np.array_equal(got["desc"], want["desc"])
        assert all((want["octave"] == l).any() for l in range(d["levels"]))
        totals.append(len(want["x"]))
    return totals


@pytest.mark.parametrize("w,h,levels,thr,max_kpts,kind,seed", [
    (96, 80, 3, 20, 300, "noise", 1),        # 86 keypoints: the last workgroup has two idle waves
    (96, 80, 4, 20, 300, "noise", 2),        # 73: one wave in the last workgroup
    (200, 150, 4, 20, 700, "noise", 3),      # 418
    (200, 150, 3, 15, 500, "synth", 4),      # 292 = 4 * 73: every workgroup full
])
def test_single_frames_bit_exact(oracle, ctx, w, h, levels, thr, max_kpts, kind, seed):
    total, = _check(oracle, ctx, _frame(oracle, kind, w, h, seed)[None], levels=levels, fast_threshold=thr, max_kpts=max_kpts)
    assert (total % 4 == 0) == (kind == "synth")


def test_batch_of_three_bit_exact(oracle, ctx):
    imgs = np.stack([_frame(oracle, "noise", 200, 150, 3), _frame(oracle, "synth", 200, 150, 4), _frame(oracle, "noise", 200, 150, 11)])
    totals = _check(oracle, ctx, imgs, levels=4, fast_threshold=20, max_kpts=700)
    assert any(t % 4 for t in totals)
