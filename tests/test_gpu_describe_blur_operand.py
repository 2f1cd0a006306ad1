"""GPU parity of k_describe's blur with pass 1's result as pass 2's B operand (csrc/describe_lanes.h: vert_operand, blur_store_*): small single
frames and a 3-frame batch, bit-exact against the CPU oracle in x, y, angle, octave and all 8 descriptor words, at forced strips of 1 and 8
keypoints per wave and with the blocks dealt per XCD alone (order 1) and with the spatial visit order as well (order 3).

Every BRIEF test reads two bytes of the 39 x 39 blurred patch, so a wrong column tile (t = 2 with its 7 valid columns), a wrong row tile (yt = 2
with its 7 valid rows), a wrong K group of the permuted vertical operand or a row / column mix-up in the column-major patch index changes
descriptor bits of nearly every keypoint.  Each case asserts, from the oracle's per-level detections, that keypoints with the window inside their
level AND keypoints on the REFLECT_101 path are present, and that every level has a keypoint.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_BASE = dict(scale_factor=1.2, lk_track_level=0, min_distance=0.0)
_CASES = {                                      # name -> (frames as (kind, seed), w, h, levels, threshold, max_kpts)
    "96x80-3-noise": ([("noise", 1)], 96, 80, 3, 20, 300),
    "200x150-4-noise": ([("noise", 3)], 200, 150, 4, 20, 700),
    "200x150-4-synth": ([("synth", 4)], 200, 150, 4, 15, 700),
    "200x150-4-batch3": ([("noise", 3), ("synth", 4), ("noise", 11)], 200, 150, 4, 20, 700),
}
_ref = {}                                       # case -> (frames, settings, the oracle's keypoints per frame), computed once


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


def _reference(oracle, case):
    if case not in _ref:
        frames, w, h, levels, thr, max_kpts = _CASES[case]
        d = dict(_BASE, levels=levels, fast_threshold=thr, max_kpts=max_kpts)
        ocfg = oracle.cfg(**d)
        imgs = np.stack([_frame(oracle, kind, w, h, seed) for kind, seed in frames])
        want = []
        for f in range(len(imgs)):
            k = oracle.orb_extract(ocfg, imgs[f])
            ni, nb = _inner_and_border(oracle, ocfg, d, imgs[f])
            print("%s frame %d: %d keypoints, %d with the window inside the level, %d on the reflect path" % (case, f, len(k["x"]), ni, nb))
            assert ni > 0 and nb > 0 and ni + nb == len(k["x"])
            assert all((k["octave"] == l).any() for l in range(levels))
            want.append(k)
        _ref[case] = (imgs, d, want)
    return _ref[case]


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("r", [1, 8])
@pytest.mark.parametrize("case", list(_CASES))
def test_bit_exact(oracle, ctx, case, r, order):
    import mi355slam
    imgs, d, want = _reference(oracle, case)
    n, h, w = imgs.shape
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=d["levels"], scale_factor=d["scale_factor"], max_kpts=d["max_kpts"], lk_track_level=0,
                                fast_threshold=d["fast_threshold"], max_tracks=0, max_batch=n, min_distance=0.0)
    ex.set_describe_strip(r)
    ex.set_describe_order(order)
    ex.extract(imgs)
    for f in range(n):
        got = ex.download(f)
        assert len(got["x"]) == len(want[f]["x"])
        for k in ("x", "y", "angle"):
            assert np.array_equal(got[k].view(np.uint32), want[f][k].view(np.uint32)), (f, k)
        assert np.array_equal(got["octave"], want[f]["octave"]), f
        assert got["desc"].shape == (len(want[f]["x"]), 8) and np.array_equal(got["desc"], want[f]["desc"]), f
