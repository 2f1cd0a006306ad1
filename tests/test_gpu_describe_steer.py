"""GPU parity of k_describe's steering arithmetic (csrc/describe_steer.h: one division and one polynomial in the arc tangent, cosine and sine from
one evaluation on two lanes): one 160 x 120 synthetic frame, its three 90-degree rotations and two mirror images, 2 levels, so that every sign
and octant of the moments (m10, m01) occurs.  Keypoints, angles and descriptors must be exactly the oracle's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CFG = dict(levels=2, scale_factor=1.2, lk_track_level=0, min_distance=0.0, fast_threshold=20, max_kpts=500)


@pytest.fixture(scope="module")
def views(oracle):
    """The frame's six views with the oracle's result for each, computed once."""
    base = oracle.synth_frame(160, 120, 21)
    imgs = [base, np.rot90(base, 1), np.rot90(base, 2), np.rot90(base, 3), base[:, ::-1], base[::-1, :]]
    imgs = [np.ascontiguousarray(v) for v in imgs]
    ocfg = oracle.cfg(**_CFG)
    return [(v, oracle.orb_extract(ocfg, v)) for v in imgs]


def test_every_octant_and_sign_occurs(views):
    ang = np.concatenate([w["angle"] for _, w in views])
    assert len(ang) > 300
    octants = np.unique((ang // 45.0).astype(np.int64) % 8)
    print("%d keypoints, per octant:" % len(ang), np.bincount((ang // 45.0).astype(np.int64) % 8, minlength=8))
    assert len(octants) == 8                                      # both signs of m10 and of m01, |m10| above and below |m01|


@pytest.mark.parametrize("view", range(6))
def test_views_bit_exact(ctx, views, view):
    import mi355slam
    img, want = views[view]
    h, w = img.shape
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=_CFG["levels"], scale_factor=_CFG["scale_factor"], max_kpts=_CFG["max_kpts"], lk_track_level=0,
                                fast_threshold=_CFG["fast_threshold"], max_tracks=0, max_batch=1, min_distance=0.0)
    ex.extract(img[None])
    got = ex.download(0)
    assert len(got["x"]) == len(want["x"]) > 20
    for k in ("x", "y", "angle"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert np.array_equal(got["octave"], want["octave"])
    assert got["desc"].shape == (len(want["x"]), 8) and np.array_equal(got["desc"], want["desc"])
