"""GPU parity of k_describe's strip walk (csrc/describe_strips.h): a wave describes r keypoints one after another, r in {1, 2, 3, 4, 8} forced
through OrbExtractor.set_describe_strip.  For every r the outputs are bit-exact against the CPU oracle (x, y, angle, octave, track id and all 8
descriptor words) and equal to the r = 1 run, array for array.

The shapes are those of tests/test_gpu_describe_lanes.py (96 x 80 and 200 x 150, 3 - 4 levels: 86, 73, 418 and 292 keypoints).  What a case is
there for is asserted from the oracle's output: a total that is not a multiple of 4 r (ragged last strip, waves with fewer than r keypoints), a
total below 4, a batch whose middle frame is blank, an inner keypoint followed by a border (REFLECT_101) one and the reverse inside a wave's strip
(slots 4 apart), a strip across the tracker / detection boundary, and two extracts of different frames on one extractor.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_BASE = dict(scale_factor=1.2, lk_track_level=0, min_distance=0.0)
_KEYS = ("x", "y", "angle", "octave", "desc", "track_id")
_RS = [1, 2, 3, 4, 8]
_SINGLE = {                                     # name -> (w, h, levels, threshold, max_kpts, kind, seed): test_gpu_describe_lanes.py's shapes
    "96x80-3": (96, 80, 3, 20, 300, "noise", 1),
    "96x80-4": (96, 80, 4, 20, 300, "noise", 2),
    "200x150-4": (200, 150, 4, 20, 700, "noise", 3),
    "200x150-3": (200, 150, 3, 15, 500, "synth", 4),
}
_TRACKS = np.array([[60.5, 50.25], [100.0, 75.0], [21.0, 70.0], [150.75, 120.5], [178.0, 20.0]], np.float32)   # two of them within 24 px of a border
_TRACK_IDS = np.array([11, 12, 13, 14, 15], np.int32)
_ref = {}                                       # case -> the oracle's keypoints per frame, computed once
_r1 = {}                                        # case -> the r = 1 run's arrays per frame


def _frame(oracle, kind, w, h, seed):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "blank":
        return np.full((h, w), 90, np.uint8)
    return oracle.synth_frame(w, h, seed)


def _extractor(ctx, w, h, d, n, r, max_tracks=0):
    import mi355slam
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=d["levels"], scale_factor=d["scale_factor"], max_kpts=d["max_kpts"], lk_track_level=0,
                                fast_threshold=d["fast_threshold"], max_tracks=max_tracks, max_batch=n, min_distance=0.0)
    ex.set_describe_strip(r)
    return ex


def _same(got, want):
    assert len(got["x"]) == len(want["x"])
    for k in ("x", "y", "angle"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    for k in ("octave", "track_id", "desc"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def _run(oracle, ctx, case, imgs, r, tracks=None, ids=None, **kw):
    """Extract at strip length r, compare with the oracle and with the r = 1 run; returns the oracle's keypoints per frame."""
    d = dict(_BASE, **kw)
    n, h, w = imgs.shape
    if case not in _ref:
        ocfg = oracle.cfg(**d)
        _ref[case] = [oracle.orb_extract(ocfg, imgs[f], track_xy=None if tracks is None else tracks[f], track_id=None if ids is None else ids[f]) for f in range(n)]

    def extract(rr):
        ex = _extractor(ctx, w, h, d, n, rr, max_tracks=0 if tracks is None else 8)
        ex.extract(imgs, track_xy=tracks, track_id=ids)
        return [ex.download(f) for f in range(n)]

    if case not in _r1:
        _r1[case] = extract(1)
    got = _r1[case] if r == 1 else extract(r)
    for f in range(n):
        _same(got[f], _ref[case][f])
        for k in _KEYS:
            assert np.array_equal(got[f][k], _r1[case][f][k]), (f, k)
    return _ref[case]


def _inner_flags(oracle, d, img):
    """Per output slot of a frame without tracker points: does the keypoint's 45 x 48-byte window lie inside its level (k_describe's test)?"""
    ocfg = oracle.cfg(**d)
    levels, _ = oracle.build_pyramid(ocfg, img)
    quotas = oracle.level_quotas(d["levels"], d["scale_factor"], d["max_kpts"])
    flags, octs = [], []
    for l in range(d["levels"]):
        h, w = levels[l].shape
        xs, ys, _ = oracle.detect_level(levels[l], d["fast_threshold"], int(quotas[l]))
        flags.append((xs >= 23) & (xs + 24 < w) & (ys >= 22) & (ys + 22 < h))
        octs.append(np.full(len(xs), l, np.int32))
    return np.concatenate(flags), np.concatenate(octs)


@pytest.mark.parametrize("r", _RS)
@pytest.mark.parametrize("name", list(_SINGLE))
def test_single_frames(oracle, ctx, name, r):
    w, h, levels, thr, max_kpts, kind, seed = _SINGLE[name]
    img = _frame(oracle, kind, w, h, seed)
    kw = dict(levels=levels, fast_threshold=thr, max_kpts=max_kpts)
    want, = _run(oracle, ctx, name, img[None], r, **kw)
    total = len(want["x"])
    print("%s r=%d: %d keypoints, %d in the last strip" % (name, r, total, total % (4 * r)))
    assert total == {"96x80-3": 86, "96x80-4": 73, "200x150-4": 418, "200x150-3": 292}[name]
    if name != "200x150-3":
        assert total % (4 * r) != 0                 # a ragged last strip: waves with fewer than r keypoints (292 = 4 x 73 is the full case at r = 1)
    inner, octs = _inner_flags(oracle, dict(_BASE, **kw), img)
    assert len(inner) == total and np.array_equal(octs, want["octave"])
    assert inner.any() and (~inner).any()
    if r >= 2 and w == 200:
        s = np.arange(total - 4)
        same_strip = s // (4 * r) == (s + 4) // (4 * r)         # slots s and s + 4 are consecutive trips of one wave
        to_border = int((same_strip & inner[s] & ~inner[s + 4]).sum()); to_inner = int((same_strip & ~inner[s] & inner[s + 4]).sum())
        print("    inside strips: %d inner -> border, %d border -> inner" % (to_border, to_inner))
        assert to_border > 0 and to_inner > 0


@pytest.mark.parametrize("r", _RS)
def test_fewer_than_four_keypoints(oracle, ctx, r):
    img = _frame(oracle, "noise", 96, 80, 1)
    want, = _run(oracle, ctx, "tiny", img[None], r, levels=1, fast_threshold=20, max_kpts=5)
    assert len(want["x"]) == 3                      # one workgroup, its fourth wave idle


@pytest.mark.parametrize("r", _RS)
def test_batch_with_a_blank_middle_frame(oracle, ctx, r):
    imgs = np.stack([_frame(oracle, "noise", 200, 150, 3), _frame(oracle, "blank", 200, 150, 0), _frame(oracle, "synth", 200, 150, 4)])
    want = _run(oracle, ctx, "batch3", imgs, r, levels=4, fast_threshold=20, max_kpts=700)
    totals = [len(w["x"]) for w in want]
    print("r=%d totals %s" % (r, totals))
    assert totals[1] == 0 and totals[0] > 0 and totals[2] > 0 and totals[0] != totals[2]


@pytest.mark.parametrize("r", _RS)
def test_strip_across_the_tracker_boundary(oracle, ctx, r):
    img = _frame(oracle, "noise", 200, 150, 3)
    want, = _run(oracle, ctx, "tracks", img[None], r, tracks=[_TRACKS], ids=[_TRACK_IDS], levels=4, fast_threshold=20, max_kpts=700)
    # five tracker points in slots 0 .. 4, detections behind them: for r >= 2 wave 1 of the first block walks slot 1 (a tracker point) and slot 5 (a detection)
    assert np.array_equal(want["track_id"][:5], _TRACK_IDS) and (want["track_id"][5:] == -1).all() and len(want["x"]) > 5 + 4 * r


@pytest.mark.parametrize("r", _RS)
def test_two_extracts_on_one_extractor(oracle, ctx, r):
    """Nothing of a strip survives a call: a frame of many keypoints, then one of fewer, on the same extractor."""
    d = dict(_BASE, levels=4, fast_threshold=20, max_kpts=700)
    ocfg = oracle.cfg(**d)
    a, b = _frame(oracle, "noise", 200, 150, 3), _frame(oracle, "synth", 200, 150, 4)
    if "two" not in _ref:
        _ref["two"] = [oracle.orb_extract(ocfg, a), oracle.orb_extract(ocfg, b)]
    ex = _extractor(ctx, 200, 150, d, 1, r)
    ex.extract(a[None])
    got_a = ex.download(0)
    ex.extract(b[None])
    got_b = ex.download(0)
    assert len(_ref["two"][0]["x"]) > len(_ref["two"][1]["x"]) > 0
    _same(got_a, _ref["two"][0])
    _same(got_b, _ref["two"][1])


def test_strip_length_out_of_range_is_refused(ctx):
    import mi355slam
    ex = mi355slam.OrbExtractor(ctx, 96, 80, levels=3, max_kpts=300)
    for r in (-1, 9, 100):
        with pytest.raises(mi355slam.MsError):
            ex.set_describe_strip(r)
    ex.set_describe_strip(0)
