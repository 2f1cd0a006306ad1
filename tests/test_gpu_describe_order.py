"""GPU parity of k_describe's block and visit order (csrc/describe_strips.h: remap; csrc/describe_order.h; k_slots): modes {0, 1, 2, 3} of
OrbExtractor.set_describe_order (bit 0 = XCD-contiguous blocks, bit 1 = spatial visit order) x forced strips r in {1, 4}.  Every run is bit-exact
against the CPU oracle (x, y, angle, octave, track id and all 8 descriptor words) and equal to the mode 0 run of the same r, array for array: only
which workgroup describes which slot changes, never what lands in the slot.

What a case is there for is asserted from the oracle's output: a block count that is no multiple of 8 (96 x 80: 86 keypoints + capacity padding),
several levels with different totals (200 x 150: 154 / 101 / 95 / 68), a level of 508 detections (more than one trip of k_slots' 256 threads, just
under the next power of two of its sort), fewer than 8 blocks, a blank middle frame in a batch, tracker points whose slots must not move, and two
extracts of different frames on one extractor.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_BASE = dict(scale_factor=1.2, lk_track_level=0, min_distance=0.0)
_KEYS = ("x", "y", "angle", "octave", "desc", "track_id")
_MODES = [0, 1, 2, 3]
_RS = [1, 4]
_SINGLE = {                                     # name -> (w, h, levels, threshold, max_kpts, seed), noise frames
    "96x80-3": (96, 80, 3, 20, 300, 1),
    "200x150-4": (200, 150, 4, 20, 700, 3),
    "320x240-2": (320, 240, 2, 20, 1200, 5),
}
_TRACKS = np.array([[60.5, 50.25], [100.0, 75.0], [21.0, 70.0], [150.75, 120.5], [178.0, 20.0]], np.float32)   # two of them within 24 px of a border
_TRACK_IDS = np.array([11, 12, 13, 14, 15], np.int32)
_ref = {}                                       # case -> the oracle's keypoints per frame, computed once
_m0 = {}                                        # (case, r) -> the mode 0 run's arrays per frame


def _frame(oracle, kind, w, h, seed):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "blank":
        return np.full((h, w), 90, np.uint8)
    return oracle.synth_frame(w, h, seed)


def _extractor(ctx, w, h, d, n, mode, r, max_tracks=0):
    import mi355slam
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=d["levels"], scale_factor=d["scale_factor"], max_kpts=d["max_kpts"], lk_track_level=0,
                                fast_threshold=d["fast_threshold"], max_tracks=max_tracks, max_batch=n, min_distance=0.0)
    ex.set_describe_strip(r)
    ex.set_describe_order(mode)
    return ex


def _same(got, want):
    assert len(got["x"]) == len(want["x"])
    for k in ("x", "y", "angle"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    for k in ("octave", "track_id", "desc"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def _run(oracle, ctx, case, imgs, mode, r, tracks=None, ids=None, **kw):
    """Extract in the given mode at strip length r, compare with the oracle and with the mode 0 run; returns the oracle's keypoints per frame."""
    d = dict(_BASE, **kw)
    n, h, w = imgs.shape
    if case not in _ref:
        ocfg = oracle.cfg(**d)
        _ref[case] = [oracle.orb_extract(ocfg, imgs[f], track_xy=None if tracks is None else tracks[f], track_id=None if ids is None else ids[f]) for f in range(n)]

    def extract(m):
        ex = _extractor(ctx, w, h, d, n, m, r, max_tracks=0 if tracks is None else 8)
        ex.extract(imgs, track_xy=tracks, track_id=ids)
        return [ex.download(f) for f in range(n)]

    if (case, r) not in _m0:
        _m0[(case, r)] = extract(0)
    got = _m0[(case, r)] if mode == 0 else extract(mode)
    for f in range(n):
        _same(got[f], _ref[case][f])
        for k in _KEYS:
            assert np.array_equal(got[f][k], _m0[(case, r)][f][k]), (f, k)
    return _ref[case]


@pytest.mark.parametrize("r", _RS)
@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("name", list(_SINGLE))
def test_single_frames(oracle, ctx, name, mode, r):
    import mi355slam
    w, h, levels, thr, max_kpts, seed = _SINGLE[name]
    img = _frame(oracle, "noise", w, h, seed)
    want, = _run(oracle, ctx, name, img[None], mode, r, levels=levels, fast_threshold=thr, max_kpts=max_kpts)
    total = len(want["x"])
    per_level = np.bincount(want["octave"], minlength=levels).tolist()
    print("%s mode=%d r=%d: %d keypoints, levels %s" % (name, mode, r, total, per_level))
    assert total == {"96x80-3": 86, "200x150-4": 418, "320x240-2": 918}[name]
    if name == "96x80-3":
        ex = mi355slam.OrbExtractor(ctx, w, h, levels=levels, scale_factor=1.2, max_kpts=max_kpts, lk_track_level=0, fast_threshold=thr, max_batch=1, min_distance=0.0)
        blocks = (ex.capacity + 3) // 4            # the launch at r = 1: one block per four slots of the capacity
        print("    capacity %d: %d blocks at r = 1" % (ex.capacity, blocks))
        assert blocks == 75 and blocks % 8 != 0
    if name == "200x150-4":
        assert per_level == [154, 101, 95, 68]
    if name == "320x240-2":
        assert per_level[0] == 508 and 256 < per_level[0] < 512          # two trips of k_slots' block, padded to 512 in its sort


@pytest.mark.parametrize("r", _RS)
@pytest.mark.parametrize("mode", _MODES)
def test_fewer_than_eight_blocks(oracle, ctx, mode, r):
    img = _frame(oracle, "noise", 96, 80, 1)
    want, = _run(oracle, ctx, "tiny", img[None], mode, r, levels=1, fast_threshold=20, max_kpts=5)
    assert len(want["x"]) == 3                      # max_kpts 5: two blocks at r = 1, one at r = 4 -- a region that the remap leaves alone


@pytest.mark.parametrize("r", _RS)
@pytest.mark.parametrize("mode", _MODES)
def test_batch_with_a_blank_middle_frame(oracle, ctx, mode, r):
    imgs = np.stack([_frame(oracle, "noise", 200, 150, 3), _frame(oracle, "blank", 200, 150, 0), _frame(oracle, "synth", 200, 150, 4)])
    want = _run(oracle, ctx, "batch3", imgs, mode, r, levels=4, fast_threshold=20, max_kpts=700)
    totals = [len(w["x"]) for w in want]
    print("mode=%d r=%d totals %s" % (mode, r, totals))
    assert totals[1] == 0 and totals[0] > 0 and totals[2] > 0 and totals[0] != totals[2]


@pytest.mark.parametrize("r", _RS)
@pytest.mark.parametrize("mode", _MODES)
def test_tracker_slots_do_not_move(oracle, ctx, mode, r):
    img = _frame(oracle, "noise", 200, 150, 3)
    want, = _run(oracle, ctx, "tracks", img[None], mode, r, tracks=[_TRACKS], ids=[_TRACK_IDS], levels=4, fast_threshold=20, max_kpts=700)
    # five tracker points in slots 0 .. 4 in their own order, the detections behind them
    assert np.array_equal(want["track_id"][:5], _TRACK_IDS) and (want["track_id"][5:] == -1).all() and len(want["x"]) > 5 + 4 * r


@pytest.mark.parametrize("r", _RS)
@pytest.mark.parametrize("mode", _MODES)
def test_two_extracts_on_one_extractor(oracle, ctx, mode, r):
    """Nothing of a call's visit order survives it: a frame of many keypoints, then one of fewer, on the same extractor."""
    d = dict(_BASE, levels=4, fast_threshold=20, max_kpts=700)
    ocfg = oracle.cfg(**d)
    a, b = _frame(oracle, "noise", 200, 150, 3), _frame(oracle, "synth", 200, 150, 4)
    if "two" not in _ref:
        _ref["two"] = [oracle.orb_extract(ocfg, a), oracle.orb_extract(ocfg, b)]
    ex = _extractor(ctx, 200, 150, d, 1, mode, r)
    ex.extract(a[None])
    got_a = ex.download(0)
    ex.extract(b[None])
    got_b = ex.download(0)
    assert len(_ref["two"][0]["x"]) > len(_ref["two"][1]["x"]) > 0
    _same(got_a, _ref["two"][0])
    _same(got_b, _ref["two"][1])


def test_mode_out_of_range_is_refused(ctx):
    import mi355slam
    ex = mi355slam.OrbExtractor(ctx, 96, 80, levels=3, max_kpts=300)
    for mode in (-1, 4, 5, 8, 100):
        with pytest.raises(mi355slam.MsError):
            ex.set_describe_order(mode)
    for mode in (0, 1, 2, 3):
        ex.set_describe_order(mode)
