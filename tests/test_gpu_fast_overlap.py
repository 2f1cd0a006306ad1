"""GPU parity of k_fast in two launches -- level 0's tiles on the extractor's side stream beside the resize chain, the other levels' behind it
(csrc/orb.hip: orb_enqueue_kernels; OrbExtractor.set_fast_overlap: 0 = automatic, 1 = never, 2 = always) -- against the single launch.  Compared
byte for byte: x, y, angle, octave, descriptors, track ids and the count of every frame, download_detections of every (frame, level), and
last_candidate_counts.  Every case also reads last_fast_launches, so that it is the split (or the single launch) it is there for that ran.

The cases: one frame below the pruning rule (both parts run the plain kernel); a batch of three; frames in DEVICE memory, the benchmark's path,
in automatic mode -- the smallest batch for which the rule itself splits, worked out here from level_sizes and the tile cover, one frame fewer
(one launch), and a larger batch of larger frames, with the pruning instantiation in both parts; three different frame sets enqueued back to back
on one extractor without a host wait (a call's counters, bins and lists against the next call's part-launches); host frames in four pieces (the
chunked path), forced to split and, in automatic mode, left alone; a one-level pyramid, which must keep its single launch; a mode out of range.

last_candidate_counts under pruning: how many candidates a pruning launch appends depends on what each tile had seen of the others when it ran
(include/mi355slam.h says so at ms_orb_last_candidate_counts: "vary from run to run; the selected keypoints do not"), between two runs of the
single launch already.  Where the launches do not prune -- every case but the device-memory ones -- the counts are compared exactly.  In those
each mode's counts are held between what must be there in any run, the level's selected detections, and what an unpruned one-frame call finds;
and both modes' keypoints are also held against those one-frame calls.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_PRUNE_MIN_BLOCKS = 2 * 4 * 256         # csrc/orb_geom.h: kFastPruneMinBlocks
_KEYS = ("x", "y", "angle", "octave", "desc", "track_id")


def _level_tiles(w, h):
    """Workgroups of k_fast on a level of w x h (csrc/fast_tiles.h: cover), counted from its rules: full columns of 248 outputs in rows of 30,
    the remaining width in the layouts (248 x 30, 120 x 62, 56 x 126 outputs) that need the fewest workgroups."""
    out_w = {1: 248, 2: 120, 4: 56}
    rows = lambda s: (h - 3 + 32 * s - 2 - 1) // (32 * s - 2)

    def strip(r):
        return min(rows(s) + (strip(r - out_w[s]) if r > out_w[s] else 0) for s in (1, 2, 4))

    full, r = divmod(w - 3, 248)
    return full * rows(1) + (strip(r) if r else 0)


def _tiles(levels, w, h):
    import mi355slam
    return [_level_tiles(int(a), int(b)) for a, b in zip(*mi355slam.level_sizes(levels, 1.2, w, h))]


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _frames(n, w, h, seed):
    """n frames: the benchmark's synthetic sequences, every third frame noise (many more corners than any quota)."""
    import synth
    out = synth.synth_sequences(n, w, h, seed, n_seq=(n + 7) // 8)
    for f in range(2, n, 3):
        out[f] = _noise(w, h, seed + f)
    return out


def _extractor(ctx, w, h, levels, max_batch, mode, max_kpts=500):
    import mi355slam
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=levels, scale_factor=1.2, max_kpts=max_kpts, fast_threshold=20, max_batch=max_batch)
    ex.set_fast_overlap(mode)
    return ex


def _snapshot(ex, levels):
    n = ex.n_frames
    return dict(frames=[ex.download(f) for f in range(n)], cand=ex.last_candidate_counts().copy(), launches=ex.last_fast_launches(),
                dets=[[ex.download_detections(f, l) for l in range(levels)] for f in range(n)])


def _same_frames(got, want):
    assert len(got["frames"]) == len(want["frames"])
    for f, (a, b) in enumerate(zip(got["frames"], want["frames"])):
        assert len(a["x"]) == len(b["x"]), (f, len(a["x"]), len(b["x"]))
        for k in _KEYS:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (f, k)
    for f, (da, db) in enumerate(zip(got["dets"], want["dets"])):
        for l, (a, b) in enumerate(zip(da, db)):
            for i in range(3):
                assert a[i].tobytes() == b[i].tobytes(), (f, l, "xys"[i])


def _same(got, want):
    _same_frames(got, want)
    assert got["cand"].tobytes() == want["cand"].tobytes(), (got["cand"], want["cand"])


def _both_modes(ctx, imgs, levels, mode, device=False, **kw):
    """The frames through an extractor in `mode` and through one in mode 1; device: from device memory, in place (else a host array)."""
    n, h, w = imgs.shape
    out = []
    for m in (mode, 1):
        ex = _extractor(ctx, w, h, levels, n, m, **kw)
        if device:
            dev = ctx.upload(imgs)
            ex.extract(dev, n_frames=n, frame_stride=w * h, row_stride=w)
            out.append(_snapshot(ex, levels))
            dev.free()
        else:
            ex.extract(imgs)
            out.append(_snapshot(ex, levels))
        ex.close()
    return out


def test_one_frame_below_the_pruning_rule(ctx):
    imgs = _frames(1, 200, 150, 3)
    assert sum(_tiles(3, 200, 150)) <= _PRUNE_MIN_BLOCKS
    got, want = _both_modes(ctx, imgs, 3, 2)
    assert got["launches"] == (2, 0) and want["launches"] == (1, 0)
    assert len(want["frames"][0]["x"]) > 100 and (want["cand"] > 0).all()
    _same(got, want)


def test_batch_of_three(ctx):
    imgs = _frames(3, 96, 80, 11)
    got, want = _both_modes(ctx, imgs, 4, 2)
    assert got["launches"] == (2, 0) and want["launches"] == (1, 0)
    assert all(len(f["x"]) > 0 for f in want["frames"])
    _same(got, want)


def _automatic_on_device(ctx, w, h, levels, n, max_kpts, seed):
    """n frames in device memory, mode 0 against mode 1: the split with the pruning kernel in both parts.  Returns (got, want)."""
    tiles = _tiles(levels, w, h)
    assert n * min(tiles[0], sum(tiles[1:])) > _PRUNE_MIN_BLOCKS
    imgs = _frames(n, w, h, seed)
    got, want = _both_modes(ctx, imgs, levels, 0, device=True, max_kpts=max_kpts)      # max_batch = n: the side stream comes from ms_orb_create's own rule
    assert got["launches"] == (2, 2), got["launches"]                    # level 0 and the other levels, both k_fast<true>
    assert want["launches"] == (1, 1), want["launches"]
    _same_frames(got, want)
    # one frame at a time prunes nothing: all candidates of every level, and the keypoints both batch runs must give
    one = _extractor(ctx, w, h, levels, 1, 1, max_kpts=max_kpts)
    full = np.zeros((n, levels), np.int32)
    for f in range(n):
        one.extract(imgs[f])
        assert one.last_fast_launches() == (1, 0)
        full[f] = one.last_candidate_counts()[0]
        alone = one.download(0)
        for k in _KEYS:
            assert alone[k].tobytes() == want["frames"][f][k].tobytes(), (f, k)
    one.close()
    kept = np.array([[len(want["dets"][f][l][0]) for l in range(levels)] for f in range(n)], np.int32)
    print("%dx%d, n = %d frames, tiles per level %s; candidates per call: unpruned %d, single launch %d, split %d, selected %d"
          % (w, h, n, tiles, full.sum(), want["cand"].sum(), got["cand"].sum(), kept.sum()))
    assert (kept < full).any()                                           # there was something a raised threshold could skip
    for run in (got, want):
        assert (kept <= run["cand"]).all() and (run["cand"] <= full).all()
    return got, want


def test_smallest_batch_the_automatic_rule_splits(ctx):
    w, h, levels = 320, 200, 4
    tiles = _tiles(levels, w, h)
    part = min(tiles[0], sum(tiles[1:]))
    n = _PRUNE_MIN_BLOCKS // part + 1                                   # the first n with n x (the smaller part) > kFastPruneMinBlocks
    assert (n - 1) * part <= _PRUNE_MIN_BLOCKS < n * part
    _automatic_on_device(ctx, w, h, levels, n, 500, 100)
    # one frame fewer, on the same kind of extractor: one launch, still the pruning kernel
    imgs = _frames(n - 1, w, h, 100)
    ex = _extractor(ctx, w, h, levels, n, 0)
    dev = ctx.upload(imgs)
    ex.extract(dev, n_frames=n - 1, frame_stride=w * h, row_stride=w)
    ctx.sync()
    assert ex.last_fast_launches() == (1, 1)
    dev.free()
    ex.close()


def test_automatic_split_well_above_the_rule(ctx):
    """96 frames of 640 x 480: about twice the workgroups of the rule in level 0 alone, so that later tiles of a frame do see what earlier ones found."""
    _automatic_on_device(ctx, 640, 480, 4, 96, 300, 300)


def test_three_calls_back_to_back(ctx):
    """Calls 1 .. k on one extractor in mode 2 without a host wait in between, for k = 1, 2, 3; the last call's results against the single launch."""
    w, h, levels = 200, 150, 3
    sets = [_frames(3, w, h, 40), _frames(3, w, h, 50)[::-1].copy(), np.stack([_noise(w, h, 7), np.full((h, w), 90, np.uint8), _noise(w, h, 8)])]
    ref = _extractor(ctx, w, h, levels, 3, 1)
    want = []
    for s in sets:
        ref.extract(s)
        want.append(_snapshot(ref, levels))
    assert len({int(s["cand"].sum()) for s in want}) == 3 and len(want[2]["frames"][1]["x"]) == 0      # three different loads, a blank frame in the last
    ex = _extractor(ctx, w, h, levels, 3, 2)
    keep = []                                                            # the host copies stay alive while their uploads are in flight
    for k in range(3):
        for s in sets[:k + 1]:
            keep.append(s.copy())
            ex.extract(keep[-1])
        got = _snapshot(ex, levels)
        assert got["launches"] == (2, 0)
        _same(got, want[k])
    ex.close()
    ref.close()


def test_pinned_host_frames_in_pieces(ctx):
    """34 frames from page-locked memory with profiling off: four pieces of 9, 9, 9 and 7 frames.  Mode 2 gives each piece its own fork and join
    (eight launches), twice, so that the second call's copies wait for the first call's pieces; automatic mode leaves the pieces of a host batch
    alone (four launches), from pinned and from pageable memory."""
    n, w, h, levels = 34, 96, 80, 3
    imgs = ctx.pinned((n, h, w))
    imgs[:] = _frames(n, w, h, 200)
    out = []
    for m in (2, 1, 0):
        ex = _extractor(ctx, w, h, levels, n, m)
        ex.extract(imgs)
        ex.extract(imgs)
        out.append(_snapshot(ex, levels))
        if m == 0:
            ex.extract(np.array(imgs))
            assert ex.last_fast_launches() == (4, 0)
        ex.close()
    assert [o["launches"] for o in out] == [(8, 0), (4, 0), (4, 0)]
    assert sum(len(f["x"]) for f in out[1]["frames"]) > n
    _same(out[0], out[1])
    _same(out[2], out[1])
    # and the same frames as one piece (profiling on) from pageable memory
    ex = _extractor(ctx, w, h, levels, n, 2)
    ex.set_profiling(True)
    ex.extract(np.array(imgs))
    got = _snapshot(ex, levels)
    assert got["launches"] == (2, 0)
    _same(got, out[1])
    assert sum(ex.stage_ms().values()) > 0
    ex.close()


def test_one_level_keeps_its_single_launch(ctx):
    imgs = _frames(2, 100, 100, 5)
    got, want = _both_modes(ctx, imgs, 1, 2)
    assert got["launches"] == (1, 0) and want["launches"] == (1, 0)
    assert len(want["frames"][0]["x"]) > 0
    _same(got, want)


def test_mode_out_of_range_is_refused(ctx):
    import mi355slam
    ex = mi355slam.OrbExtractor(ctx, 96, 80, levels=3, max_kpts=300)
    for mode in (3, -1, 4, 100):
        with pytest.raises(mi355slam.MsError):
            ex.set_fast_overlap(mode)
    for mode in (0, 1, 2, 0):
        ex.set_fast_overlap(mode)
    ex.close()
