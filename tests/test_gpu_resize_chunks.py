"""GPU parity of k_resize8 (8 destination pixels per lane; slam-module_amd/csrc/resize_plan.h): every level bit-exact against the oracle's pyramid
for px in {4, 8} x map in {tiles across the device, a frame per XCD} forced through OrbExtractor.set_resize_plan, and for the automatic plan, on
small frames chosen so that each branch runs (tests/resize_chunks_cases.py rebuilds the column rule on the CPU; a CPU test here checks that the
sizes show what they are named for).

  333 x 119, 3 levels, 1.2, 2 / 3 / 5 / 11 frames   widths 277 and 231 (w mod 8 = 5 and 7): 35 and 29 chunks, one edge wave per row group; by frame, 8
                                                    workgroups per tile of which 2, 3, 5 work (the rest are masked), and with 11 frames a second
                                                    layer of 3; seven-row groups and clamped last groups
  144 x 120, 3 levels, 1.2                          level 1 is 120 px, a multiple of 8; six-row groups only
  640 x 480, 4 levels, 1.2, 2 frames                67 / 56 / 47 chunks: a second wave of 3 lanes, several workgroups in both directions (by frame: the
                                                    tile index is divided by 2 tiles across)
  200 x 150, 4 levels, 1.1                          eligible at another ratio
  200 x 150, 4 levels, 1.5                          not eligible: px = 8 runs the 4-pixel kernel, same pixels
  640 x 480, 2 frames, whole extraction             px = 4 against px = 8: identical keypoints and descriptors (a reader of the pitch padding would differ)
  320 x 240, 3 levels, device-resident frames       level 0 used in place (16-aligned pointer, row_stride = w), the path the benchmark takes
"""
import numpy as np
import pytest

import resize_chunks_cases as rc
import resize_rows_pattern as rp

CASES = rc.CASES


def test_the_cases_show_what_they_are_named_for():
    p = rc.level_plan(CASES["odd_widths_2"])
    assert [x["dw"] for x in p] == [277, 231] and [x["dw"] % 8 for x in p] == [5, 7] and all(x["eligible"] for x in p)
    assert all(x["chunks"] <= 64 for x in p) and all(any(rc.edge_lanes(x["sw"], x["dw"])) for x in p)            # one wave per row group, an edge wave
    g = [g for x in p for g in rp.groups(x["sh"], x["dh"])]
    assert any(x["switch"] < rp.ROWS and x["rows"] == rp.ROWS for x in g) and any(x["clamped"] for x in g) and any(x["rows"] < rp.ROWS for x in g)
    assert [CASES[n]["frames"] for n in ("odd_widths_2", "odd_widths_3", "odd_widths_5", "odd_widths_11")] == [2, 3, 5, 11]      # by frame: masked blocks, and a second layer of 3
    p = rc.level_plan(CASES["multiple_of_8"])
    assert p[0]["dw"] == 120 and all(x["eligible"] for x in p)
    assert all(x["switch"] == rp.ROWS for x in rp.groups(p[0]["sh"], p[0]["dh"]))
    p = rc.level_plan(CASES["vga"])
    assert [x["chunks"] for x in p] == [67, 56, 47] and all(x["eligible"] for x in p) and p[0]["dh"] > 4 * rp.ROWS * 2        # 2 tiles across, > 2 down
    assert all(x["eligible"] for x in rc.level_plan(CASES["ratio_1p1"]))
    assert not any(x["eligible"] for x in rc.level_plan(CASES["ratio_1p5"]))


_pyramids = {}


def _case(oracle, name):
    """frames and the oracle's pyramids of a case, computed once"""
    if name not in _pyramids:
        c = CASES[name]
        imgs = np.stack([oracle.synth_frame(c["w"], c["h"], 4100 + 7 * i, 3 * i, i) for i in range(c["frames"])])
        ocfg = oracle.cfg(levels=c["levels"], scale_factor=c["f"], max_kpts=500)
        _pyramids[name] = (imgs, [oracle.build_pyramid(ocfg, imgs[f])[0] for f in range(c["frames"])])
    return _pyramids[name]


def _check_levels(ex, want, tag):
    for f, levels in enumerate(want):
        for l, ref in enumerate(levels):
            assert ex.level_size(l) == (ref.shape[1], ref.shape[0])
            got = ex.download_level(f, l, False)
            bad = np.argwhere(got != ref)
            assert len(bad) == 0, "%s frame %d level %d: %d pixels differ, first at (row, col) %s" % (tag, f, l, len(bad), bad[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_levels_bit_exact_for_every_plan(oracle, ctx, name):
    import mi355slam
    c = CASES[name]
    imgs, want = _case(oracle, name)
    ex = mi355slam.OrbExtractor(ctx, c["w"], c["h"], levels=c["levels"], scale_factor=c["f"], max_kpts=500, max_batch=c["frames"])
    for px, m in rc.PLANS + [(0, 0)]:
        ex.set_resize_plan(px, m)
        ex.extract(imgs)
        _check_levels(ex, want, "px %d map %d" % (px, m))


@pytest.mark.gpu
def test_automatic_plan_on_a_launch_that_fills_the_device(oracle, ctx):
    """261 frames (4 different ones) of 333 x 119: both levels are 5 tiles x 261 frames = 1305 workgroups, past the launch-size gate (1280), so the
    automatic plan runs the 8-pixel kernel with a frame per XCD, and 3 of the last layer's 8 workgroups per tile are masked."""
    import mi355slam
    n, c = 261, CASES["odd_widths_5"]
    p = rc.level_plan(c)
    assert all(-(-x["chunks"] // 64) * -(-x["dh"] // (4 * rp.ROWS)) * n >= 1280 for x in p) and n >= 32 and n % 8 == 5
    imgs, want = _case(oracle, "odd_widths_5")
    pick = [(3 * i) % 4 for i in range(n)]
    ex = mi355slam.OrbExtractor(ctx, c["w"], c["h"], levels=c["levels"], scale_factor=c["f"], max_kpts=100, max_batch=n)
    buf = ctx.upload(imgs[pick])                       # frames on the device: one call for all 261 (host frames would come in four pieces below the gate)
    ex.extract(buf, n_frames=n, frame_stride=c["w"] * c["h"], row_stride=c["w"])
    _check_levels(ex, [want[i] for i in pick], "automatic plan")
    buf.free()


@pytest.mark.gpu
def test_keypoints_and_descriptors_do_not_depend_on_the_kernel(ctx, oracle):
    import mi355slam
    imgs, _ = _case(oracle, "vga")
    out = {}
    for px in (4, 8):
        ex = mi355slam.OrbExtractor(ctx, 640, 480, max_batch=2)
        ex.set_resize_plan(px, 2)
        ex.extract(imgs)
        out[px] = [ex.download(f) for f in range(2)]
    for f in range(2):
        assert len(out[4][f]["x"]) > 500
        for k in out[4][f]:
            assert np.array_equal(out[4][f][k].view(np.uint32) if out[4][f][k].dtype == np.float32 else out[4][f][k],
                                  out[8][f][k].view(np.uint32) if out[8][f][k].dtype == np.float32 else out[8][f][k]), "frame %d: %s differs" % (f, k)


@pytest.mark.gpu
def test_device_resident_level0_in_place(ctx, oracle):
    import mi355slam
    w, h, n = 320, 240, 3
    imgs = np.stack([oracle.synth_frame(w, h, 5200 + i, 2 * i, i) for i in range(n)])
    ocfg = oracle.cfg(levels=3, scale_factor=1.2, max_kpts=500)
    want = [oracle.build_pyramid(ocfg, imgs[f])[0] for f in range(n)]
    buf = ctx.upload(imgs)
    assert buf.ptr % 16 == 0 and w % 16 == 0
    ex = mi355slam.OrbExtractor(ctx, w, h, levels=3, scale_factor=1.2, max_kpts=500, max_batch=n)
    for px, m in rc.PLANS:
        ex.set_resize_plan(px, m)
        ex.extract(buf, n_frames=n, frame_stride=w * h, row_stride=w)
        _check_levels(ex, want, "px %d map %d" % (px, m))
    buf.free()


@pytest.mark.gpu
def test_plan_values_are_checked(ctx):
    import mi355slam
    ex = mi355slam.OrbExtractor(ctx, 96, 80, levels=3, max_kpts=300)
    for px, m in ((1, 0), (16, 0), (-4, 0), (8, 3), (8, 8), (0, -1)):
        with pytest.raises(mi355slam.MsError):
            ex.set_resize_plan(px, m)
    ex.set_resize_plan(0, 0)
