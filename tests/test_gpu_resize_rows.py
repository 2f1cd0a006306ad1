"""GPU parity of k_resize's shared-row path: every level bit-exact against the oracle's pyramid, on small frames chosen so that each
branch of the path runs (tests/resize_rows_pattern.py rebuilds the row pattern on the CPU and the test checks that the chosen sizes
really show what they are named for).

  144 x 120, 3 levels       120 -> 100 rows is an exact 1.2: six source rows per group everywhere (d_4 = 4); 100 -> 83 ends in a group of 3
  333 x 119, 3 levels, x 2  119 -> 99 -> 83 rows: seven-row groups with the switch to d_r = r + 1 at every r = 1 .. 4 beside six-row groups, last
                            groups of 4 and 3 rows whose loaded rows clamp at the source's last row; 278 px = a full wave and an edge wave,
                            231 px = one edge wave; two frames in the batch
  200 x 150, 4 levels, 1.1  every group shares its rows at this ratio too
  200 x 150, 4 levels, 1.5  d_2 = 3: the general path, beside the few (short last) groups that pass the test, in the same launch
  640 x 480, 4 levels       the largest: several workgroups per level in both directions

Not reachable: the path's three-dword form for a source level narrower than 12 bytes -- the extractor refuses levels below 40 x 40, so every
edge wave here is of the `last >= 8` kind.
"""
import numpy as np
import pytest

import resize_rows_pattern as rp

pytestmark = pytest.mark.gpu

CASES = {
    "exact_1p2": dict(w=144, h=120, levels=3, f=1.2, frames=1),
    "all_switches": dict(w=333, h=119, levels=3, f=1.2, frames=2),
    "ratio_1p1": dict(w=200, h=150, levels=4, f=1.1, frames=1),
    "ratio_1p5": dict(w=200, h=150, levels=4, f=1.5, frames=1),
    "vga": dict(w=640, h=480, levels=4, f=1.2, frames=1),
}


def _groups(c):
    _, hs = rp.level_sizes(c["levels"], c["f"], c["w"], c["h"])
    return [g for l in range(1, c["levels"]) for g in rp.groups(hs[l - 1], hs[l])]


def test_the_cases_show_what_they_are_named_for():
    g = _groups(CASES["exact_1p2"])
    assert all(x["shared"] for x in g) and all(x["switch"] == rp.ROWS for x in g[:20]) and g[-1]["rows"] == 3
    g = _groups(CASES["all_switches"])
    full = [x for x in g if x["rows"] == rp.ROWS]
    assert all(x["shared"] for x in g) and {x["switch"] for x in full} == {1, 2, 3, 4, 5}
    assert sorted(x["rows"] for x in g if x["rows"] < rp.ROWS) == [3, 4] and any(x["clamped"] for x in g)
    ws, _ = rp.level_sizes(3, 1.2, 333, 119)
    assert ws[1] > 256 > ws[2]
    assert all(x["shared"] for x in _groups(CASES["ratio_1p1"]))
    g = _groups(CASES["ratio_1p5"])
    assert 0 < sum(x["shared"] for x in g) < len(g) / 2


@pytest.mark.parametrize("name", list(CASES))
def test_levels_bit_exact(oracle, ctx, name):
    import mi355slam
    c = CASES[name]
    imgs = np.stack([oracle.synth_frame(c["w"], c["h"], 3100 + 7 * i, 3 * i, i) for i in range(c["frames"])])
    ex = mi355slam.OrbExtractor(ctx, c["w"], c["h"], levels=c["levels"], scale_factor=c["f"], max_kpts=500, max_batch=c["frames"])
    ex.extract(imgs)
    ocfg = oracle.cfg(levels=c["levels"], scale_factor=c["f"], max_kpts=500)
    for f in range(c["frames"]):
        levels, _ = oracle.build_pyramid(ocfg, imgs[f])
        for l in range(c["levels"]):
            assert ex.level_size(l) == (levels[l].shape[1], levels[l].shape[0])
            got = ex.download_level(f, l, False)
            bad = np.argwhere(got != levels[l])
            assert len(bad) == 0, "frame %d level %d: %d pixels differ, first at (row, col) %s" % (f, l, len(bad), bad[0])
