"""CPU only: what k_resize's shared-row path rests on.  In the 720p and the 640 x 480 pyramid (8 levels, 1.2) the five destination rows of
every group read six or seven consecutive source rows: d_r = sy0[r] - sy0[0] is r or r + 1 and never falls back."""
import numpy as np
import pytest

import resize_rows_pattern as rp


def test_level_sizes_are_the_oracles(oracle):
    for w, h, f in ((1280, 720, 1.2), (640, 480, 1.2), (200, 150, 1.1), (200, 150, 1.5)):
        ws, hs = oracle.level_sizes(8, f, w, h)
        assert (list(ws), list(hs)) == rp.level_sizes(8, f, w, h)


@pytest.mark.parametrize("w,h", [(1280, 720), (640, 480)])
def test_every_group_of_the_pyramid_shares_its_rows(w, h):
    _, hs = rp.level_sizes(8, 1.2, w, h)
    total = shared = six = 0
    for l in range(1, 8):
        g = rp.groups(hs[l - 1], hs[l])
        assert all(x["shared"] and x["monotone"] for x in g), "level %d (%d -> %d rows)" % (l, hs[l - 1], hs[l])
        total += len(g)
        shared += sum(x["shared"] for x in g)
        six += sum(x["switch"] == rp.ROWS for x in g)
    print("%dx%d: %d of %d groups on the shared path (%.3f), %d of them with six source rows" % (w, h, shared, total, shared / total, six))
    assert shared == total


def test_the_two_largest_720p_levels_read_six_rows_per_group():
    """720 -> 600 -> 500 rows is an exact 1.2: every group starts at the same phase, d_4 = 4, and ten tap-row loads become six."""
    _, hs = rp.level_sizes(8, 1.2, 1280, 720)
    assert hs[:3] == [720, 600, 500]
    for l in (1, 2):
        assert all(x["switch"] == rp.ROWS and x["rows"] == rp.ROWS for x in rp.groups(hs[l - 1], hs[l]))


def test_other_ratios_fall_back():
    assert not all(x["shared"] for x in rp.groups(150, 100))      # 1.5: d_2 = 3
    assert all(x["shared"] for x in rp.groups(150, 136))          # 1.1 stays within {r, r + 1}
    sy0, sy1 = rp.row_taps(150, 100)
    assert np.all(sy1 == np.minimum(sy0 + 1, 149))


@pytest.mark.parametrize("sh,dh", [(720, 600), (500, 417), (119, 99), (99, 83), (150, 136), (150, 100), (67, 44), (480, 400), (278, 231)])
def test_the_loaded_rows_are_the_tables_rows(sh, dh):
    """What the kernel relies on once a group has passed its test: with rows min(s0 + i, sh - 1) loaded for i = 0 .. 6, row r's taps are
    loaded rows d_r and d_r + 1 -- including the last group, whose loaded rows run into the clamp."""
    sy0, sy1 = rp.row_taps(sh, dh)
    for k, g in enumerate(rp.groups(sh, dh)):
        if not g["shared"]:
            continue
        s0 = int(sy0[rp.ROWS * k])
        loaded = [min(s0 + i, sh - 1) for i in range(7)]
        for r in range(g["rows"]):
            d = int(sy0[rp.ROWS * k + r]) - s0
            assert d <= (5 if g["switch"] < rp.ROWS else 4)
            assert loaded[d] == sy0[rp.ROWS * k + r] and loaded[d + 1] == sy1[rp.ROWS * k + r]
