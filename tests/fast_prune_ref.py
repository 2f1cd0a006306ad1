"""CPU model of k_fast's raised threshold ("skip corners that cannot reach their level's quota").

The selection of a (frame, level) looks at the K strongest candidates only (K = quota, or min(4 quota, 4096) with a minimum distance), and keys
order by score first.  Once K candidates of score > sigma are known, a tile may run all of FAST -- corner test and 3x3 NMS -- with
max(threshold, sigma).  The model runs the tiles of a level in a given order, `in_flight` at a time; every tile of a group reads the score
histogram as it stood when the group started (the stalest read the device can make), works with the bound that histogram gives, and adds the
candidates it found when the group is done.  `select` is the selection's first step: the K smallest keys.

`score_map` is the FAST-9/16 score in numpy (the oracle's fast_score_map calls into C once per pixel, too slow for a batch); the CPU test holds
the two equal.
"""
import numpy as np

RING_DX = (0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1)
RING_DY = (3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3)
MAX_SELECT = 4096                # the selection's capacity


def score_map(img):
    """FAST score of every position with a full ring (3 px from the border), 0 elsewhere and where no arc of 9 is all darker / all brighter."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return out
    c = img[3:h - 3, 3:w - 3].astype(np.int16)
    d = np.stack([c - img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx].astype(np.int16) for dx, dy in zip(RING_DX, RING_DY)])

    def arcs(a, op):             # op over every run of 9 consecutive ring pixels: runs of 2, 4, 8, then one more
        a2 = op(a, np.roll(a, -1, 0)); a4 = op(a2, np.roll(a2, -2, 0)); a8 = op(a4, np.roll(a4, -4, 0))
        return op(a8, np.roll(a, -8, 0))

    best = np.maximum(arcs(d, np.minimum).max(0), -arcs(d, np.maximum).min(0))
    out[3:h - 3, 3:w - 3] = np.maximum(best, 0)
    return out


def nms_keys(scores, thr, x0=0, y0=0, x1=None, y1=None):
    """Keys ((255 - score) << 24 | y * w + x) of the strict 3x3 maxima of `scores` above `thr` inside [x0, x1) x [y0, y1).  Scores <= thr count as 0,
    also for the neighbours outside the rectangle (a tile's halo): exactly what a tile working with threshold `thr` sees."""
    h, w = scores.shape
    x1 = w if x1 is None else x1
    y1 = h if y1 is None else y1
    s = np.zeros((y1 - y0 + 2, x1 - x0 + 2), np.int32)
    ya, yb, xa, xb = max(y0 - 1, 0), min(y1 + 1, h), max(x0 - 1, 0), min(x1 + 1, w)
    s[ya - (y0 - 1):yb - (y0 - 1), xa - (x0 - 1):xb - (x0 - 1)] = scores[ya:yb, xa:xb]
    s[s <= thr] = 0
    c = s[1:-1, 1:-1]
    keep = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                keep &= c > s[1 + dy:s.shape[0] - 1 + dy, 1 + dx:s.shape[1] - 1 + dx]
    ys, xs = np.nonzero(keep)
    return ((255 - c[ys, xs]).astype(np.uint32) << np.uint32(24)) | ((ys + y0) * w + xs + x0).astype(np.uint32)


def key_scores(keys):
    return 255 - (np.asarray(keys, np.uint32) >> np.uint32(24)).astype(np.int64)


def select_count(quota, min_dist):
    """How many of the strongest candidates the selection of a level looks at."""
    return min(4 * quota, MAX_SELECT) if min_dist >= 2 else quota


def bound(hist, thr, K):
    """The largest s >= thr with at least K known candidates of score > s; thr when there is none (or nothing is to be selected)."""
    if K <= 0:
        return thr
    above = np.concatenate([np.cumsum(hist[::-1])[::-1][1:], [0]])       # above[s] = sum of hist[s + 1:]
    ok = np.nonzero(above >= K)[0]
    return max(thr, int(ok[-1])) if len(ok) else thr


def tiles_of(w, h, tw, th):
    return [(x, y, min(x + tw, w), min(y + th, h)) for y in range(0, h, th) for x in range(0, w, tw)]


def select(keys, K):
    return np.sort(np.asarray(keys, np.uint32))[:max(K, 0)]


def pruned_keys(scores, thr, K, tiles, order, in_flight):
    """Candidates of one level with the raised threshold.  Returns (keys, bounds used per tile in processing order)."""
    hist = np.zeros(256, np.int64)
    out, used = [], []
    for g in range(0, len(order), in_flight):
        t = bound(hist, thr, K)                                          # every tile of the group read the histogram before any of them added to it
        found = [nms_keys(scores, t, *tiles[i]) for i in order[g:g + in_flight]]
        used += [t] * len(found)
        for k in found:
            np.add.at(hist, key_scores(k), 1)
            out.append(k)
    return (np.concatenate(out) if out else np.zeros(0, np.uint32)), used


def stamp_frame(w, h, n_strong=0, step=12, margin=24):
    """A flat frame of identical corner stamps: single pixels 60 above the background on a grid, each one FAST corner of score exactly 60 (the whole
    ring is 60 darker, and no other position has 9 ring pixels in a row that differ from it).  `n_strong` more single pixels, 90 above, sit between the
    grid points: corners of score exactly 90.  Returns (frame, number of grid stamps)."""
    img = np.full((h, w), 100, np.uint8)
    ys, xs = np.arange(margin, h - margin, step), np.arange(margin, w - margin, step)
    img[np.ix_(ys, xs)] = 160
    between = [(y + step // 2, x + step // 2) for y in ys[:-1] for x in xs[:-1]]
    assert n_strong <= len(between)
    pick = np.random.default_rng(5).permutation(len(between))[:n_strong]
    for i in pick:
        img[between[i]] = 190
    return img, len(ys) * len(xs)
