"""The row-tap pattern of k_resize's groups of five destination rows, rebuilt on the CPU (numpy; shared by two test files).

ms_orb_create builds, per destination row d of a level, the tap rows sy0 = clip(s, 0, sh - 1), sy1 = clip(s + 1, 0, sh - 1) with
s = floor(float32((d + 0.5) * sh / dh - 0.5)).  A wave of k_resize owns rows 5g .. 5g + 4; its shared-row path applies when, with
d_r = sy0[5g + r] - sy0[5g], every row that exists has d_r in {r, r + 1} and sy1 = min(sy0 + 1, sh - 1).
"""
import numpy as np

ROWS = 5     # kResizeRows


def level_sizes(levels, f, w0, h0):
    s = np.zeros(levels, np.float32)
    s[0] = 1.0
    for l in range(1, levels):
        s[l] = np.float32(f) * s[l - 1]                # float32 product chain
    return ([int(np.round(w0 * 1.0 / float(x))) for x in s], [int(np.round(h0 * 1.0 / float(x))) for x in s])


def row_taps(sh, dh):
    scale = 1.0 / (float(dh) / sh)
    s = np.floor(((np.arange(dh) + 0.5) * scale - 0.5).astype(np.float32)).astype(np.int64)
    return np.clip(s, 0, sh - 1), np.clip(s + 1, 0, sh - 1)


def groups(sh, dh):
    """One dict per group of a level: shared (the kernel's test), monotone, switch (first r with d_r = r + 1, 5 when none: six source
    rows instead of seven), rows (5, fewer in the last group), clamped (a loaded row index s0 + i runs into sh - 1)."""
    sy0, sy1 = row_taps(sh, dh)
    out = []
    for g in range(0, dh, ROWS):
        n = min(ROWS, dh - g)
        off = [int(sy0[g + r] - sy0[g]) - r for r in range(n)]
        shared = all(o in (0, 1) for o in off) and all(sy1[g + r] == min(sy0[g + r] + 1, sh - 1) for r in range(n))
        switch = next((r for r in range(n) if off[r] == 1), ROWS)
        nrows = 7 if (n == ROWS and off[ROWS - 1] == 1) else 6
        out.append(dict(shared=shared, monotone=all(off[r + 1] >= off[r] for r in range(n - 1)), switch=switch, rows=n,
                        clamped=int(sy0[g]) + nrows - 1 > sh - 1))
    return out
