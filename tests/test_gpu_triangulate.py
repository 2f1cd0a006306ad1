"""ms_triangulate on the device against tests/triangulate_ref.py, its specification.  status, reason, n_pass and the flags
must be equal; positions must lie within triangulate_ref.GPU_POSITION_TOLERANCE (100 times the difference between the restatement and a
LAPACK evaluation of the same definitions over these fixtures -- never a number read off the device); rows the call does not list, and
positions of points that fail (the entry position, or what the reference had written by then: the depth branch of :622, :746 / :776 of the
first / last variant), must be bit-equal.  tests/test_triangulate_ref.py shows that no decision of these fixtures lies within a relative
1e-6 of its threshold, so nothing is left out of the comparison.

Shapes: 0, 1, 2, 3, 15, 16, 17, 33, 65 and 300 observations per point (a group takes 16 per round), 1, 3, 4, 5, 63, 64, 65 and 1003 points
per call (4 points per wave, 16 per block), 70 keyframes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mi355slam
import triangulate_ref as R

pytestmark = pytest.mark.gpu

N_MP = R.N_MP


class _Scene:
    """The fixture scene, built on first use (R.fixture shares it): collecting this file costs nothing."""

    def __getitem__(self, key):
        if "scene" not in R._CACHE:
            R._CACHE["scene"] = R.make_scene()
        return R._CACHE["scene"][key]


SCENE = _Scene()


class Device:
    """The scene's tables on the device, reset to the entry state before every call."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.table = mi355slam.MapPointTable(ctx, SCENE["mp_pos"], np.zeros((N_MP, 3), np.float32), np.ones(N_MP, np.float32), np.ones(N_MP, np.float32),
                                             np.zeros((N_MP, 8), np.uint32))
        self.poses = mi355slam.KeyframePoseTable(ctx, SCENE["poses"])
        self.flags = ctx.upload(SCENE["mp_flags"])

    def reset(self):
        self.table.update(0, N_MP, pos=SCENE["mp_pos"])
        self.ctx.check(mi355slam.lib().ms_dev_upload(self.ctx._h, C.c_void_p(self.flags.ptr), mi355slam._vp(SCENE["mp_flags"]), C.c_size_t(N_MP)), "ms_dev_upload")

    def run(self, prob, settings, mode, flags=True, outputs=True, reset=True):
        if reset:
            self.reset()
        out = self.table.triangulate(self.poses, SCENE["cams"], SCENE["focal"], prob, settings, mode, flags=self.flags if flags else None, outputs=outputs)
        return out, self.table.pos.download(np.float64, (N_MP, 3)), self.flags.download(np.uint8, (N_MP,))


@pytest.fixture(scope="module")
def dev(ctx):
    return Device(ctx)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def assert_matches(got, pos, flags, want, entries):
    """The device's answer for the entries `entries` of the fixture `want` (a call that listed exactly those)."""
    status, reason, n_pass = got
    entries = np.asarray(entries, np.int64)
    rows = np.asarray(want["prob"]["rows"])[entries]
    assert status.dtype == np.uint8 and np.array_equal(status, want["status"][entries])
    assert np.array_equal(reason, want["reason"][entries])
    assert n_pass.dtype == np.int32 and np.array_equal(n_pass, want["n_pass"][entries])
    w_flags, w_pos = SCENE["mp_flags"].copy(), SCENE["mp_pos"].copy()
    w_flags[rows], w_pos[rows] = want["flags"][rows], want["pos"][rows]
    assert np.array_equal(flags, w_flags)
    exact = np.ones(N_MP, bool)
    exact[rows[want["status"][entries] != 0]] = False       # untouched rows and every failure path: bit for bit
    assert same_bits(pos[exact], w_pos[exact])
    difference = R.relative_difference(pos[~exact], w_pos[~exact]) if (~exact).any() else 0.0
    print("%d rows, %d triangulated, largest relative difference %.3e" % (len(rows), int((~exact).sum()), difference))
    assert difference <= R.GPU_POSITION_TOLERANCE


@pytest.mark.parametrize("mode,with_depth,dense", R.FIXTURES)
def test_every_call_size_against_the_restatement(dev, mode, with_depth, dense):
    want = R.fixture(mode, with_depth, dense)
    for n in R.POINTS_PER_CALL:
        prob = R.sub_problem(want["prob"], range(n), with_depth)
        assert_matches(*dev.run(prob, want["settings"], mode), want, range(n))
    if not dense:
        assert set(want["reason"].tolist()) == ({0, 1, 2, 3, 6} if mode == R.FIRST_LAST else {0, 1, 2, 3, 4, 5})


def test_dense_stereo_flag_gives_reason_7(dev):
    want = R.fixture(R.FIRST_LAST, True, True)
    assert 7 in want["reason"] and 0 in want["reason"]
    got, _, _ = dev.run(R.sub_problem(want["prob"], range(65)), want["settings"], R.FIRST_LAST)
    assert np.array_equal(got[1], want["reason"][:65]) and 7 in got[1]


@pytest.mark.parametrize("mode", (R.TME, R.MIDPOINT, R.FIRST_LAST))
def test_same_bits_alone_first_last_and_on_a_second_call(dev, mode):
    want = R.fixture(mode, True)
    counts = np.diff(want["prob"]["obs_start"])
    probes = []
    for n in (2, 3, 16, 17, 65, 300):                        # a point of that length that triangulates, where the fixture has one
        fits = np.flatnonzero((counts == n) & (want["status"] != 0))
        probes.append(int(fits[0]) if len(fits) else int(np.flatnonzero(counts == n)[0]))
    probes += [int(np.flatnonzero(want["reason"] == r)[0]) for r in sorted(set(want["reason"].tolist()) - {0})]
    others = [e for e in range(200) if e not in probes]
    for probe in probes:
        row = want["prob"]["rows"][probe]
        seen = []
        for entries, at in (([probe], 0), ([probe] + others, 0), (others + [probe], len(others)), (others + [probe], len(others))):
            (status, reason, n_pass), pos, flags = dev.run(R.sub_problem(want["prob"], entries), want["settings"], mode)
            seen.append((int(status[at]), int(reason[at]), int(n_pass[at]), int(flags[row]), pos[row].view(np.uint64).tolist()))
        assert seen[0] == seen[1] == seen[2] == seen[3], probe
        assert seen[0][:3] == (want["status"][probe], want["reason"][probe], want["n_pass"][probe])


def test_flags_and_outputs_are_optional(dev):
    want = R.fixture(R.TME, True)
    prob = R.sub_problem(want["prob"], range(65))
    full = dev.run(prob, want["settings"], R.TME)
    got, pos, flags = dev.run(prob, want["settings"], R.TME, flags=False)
    assert np.array_equal(flags, SCENE["mp_flags"]) and same_bits(pos, full[1]) and all(np.array_equal(a, b) for a, b in zip(got, full[0]))
    got, pos, flags = dev.run(prob, want["settings"], R.TME, outputs=False)
    assert got is None and same_bits(pos, full[1]) and np.array_equal(flags, full[2])


def test_empty_call_and_empty_lists(dev):
    want = R.fixture(R.MIDPOINT, True)
    none = R.sub_problem(want["prob"], [])
    got, pos, flags = dev.run(none, want["settings"], R.MIDPOINT)
    assert len(got[0]) == 0 and same_bits(pos, SCENE["mp_pos"]) and np.array_equal(flags, SCENE["mp_flags"])
    empty = [int(e) for e in np.flatnonzero(np.diff(want["prob"]["obs_start"]) == 0)[:5]]
    prob = R.sub_problem(want["prob"], empty)
    assert len(prob["obs_kf"]) == 0
    got, pos, flags = dev.run(prob, want["settings"], R.MIDPOINT)
    assert got[1].tolist() == [1] * 5 and got[0].tolist() == [0] * 5 and same_bits(pos, SCENE["mp_pos"])
    assert np.all(flags[want["prob"]["rows"][empty]] == 0)   # the status is reset at entry


def test_invalid_call_leaves_the_tables_bit_equal(dev):
    want = R.fixture(R.TME, True)
    dev.reset()
    for change in ("twice", "slot", "octave", "mode", "setting"):
        prob = {k: (None if v is None else np.array(v)) for k, v in R.sub_problem(want["prob"], range(65)).items()}
        settings, mode = dict(want["settings"]), R.TME
        if change == "twice":
            prob["rows"][64] = prob["rows"][0]
        elif change == "slot":
            prob["obs_kf"][-1] = R.N_KF
        elif change == "octave":
            prob["obs_octave"][0] = 8
        elif change == "mode":
            mode = 3
        else:
            settings["min_angle_two_obs"] = float("nan")
        with pytest.raises(mi355slam.MsError, match="triangulate: "):
            dev.run(prob, settings, mode, reset=False)
        assert same_bits(dev.table.pos.download(np.float64, (N_MP, 3)), SCENE["mp_pos"])
        assert np.array_equal(dev.flags.download(np.uint8, (N_MP,)), SCENE["mp_flags"])


def test_allocations_stay_flat(dev):
    allocs = mi355slam.lib().ms_debug_host_allocs
    allocs.restype = C.c_longlong
    want = R.fixture(R.TME, True)
    dev.run(want["prob"], want["settings"], R.TME)           # warm-up: the largest call
    before = allocs()
    for i in range(12):
        n = R.POINTS_PER_CALL[i % len(R.POINTS_PER_CALL)]
        dev.run(R.sub_problem(want["prob"], range(n), i % 2 == 0), want["settings"], i % 3, outputs=i % 4 > 0, reset=False)
    assert allocs() == before


def write_scene(path, entries):
    """The text file tests/triangulate_smoke.cpp reads: sizes, settings, tables, lists, then per mode what the restatement expects."""
    S = R.settings()
    prob = R.sub_problem(SCENE["prob"], entries)
    rows = np.asarray(prob["rows"])

    def hx(a):
        return " ".join(float(v).hex() for v in np.asarray(a, np.float64).reshape(-1))

    def ints(a):
        return " ".join(str(int(v)) for v in np.asarray(a).reshape(-1))
    lines = ["%d %d %d %d %d 1" % (R.N_KF, N_MP, len(rows), len(prob["obs_kf"]), len(S["level_sigma_sq"])),
             hx([S["min_angle_two_obs"], S["min_angle_multiple_obs"], S["rel_reprojection_threshold"], R.GPU_POSITION_TOLERANCE]),
             hx(SCENE["poses"]), hx(SCENE["cams"]), ints(SCENE["focal"]), hx(S["level_sigma_sq"]), hx(SCENE["mp_pos"]), ints(SCENE["mp_flags"]),
             ints(rows), ints(prob["was_triangulated"]), ints(prob["obs_start"]), ints(prob["obs_kf"]), hx(prob["obs_x"]), hx(prob["obs_y"]),
             ints(prob["obs_octave"]), hx(prob["obs_depth"])]
    for mode in (R.TME, R.MIDPOINT, R.FIRST_LAST):
        want = R.fixture(mode, True)
        e = np.asarray(list(entries), np.int64)
        flags, pos = SCENE["mp_flags"].copy(), SCENE["mp_pos"].copy()
        flags[rows], pos[rows] = want["flags"][rows], want["pos"][rows]
        lines += [ints(want["status"][e]), ints(want["reason"][e]), ints(want["n_pass"][e]), ints(flags), hx(pos)]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_mirror_smoke_on_the_device(tmp_path):
    import test_triangulate_abi
    scene = os.path.join(str(tmp_path), "scene.txt")
    write_scene(scene, range(65))
    out = subprocess.check_output([test_triangulate_abi.build_smoke(), "--gpu", scene], text=True)
    for name in ("TME", "MIDPOINT", "FIRST_LAST"):
        assert "ok %s 65 rows" % name in out, out
