"""GPU parity of the bundle adjuster on the scenes of ba_scenes: arbitrary world frames, either quaternion sign, full and non-symmetric information
matrices, Huber off / tight / wide, SE3 errors on both sides of se3_log's switch and at tens of degrees, kilometres and millimetres, points centimetres
from a camera, degenerate graphs, a pose graph without points, a window without SE3 edges.  Every scene goes through each solver it routes to (k_ba_lm,
k_ba_one_pose, k_ba_pose_only), alone, with set_team(1) and set_team(4), as a short solve (far from convergence: compared step for step) and a full-length one.

Two references.  The oracle, through test_gpu_ba._check: residuals < 1e-5, chi2_final to 1e-8 and chi2_init to 1e-10 relative, the LM trajectory equal
(short solves) or, where a full-length solve may fork at convergence, tools/ba_fuzz.py's rule (the same path, or chi2_final equal to 1e-10 relative).
And ba_ref_ld, the edge arithmetic in extended precision, evaluated at the state the GPU RETURNED: chi2_per_obs, chi2_initial and chi2_final.

Bars against ba_ref_ld, next to the measured baseline (the ORACLE's largest gap to ba_ref_ld on the same solves, tests/test_ba_scenes_ref.py; the solver is
allowed 4 x that -- its 1 / z and rsqrt substitutions cost an ulp or two per entry -- and the sums never less than n_terms * 2^-52, n_terms = observations + SE3 edges):

    group        baseline (oracle):  chi2_init  chi2_final  per obs   |  bar (solver):  chi2_init  chi2_final  per obs
    world                            2.3e-15    6.6e-15     1.6e-12   |                 1.4e-13    1.4e-13     6.4e-12
    qsign                            1.9e-15    3.1e-15     4.4e-13   |                 1.4e-13    1.4e-13     1.8e-12
    info                             3.9e-15    3.8e-15     3.3e-13   |                 1.4e-13    1.4e-13     1.3e-12
    huber                            1.7e-15    2.2e-15     5.3e-13   |                 2.2e-13    2.2e-13     2.1e-12
    edges                            1.5e-14    5.1e-15     5.2e-13   |                 1.4e-13    1.4e-13     2.1e-12
    scale                            1.4e-15    3.1e-15     6.4e-13   |                 1.4e-13    1.4e-13     2.6e-12
    near                             9.1e-16    3.9e-15     1.3e-11   |                 1.3e-13    1.3e-13     5.2e-11
    degenerate                       1.7e-15    2.6e-15     5.0e-13   |                 1.3e-13    1.3e-13     2.0e-12
    shape (pose graph, 11 terms)     2.2e-14    1.5e-14     3.8e-13   |                 8.8e-14    6.0e-14     1.5e-12
    mixed                            2.1e-15    8.6e-15     3.0e-12   |                 2.7e-13    2.7e-13     1.2e-11

(The sums' bars are n_terms * 2^-52 wherever that exceeds 4 x baseline: 609 terms in most scenes, 971 in the huber window, 1213 in the mixed one; only the
pose graph's 11 terms leave 4 x baseline on top.  _bars() computes them from ba_scenes.ORACLE_GAP and the window; this table is for the reader.)

test_domain_summary prints, per group, the routes exercised and the largest gaps met."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ba_ref_ld
import ba_scenes
import ba_synth
from test_gpu_ba import _check

pytestmark = pytest.mark.gpu
NAMES = [s.name for s in ba_scenes.scenes()]
_summary = {}


def _solve(ctx, p, iters, team):
    import mi355slam
    ba = mi355slam.BundleAdjuster(ctx, [p], max_iters=iters)
    ba.set_team(team); ba.solve()
    got = ba.download(0)
    assert ba.team_fallbacks() == 0
    ba.close()
    return got


def _bars(group, p):
    base = ba_scenes.ORACLE_GAP[group]
    floor = (len(p["obs_pose"]) + len(p["edge_i"])) * 2.0 ** -52
    return max(4 * base[0], floor), max(4 * base[1], floor), 4 * base[2]


def _check_fixed_unmoved(p, got):
    pf = p["pose_fixed"] != 0
    assert np.array_equal(got["pose"][pf], p["pose"][pf])
    if p.get("point_fixed") is not None:
        lf = p["point_fixed"] != 0
        assert np.array_equal(got["point"][lf], p["point"][lf])


@pytest.mark.parametrize("name", NAMES)
def test_scene_matches_the_oracle_and_extended_precision(name, oracle, ctx):
    sc = ba_scenes.scene(name)
    note = _summary.setdefault(sc.group, dict(routes=set(), res=0.0, chi2=0.0, ld=[0.0, 0.0, 0.0], solves=0))
    for shape in ba_scenes.SHAPES:
        p = sc.shaped(shape)
        ref0 = ba_ref_ld.evaluate(p, p["pose"], p["point"])
        bars = _bars(sc.group, p)
        for iters in (sc.short_iters, ba_scenes.FULL_ITERS):
            want = oracle.ba_solve(p, iters, False)
            for team in (1, 4):
                r = ba_scenes.route([p], team)
                assert r == sc.expected_route(shape, team)
                got = _solve(ctx, p, iters, team)
                gs, ws = got["stats"], want["stats"]
                rg, rw = ba_synth.residuals(p, got["pose"], got["point"]), ba_synth.residuals(p, want["pose"], want["point"])
                dres = float(np.abs(rg - rw).max()) if rg.size else float(np.abs(got["pose"] - want["pose"]).max())
                dchi = abs(gs["chi2_final"] - ws["chi2_final"]) / abs(ws["chi2_final"])
                ref1 = ba_ref_ld.evaluate(p, got["pose"], got["point"])
                gaps = (ba_ref_ld.sum_gap(gs["chi2_init"], ref0["total"]), ba_ref_ld.sum_gap(gs["chi2_final"], ref1["total"]), ba_ref_ld.obs_gap(got["chi2"], ref1["chi2_obs"]))
                print("%s %s iters=%d team=%d route=%s: iters/trials %d/%d (oracle %d/%d); to the oracle: residuals %.1e chi2_final %.1e; to extended precision: "
                      "chi2_init %.1e chi2_final %.1e per observation %.1e (bars %.1e %.1e %.1e)" % ((name, shape, iters, team, r, gs["iters"], gs["trials"], ws["iters"], ws["trials"], dres, dchi) + gaps + bars))
                note["routes"].add(r); note["solves"] += 1
                note["res"], note["chi2"] = max(note["res"], dres), max(note["chi2"], dchi)
                note["ld"] = [max(a, b) for a, b in zip(note["ld"], gaps)]
                if iters == sc.short_iters:
                    _check(p, got, want)                                    # step for step
                else:
                    _check(p, got, want, strict_trajectory=False)
                    same_path = (gs["iters"], gs["trials"], gs["stop"]) == (ws["iters"], ws["trials"], ws["stop"])
                    assert same_path or abs(gs["chi2_final"] - ws["chi2_final"]) <= 1e-10 * abs(ws["chi2_final"])
                if not rg.size:                                             # a pose graph: the poses themselves stand in for the residuals
                    assert dres < 1e-7
                for k in range(3):
                    assert gaps[k] <= bars[k], (shape, iters, team, k, gaps[k], bars[k])
                _check_fixed_unmoved(p, got)
                if name == "degenerate" and shape == "general":
                    f = p["degenerate"]
                    assert np.array_equal(got["pose"][f["isolated_pose"]], p["pose"][f["isolated_pose"]])         # bit for bit
                    assert np.array_equal(got["point"][f["no_obs_point"]], p["point"][f["no_obs_point"]])
                    a, b = f["double_obs"]
                    assert got["chi2"][a] == got["chi2"][b]


@pytest.mark.parametrize("name", ["qsign_all", "qsign_half", "edges_large", "mixed"])
def test_quaternion_sign_changes_nothing(name, oracle, ctx):
    """q and -q are the same rotation: flipped poses and measurements give the same residuals to 1e-9 (the run-to-run bound of a team's atomic sums), in
    every shape, and the same LM path."""
    sc = ba_scenes.scene(name)
    for shape in ba_scenes.SHAPES:
        a = sc.shaped(shape)
        rng = np.random.default_rng(5)
        b = ba_scenes.flip_quaternion_signs(a, rng.random(len(a["pose"])) < 0.5, rng.random(len(a["edge_i"])) < 0.5)
        for team in (1, 4):
            ga, gb = _solve(ctx, a, sc.short_iters + 1, team), _solve(ctx, b, sc.short_iters + 1, team)
            assert np.abs(ba_synth.residuals(a, ga["pose"], ga["point"]) - ba_synth.residuals(b, gb["pose"], gb["point"])).max() < 1e-9
            assert (ga["stats"]["iters"], ga["stats"]["trials"]) == (gb["stats"]["iters"], gb["stats"]["trials"])
            assert abs(ga["stats"]["chi2_final"] - gb["stats"]["chi2_final"]) <= 1e-12 * ga["stats"]["chi2_final"]
            assert abs(ga["stats"]["chi2_init"] - gb["stats"]["chi2_init"]) <= 1e-13 * ga["stats"]["chi2_init"]


def test_huber_off_is_huber_wide_and_not_huber_default(oracle, ctx):
    """huber_delta <= 0 disables the robust kernel: the same solve as delta = 1e6 where no chi2 exceeds 1e12 (there every edge is quadratic too), in all three
    kernels; and a different one from sqrt(5.991) on this window with 12 % outliers."""
    off, neg, wide, dflt = (ba_scenes.scene(n) for n in ("huber_0", "huber_neg", "huber_1e6", "huber_default"))
    for shape in ba_scenes.SHAPES:
        for team in (1, 4):
            g = [_solve(ctx, s.shaped(shape), 4, team) for s in (off, neg, wide, dflt)]
            p = off.shaped(shape)
            assert g[2]["chi2"].max() < 1e12
            r = [ba_synth.residuals(p, x["pose"], x["point"]) for x in g]
            for k in (0, 1):
                assert np.abs(r[k] - r[2]).max() < 1e-9
                assert (g[k]["stats"]["iters"], g[k]["stats"]["trials"]) == (g[2]["stats"]["iters"], g[2]["stats"]["trials"])
                assert abs(g[k]["stats"]["chi2_final"] - g[2]["stats"]["chi2_final"]) <= 1e-12 * g[2]["stats"]["chi2_final"]
                assert abs(g[k]["stats"]["chi2_init"] - g[2]["stats"]["chi2_init"]) <= 1e-13 * g[2]["stats"]["chi2_init"]
            assert g[3]["stats"]["chi2_init"] < 0.5 * g[0]["stats"]["chi2_init"] and np.abs(r[3] - r[0]).max() > 1e-4


def test_domain_fuzz_tool():
    """tools/ba_fuzz.py with `domain`: 80 random windows, each moved / flipped / re-weighted / rescaled ... by a random subset of ba_scenes' transforms."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "ba_fuzz.py"), "80", "2025", "domain"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 mismatches" in r.stdout
    m = re.search(r"routes: pose_only=(\d+) one_pose=(\d+) general=(\d+)", r.stdout)
    assert m and all(int(k) > 0 for k in m.groups()), r.stdout[-2000:]


def test_domain_summary(capsys):
    """Not a check of its own: prints what the scene tests of this run met."""
    with capsys.disabled():
        print("\nBA domain scenes: per group, the routes exercised and the largest gaps (to the oracle: residuals, chi2_final relative; to extended precision: chi2_init, chi2_final, per observation)")
        for g in ba_scenes.GROUPS:
            if g in _summary:
                n = _summary[g]
                print("  %-11s %3d solves  routes %-28s oracle %.1e %.1e   extended precision %.1e %.1e %.1e" % ((g, n["solves"], ",".join(sorted(n["routes"])), n["res"], n["chi2"]) + tuple(n["ld"])))
