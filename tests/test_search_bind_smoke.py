"""The matchLocalMapPoints part of the host mirror (matchLocalMapPoints in slam-module_amd/host/mi355slam/map_update.hpp, searchByProjectionOnTables
in keyframe_matcher.hpp) compiles, links against the C ABI and, on the GPU, leaves the tables, the match list and the matcher mask of a walk
over a std::set of local map points and std::map observations (tests/search_bind_smoke.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "search_bind_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "search_bind_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_compiles_links_and_the_validation_runs_without_a_device():
    build_smoke()
    out = subprocess.check_output([EXE, "--no-gpu"], text=True)
    assert "link ok 1" in out and re.search(r"no-gpu ok 12 cases", out), out


def body_of(code, start):
    body = code[code.index(start):]
    return body[:body.index("\n}\n")]


def test_nothing_of_the_walk_comes_to_the_host_in_the_mirror():
    """No download of top-4 lists or query arrays and no upload of kf_mp or n_obs in the new-keyframe path's matchLocalMapPoints."""
    host = os.path.join(ROOT, "slam-module_amd", "host", "mi355slam")
    strip = lambda path: re.sub(r"//[^\n]*", "", open(os.path.join(host, path)).read())
    outer = body_of(strip("map_update.hpp"), "inline SearchBindResult matchLocalMapPoints")
    inner = body_of(strip("keyframe_matcher.hpp"), "inline SearchBindResult searchByProjectionOnTables")
    gate = body_of(strip("keyframe_matcher.hpp"), "inline DeviceGatedLists gate_and_score_device")
    for body in (outer, inner, gate):
        assert "ms_dev_upload" not in body and ".update(" not in body and "replay_search" not in body and "rescan_on_host" not in body and "std::map" not in body
    assert "download" not in outer and "download" not in gate
    assert inner.count("download") == 1 and "if (matchKp) out.matchKp = ctx.download(matchKp, ne)" in inner          # the match list, on request only
    assert "localMapPoints(" in outer and "searchByProjectionOnTables(" in outer and "view.indices.empty()" in outer
    assert gate.index("ms_bound_mask(") < gate.index("ms_project_gate(") < gate.index("ms_projection_topk(")
    assert inner.index("gate_and_score_device(") < inner.index("ms_search_bind(")


def test_the_existing_search_by_projection_is_unchanged():
    """searchByProjection and searchByProjectionCore stay as they are: they are the yardstick of the new path."""
    code = open(os.path.join(ROOT, "slam-module_amd", "host", "mi355slam", "keyframe_matcher.hpp")).read()
    body = body_of(code, "inline std::vector<int> searchByProjection(Context &ctx")
    assert "detail::gate_and_score(ctx, table, {view}, {&kf}, settings, &bound)" in body and "detail::replay_search(g.lists, 0, nq, bound, rescan" in body
    core = body_of(code, "inline std::vector<int> searchByProjectionCore(")
    assert "detail::score_candidates(ctx, kf, queries, &bound)" in core and "detail::replay_search(s, 0, queries.size(), bound" in core


@pytest.mark.gpu
def test_mirror_equals_the_std_map_walk():
    build_smoke()
    out = subprocess.check_output([EXE, "--gpu"], text=True)
    assert "matchLocalMapPoints ok" in out and "empty list ok" in out, out
