"""tests/covis_ref.py (the numpy restatement that specifies ms_covisibility / ms_map_point_union) against sequential models written the way
the reference writes its loops: a dictionary for Keyframe::getNeighbors (keyframe.cpp:192-230: seed previous / next with minCovisibilities,
walk the observations of the keyframe's map points, then threshold), a set and a first-claim dictionary for the unions (mapper_helpers.cpp:
241-261, loop_closer.cpp:418-433).  Exact equality of integers everywhere."""
import numpy as np
import pytest

import covis_ref as R

N_KF, STRIDE, N_MP = 70, 100, 1003


@pytest.fixture(scope="module")
def scene():
    # the CPU scene carries the whole range of "none": a negative other than -1, the largest int32, the first row past the table
    kf_mp, flags = R.make_scene(odd_entries=(-7, 2 ** 31 - 1, N_MP))
    observations = {}                                        # MapPoint::observations: row -> the slots that list it, ascending
    for k in range(N_KF):
        for r in kf_mp[k]:
            if 0 <= r < N_MP:
                observations.setdefault(int(r), []).append(k)
    return kf_mp, flags, observations


def get_neighbors(kf_mp, flags, observations, slot, previous, next_, min_covisibilities, triangulated_only):
    covisibilities = {}
    if previous != -1:
        covisibilities.setdefault(previous, min_covisibilities)          # emplace
    if next_ != -1:
        covisibilities.setdefault(next_, min_covisibilities)
    for mp in kf_mp[slot]:
        if not 0 <= mp < N_MP:
            continue
        if triangulated_only and not flags[mp] & 1:
            continue
        for kf in observations[int(mp)]:
            if kf in covisibilities:
                covisibilities[kf] += 1
            else:
                covisibilities[kf] = 1
    return [kf for kf in sorted(covisibilities) if kf != slot and covisibilities[kf] >= min_covisibilities], covisibilities


def test_scene_is_the_one_the_issue_describes(scene):
    kf_mp, flags, observations = scene
    assert kf_mp.shape == (N_KF, STRIDE) and len(flags) == N_MP
    assert (kf_mp[13] == -1).all()
    assert sorted(int(r) for r in kf_mp[20] if not -1 <= r < N_MP) == [-7, N_MP, 2 ** 31 - 1]
    assert max(len(o) for o in observations.values()) <= 8
    for k in range(N_KF):                                    # the reference's invariant: a keyframe lists a map point at most once
        r = kf_mp[k][R.valid(kf_mp[k], N_MP)]
        assert len(set(r.tolist())) == len(r)
    assert all(o[-1] - o[0] < 8 for o in observations.values())          # within 8 consecutive slots (the emptied slot leaves a gap)


def test_neighbours_equal_the_dictionary_model(scene):
    kf_mp, flags, observations = scene
    cases, lengths, top = 0, set(), 0
    for min_covis in R.MIN_COVIS:
        for require in R.REQUIRE:
            for forced in R.FORCED:
                queries = R.scene_queries(N_KF, min_covis, require, forced)
                count, neighbours, n_nb = R.covisibility(kf_mp, N_MP, flags, queries)
                for q, (slot, fa, fb, _, _) in enumerate(queries):
                    want, cov = get_neighbors(kf_mp, flags, observations, slot, fa, fb, min_covis, require == 1)
                    assert neighbours[q].tolist() == want, (slot, min_covis, require, forced)
                    assert n_nb[q] == len(want)
                    for k in range(N_KF):                    # the map's value, less the seed of a forced slot
                        seed = min_covis if k in (fa, fb) else 0
                        assert count[q, k] == cov.get(k, seed) - seed
                    cases += 1
                    lengths.add(len(want))
                    top = max(top, int(count[q].max()))
    assert cases == 2100
    assert 0 in lengths and max(lengths) >= 10 and top >= 15        # not vacuous: empty and long lists, counts past the largest threshold


def union_model(kf_mp, flags, kf_list, exclude, require):
    claimed = {}                                             # localMapPoints.emplace(mpId, position): the first keyframe wins
    for p, slot in enumerate(kf_list):
        for mp in kf_mp[slot]:
            if 0 <= mp < N_MP:
                claimed.setdefault(int(mp), p)
    excluded = set(int(mp) for mp in kf_mp[exclude] if 0 <= mp < N_MP) if exclude != -1 else set()
    rows = [mp for mp in sorted(claimed) if (flags[mp] & require) == require and mp not in excluded]
    return rows, [claimed[mp] for mp in rows]


def union_cases():
    rng = np.random.default_rng(11)
    lists = [list(range(30, 42)), [], [44, 43, 42, 44, 41, 20, 13], [20], rng.integers(0, N_KF, 25).tolist(), list(range(N_KF))]
    out = []
    for l in lists:
        for exclude in (-1, 40, 13, 20):
            for require in (0, 1, 2, 3):
                out.append((l, exclude, require))
    return out


def test_unions_equal_the_set_and_first_claim_model(scene):
    kf_mp, flags, _ = scene
    cases = union_cases()
    kf_list, problems = [], []
    for l, exclude, require in cases:
        problems.append((len(kf_list), len(l), exclude, require))
        kf_list += l
    rows, owner, n_rows = R.map_point_union(kf_mp, N_MP, flags, np.array(kf_list, np.int32), problems)
    sizes = set()
    for u, (l, exclude, require) in enumerate(cases):
        want_rows, want_owner = union_model(kf_mp, flags, l, exclude, require)
        assert rows[u].tolist() == want_rows and owner[u].tolist() == want_owner and n_rows[u] == len(want_rows), (l, exclude, require)
        sizes.add(len(want_rows))
    assert 0 in sizes and max(sizes) > 900


def test_owner_is_the_list_position_not_the_slot(scene):
    kf_mp, flags, _ = scene
    l = [44, 43, 42, 44]
    rows, owner, _ = R.map_point_union(kf_mp, N_MP, flags, np.array(l, np.int32), [(0, 4, -1, 0)])
    assert set(owner[0].tolist()) == {0, 1, 2}               # the repeated slot at position 3 claims nothing
    for r, p in zip(rows[0], owner[0]):
        assert r in kf_mp[l[p]] and all(r not in kf_mp[l[i]] for i in range(p))
