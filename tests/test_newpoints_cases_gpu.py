"""The kernels of CreateNewMapPoints (k_newpts_match, k_newpts_depth, k_newpts_triangulate, k_newpts_replay) against the constructed cases of
newpoints_cases.py, through BOTH instantiations: rumi_create_new_map_points (BlockView) and rumi_create_new_map_points_resident (ResidentView)
over a covisibility store filled from the case.  Every comparison is exact: the accepted list, the counts and the skip flags equal the case's
stated expectation and the C++ oracle; the x3D bits equal the oracle's; the two entries agree byte for byte; for the search families the
stage-1+3 matches of the block entry (rumi_hook_newpts_matches) equal the stated ones."""
import types

import numpy as np
import pytest

import newpoints_cases as N
from newpoints_scene import build_oracle
from resident_scene import ResidentScene, slot_of, view_pose
from test_newpoints_cases_cpu import check_against, oracle_of

pytestmark = pytest.mark.gpu

CASES = N.all_cases()


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("newpoints_cases_gpu"))


@pytest.fixture(scope="module")
def matchers():
    """One matcher per check_orientation value for the whole module."""
    from rumi_slam_amd.matcher import ORBmatcher
    ms = {0: ORBmatcher(0.6, False), 1: ORBmatcher(0.6, True)}
    yield ms
    for m in ms.values():
        m.close()


def run_case(c, L, m):
    from rumi_slam_amd.mapping import CreateNewMapPoints, CreateNewMapPointsResident, last_matches
    cur, neigh = c.views()
    want = oracle_of(L, c)
    # ---- the block entry
    pts, per, skipped = CreateNewMapPoints(m, cur, neigh, c.rf, bool(c.coarse), bool(c.far), c.th_far)
    matches = last_matches(m, len(neigh), cur.frame.n)
    check_against(c, dict(points=pts, per_neigh=per, skipped=skipped, matches=matches))
    assert np.array_equal(per, want["per_neigh"]) and np.array_equal(skipped, want["skipped"]), f"{c.id}: counts or skip flags differ from the oracle"
    assert np.array_equal(matches, want["matches"]), f"{c.id}: matches differ from the oracle"
    assert pts.tobytes() == want["points"].tobytes(), f"{c.id}: the points (x3D bit for bit) differ from the oracle: {pts} / {want['points']}"
    # ---- the resident entry over a store filled from the case
    rs = ResidentScene(types.SimpleNamespace(cur=cur, neigh=neigh))
    ks = list(range(1, len(neigh) + 1))
    res = CreateNewMapPointsResident(m, rs.store, slot_of(0), view_pose(cur), [slot_of(k) for k in ks], [view_pose(neigh[k - 1]) for k in ks], c.rf,
                                     bool(c.coarse), bool(c.far), c.th_far)
    check_against(c, dict(points=res[0], per_neigh=res[1], skipped=res[2], matches=matches))       # (the hook replays block calls only)
    for a, b, what in zip(res, (pts, per, skipped), ("points", "counts", "skip flags")):
        assert a.tobytes() == b.tobytes(), f"{c.id}: the {what} of the resident entry differ from the block entry's"
    return len(pts), int((matches >= 0).sum())


@pytest.mark.parametrize("family", N.FAMILIES)
def test_both_entries_equal_the_stated_expectation_and_the_oracle(oracle, matchers, family):
    ran = points = pairs = 0
    for c in (c for c in CASES if c.family == family):
        p, m = run_case(c, oracle, matchers[c.ori])
        ran, points, pairs = ran + 1, points + p, pairs + m
    print(f"family {family}: {ran} cases through both entries, {pairs} matched pairs, {points} created points, all equal to the statement and the oracle")
    assert ran == len(N.COVERAGE[family]) > 0


def test_search_families_state_their_matches():
    """check_against compares last_matches only where a case states them: every case of a search family, of the replay families too, does."""
    for c in CASES:
        if c.family in N.SEARCH_FAMILIES + "OG":
            assert c.matches is not None, c.id
