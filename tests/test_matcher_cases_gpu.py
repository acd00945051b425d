"""The matcher kernels against the constructed cases of match_cases.py: each entry equals the hand-written expectation and the oracle."""
import numpy as np
import pytest

import match_cases as MC
import oracle_lib as O
from test_matcher_cases_cpu import check

pytestmark = pytest.mark.gpu

CASES = MC.all_cases()


@pytest.fixture(scope="module")
def handles():
    """One matcher handle per member for the whole module; nnratio / checkOrientation are set per case."""
    from rumi_slam_amd import matcher as M
    hs = {m: M.ORBmatcher(0.8, False, max_features=1024, max_queries=1024) for m in MC.MEMBERS + ["MP_FUSED", "BOW_BATCH"]}
    yield M, hs
    for h in hs.values():
        h.close()


def _member_cases(m):
    return [c for c in CASES if c.member == m]


@pytest.mark.parametrize("member", MC.MEMBERS)
def test_kernel_equals_expected_and_oracle(handles, member):
    M, hs = handles
    for c in _member_cases(member):
        got = MC.call_gpu(M, hs[member], c)
        check(c, got, "kernel")
        ref = MC.call_oracle(O, c)
        assert got[0] == ref[0] and np.array_equal(got[1], ref[1]), f"{c.id}: kernel and oracle differ"


def test_bow_cases_through_the_batch_entry(handles):
    M, hs = handles
    for c in _member_cases("BOW_F"):
        nm, got = MC.call_gpu_bow_batch(M, hs["BOW_BATCH"], c, 3)
        for k in range(3):
            check(c, (int(nm[k]), got[k]), f"batch candidate {k}")


def test_mappoint_cases_through_the_fused_local_points_entry(handles):
    M, hs = handles
    for c in _member_cases("MP"):
        check(c, MC.call_gpu_fused(M, hs["MP_FUSED"], c), "fused entry")
