"""The matcher oracle against the constructed cases of match_cases.py: every expectation there is written down from the reference's
rule, so a misreading shared by oracle and kernels shows up here."""
import numpy as np
import pytest

import match_cases as MC
import oracle_lib as O

CASES = MC.all_cases()


def check(c, got, who):
    assert got[0] == c.count, f"{c.id} ({c.cite}): {who} count {got[0]}, expected {c.count}"
    assert np.array_equal(np.asarray(got[1]), c.arr), f"{c.id} ({c.cite}): {who} {np.asarray(got[1]).tolist()}, expected {c.arr.tolist()}"
    if c.pm is not None:
        assert np.array_equal(got[2], c.pm), f"{c.id} ({c.cite}): {who} vbPrevMatched differs"


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_oracle_equals_expected(c):
    check(c, MC.call_oracle(O, c), "oracle")


def test_every_member_family_cell_is_covered_or_named_not_applicable():
    cov = MC.coverage()
    for m in MC.MEMBERS:
        for f in MC.FAMILIES:
            has, na = bool(cov.get((m, f))), (m, f) in MC.NOT_APPLICABLE
            assert has != na, f"{MC.MEMBER_NAMES[m]} x family {f}: " + ("both covered and marked not applicable" if has else "no case and no reason")
            if na:
                assert len(MC.NOT_APPLICABLE[(m, f)]) > 10
    assert set(MC.NOT_APPLICABLE) <= {(m, f) for m in MC.MEMBERS for f in MC.FAMILIES}


def test_helpers():
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    for k in (0, 1, 50, 256):
        assert int(np.unpackbits(base ^ MC.desc_at(base, k, rng)).sum()) == k
    assert [MC.c_round(v) for v in (0.5, 1.5, 2.5, -0.5, 0.49999997)] == [1, 2, 3, -1, 0]
    # the placer's visit order is the one GetFeaturesInArea has (pinned by test_features_in_area_matches_definition)
    xy = [(MC.U0 + dx, MC.V0 + dy) for dx in (-6, 0, 6) for dy in (6, -6)]
    keys = np.zeros(len(xy), O.KP_DTYPE)
    keys["x"], keys["y"] = np.array(xy, np.float32).T
    assert O.features_in_area(keys, 640, 480, MC.U0, MC.V0, 8.0, -1, -1).tolist() == MC.visit_order(xy, 640, 480)
    assert MC.KP_DTYPE == O.KP_DTYPE
