"""The oracle against the constructed projection-gate cases of gate_cases.py: every expectation there is written down from the reference's rule,
so a misreading shared by oracle and kernels shows up here.  Needs no GPU."""
import collections

import numpy as np
import pytest

import gate_cases as G
import match_cases as MC
import oracle_lib as O
from test_matcher_cases_cpu import check

CASES = G.all_cases()


def check_frustum(c, got, who):
    rows = np.nonzero(c.skip == 0)[0] if who in ("oracle", "isInFrustum") else None       # entries without a skip flag evaluate every point
    bad = G.same_bytes(got, c.exp, rows)
    assert not bad, f"{c.id} ({c.cite}): {who} differs in {bad}: " + "; ".join(f"{k} {np.asarray(got[k]).tolist()} expected {c.exp[k].tolist()}" for k in bad)


def run_oracle(c):
    if c.member == "FRUSTUM":
        check_frustum(c, G.oracle_frustum(O, c), "oracle")
        return
    if c.member == "MP":
        n, fm, fr = G.oracle_mp(O, c)
        bad = G.same_bytes(fr, c.fields)
        assert not bad, f"{c.id} ({c.cite}): the oracle's frustum fields differ in {bad}"
        check(c, (n, fm), "oracle")
        # the same search on the expected fields themselves (what k_queries_mappoints is given)
        i = c.inp
        check(c, O.search_by_projection_mappoints(i["keys"], i["desc"], G.W, G.H, MC.SF, G.mp_from_fields(c), np.full(len(i["keys"]), -1, np.int32), i["R"] / 4.0,
                                                  bool(i.get("far", False)), float(i.get("th_far", 50.0)), c.nnratio), "oracle on the expected fields")
        return
    check(c, MC.call_oracle(O, c), "oracle")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_oracle_equals_expected(c):
    run_oracle(c)


def test_every_case_runs_and_every_family_has_cases(capsys):
    """No case is skipped at run time: this loop runs each one and counts them; a builder search that found nothing has already failed the import."""
    ran = collections.Counter()
    for c in CASES:
        run_oracle(c)
        ran[c.family] += 1
    assert sum(ran.values()) == len(CASES) and set(ran) == set(G.FAMILIES)
    with capsys.disabled():                                     # the count is part of the report, captured output or not
        print("\ngate cases per family: " + ", ".join(f"{f} {ran[f]}" for f in G.FAMILIES) + f"; {len(CASES)} in all")


def test_every_member_family_cell_is_covered_or_named_not_applicable():
    cov = G.coverage()
    for m in G.MEMBERS:
        for f in G.FAMILIES:
            has, na = bool(cov.get((m, f))), (m, f) in G.NOT_APPLICABLE
            assert has != na, f"{G.MEMBER_NAMES[m]} x family {f}: " + ("both covered and marked not applicable" if has else "no case and no reason")
            if na:
                why = G.NOT_APPLICABLE[(m, f)]
                assert len(why) > 10 and (".cc:" in why), f"{m} x {f}: the reason cites no reference line"
    assert set(G.NOT_APPLICABLE) <= {(m, f) for m in G.MEMBERS for f in G.FAMILIES}


def test_builder_self_checks():
    # the bounds the I family stands on are the oracle's ComputeImageBounds of the EuRoC camera
    assert O.image_bounds(752, 480, G.EUROC_K, G.EUROC_DIST).tolist() == list(G.EUROC_BOUNDS)
    # float and double forms of the viewing-cosine gate cannot be told apart by any input (the docstring has the argument)
    assert G.cos_disagreement_search() == []
    # the level steps: both neighbours at least 1e-9 from the integer, the closest at k = 7
    assert len(G.LEVEL_STEPS) == 8 and min(hi for *_, hi in G.LEVEL_STEPS) == G.LEVEL_STEPS[7][4] and 1e-8 < G.LEVEL_STEPS[7][4] < 2e-8
    for k, r, r_up, lo, hi in G.LEVEL_STEPS:
        assert r_up == np.nextafter(r, np.float32(np.inf)) and abs(float(r) - 1.2 ** k) < 1e-5
    # the distance-gate constants
    assert float(G.MAX_IN) == 3.3333332538604736 and np.float32(1.2) * G.MAX_IN == 4 and np.float32(0.8) * np.float32(5) == 4 and 0.8 * 5.0 == 4.0
    assert float(np.float32(0.8)) * 5.0 > 4.0
    # the two projection forms disagree for the V family's point
    for x, z, ud, ui, bound in G.DIVISION_PAIRS:
        assert (0 <= float(ud) < 640) != (0 <= float(ui) < 640)
    # every case is small
    for c in CASES:
        if c.member == "FRUSTUM":
            assert len(c.specs) <= 8
        else:
            assert len(c.inp["keys"]) <= 8 and c.inp["nq"] <= 8
    # POSE_X is a real pose: Ow = -R^T t is not the origin and R is not the identity
    assert G.POSE_X.Ow.any() and not np.array_equal(G.POSE_X.R, np.eye(3))


def test_existing_helpers_are_unchanged_for_existing_cases():
    """Proj.query's new overrides default to None: a query without them builds the arrays it always built."""
    s = MC.Proj(1)
    b = s.base()
    s.feat(100, 100, b)
    s.query(100, 100, b, level=3)
    a = s.arrays()
    assert a["pos"].tolist() == [[(100 - 320) / 128, (100 - 240) / 128, 4.0]] and a["level"].tolist() == [3] and a["min_dist"].tolist() == [np.float32(0.1)]
    assert abs(float(a["normal"][0] @ a["pos"][0]) / float(np.linalg.norm(a["pos"][0])) - 0.906) < 1e-3
