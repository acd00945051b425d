"""The constructed CreateNewMapPoints cases of newpoints_cases.py against the C++ oracle (tests/cpp/newpoints_oracle.cc), and against the mutants of
the builder's own restatement.  Every expectation there is written down from the reference's rule and asserted against a restatement in numpy
float32 and Python doubles, so a misreading shared by the oracle and the kernels shows up here.  Needs no GPU."""
import collections

import numpy as np
import pytest

import newpoints_cases as N
from newpoints_scene import GATES, build_oracle, params, run_oracle

CASES = N.all_cases()
assert GATES == N.GATES


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("newpoints_cases"))


def oracle_of(L, c):
    cur, neigh = c.views()
    return run_oracle(L, cur, neigh, params(c.coarse, c.ori, c.far, c.th_far, c.rf))


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def check_against(c, want):
    """The oracle's (or an entry's) lists against the case's stated expectation."""
    got = [(int(p["neigh"]), int(p["idx1"]), int(p["idx2"])) for p in want["points"]]
    assert got == c.expect, f"{c.id} ({c.cite}): accepted {got}, stated {c.expect}"
    assert want["per_neigh"].tolist() == c.per and want["skipped"].tolist() == c.skipped, f"{c.id} ({c.cite}): counts {want['per_neigh']}, skipped {want['skipped']}"
    if c.matches is not None:
        assert want["matches"].tolist() == c.matches, f"{c.id} ({c.cite}): matches {want['matches'].tolist()}, stated {c.matches}"


@pytest.mark.parametrize("family", N.FAMILIES)
def test_oracle_equals_the_restatement(oracle, family):
    """List, counts, skip flags and matches; per traced pair the gate and the bits of x3D: Python doubles with math.sqrt are IEEE and never contracted, so
    the builder's Jacobi iteration is expected to give the oracle's point bit for bit."""
    ran = 0
    for c in (c for c in CASES if c.family == family):
        want, r = oracle_of(oracle, c), c.res
        check_against(c, want)
        assert want["matches"].tolist() == r.matches, f"{c.id}: matches of the oracle and of the restatement differ"
        tr = want["trace"]
        assert [(int(t["neigh"]), int(t["idx1"]), int(t["idx2"]), GATES[t["gate"]]) for t in tr] == [t[:4] for t in r.trace], f"{c.id}: traces differ"
        for t, mine in zip(tr, r.trace):
            assert bits(t["x3D"]) == bits(mine[4]), f"{c.id}: x3D of pair {mine[:3]}: oracle {t['x3D']}, restatement {mine[4]}"
        x3d = {t[:3]: t[4] for t in r.trace}
        for p in want["points"]:
            assert bits(p["x3D"]) == bits(x3d[(int(p["neigh"]), int(p["idx1"]), int(p["idx2"]))])
        ran += 1
    assert ran == len(N.COVERAGE[family]) > 0


def test_every_case_is_live(oracle, capsys):
    """No case is skipped at run time: this loop runs each one.  A case that states a gate has its pair, with the stated idx2, in the oracle's trace; of an
    adjacent pair of the gate families both members have it, of the search and baseline families the member on the accepting side (on the other side
    the pair is what the search or the skipped neighbour did not produce)."""
    ran = collections.Counter()
    by = {c.name: c for c in CASES}
    for c in CASES:
        want = oracle_of(oracle, c)
        traced = {(int(t["neigh"]), int(t["idx1"]), int(t["idx2"])) for t in want["trace"]}
        assert traced == set(c.stops), c.id
        if c.twin is not None:
            both = [c, by[c.twin]]
            assert any(x.stops for x in both), c.id
            if c.family in "PRFS":
                assert len(c.stops) == 1 and set(c.stops) == set(by[c.twin].stops), c.id
        ran[c.family] += 1
    assert sum(ran.values()) == len(CASES) and set(ran) == set(N.FAMILIES)
    with capsys.disabled():
        print("\nnewpoints cases per family: " + ", ".join(f"{f} {ran[f]}" for f in N.FAMILIES) + f"; {len(CASES)} in all, 0 left out")


def test_cases_are_well_formed_and_the_tables_complete():
    assert set(N.COVERAGE) == set(N.FAMILIES) and all(N.COVERAGE[f] for f in N.FAMILIES)
    assert sorted(n for names in N.COVERAGE.values() for n in names) == sorted(c.name for c in CASES)
    for table in (N.NOT_APPLICABLE, N.STRICTNESS_NOT_APPLICABLE, N.FLOAT_NOT_APPLICABLE):
        for what, why in table.items():
            assert len(why) > 40 and (".cc:" in why), f"{what}: the reason cites no reference line"
    assert {"W", "D"} <= set(N.NOT_APPLICABLE)
    twins = [c for c in CASES if c.twin is not None]
    assert len(twins) % 2 == 0 and len(twins) >= 40
    for c in CASES:
        assert c.cur.n <= 65 and len(c.neigh) <= 3 and all(nb.n <= 2052 for nb in c.neigh)
        assert max(nb.n for nb in c.neigh) <= 70 or c.name.startswith("median_behind_the_tile")
        for kf in [c.cur] + c.neigh:                                           # poses exact in float32: entries 0 / +-1, dyadic translations
            assert set(np.abs(kf.R).ravel().tolist()) <= {0.0, 1.0} and np.array_equal(kf.t * 1024, np.round(kf.t * 1024))
    # the restatement's Jacobi iteration on a matrix whose null vector is known: A (x, y, z, 1)^T = 0 for the point (0.5, 0.25, 4)
    c = next(c for c in CASES if c.name == "dist50")
    x = c.res.trace[0][4]
    assert np.allclose(np.array(x, np.float64), [0.5, 0.25, 4.0], rtol=1e-6)


def test_every_mutant_is_killed(capsys):
    """For every subtle error of VARIANTS at least one committed case changes its accepted list."""
    lines, unkilled = [], []
    for variant, what in N.VARIANTS.items():
        killers = [c.id for c in CASES if N.create(c, variant).points != c.expect]
        lines.append(f"  {variant:22s} killed by {len(killers):2d}: {', '.join(killers[:4])}{' ...' if len(killers) > 4 else ''}")
        if not killers:
            unkilled.append(variant)
    with capsys.disabled():
        print("\nvariants of the restatement and the cases whose accepted list they change:\n" + "\n".join(lines))
        for table in (N.STRICTNESS_NOT_APPLICABLE, N.FLOAT_NOT_APPLICABLE):
            for what, why in table.items():
                print(f"  no variant for {what}: {why}")
    assert not unkilled, f"no case kills {unkilled}: a gap in the cases"
    # the restatement without a variant is what the cases were asserted against
    assert all(N.create(c).points == c.expect for c in CASES[:10])
