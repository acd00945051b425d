"""The constructed key-frame database cases (tests/kfdb_cases.py) on the CPU: every case's spelled lines equal the C++ oracle
(tests/cpp/kfdb_oracle.cc) and the Python restatement (kfdb_cases.PyDB); the coverage table is full; and the cases bite: under each deviation a
kernel could carry, the named cases fail.  No GPU."""
import pytest

import kfdb_cases as KC
from kfdb_scene import build_oracle, run_oracle


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("kfdb_cases"))


@pytest.mark.parametrize("case", KC.CASES, ids=repr)
def test_case_lines_equal_oracle_and_restatement(oracle, case):
    assert KC.PyDB().run(case.script) == case.expect
    assert run_oracle(oracle, case.oracle_script) == case.expect


def test_every_case_is_described():
    for c in KC.CASES:
        assert c.rule and c.edge and c.expect and c.kinds, c.name
        assert len(c.expect) == sum(1 for x in c.script if x[0] in "RN"), c.name
        assert any(ch.isdigit() for ch in c.rule), (c.name, "the rule is cited by file and line")


def test_coverage_is_full_or_explained():
    assert set(KC.COVERAGE) == {(f, k) for f in KC.FAMILIES for k in "RN"}
    for cell, names in KC.COVERAGE.items():
        assert bool(names) != (cell in KC.NOT_APPLICABLE), cell
        assert all(n in KC.BY_NAME for n in names)
    assert all(KC.NOT_APPLICABLE.values())
    assert {n for names in KC.COVERAGE.values() for n in names} == set(KC.BY_NAME)          # every case sits in a cell


def test_shifted_ids():
    s, lines = KC.shifted(KC.BY_NAME["A_cov_other_map"], 1000, 5000)
    assert lines == ["R 5070 | 1001:3e800000 1002:3f000000 |", "N 5071 | 1001:3e800000 1002:3f000000 | | 1002"]
    assert KC.PyDB().run(s) == lines
    for c in KC.CASES:
        assert KC.shifted(c, 0, 0)[1] == c.expect


@pytest.mark.parametrize("deviation", KC.DEVIATIONS)
def test_cases_bite(deviation):
    """Each deviation is one subtle error of a kernel; the cases named for it in BITES fail, and no other case does."""
    failing = [c.name for c in KC.CASES if KC.PyDB(deviation).run(c.script) != c.expect]
    assert KC.BITES[deviation], deviation
    assert sorted(failing) == sorted(KC.BITES[deviation])


def test_near_edges_sees_an_undeclared_edge():
    """The audit of the builders: a threshold case declared without its edge does not build."""
    c = KC.BY_NAME["R_equal_075"]
    with pytest.raises(AssertionError):
        KC.Case("R_tmp", "R", c.script, c.expect, c.rule, c.edge, edges=())
    assert KC.near_edges([]) == set()
