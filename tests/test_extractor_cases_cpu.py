"""The extractor oracle (and the product's host quadtree) against the constructed cases of extract_cases.py: every expectation there is
written down from the reference's rule or computed by a plain numpy model of its arithmetic, so a misreading shared by oracle and kernels
shows up here."""
import ctypes as C

import numpy as np
import pytest

import extract_cases as EC
import oracle_lib as O
from rumi_slam_amd import capi

PRIMS = EC.Prims(O, capi.hooks())
PAT = EC.pattern()
CASES = EC.all_cases()
BIG = EC.big_octree_cases(PRIMS.std_sort)
B_CASES = [c for c in CASES + BIG if c.family == "B"]


@pytest.mark.parametrize("c", CASES + BIG, ids=[c.id for c in CASES + BIG])
def test_oracle_equals_expected(c):
    EC.check(c, EC.run_oracle(O, c), "oracle", PRIMS, PAT)


def _rel(c):
    return [(x - 16, y - 16, r) for x, y, r in c.cand[0]]


@pytest.mark.parametrize("c", B_CASES, ids=[c.id for c in B_CASES])
def test_host_quadtree_and_oracle_octree_equal_expected(c):
    """rumi_hook_quadtree (the product's array quadtree compiled for the host) and orc_octree on the case's candidate list."""
    h, w = c.frame.shape
    rel, want = _rel(c), [(x - 16, y - 16, r) for x, y, r in c.sel[0]]
    x, y, s = (np.array(v, np.uint32) for v in zip(*rel))
    packed = (x | (y << 12) | (s << 24)).astype(np.uint32)
    out, m = np.zeros(len(rel) + 8, np.int32), C.c_int32()
    assert capi.hooks().rumi_hook_quadtree(capi.ptr(packed), len(rel), 16, w - 16, 16, h - 16, c.ctor[0], capi.ptr(out), len(out), C.byref(m)) == 0
    assert [rel[i] for i in out[:m.value]] == want, f"{c.id} ({c.cite}): host quadtree"
    cand = np.zeros(len(rel), O.KP_DTYPE)
    cand["x"], cand["y"], cand["response"] = x, y, s
    ref = O.octree(cand, 16, w - 16, 16, h - 16, c.ctor[0])
    assert [(int(k["x"]), int(k["y"]), int(k["response"])) for k in ref] == want, f"{c.id} ({c.cite}): oracle octree"


def test_transcription_reproduces_every_hand_written_case():
    """py_octree may serve as the reference of the 64-dot cases only because it gives every literal of family B."""
    hand = [c for c in CASES if c.family == "B"]
    assert len(hand) >= 13
    for c in hand:
        h, w = c.frame.shape
        rel = _rel(c)
        got = [rel[i] for i in EC.py_octree(rel, w - 32, h - 32, c.ctor[0], PRIMS.std_sort)]
        assert got == [(x - 16, y - 16, r) for x, y, r in c.sel[0]], c.id


def test_every_family_rule_cell_has_a_case_or_a_reason():
    cov = EC.coverage(CASES + BIG)
    for fam, rules in EC.RULES.items():
        for r in rules:
            has, na = bool(cov.get((fam, r))), (fam, r) in EC.NO_CASE
            assert has != na, f"family {fam}, rule {r}: " + ("both a case and a reason" if has else "no case and no reason")
            if na:
                assert len(EC.NO_CASE[(fam, r)]) > 20
    assert set(cov) | set(EC.NO_CASE) == {(f, r) for f, rs in EC.RULES.items() for r in rs}
    assert len({c.id for c in CASES + BIG}) == len(CASES + BIG)
    for c in CASES + BIG:
        assert c.cite.startswith("lib_src/ORBextractor.cc:") and (c.frame.shape[1] <= 320 and c.frame.shape[0] <= 240 or c.name == "skip-column")


@pytest.mark.parametrize("th", [7, 20, 100])
def test_dot_property(th):
    """One pixel of b + c on a flat field is a corner of cv::FAST exactly when c > th, with response c - 1, and nothing else is."""
    for c, n in ((th, 0), (th + 1, 1), (255 - EC.B0, 1)):
        img = np.full((21, 23), EC.B0, np.uint8)
        img[10, 11] = EC.B0 + c
        k = O.fast_cell(img, th)
        assert len(k) == n, (th, c)
        if n:
            assert (k["x"][0], k["y"][0], k["response"][0], k["size"][0], k["angle"][0]) == (11, 10, c - 1, 7, -1)
    img = np.full((21, 23), 250, np.uint8)                       # a dark dot works the same way
    img[10, 11] = 250 - (th + 1)
    assert O.fast_cell(img, th)["response"].tolist() == [th]


def test_model_tables():
    """The model's literals against the constructor tables of oracle and product, and the helper grid against the A literals."""
    assert O.OracleExtractor(1000, 1.2, 8, 20, 7).tables()["umax"].tolist() == EC.UMAX
    from rumi_slam_amd.extractor import tables
    assert tables(1000, 1.2, 8)["umax"].tolist() == EC.UMAX
    assert np.array_equal(np.array(EC.scale_table(1.2, 8), np.float32), tables(1000, 1.2, 8)["scale"])
    assert PAT[:4].tolist() == [[8, -3], [9, 5], [4, 2], [7, -12]]
    for c in CASES:
        if c.family == "A":                                       # cell_major orders the B candidates: it must give the A literals
            h, w = c.frame.shape
            assert [p[:2] for p in EC.cell_major(w, h, c.cand[0])] == [p[:2] for p in c.cand[0]], c.id
    assert [EC.c_round(v) for v in (1.49, 1.5, 2.5, 0.49)] == [1, 2, 3, 0]
    unb = next(c for c in CASES if c.name == "unblurred")       # the case can tell the two levels apart: the model's angles differ
    assert EC.np_angle(unb.frame, EC.CX, EC.CX, PRIMS) != EC.np_angle(EC.np_blur(unb.frame), EC.CX, EC.CX, PRIMS)


def test_geometry_searches():
    """The searches the cases rest on, run here: smallest skip geometries and level sizes that depend on the rounding."""
    assert EC.search_skips() == EC.SKIP_SEARCH
    assert EC.search_level_sizes() == EC.LEVEL_SIZE_SEARCH


def test_skip_rules_only_skip_empty_regions():
    """:752 and :760 differ (maxBorderY - 3 against maxBorderX - 6) but neither loses a pixel: over every accepted size the cells that run tile
    19 .. n - 20 exactly once, and a skipped cell's range would have been empty."""
    for n in list(range(67, 700)) + [1222, 1223, 1224, 1259]:
        cols = sorted({(c[2], c[3]) for c in EC.cells(n, 67)})
        rows = sorted({(c[4], c[5]) for c in EC.cells(max(67, (n + 1) // 2), n)})
        assert all(a <= b for a, b in cols), n                   # the column rule lets no degenerate window through; the row rule may (< 7 rows)
        for spans in (cols, [s for s in rows if s[0] <= s[1]]):
            assert spans[0][0] == 19 and spans[-1][1] == n - 20, n
            assert all(a[1] + 1 == b[0] for a, b in zip(spans, spans[1:])), n
    # the row skip at its smallest size, through the oracle: a dot on the last detectable row next to the skipped cell row is found once
    h, w = EC.SKIP_SEARCH[1], 644
    assert len({c[0] for c in EC.cells(w, h)}) == EC.grid(w, h)[1] - 1
    img = EC.dots(w, h, [(300, h - 20, 50), (320, h - 19, 50)])
    o = O.OracleExtractor(50, 1.2, 1, 20, 7)
    o.extract(img, (0, 1000))
    assert [(int(k["x"]) + 16, int(k["y"]) + 16, int(k["response"])) for k in o.keypoints(0, False)] == [(300, h - 20, 49)]
