"""CPU side of the sub-map alignment session (include/rumi_opt.h, rumi_submap_sim3_*): the plain-Python replay of the loop of CloudMerging.cc:643-741
against hand-written outcomes, SubmapSim3's drawing of the minimal sets against the C library's rand() and the oracle's draw, and the declarations."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import submap_sim3_cases as SC
from rumi_slam_amd import capi
from rumi_slam_amd.sim3solver import GlibcRand
from rumi_slam_amd.submap import SUBMAP_RESULT_DTYPE, SUBMAP_SOLVER_DTYPE, SubmapSolver, draw_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = SC.constructed_tables()


def _same(got, want):
    assert (got.state, got.its, got.best_hyp, got.best_inliers) == (want.state, want.its, want.best_hyp, want.best_inliers)
    assert np.float32(got.best_ratio_after) == np.float32(want.best_ratio_after)


@pytest.mark.parametrize("t", TABLES, ids=[t.id for t in TABLES])
def test_replay_against_hand_written_outcomes(t):
    res, used, ratio = SC.replay(t.solvers, t.tables, t.best_ratio_in)
    assert used == t.its_consumed and np.float32(ratio) == np.float32(t.best_ratio)
    assert len(res) == len(t.expect)
    for got, want in zip(res, t.expect):
        _same(got, want)


@pytest.mark.parametrize("block", [1, 7, 20, 1000])
def test_replay_does_not_depend_on_the_block(block):
    for t in TABLES:
        res, used, _ = SC.replay(t.solvers, t.tables, t.best_ratio_in, block=block)
        assert used == t.its_consumed
        for got, want in zip(res, t.expect):
            _same(got, want)


def test_table_covers_what_it_claims():
    ids = {t.id for t in TABLES}
    for need in ("converge_at_0", "converge_at_last_of_solver0", "converge_at_first_of_solver1", "nothing_converges", "tie_later_wins", "ratio_0.1f_converges",
                 "ratio_0.1f_min_inliers", "one_step_below_best", "carried_ratio_blocks", "degenerate_first", "degenerate_middle", "best_ratio_in"):
        assert need in ids
    assert SC.R01 > 0.10 and SC.BELOW(SC.R01) < 0.10          # what the 0.1f cases rest on


def _solver(n, its):
    z = np.zeros((n, 3), np.float32)
    return SubmapSolver(z, z, np.ones(n, np.float32), np.ones(n, np.float32), [1, 1, 0, 0], [1, 1, 0, 0], np.zeros(8), np.zeros(8), 6, its)


def test_draws_share_one_stream():
    """Solvers of different n draw their segments one after the other from the one generator: against the C library's rand() through the oracle's draw
    (srand once, then one orc_sim3_draw_triples per solver) and against GlibcRand.draw_window on the advanced generator."""
    solvers = [_solver(3, 1), _solver(40, 7), _solver(90, 20), _solver(129, 33)]
    rng = GlibcRand(11)
    tri = draw_stream(solvers, rng)
    assert tri.shape == (61, 3)
    L = O._olib()
    L.orc_sim3_draw_triples.restype = None
    L.orc_sim3_draw_triples.argtypes = [O.C.c_int32, O.C.c_int32, O.C.c_void_p]
    O.libc_srand(11)
    h = 0
    ref = GlibcRand(11)
    for s in solvers:
        want = np.zeros((s.its, 3), np.int32)
        L.orc_sim3_draw_triples(s.N, s.its, want.ctypes.data_as(O.C.c_void_p))
        assert np.array_equal(tri[h:h + s.its], want)
        assert np.array_equal(tri[h:h + s.its], ref.draw_window(s.N, s.its))
        ref.advance(s.its)
        seg = tri[h:h + s.its]
        assert seg.min() >= 0 and seg.max() < s.N and all(len(set(r)) == 3 for r in seg.tolist())
        h += s.its
    # the generator stands after the last draw
    assert rng.rand() == O.libc_rand() == ref.rand()
    # the first solver's segment is what a lone solver draws from the same seed
    assert np.array_equal(tri[:1], O.sim3_draw_triples(11, 3, 1))


def test_generator_position_after_a_partial_run():
    """What SubmapSim3.ransac does with the generator: back to the start, then three draws per consumed iteration."""
    solvers = [_solver(10, 5), _solver(20, 5)]
    rng = GlibcRand(3)
    start = rng.state()
    draw_stream(solvers, rng)
    rng.set_state(start)
    rng.advance(7)
    ref = GlibcRand(3)
    for _ in range(21):
        ref.rand()
    assert rng.rand() == ref.rand()


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"\b(rumi_[a-z0-9_]+)\s*\(", text))


def test_declarations_and_record_sizes():
    opt = _declared("rumi_opt.h")
    for name in ("rumi_submap_sim3_begin", "rumi_submap_sim3_end", "rumi_submap_sim3_score", "rumi_submap_sim3_ransac"):
        assert name in opt and name in capi.OPT_SYMBOLS
    assert "rumi_hook_submap_sim3_set_chunk" in _declared("rumi_testhooks.h") and "rumi_hook_submap_sim3_set_chunk" in capi.HOOK_SYMBOLS
    # the records as the header lays them out: 5 int32, 8 float, 4 bytes of padding before the doubles; 4 int32, 17 float
    assert SUBMAP_SOLVER_DTYPE.itemsize == 184 and SUBMAP_SOLVER_DTYPE.fields["S_kf1w"][1] == 56 and SUBMAP_SOLVER_DTYPE.fields["S_kf2w"][1] == 120
    assert SUBMAP_RESULT_DTYPE.itemsize == 84 and SUBMAP_RESULT_DTYPE.fields["T12"][1] == 20
    lib = capi.lib()
    for name in ("rumi_submap_sim3_begin", "rumi_submap_sim3_end", "rumi_submap_sim3_score", "rumi_submap_sim3_ransac", "rumi_hook_submap_sim3_set_chunk"):
        getattr(lib, name)


def test_entries_refuse_a_null_handle():
    """Validation comes before anything that needs a device."""
    from rumi_slam_amd.optimizer import _lib
    L = _lib()
    import ctypes as C
    L.rumi_submap_sim3_begin.argtypes = [C.c_void_p, C.c_void_p]
    L.rumi_submap_sim3_end.argtypes = [C.c_void_p]
    assert L.rumi_submap_sim3_begin(None, None) == capi.RUMI_E_INVALID
    assert L.rumi_submap_sim3_end(None) == capi.RUMI_E_INVALID
    assert capi.hooks().rumi_hook_submap_sim3_set_chunk(None, 4) == capi.RUMI_E_INVALID
