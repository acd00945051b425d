"""CPU checks of what the batched Sim3 RANSAC (rumi_sim3_ransac_batch, rumi_slam_amd.sim3solver.Sim3SolverBatch) rests on: a window of the
shared rand() stream drawn per solver without consuming it, the local convergence rule (the first valid iteration above mRansacMinInliers
returns; a solver that never converges uses exactly its mRansacMaxIts), and the round scheduler, with the CPU oracle standing in for
the device."""
import numpy as np
import pytest

import oracle_lib as O
from rumi_slam_amd.sim3solver import GlibcRand, Sim3Solver, Sim3SolverBatch
from sim3_batch_scene import RUNS, OracleOptimizer, assert_same_results, make_solvers, reference_loop


@pytest.mark.parametrize("N", [3, 64, 90])
def test_draw_window_equals_sequential_draws_and_keeps_the_state(N):
    g = GlibcRand(0)
    for _ in range(17):                                  # somewhere inside the stream
        g.rand()
    before = g.state()
    win = g.draw_window(N, 50)
    assert g.state() == before
    s = Sim3Solver(None, np.ones((N, 3)), np.ones((N, 3)), np.ones(N), np.ones(N), np.ones(4), np.ones(4), rng=g)
    seq, _ = s._draw_block(50)
    assert np.array_equal(win, seq)
    # the window of a second solver starts at a whole triple of the stream, wherever the first stopped
    g.set_state(before)
    g.advance(20)
    after20 = g.state()
    g.set_state(before)
    s._draw_block(20)
    assert g.state() == after20


def _local_rule(solvers, rng, spoil=None):
    """Per solver, from the generator's current state: evaluate all its_left iterations at once on the oracle, return at the first valid one above
    mRansacMinInliers, else consume them all.  spoil(k, tri, X1, X2) may alter a solver's scene once its triples are known.
    Returns [(converged, iterations, triple of the returning iteration)]."""
    out = []
    for k, s in enumerate(solvers):
        left = s.mRansacMaxIts - s.mnIterations
        tri = rng.draw_window(s.N, left)
        o = O.sim3_ransac(s.X1, s.X2, s.s1, s.s2, s.K1, s.K2, tri, fix_scale=s.fix_scale)
        hit = np.nonzero(o["valid"] & (o["n_inliers"] > s.mRansacMinInliers))[0]
        its = int(hit[0]) + 1 if len(hit) else left
        rng.advance(its)
        out.append((len(hit) > 0, its, tri[its - 1].copy(), o))
    return out


@pytest.mark.parametrize("run", ["run1", "run2"])
def test_local_convergence_rule_equals_the_replay(run):
    opt = OracleOptimizer()
    g_ref, g_loc = GlibcRand(0), GlibcRand(0)
    want = reference_loop(make_solvers(opt, RUNS[run], g_ref))
    got = _local_rule(make_solvers(opt, RUNS[run], g_loc), g_loc)
    assert [(w[0], w[4]) for w in want] == [(x[0], x[1]) for x in got]
    assert g_ref.state() == g_loc.state()
    assert want[0][0] and want[0][4] > 20 and want[2][0], "the scene must need more than one block of the first solver"
    if run == "run2":
        assert not want[1][0] and want[1][4] == make_solvers(opt, RUNS[run], GlibcRand(0))[1].mRansacMaxIts, "the middle solver exhausts its iterations"


def test_degenerate_set_does_not_converge():
    """The minimal set of the iteration at which the first solver would return is made degenerate (its three correspondences coincide, as
    test_sim3solver_gpu.test_degenerate_set_and_bad_arguments builds one): upstream keeps the previous iteration's transform there (:493-494),
    whose count did not return, so neither rule may return at that iteration; both still agree on where the solver stops."""
    opt = OracleOptimizer()
    g0 = GlibcRand(0)
    first = _local_rule(make_solvers(opt, RUNS["run1"], g0)[:1], g0)[0]
    assert first[0]
    h, tri = first[1] - 1, first[2]

    def spoiled(rng):
        sv = make_solvers(opt, RUNS["run1"], rng)
        s = sv[0]
        s.X1, s.X2 = s.X1.copy(), s.X2.copy()
        s.X1[tri] = s.X1[tri[0]]; s.X2[tri] = s.X2[tri[0]]
        return sv

    g_ref, g_loc = GlibcRand(0), GlibcRand(0)
    want = reference_loop(spoiled(g_ref))
    got = _local_rule(spoiled(g_loc), g_loc)
    assert not got[0][3]["valid"][h], "the constructed set must be degenerate"
    assert got[0][1] != h + 1 and want[0][4] != h + 1
    assert [(w[0], w[4]) for w in want] == [(x[0], x[1]) for x in got]
    assert g_ref.state() == g_loc.state()


@pytest.fixture(scope="module")
def references():
    out = {}
    for run in RUNS:
        g = GlibcRand(0)
        out[run] = (reference_loop(make_solvers(OracleOptimizer(), RUNS[run], g)), g.rand())
    return out


@pytest.mark.parametrize("window", [7, 20, 60, 400, None])
@pytest.mark.parametrize("run", ["run1", "run2"])
def test_round_scheduler_equals_the_per_candidate_loop(references, run, window):
    want, next_rand = references[run]
    g = GlibcRand(0)
    opt = OracleOptimizer()
    solvers = make_solvers(opt, RUNS[run], g)
    got, rounds = Sim3SolverBatch(opt, solvers, g).run(window)
    assert_same_results(got, want)
    assert g.rand() == next_rand
    total = sum(w[4] for w in want)
    if window == 400:
        assert rounds == 1
    elif window is not None:
        assert rounds >= -(-total // window)
    assert [s.mnIterations for s in solvers] == [w[4] for w in want]


def test_solver_below_min_inliers_draws_nothing():
    """:228-231: N < mRansacMinInliers returns bNoMore at once; the next solver starts at the same place of the stream."""
    opt = OracleOptimizer()
    g_ref, g = GlibcRand(0), GlibcRand(0)
    ref = make_solvers(opt, RUNS["run1"], g_ref)
    ref[0].SetRansacParameters(0.99, 91, 300)
    want = reference_loop(ref)
    sv = make_solvers(opt, RUNS["run1"], g)
    sv[0].SetRansacParameters(0.99, 91, 300)
    got, _ = Sim3SolverBatch(opt, sv, g).run(20)
    assert not got[0][0] and got[0][4] == 0
    assert_same_results(got, want)
    assert g.rand() == g_ref.rand()
