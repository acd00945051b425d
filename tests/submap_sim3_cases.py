"""The sequential rule of the RANSAC of CloudMerging::ComputeSubmapSim3 (R/lib_src/CloudMerging.cc:643-741 around the rumination overload of
Sim3Solver::iterate, R/lib_src/Sim3Solver.cc:292-404) as plain Python, and constructed per-iteration tables with hand-written outcomes.

``replay`` walks the solvers as upstream does: one Sim3Solver after the other, ``while (!bNoMore && !bConverge) iterate(20, ...)``, the shared
bestInlierRatio passed by reference, ``break`` at the first convergence.  Its input is, per solver, the (valid, nIn, ratio) of every iteration the
solver could run; a degenerate minimal set (valid == 0) follows rumi_slam_amd.sim3solver.Sim3Solver._hyp: it repeats the solver's last valid
iteration, or counts 0 inliers under its own ratio when the solver has none yet.

test_submap_sim3_cpu.py holds ``replay`` to the hand-written outcomes, test_submap_sim3_gpu.py holds rumi_submap_sim3_ransac to ``replay``."""
import collections

import numpy as np

F32 = np.float32
NOT_REACHED, CONVERGED, EXHAUSTED = 0, 1, 2
R01 = float(F32(0.1))                        # 0.1f = 0.100000001490116...: (double)0.1f > 0.10 holds
BELOW = lambda x: float(np.nextafter(F32(x), F32(-1)))

Result = collections.namedtuple("Result", "state its best_hyp best_inliers best_ratio_after")


def replay(solvers, tables, best_ratio_in=0.0, block=20):
    """solvers: [(min_inliers, its)]; tables: per solver (valid [its], nIn [its], ratio [its]).  Returns (results per solver, its_consumed, the shared ratio
    at the end).  best_hyp is a position in the stream of all solvers' iterations: that of the iteration whose transform the solver holds as mBest*."""
    best_ratio = F32(best_ratio_in)
    out, pos, done = [], 0, False
    for (min_inl, its), (valid, n_in, ratio) in zip(solvers, tables):
        if done:
            out.append(None)
            continue
        best_n, best_hyp, last, used, conv = 0, -1, None, 0, False
        while used < its and not conv:                    # one iterate(block, ...) per turn
            for _ in range(block):
                if used >= its:
                    break
                h = used
                if valid[h]:
                    last = (int(n_in[h]), F32(ratio[h]), pos + h)
                elif last is None:
                    last = (0, F32(ratio[h]), pos + h)
                used += 1
                if last[1] >= best_ratio and last[0] >= best_n:
                    best_n, best_ratio, best_hyp = last[0], last[1], last[2]
                    if float(last[1]) > 0.10 and last[0] > min_inl:
                        conv = True
                        break
        pos += used
        out.append(Result(CONVERGED if conv else EXHAUSTED, used, best_hyp, best_n, float(best_ratio)))
        done = conv
    out = [r if r is not None else Result(NOT_REACHED, 0, -1, 0, float(best_ratio)) for r in out]
    return out, pos, float(best_ratio)


Table = collections.namedtuple("Table", "id why solvers tables best_ratio_in expect its_consumed best_ratio")


def _t(rows):
    """rows of (valid, nIn, ratio) -> the three arrays"""
    return (np.array([r[0] for r in rows], bool), np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], F32))


def constructed_tables():
    """Hand-written outcomes: every expectation below was worked out from the rule's text, not from a run."""
    T = []
    ok, weak = (1, 30, 0.5), (1, 5, 0.05)               # converges under min_inliers 20; taken (from 0) but converges nowhere
    # 1: the very first iteration converges
    T.append(Table("converge_at_0", "stream position 0 converges; the second solver is not reached", [(20, 4), (20, 3)], [_t([ok, weak, weak, weak]), _t([ok] * 3)], 0.0,
                   [Result(CONVERGED, 1, 0, 30, 0.5), Result(NOT_REACHED, 0, -1, 0, 0.5)], 1, 0.5))
    # 2: the last iteration of solver 0
    T.append(Table("converge_at_last_of_solver0", "solver 0 converges on its last iteration", [(20, 3), (20, 3)], [_t([weak, weak, ok]), _t([ok] * 3)], 0.0,
                   [Result(CONVERGED, 3, 2, 30, 0.5), Result(NOT_REACHED, 0, -1, 0, 0.5)], 3, 0.5))
    # 3: the first iteration of solver 1; solver 0's two weak iterations are equal, the later (1) is held
    T.append(Table("converge_at_first_of_solver1", "solver 0 is exhausted, solver 1 converges at once", [(20, 2), (20, 3)], [_t([weak, weak]), _t([ok, weak, weak])], 0.0,
                   [Result(EXHAUSTED, 2, 1, 5, 0.05), Result(CONVERGED, 1, 2, 30, 0.5)], 3, 0.5))
    # 4: nothing converges: ratio never above 0.1 or count never above min_inliers
    T.append(Table("nothing_converges", "every solver exhausted, its_consumed = the sum", [(20, 3), (20, 25), (20, 2)],
                   [_t([(1, 30, 0.05), (1, 19, 0.06), (1, 30, 0.04)]), _t([(1, 20, 0.3)] + [(1, 3, 0.01)] * 24), _t([(1, 25, 0.2), (1, 25, 0.29)])], 0.0,
                   # solver 0: it 0 taken (30, .05); it 1 has 19 < 30: not taken; it 2 ratio .04 < .05: not taken.  solver 1: (20, .3) taken at stream 3, 20 is not > 20.
                   # solver 2: ratios .2 and .29 are below .3: nothing taken
                   [Result(EXHAUSTED, 3, 0, 30, 0.05), Result(EXHAUSTED, 25, 3, 20, float(F32(0.3))), Result(EXHAUSTED, 2, -1, 0, float(F32(0.3)))], 30, float(F32(0.3))))
    # 5: two identical iterations: the later one is held
    T.append(Table("tie_later_wins", "two identical iterations: >= on both tests, the later is best_hyp", [(20, 4)], [_t([(1, 7, 0.08), (1, 3, 0.08), (1, 7, 0.08), (1, 6, 0.09)])], 0.0,
                   [Result(EXHAUSTED, 4, 2, 7, float(F32(0.08)))], 4, float(F32(0.08))))
    # 6: ratio exactly 0.1f
    T.append(Table("ratio_0.1f_converges", "ratio == 0.1f with nIn == min_inliers + 1: (double)0.1f > 0.10", [(20, 2)], [_t([(1, 21, R01), weak])], 0.0,
                   [Result(CONVERGED, 1, 0, 21, R01)], 1, R01))
    T.append(Table("ratio_0.1f_min_inliers", "ratio == 0.1f with nIn == min_inliers: taken, does not converge", [(20, 2)], [_t([(1, 20, R01), weak])], 0.0,
                   [Result(EXHAUSTED, 2, 0, 20, R01)], 2, R01))
    T.append(Table("ratio_below_0.1f", "the float below 0.1f is below 0.10 in double: no convergence whatever the count", [(20, 1)], [_t([(1, 99, BELOW(R01))])], 0.0,
                   [Result(EXHAUSTED, 1, 0, 99, BELOW(R01))], 1, BELOW(R01)))
    # 7: one float step below bestRatio: not taken
    T.append(Table("one_step_below_best", "a ratio one float step below bestRatio is not taken, the same ratio is", [(20, 3)],
                   [_t([(1, 5, 0.07), (1, 50, BELOW(F32(0.07))), (1, 6, 0.07)])], 0.0, [Result(EXHAUSTED, 3, 2, 6, float(F32(0.07)))], 3, float(F32(0.07))))
    # 8: bestRatio carried over blocks solver 1's better count
    T.append(Table("carried_ratio_blocks", "bestRatio of solver 0 (0.09) blocks solver 1's 40 inliers at ratio 0.08; mnBestInliers is per solver", [(20, 2), (20, 3)],
                   [_t([(1, 10, 0.09), (1, 4, 0.02)]), _t([(1, 40, 0.08), (1, 2, 0.09), (1, 1, 0.09)])], 0.0,
                   # solver 1: it 0 ratio .08 < .09: no.  it 1: .09 >= .09 and 2 >= 0: taken.  it 2: 1 < 2: not taken
                   [Result(EXHAUSTED, 2, 0, 10, float(F32(0.09))), Result(EXHAUSTED, 3, 3, 2, float(F32(0.09)))], 5, float(F32(0.09))))
    # 9: degenerate sets
    T.append(Table("degenerate_first", "a degenerate set first: 0 inliers under its own ratio, repeated by the next degenerate set; never converges on it", [(20, 4)],
                   [_t([(0, 30, 0.5), (0, 30, 0.9), (1, 25, 0.5), (1, 30, 0.6)])], 0.0,
                   # it 0: (0, .5) taken, best_hyp 0, 0 > 20 fails.  it 1 repeats it 0: .5 >= .5 and 0 >= 0: taken again, best_hyp stays 0.  it 2: (25, .5) taken and converges
                   [Result(CONVERGED, 3, 2, 25, 0.5)], 3, 0.5))
    T.append(Table("degenerate_middle", "a degenerate set in the middle repeats the last valid iteration and is taken as its equal", [(20, 4), (20, 2)],
                   [_t([(1, 8, 0.06), (1, 2, 0.01), (0, 30, 0.5), (1, 8, 0.05)]), _t([(0, 30, 0.5), (1, 30, 0.5)])], 0.0,
                   # solver 0: it 0 taken.  it 1 (2, .01) not taken but becomes `last`.  it 2 degenerate repeats (2, .01): not taken.  it 3: ratio .05 < .06: no.
                   # solver 1 starts without a last: it 0 degenerate counts 0 under .5: taken (best_hyp 4), no convergence.  it 1 converges.
                   [Result(EXHAUSTED, 4, 0, 8, float(F32(0.06))), Result(CONVERGED, 2, 5, 30, 0.5)], 6, 0.5))
    T.append(Table("degenerate_repeats_best", "a degenerate set right after the best iteration repeats it: taken, best_hyp stays the valid one", [(50, 3)],
                   [_t([(1, 9, 0.07), (0, 0, 0.0), (1, 8, 0.07)])], 0.0, [Result(EXHAUSTED, 3, 0, 9, float(F32(0.07)))], 3, float(F32(0.07))))
    # 10: best_ratio_in > 0
    T.append(Table("best_ratio_in", "best_ratio_in = 0.2 blocks everything below it: nothing is taken, best_hyp stays -1", [(20, 2), (20, 2)],
                   [_t([(1, 30, 0.15), (1, 30, 0.19)]), _t([(1, 30, 0.2), (1, 5, 0.1)])], 0.2,
                   [Result(EXHAUSTED, 2, -1, 0, float(F32(0.2))), Result(CONVERGED, 1, 2, 30, float(F32(0.2)))], 3, float(F32(0.2))))
    # 11: more than one block of 20 in a solver, converging inside the second
    T.append(Table("second_block", "a solver of 45 iterations converging at its 31st", [(20, 45)], [_t([weak] * 30 + [ok] + [weak] * 14)], 0.0,
                   [Result(CONVERGED, 31, 30, 30, 0.5)], 31, 0.5))
    ids = [t.id for t in T]
    assert len(set(ids)) == len(ids)
    return T
