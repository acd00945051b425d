"""Shared by the CPU and GPU tests of the batched Sim3 RANSAC: the two three-solver scenes, the reference's per-candidate loop over mirror
solvers, and an optimizer whose two RANSAC entries are the CPU oracle (``O.sim3_ransac``) plus the select rule restated in Python."""
import numpy as np

import oracle_lib as O
from rumi_slam_amd.optimizer import SIM3_CONVERGED, SIM3_EXHAUSTED, SIM3_NOT_REACHED, SIM3_WINDOW_ENDED
from rumi_slam_amd.sim3solver import Sim3Solver
from sim3_scene import sim3_ransac_problem

# (seed, n_solver, outlier_frac, mRansacMinInliers) per candidate, SetRansacParameters(0.99, min, 300)
RUN1 = [(7, 90, 0.45, 40), (8, 65, 0.50, 25), (9, 120, 0.55, 45)]
RUN2 = [(7, 90, 0.45, 40), (9, 40, 0.90, 12), (8, 65, 0.50, 25)]       # the middle solver never converges: all of its mRansacMaxIts
RUNS = {"run1": RUN1, "run2": RUN2}

_problems = {}


def problem(seed, n_solver, outlier_frac):
    key = (seed, n_solver, outlier_frac)
    if key not in _problems:
        _problems[key] = sim3_ransac_problem(seed, n_solver=n_solver, outlier_frac=outlier_frac)
    return _problems[key]


def make_solvers(opt, run, rng, fix_scale=None, max_its=None):
    """One mirror Sim3Solver per candidate over the shared generator; indices1 spreads the correspondences over mN1 = 2 N slots.
    fix_scale / max_its: optional per-candidate overrides (max_its replaces mRansacMaxIts after SetRansacParameters)."""
    out = []
    for k, (seed, n, frac, min_inl) in enumerate(run):
        pr = problem(seed, n, frac)
        s = Sim3Solver(opt, pr["X1"], pr["X2"], pr["sigma2_1"], pr["sigma2_2"], pr["K"], pr["K"], fix_scale=bool(fix_scale[k]) if fix_scale else False,
                       indices1=np.arange(n) * 2, mN1=2 * n, rng=rng)
        s.SetRansacParameters(0.99, min_inl, 300)
        if max_its and max_its[k] is not None:
            s.mRansacMaxIts = int(max_its[k])
        out.append(s)
    return out


def reference_loop(solvers):
    """LoopClosing.cc:655-676 per candidate: while (!bConverge && !bNoMore) iterate(20, bNoMore, vbInliers, nInliers, bConverge).
    Per solver (converged, T12, vbInliers, nInliers, iterations), in the form Sim3SolverBatch.run returns."""
    out = []
    for s in solvers:
        conv = no_more = False
        while not conv and not no_more:
            T, no_more, vb, n_in, conv = s.iterate_converge(20)
        out.append((True, T, vb, n_in, s.mnIterations) if conv else (False, np.eye(4, dtype=np.float32), np.zeros(s.mN1, bool), 0, s.mnIterations))
    return out


def assert_same_results(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[4] == w[4], f"solver {k}: converged / iterations {g[0], g[4]} vs {w[0], w[4]}"
        assert g[3] == w[3], f"solver {k}: inliers {g[3]} vs {w[3]}"
        assert g[1].dtype == w[1].dtype and g[1].tobytes() == w[1].tobytes(), f"solver {k}: T12"
        assert np.array_equal(g[2], w[2]), f"solver {k}: inlier mask"


def select(valid, n_inliers, min_inliers, its_left, R):
    """The sequential rule of rumi_sim3_ransac_batch over per-(solver, iteration) results: state, its, hyp per solver."""
    J = len(min_inliers)
    state, its, hyp = np.zeros(J, np.int32), np.zeros(J, np.int32), np.full(J, -1, np.int32)
    pos, ended = 0, False
    for j in range(J):
        if ended:
            state[j] = SIM3_NOT_REACHED
            continue
        end = min(pos + int(its_left[j]), R)
        hit = [h for h in range(pos, end) if valid[j][h] and n_inliers[j][h] > min_inliers[j]]
        if hit:
            state[j], its[j], hyp[j] = SIM3_CONVERGED, hit[0] - pos + 1, hit[0]
            pos = hit[0] + 1
        elif pos + int(its_left[j]) <= R:
            state[j], its[j] = SIM3_EXHAUSTED, its_left[j]
            pos += int(its_left[j])
        else:
            state[j], its[j] = SIM3_WINDOW_ENDED, R - pos
            ended = True
    return state, its, hyp


class OracleOptimizer:
    """Stands in for the device: Sim3Ransac and Sim3RansacBatch of rumi_slam_amd.optimizer.Optimizer over the CPU oracle."""

    def Sim3Ransac(self, X1, X2, s1, s2, K1, K2, tri, fix_scale=False, score=None, want_inliers=True):
        return O.sim3_ransac(X1, X2, s1, s2, K1, K2, tri, fix_scale=fix_scale, score=score)

    def Sim3RansacBatch(self, solvers, X1, X2, s1, s2, triples, want_all=False):
        J, R = len(solvers), triples.shape[1]
        per = []
        for j, rec in enumerate(solvers):
            a, b = int(rec["first"]), int(rec["first"] + rec["n"])
            per.append(O.sim3_ransac(X1[a:b], X2[a:b], s1[a:b], s2[a:b], rec["K4_1"], rec["K4_2"], triples[j], fix_scale=bool(rec["fix_scale"])))
        state, its, hyp = select([p["valid"] for p in per], [p["n_inliers"] for p in per], solvers["min_inliers"], solvers["its_left"], R)
        T12, n_in, inl = np.zeros((J, 16), np.float32), np.zeros(J, np.int32), np.zeros(len(X1), bool)
        for j, rec in enumerate(solvers):
            if hyp[j] >= 0:
                p, h = per[j], hyp[j]
                T12[j, :9], T12[j, 9:12], T12[j, 12], T12[j, 13] = p["R"][h].ravel(), p["t"][h], p["s"][h], 1
                n_in[j] = p["n_inliers"][h]
                inl[rec["first"]:rec["first"] + rec["n"]] = p["inliers"][h]
        return dict(state=state, its=its, hyp=hyp, n_inliers=n_in, T12=T12, inliers=inl)
