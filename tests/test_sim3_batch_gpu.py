"""GPU checks of the batched Sim3 entries of place recognition (include/rumi_opt.h): rumi_sim3_ransac_batch returns, per (solver, iteration),
the bytes rumi_sim3_ransac returns and applies the sequential rule as the per-candidate loop does; rumi_optimize_sim3_batch returns, per
problem, the bytes of rumi_optimize_sim3.  Against the CPU oracle the tolerances are those of test_sim3solver_gpu.py (1e-4 on R, t, s;
integer outputs equal) and of test_optimizer_gpu.py (1e-4 on the Sim3, counts and status equal)."""
import numpy as np
import pytest

import oracle_lib as O
from rumi_slam_amd import capi
from rumi_slam_amd.optimizer import (SIM3_CONVERGED, SIM3_NOT_REACHED, SIM3_OPT_PROBLEM_DTYPE, SIM3_RANSAC_RESULT_DTYPE, SIM3_RANSAC_SOLVER_DTYPE,
                                     SIM3_WINDOW_ENDED)
from rumi_slam_amd.sim3solver import GlibcRand, Sim3SolverBatch
from sim3_batch_scene import RUNS, assert_same_results, make_solvers, problem, reference_loop
from sim3_scene import sim3_pair_problem, sim3_ransac_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def opt():
    from rumi_slam_amd.optimizer import Optimizer
    return Optimizer()


def _records(solvers, its_left=None):
    sol = np.zeros(len(solvers), SIM3_RANSAC_SOLVER_DTYPE)
    first = 0
    for k, (rec, s) in enumerate(zip(sol, solvers)):
        rec["first"], rec["n"], rec["min_inliers"], rec["fix_scale"], rec["K4_1"], rec["K4_2"] = first, s.N, s.mRansacMinInliers, int(s.fix_scale), s.K1, s.K2
        rec["its_left"] = s.mRansacMaxIts if its_left is None else its_left[k]
        first += s.N
    cat = lambda name: np.concatenate([getattr(s, name) for s in solvers])
    return sol, (cat("X1"), cat("X2"), cat("s1"), cat("s2"))


# ---- every (solver, iteration): the bytes of the single entry ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_sizes(opt):
    """N = 3, 65 (one past a wave) and 90, mixed fix_scale; the oracle's and the single entry's results of 65 iterations, computed once."""
    scenes = [(sim3_ransac_problem(4, n_solver=3, outlier_frac=0.0), True), (problem(8, 65, 0.50), False), (problem(7, 90, 0.45), True)]
    g = GlibcRand(0)
    tri = [g.draw_window(len(pr["X1"]), 65) for pr, _ in scenes]
    args = [(pr["X1"], pr["X2"], pr["sigma2_1"], pr["sigma2_2"], pr["K"], pr["K"], t) for (pr, _), t in zip(scenes, tri)]
    single = [opt.Sim3Ransac(*a, fix_scale=fix) for a, (_, fix) in zip(args, scenes)]
    oracle = [O.sim3_ransac(*a, fix_scale=fix) for a, (_, fix) in zip(args, scenes)]
    return scenes, tri, single, oracle


@pytest.mark.parametrize("R", [1, 64, 65])
def test_every_hypothesis_equals_the_single_entry(opt, three_sizes, R):
    scenes, tri, single, oracle = three_sizes
    sol = np.zeros(3, SIM3_RANSAC_SOLVER_DTYPE)
    first = 0
    for rec, (pr, fix) in zip(sol, scenes):
        n = len(pr["X1"])
        rec["first"], rec["n"], rec["min_inliers"], rec["its_left"], rec["fix_scale"], rec["K4_1"], rec["K4_2"] = first, n, n, 300, int(fix), pr["K"], pr["K"]
        first += n
    cat = lambda name: np.concatenate([pr[name] for pr, _ in scenes])
    res = opt.Sim3RansacBatch(sol, cat("X1"), cat("X2"), cat("sigma2_1"), cat("sigma2_2"), np.stack([t[:R] for t in tri]), want_all=True)
    for j in range(3):
        g, s, o = res["T12_all"][j], single[j], oracle[j]
        assert np.array_equal(res["n_inliers_all"][j], s["n_inliers"][:R]), f"solver {j}"
        mine = np.concatenate([s["R"][:R].reshape(R, 9), s["t"][:R], s["s"][:R, None], s["valid"][:R, None].astype(np.float32), np.zeros((R, 2), np.float32)], 1)
        assert g.tobytes() == mine.astype(np.float32).tobytes(), f"solver {j}: T12_all differs from rumi_sim3_ransac"
        # against the oracle, as test_sim3solver_gpu._close
        v = o["valid"][:R]
        assert np.array_equal(g[:, 13] != 0, v)
        assert np.array_equal(res["n_inliers_all"][j], o["n_inliers"][:R])
        if v.any():
            assert np.abs(g[v, :9].reshape(-1, 3, 3) - o["R"][:R][v]).max() < 1e-4
            assert np.abs(g[v, 9:12] - o["t"][:R][v]).max() < 1e-4 * max(1.0, np.abs(o["t"][:R][v]).max())
            assert np.abs(g[v, 12] - o["s"][:R][v]).max() < 1e-4 * max(1.0, np.abs(o["s"][:R][v]).max())
    # nothing has more inliers than correspondences: every solver uses the window up
    assert (res["state"] == [SIM3_WINDOW_ENDED, SIM3_NOT_REACHED, SIM3_NOT_REACHED]).all() and (res["its"] == [R, 0, 0]).all()
    assert not res["inliers"].any() and (res["hyp"] == -1).all()


# ---- the sequential rule --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def references(opt):
    """The per-candidate loop over the device's single entry, once per scene: results and the next rand()."""
    out = {}
    for run in RUNS:
        g = GlibcRand(0)
        out[run] = (reference_loop(make_solvers(opt, RUNS[run], g)), g.rand())
    return out


@pytest.mark.parametrize("window,rounds", [(250, 1), (20, None), (7, None), (None, None)])
@pytest.mark.parametrize("run", ["run1", "run2"])
def test_rounds_equal_the_per_candidate_loop(opt, references, run, window, rounds):
    want, next_rand = references[run]
    g = GlibcRand(0)
    got, used = Sim3SolverBatch(opt, make_solvers(opt, RUNS[run], g), g).run(window)
    assert_same_results(got, want)
    assert g.rand() == next_rand
    assert rounds is None or used == rounds
    if run == "run2":
        assert not want[1][0] and want[0][0] and want[2][0], "the exhausted solver sits between two that converge"


def test_converges_at_the_last_allowed_iteration_or_not_at_all(opt, references):
    want, _ = references["run1"]
    its0 = want[0][4]
    for cap, conv in [(its0, True), (its0 - 1, False)]:
        g_ref, g = GlibcRand(0), GlibcRand(0)
        ref = reference_loop(make_solvers(opt, RUNS["run1"], g_ref, max_its=[cap, None, None]))
        assert ref[0][0] == conv and ref[0][4] == cap
        got, used = Sim3SolverBatch(opt, make_solvers(opt, RUNS["run1"], g, max_its=[cap, None, None]), g).run(250)
        assert used == 1
        assert_same_results(got, ref)
        assert g.rand() == g_ref.rand()


def test_window_ends_inside_the_first_solver(opt, references):
    want, _ = references["run1"]
    assert want[0][4] > 20
    g = GlibcRand(0)
    solvers = make_solvers(opt, RUNS["run1"], g)
    sol, arrs = _records(solvers)
    res = opt.Sim3RansacBatch(sol, *arrs, np.stack([g.draw_window(s.N, 20) for s in solvers]))
    assert (res["state"] == [SIM3_WINDOW_ENDED, SIM3_NOT_REACHED, SIM3_NOT_REACHED]).all() and (res["its"] == [20, 0, 0]).all()
    assert (res["hyp"] == -1).all() and (res["n_inliers"] == 0).all() and not res["inliers"].any() and not res["T12"].any()
    # the window ends exactly where the first solver returns: the next one is reached with nothing left of the window
    R = want[0][4]
    res = opt.Sim3RansacBatch(sol, *arrs, np.stack([g.draw_window(s.N, R) for s in solvers]))
    assert (res["state"] == [SIM3_CONVERGED, SIM3_WINDOW_ENDED, SIM3_NOT_REACHED]).all() and (res["its"] == [R, 0, 0]).all()
    assert res["hyp"][0] == R - 1 and res["n_inliers"][0] == want[0][3]
    assert np.array_equal(res["inliers"][:solvers[0].N], want[0][2][0::2])


# ---- OptimizeSim3 of several candidates ----------------------------------------------------------------------------------------------
def _sim3_close(a, b, what):
    """test_optimizer_gpu._sim3_close"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.linalg.norm(a[:4] - b[:4]) <= 1e-4, f"{what}: rotation {a[:4]} vs {b[:4]}"
    assert np.linalg.norm(a[4:7] - b[4:7]) <= 1e-4 * max(np.linalg.norm(b[4:7]), 1.0), f"{what}: translation {a[4:7]} vs {b[4:7]}"
    assert abs(a[7] - b[7]) <= 1e-4 * abs(b[7]), f"{what}: scale {a[7]} vs {b[7]}"


@pytest.fixture(scope="module")
def opt_problems(opt):
    """n = 0, n = 9 (returns early: n - nBad < 10) and n = 400, with fix_scale / robust_first_pass mixed; the single entry's results, once."""
    empty = sim3_pair_problem(seed=8, n=0)
    probs = [(empty, True, True), (sim3_pair_problem(seed=7, n=9), False, True), (sim3_pair_problem(seed=3, n=400, scale=1.0), True, False)]
    single = [opt.OptimizeSim3(b["S0"], b["P1c"], b["P2c"], b["obs1"], b["obs2"], b["w1"], b["w2"], b["K"], b["K"], 10.0, fix, rob) for b, fix, rob in probs]
    return probs, single


def _opt_batch(opt, probs, order):
    rec = np.zeros(len(order), SIM3_OPT_PROBLEM_DTYPE)
    first = 0
    for r, k in zip(rec, order):
        b, fix, rob = probs[k]
        r["first"], r["n"], r["th2"], r["fix_scale"], r["robust_first_pass"], r["K4_1"], r["K4_2"] = first, len(b["w1"]), 10.0, int(fix), int(rob), b["K"], b["K"]
        first += len(b["w1"])
    cat = lambda name, w: np.concatenate([probs[k][0][name].reshape(-1, w) for k in order])
    res, S, status = opt.OptimizeSim3Batch(rec, np.stack([probs[k][0]["S0"] for k in order]), cat("P1c", 3), cat("P2c", 3), cat("obs1", 2), cat("obs2", 2),
                                           cat("w1", 1).ravel(), cat("w2", 1).ravel())
    return {k: (res[j], S[j], status[rec["first"][j]:rec["first"][j] + rec["n"][j]]) for j, k in enumerate(order)}


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)])
def test_optimize_sim3_batch_equals_the_single_entry(opt, opt_problems, order):
    probs, single = opt_problems
    got = _opt_batch(opt, probs, order)
    for k, (nin, nbad, early, S, st) in enumerate(single):
        res, Sb, stb = got[k]
        assert tuple(res) == (nin, nbad, int(early)), f"problem {k}"
        assert Sb.tobytes() == S.tobytes(), f"problem {k}: estimate differs from rumi_optimize_sim3"
        assert np.array_equal(stb, st), f"problem {k}: status"
    assert tuple(got[0][0]) == (0, 0, 1) and np.array_equal(got[0][1], probs[0][0]["S0"])
    assert got[1][0][2] == 1 and got[1][0][0] == 0 and got[2][0][2] == 0 and got[2][0][0] > 200
    for k in (1, 2):
        b, fix, rob = probs[k]
        nin_r, nbad_r, early_r, S_r, st_r = O.optimize_sim3(b["S0"], b["P1c"], b["P2c"], b["obs1"], b["obs2"], b["w1"], b["w2"], b["K"], b["K"], 10.0, fix, rob)
        assert tuple(got[k][0]) == (nin_r, nbad_r, int(early_r)) and np.array_equal(got[k][2], st_r)
        _sim3_close(got[k][1], S_r, f"problem {k}")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _raw_ransac(o, sol, arrs, tri, window):
    """The C entry with marked outputs: (status, message, outputs untouched)."""
    n, J = len(arrs[0]), len(sol)
    res = np.full(J, 0x5A, np.uint8).repeat(80).view(SIM3_RANSAC_RESULT_DTYPE); inl = np.full(n, 0x5A, np.uint8)
    nall = np.full((J, max(window, 1)), 0x5A5A5A5A, np.int32); Tall = np.full((J, max(window, 1), 16), 7.5, np.float32)
    P = capi.ptr
    rc = o._lib.rumi_sim3_ransac_batch(o._h, J, P(sol), n, *[P(a) for a in arrs], window, P(tri), P(res), P(inl), P(nall), P(Tall))
    msg = o._lib.rumi_last_error().decode()
    untouched = (res.view(np.uint8) == 0x5A).all() and (inl == 0x5A).all() and (nall == 0x5A5A5A5A).all() and (Tall == 7.5).all()
    return rc, msg, untouched


def test_ransac_batch_refusals(opt):
    from rumi_slam_amd.optimizer import Optimizer
    g = GlibcRand(0)
    solvers = make_solvers(opt, RUNS["run1"], g)[:2]
    sol, arrs = _records(solvers)
    arrs = tuple(np.ascontiguousarray(a) for a in arrs)
    tri = np.ascontiguousarray(np.stack([g.draw_window(s.N, 8) for s in solvers]))

    def refused(code, word, sol=sol, tri=tri, window=8, o=opt):
        rc, msg, untouched = _raw_ransac(o, sol, arrs, tri, window)
        assert rc == code and word in msg and untouched, (rc, msg, untouched)

    bad = sol.copy(); bad["n"][1] = 2
    refused(capi.RUMI_E_INVALID, "at least 3", sol=bad)
    bad = tri.copy(); bad[1, 7, 2] = solvers[1].N
    refused(capi.RUMI_E_INVALID, "out of range", tri=bad)
    bad = tri.copy(); bad[0, 0, 0] = -1
    refused(capi.RUMI_E_INVALID, "out of range", tri=bad)
    bad = sol.copy(); bad["its_left"][0] = 0
    refused(capi.RUMI_E_INVALID, "its_left", sol=bad)
    refused(capi.RUMI_E_INVALID, "window", window=0)
    bad = sol.copy(); bad["first"][1] -= 1
    refused(capi.RUMI_E_INVALID, "ranges", sol=bad)
    small = Optimizer(max_kf=1, max_mp=1, max_edges=1)
    refused(capi.RUMI_E_CAPACITY, "arenas hold", o=small)
    rc, msg, untouched = _raw_ransac(opt, sol, arrs, tri, 8)        # the handle still works
    assert rc == capi.RUMI_OK and not untouched


def test_optimize_batch_refusals(opt, opt_problems):
    from rumi_slam_amd.optimizer import Optimizer
    probs, _ = opt_problems
    b = probs[2][0]
    n = len(b["w1"])
    rec = np.zeros(1, SIM3_OPT_PROBLEM_DTYPE)
    rec["n"], rec["th2"], rec["K4_1"], rec["K4_2"] = n, 10.0, b["K"], b["K"]
    arrs = [np.ascontiguousarray(b[k]) for k in ("P1c", "P2c", "obs1", "obs2", "w1", "w2")]

    def call(o, rec):
        S = np.ascontiguousarray(b["S0"], np.float64).reshape(1, 8).copy(); status = np.full(n, 0x5A, np.uint8); res = np.full((1, 3), -77, np.int32)
        P = capi.ptr
        rc = o._lib.rumi_optimize_sim3_batch(o._h, 1, P(rec), n, *[P(a) for a in arrs], P(S), P(status), P(res))
        return rc, o._lib.rumi_last_error().decode(), np.array_equal(S[0], b["S0"]) and (status == 0x5A).all() and (res == -77).all()

    bad = rec.copy(); bad["n"] = -1
    rc, msg, untouched = call(opt, bad)
    assert rc == capi.RUMI_E_INVALID and "ranges" in msg and untouched
    bad = rec.copy(); bad["first"] = 1
    rc, msg, untouched = call(opt, bad)
    assert rc == capi.RUMI_E_INVALID and "ranges" in msg and untouched
    rc, msg, untouched = call(Optimizer(max_kf=1, max_mp=1, max_edges=1), rec)
    assert rc == capi.RUMI_E_CAPACITY and "arenas hold" in msg and untouched
    rc, msg, untouched = call(opt, rec)
    assert rc == capi.RUMI_OK and not untouched
