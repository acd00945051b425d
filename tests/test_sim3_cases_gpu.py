"""The constructed Sim3 cases of sim3_cases.py on the device: rumi_sim3_ransac, rumi_sim3_ransac_batch, rumi_sim3_inliers, rumi_optimize_sim3 and the host
mirror over them.  Hypotheses are held to horn64 (float64, numpy.linalg.eigh) and to the oracle within TOL_DR / TOL_DT / TOL_DS of sim3_cases.py: four times
what test_sim3_cases_cpu.py measures for the oracle against horn64 on the same triples.  CheckInliers is held to no tolerance at all: the float32
restatement, fed with the device's own hypothesis record, must give the device's mask bit for bit, thresholds one float32 step away included."""
import numpy as np
import pytest

import oracle_lib as O
import sim3_cases as S
from rumi_slam_amd.optimizer import SIM3_CONVERGED, SIM3_NOT_REACHED, SIM3_RANSAC_SOLVER_DTYPE, SIM3_WINDOW_ENDED
from rumi_slam_amd.sim3solver import Sim3SolverBatch
from sim3_batch_scene import assert_same_results, reference_loop

pytestmark = pytest.mark.gpu

CASES = S.all_cases()
IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def opt():
    from rumi_slam_amd.optimizer import Optimizer
    return Optimizer()


@pytest.fixture(scope="module")
def device(opt):
    """rumi_sim3_ransac of every case, once."""
    return {c.id: opt.Sim3Ransac(*c.args(), fix_scale=c.fix_scale, score=c.score) for c in CASES}


@pytest.fixture(scope="module")
def oracle():
    return {c.id: O.sim3_ransac(*c.args(), fix_scale=c.fix_scale, score=c.score) for c in CASES}


# ---- hypotheses ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", IDS)
def test_valid_flags_equal_the_oracle(device, oracle, id):
    c, g, o = S.case(id), device[id], oracle[id]
    assert np.array_equal(g["valid"], o["valid"]), f"{id}: hypotheses {np.flatnonzero(g['valid'] != o['valid'])}"
    if c.expect_valid is not None:
        assert np.array_equal(g["valid"], c.expect_valid)
    inv = ~g["valid"]
    assert (g["R"][inv] == np.eye(3, dtype=np.float32)).all() and (g["t"][inv] == 0).all() and (g["s"][inv] == 1).all()


@pytest.mark.parametrize("id", [c.id for c in CASES if c.keep.any()])
def test_hypotheses_against_horn64_and_the_oracle(device, oracle, id):
    c, g, o = S.case(id), device[id], oracle[id]
    assert g["valid"][c.keep].all()
    a = S.parity_error(c, g)
    b = S.parity_error(c, g, ref=o)
    print(f"{id:22s} vs horn64: dR {a[0]:.2e} dt {a[1]:.2e} ds {a[2]:.2e} self {a[3]:.2e}   vs oracle: dR {b[0]:.2e} dt {b[1]:.2e} ds {b[2]:.2e}")
    assert a[0] <= S.TOL_DR and a[1] <= S.TOL_DT and a[2] <= S.TOL_DS, f"{id} against horn64: dR {a[0]:.2e} dt {a[1]:.2e} ds {a[2]:.2e}"
    assert b[0] <= S.TOL_DR and b[1] <= S.TOL_DT and b[2] <= S.TOL_DS, f"{id} against the oracle: dR {b[0]:.2e} dt {b[1]:.2e} ds {b[2]:.2e}"
    assert a[3] <= 4 * S.ORACLE_SELF, f"{id}: a minimal set maps {a[3]:.2e} off itself"


@pytest.mark.parametrize("id", ["skinny", "degenerate", "trap_pure_scale"])
def test_weakly_determined_sets_by_properties(device, id):
    c, g = S.case(id), device[id]
    for h in np.flatnonzero(c.props):
        assert g["valid"][h]
        S.check_properties(c, g, h)


@pytest.mark.parametrize("id", [c.id for c in CASES if c.expect_n or c.expect_mask])
def test_named_outcomes(device, id):
    c, g = S.case(id), device[id]
    for h, n in c.expect_n.items():
        assert int(g["n_inliers"][h]) == n, f"{id}[{h}]: {g['n_inliers'][h]} inliers, stated {n}"
    for h, m in c.expect_mask.items():
        bad = np.flatnonzero(g["inliers"][h] != m)
        assert len(bad) == 0, f"{id}[{h}]: " + "; ".join(c.extra["why"][i] for i in bad)


# ---- CheckInliers, exactly ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", IDS)
def test_check_inliers_bit_for_bit(device, id):
    """Every hypothesis, every correspondence (n = 3, 24, 30, 129, 257), under the device's own T12_out record."""
    c, g = S.case(id), device[id]
    for h, rec in enumerate(S.records_of(g)):
        mine = S.check_inliers_f32(rec, c.X1, c.X2, c.thr1, c.thr2, c.K1, c.K2)
        assert np.array_equal(mine, g["inliers"][h]), f"{id}[{h}]: correspondences {np.flatnonzero(mine != g['inliers'][h])}"
        assert int(g["n_inliers"][h]) == int(mine.sum()), f"{id}[{h}]: n_inliers {g['n_inliers'][h]} against {int(mine.sum())} set flags"


# ---- same bytes from both entries ----------------------------------------------------------------------------------------------------------------
def _three(min_inliers):
    cs = [S.case("ladder_n129"), S.case("scale_0.5_n257"), S.case("minimal_n3")]           # K and fix_scale differ from solver to solver
    assert [c.n for c in cs] == [129, 257, 3] and len({c.fix_scale for c in cs}) == 2 and not np.array_equal(cs[2].K2, cs[0].K2)
    sol = np.zeros(3, SIM3_RANSAC_SOLVER_DTYPE)
    first = 0
    for rec, c, m in zip(sol, cs, min_inliers):
        rec["first"], rec["n"], rec["min_inliers"], rec["its_left"], rec["fix_scale"], rec["K4_1"], rec["K4_2"] = first, c.n, m, 300, int(c.fix_scale), c.K1, c.K2
        first += c.n
    cat = lambda name: np.concatenate([getattr(c, name) for c in cs])
    return cs, sol, (cat("X1"), cat("X2"), cat("s1"), cat("s2"), np.stack([c.tri for c in cs]))


def test_batch_entry_returns_the_single_entry_bytes(opt, device):
    cs, sol, arrs = _three([129, 257, 3])
    res = opt.Sim3RansacBatch(sol, *arrs, want_all=True)
    for j, c in enumerate(cs):
        g = device[c.id]
        assert res["T12_all"][j].tobytes() == S.records_of(g).tobytes(), f"{c.id}: T12_all differs from rumi_sim3_ransac"
        assert np.array_equal(res["n_inliers_all"][j], g["n_inliers"]), c.id
    assert (res["state"] == [SIM3_WINDOW_ENDED, SIM3_NOT_REACHED, SIM3_NOT_REACHED]).all() and not res["inliers"].any()
    # the masks of k_s3b_check: the first two solvers return at once (iterations 0 and 1 of the window), the third never has more than 3 inliers
    cs, sol, arrs = _three([0, 0, 3])
    res = opt.Sim3RansacBatch(sol, *arrs)
    assert (res["state"] == [SIM3_CONVERGED, SIM3_CONVERGED, SIM3_WINDOW_ENDED]).all() and res["hyp"].tolist() == [0, 1, -1] and res["its"].tolist() == [1, 1, S.N_HYP - 2]
    for j, c in enumerate(cs[:2]):
        g, h, a = device[c.id], int(res["hyp"][j]), int(sol["first"][j])
        assert np.array_equal(res["inliers"][a:a + c.n], g["inliers"][h]) and res["n_inliers"][j] == g["n_inliers"][h], c.id
        assert res["T12"][j].tobytes() == S.records_of(g)[h].tobytes()
        assert np.array_equal(res["inliers"][a:a + c.n], S.check_inliers_f32(res["T12"][j], c.X1, c.X2, c.thr1, c.thr2, c.K1, c.K2))
    assert not res["inliers"][sol["first"][2]:].any()


# ---- the sequential rule over the identity trap --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arrangement", ["first", "middle", "identical"])
def test_batch_passes_the_identity_trap(opt, arrangement):
    """The trap runs between two ordinary solvers; its degenerate set has more than min_inliers inliers, first in its part of the window and again in the
    middle.  It converges on the next valid iteration above min_inliers; maps identical throughout exhaust their iterations."""
    solvers, rng, used = S.trap_batch_solvers(opt, arrangement)
    want = reference_loop(solvers)                                   # the per-candidate loop over the single entry
    next_word = rng.state()
    for window in (40, 3):
        solvers, rng, _ = S.trap_batch_solvers(opt, arrangement)
        got, rounds = Sim3SolverBatch(opt, solvers, rng).run(window)
        assert_same_results(got, want)
        assert rng.state() == next_word == [3 * (1 + used + 1)], "rand() advanced as the per-candidate loop advances it"
        assert [g[0] for g in got] == [True, arrangement != "identical", True] and [g[4] for g in got] == [1, used, 1]
    if arrangement == "identical":
        return
    # the raw entry: state, hyp, its, count and mask are those of the returning iteration
    solvers, rng, _ = S.trap_batch_solvers(opt, arrangement)
    trap = solvers[1]
    R = 1 + used + 1
    sol = np.zeros(3, SIM3_RANSAC_SOLVER_DTYPE)
    first = 0
    for rec, s in zip(sol, solvers):
        rec["first"], rec["n"], rec["min_inliers"], rec["its_left"], rec["fix_scale"], rec["K4_1"], rec["K4_2"] = first, s.N, s.mRansacMinInliers, s.mRansacMaxIts, 0, s.K1, s.K2
        first += s.N
    cat = lambda name: np.concatenate([getattr(s, name) for s in solvers])
    tri = np.stack([rng.draw_window(s.N, R) for s in solvers])
    seq = S.SEQUENCES[arrangement]
    assert tri[1, 1:1 + used].tolist() == [S.trap_scene()["names"][k] for k in seq]
    res = opt.Sim3RansacBatch(sol, cat("X1"), cat("X2"), cat("s1"), cat("s2"), tri, want_all=True)
    assert (res["state"] == SIM3_CONVERGED).all() and res["hyp"].tolist() == [0, used, used + 1] and res["its"].tolist() == [1, used, 1]
    inv = np.array([k.startswith("I") for k in seq])
    assert np.array_equal(res["T12_all"][1, 1:1 + used, 13] == 0, inv)
    assert (res["n_inliers_all"][1, 1:1 + used][inv] > trap.mRansacMinInliers).all(), "the trap is live on the device"
    a = int(sol["first"][1])
    assert res["T12"][1].tobytes() == res["T12_all"][1, used].tobytes() and res["n_inliers"][1] == res["n_inliers_all"][1, used]
    mask = S.check_inliers_f32(res["T12"][1], trap.X1, trap.X2, S.thresholds(trap.s1), S.thresholds(trap.s2), trap.K1, trap.K2)
    assert np.array_equal(res["inliers"][a:a + trap.N], mask) and int(mask.sum()) == res["n_inliers"][1]


@pytest.mark.parametrize("mode,arrangement", [("plain", "first"), ("plain", "middle"), ("converge", "first"), ("converge", "middle"), ("rumination", "middle")])
def test_solver_passes_the_identity_trap(opt, mode, arrangement):
    s, tri, sc = S.trap_solver(opt, arrangement)
    args = (sc["X1"], sc["X2"], sc["s1"], sc["s2"], sc["K"], sc["K"], tri[:s.mRansacMaxIts])
    g = opt.Sim3Ransac(*args, score=sc["score"])
    o = O.sim3_ransac(*args, score=sc["score"])
    seq = S.SEQUENCES[arrangement]
    assert np.array_equal(g["valid"], o["valid"]) and np.array_equal(~g["valid"][:len(seq)], [k.startswith("I") for k in seq])
    want = S.replay_upstream(g["valid"], g["n_inliers"], g["median"], sc["min_inliers"], s.mRansacMaxIts, 20, mode)
    assert want[:3] == S.replay_upstream(o["valid"], o["n_inliers"], o["median"], sc["min_inliers"], s.mRansacMaxIts, 20, mode)[:3]
    want_it, _, want_calls, want_best, want_ratio = want
    assert want_it == len(seq) - 1
    got = S.drive(s, mode, sc["score"])
    assert got["conv"] and got["calls"] == want_calls and s.mnIterations == want_it + 1 and s.mnBestInliers == want_best
    assert s.rng.state() == [3 * (want_it + 1)]
    assert np.array_equal(s.GetEstimatedRotation(), g["R"][want_it]) and s.GetEstimatedScale() == g["s"][want_it]
    if mode != "rumination":
        assert got["n_in"] == g["n_inliers"][want_it] and np.array_equal(got["vb"][0::2], g["inliers"][want_it]) and not got["vb"][1::2].any()
    else:
        assert got["ratio"] == pytest.approx(want_ratio) and want_ratio > 0.10


# ---- the score path under large rotations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", [c.id for c in CASES if c.score is not None])
def test_score_path(device, oracle, id):
    """median and ratio equal the oracle's wherever the hypothesis comes from a filtered triple, and ComputeInliersNum in float64 under the device's own
    hypothesis.  The device composes gSw1w2 in its own double arithmetic (quat_from_matrix of the float R): a key-point counts as decided when both errors are
    further than 1e-6 (relative) from their thresholds, at most 2 % of the key-points of a case may be undecided under any hypothesis."""
    c, g, o = S.case(id), device[id], oracle[id]
    sc = c.score
    hyps = np.flatnonzero(c.keep) if c.keep.any() else np.flatnonzero(g["valid"])
    assert np.array_equal(g["median"][hyps], o["median"][hyps]) and np.array_equal(g["ratio"][hyps], o["ratio"][hyps]), id
    rest = (sc["K4_1"], sc["K4_2"], sc["X1"], sc["X2"], sc["kp1"], sc["kp2"], sc["sigma2_1"], sc["sigma2_2"], sc["edge1"], sc["edge2"])
    ps, den = sc["pair_start"], sc["pair_denominator"]
    undecided = np.zeros(ps[-1], bool)
    for h in hyps:
        T = (g["R"][h].astype(np.float64), g["t"][h].astype(np.float64), float(g["s"][h]))
        A = [S.sim_mul(S.sim_Rts(a), T) for a in sc["S_c1w1"]]; B = [S.sim_mul(S.sim_Rts(b), S.sim_inv(T)) for b in sc["S_c2w2"]]
        med, ratio, flags, rel = S.inliers_num_f64(ps, den, A, B, *rest, margins=True)
        loose = rel <= 1e-6
        undecided |= loose
        if not loose.any():
            assert np.array_equal(ratio, g["ratio"][h]) and med == g["median"][h], f"{id}[{h}]: ratios {g['ratio'][h]} against {ratio}"
        else:
            for p in range(len(den)):
                cnt = g["ratio"][h][p] * den[p]
                assert abs(cnt - flags[ps[p]:ps[p + 1]].sum()) <= loose[ps[p]:ps[p + 1]].sum() + 1e-3
    assert undecided.sum() <= 0.02 * len(undecided), f"{id}: {int(undecided.sum())} key-points within 1e-6 of a threshold"
    if id.startswith("rot_") and "180" in id:
        R = g["R"][hyps].astype(np.float64)
        assert (np.trace(R, axis1=1, axis2=2) <= 0).any() or id == "rot_skew180", "quat_from_matrix's trace <= 0 branches are taken"


# ---- ComputeInliersNum and OptimizeSim3 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(S.inliers_num_cases())), ids=[c["id"] for c in S.inliers_num_cases()])
def test_inliers_num(opt, k):
    c = S.inliers_num_cases()[k]
    med, ratio, flags = opt.ComputeInliersNum(*S.inliers_args(c))
    omed, oratio, oflags = O.sim3_inliers(*S.inliers_args(c))
    bad = np.flatnonzero(flags != c["expect"])
    assert len(bad) == 0, f"{c['id']}: " + "; ".join(c["why"][i] for i in bad)
    assert np.array_equal(flags, oflags) and np.array_equal(ratio, oratio) and np.float32(med) == np.float32(omed), f"{c['id']}: {ratio} / {oratio}, {med} / {omed}"


def _sim3_close(a, b, what):
    """test_optimizer_gpu._sim3_close"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.linalg.norm(a[:4] - b[:4]) <= 1e-4, f"{what}: rotation {a[:4]} vs {b[:4]}"
    assert np.linalg.norm(a[4:7] - b[4:7]) <= 1e-4 * max(np.linalg.norm(b[4:7]), 1.0), f"{what}: translation {a[4:7]} vs {b[4:7]}"
    assert abs(a[7] - b[7]) <= 1e-4 * abs(b[7]), f"{what}: scale {a[7]} vs {b[7]}"


@pytest.mark.parametrize("k", range(len(S.optimize_cases())), ids=[c["id"] for c in S.optimize_cases()])
def test_optimize_sim3(opt, k):
    c = S.optimize_cases()[k]
    nin, nbad, early, Sg, status = opt.OptimizeSim3(*S.optimize_args(c), skip12=c["skip12"], skip21=c["skip21"])
    onin, onbad, oearly, So, ostatus = O.optimize_sim3(*S.optimize_args(c), skip12=c["skip12"], skip21=c["skip21"])
    assert (nin, nbad, early) == (onin, onbad, oearly), f"{c['id']}: {(nin, nbad, early)} against {(onin, onbad, oearly)}"
    assert np.array_equal(status, ostatus), c["id"]
    _sim3_close(Sg, So, c["id"])
    e = c["expect"]
    if e.get("unchanged"):
        assert (nin, nbad, int(early)) == e["res"] and np.abs(Sg - c["S0"]).max() <= 1e-12
    else:
        assert nbad == e["nBad"] and int(early) == e["early"] and ("nIn" not in e or nin == e["nIn"])
    if "status3" in e:
        assert np.flatnonzero(status == 3).tolist() == e["status3"]
