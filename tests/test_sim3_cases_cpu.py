"""The constructed Sim3 cases of sim3_cases.py on the CPU: the oracle (oracle/opt_oracle.cc) takes the path every case is named after, horn64 and the
float32 restatement of CheckInliers agree with it where they must, and the host mirror's state machine passes the identity trap.  What is measured
here (oracle against horn64) is what sim3_cases.py records as ORACLE_* and what bounds the device in test_sim3_cases_gpu.py.  Needs no GPU."""
import numpy as np
import pytest

import oracle_lib as O
import sim3_cases as S
from sim3_batch_scene import OracleOptimizer, assert_same_results, reference_loop
from rumi_slam_amd.sim3solver import Sim3SolverBatch

CASES = S.all_cases()
IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def oracle():
    """The oracle's result of every case, once."""
    return {c.id: O.sim3_ransac(*c.args(), fix_scale=c.fix_scale, score=c.score) for c in CASES}


# ---- oracle against horn64 -------------------------------------------------------------------------------------------------------------------
def test_oracle_against_horn64(oracle):
    worst = np.zeros(4)
    for c in CASES:
        if not c.keep.any():
            continue
        e = np.array(S.parity_error(c, oracle[c.id]))
        print(f"{c.id:22s} kept {int(c.keep.sum()):2d}/{c.H}  dR {e[0]:.2e}  dt {e[1]:.2e}  ds {e[2]:.2e}  self {e[3]:.2e}")
        assert oracle[c.id]["valid"][c.keep].all(), c.id
        worst = np.maximum(worst, e)
    print(f"worst: dR {worst[0]:.3e}  dt {worst[1]:.3e}  ds {worst[2]:.3e}  self {worst[3]:.3e}")
    # the recorded measurement is honest, and the oracle itself stays inside what the device is held to
    assert worst[0] <= S.ORACLE_DR and worst[1] <= S.ORACLE_DT and worst[2] <= S.ORACLE_DS and worst[3] <= S.ORACLE_SELF
    assert worst[0] <= S.TOL_DR and worst[1] <= S.TOL_DT and worst[2] <= S.TOL_DS
    assert S.TOL_DR <= 1e-4 and S.TOL_DT <= 1e-4 and S.TOL_DS <= 1e-4
    assert sum(int(c.keep.sum()) for c in CASES) >= 900


@pytest.mark.parametrize("id", [c.id for c in CASES if c.keep.any()])
def test_conditioning_filter(id):
    c = S.case(id)
    gaps = np.array([h.gap for h in c.horn])
    assert (gaps[c.keep] >= S.G0).all() and c.keep.sum() >= 50


# ---- the float32 restatement of CheckInliers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", IDS)
def test_restatement_reproduces_the_oracle_mask(oracle, id):
    """Fed with the oracle's own record, bit for bit on every correspondence of every hypothesis, ladder rungs included."""
    c, o = S.case(id), oracle[id]
    for h, rec in enumerate(S.records_of(o)):
        mine = S.check_inliers_f32(rec, c.X1, c.X2, c.thr1, c.thr2, c.K1, c.K2)
        assert np.array_equal(mine, o["inliers"][h]), f"{id}[{h}]: correspondences {np.flatnonzero(mine != o['inliers'][h])}"
        assert int(mine.sum()) == int(o["n_inliers"][h])


def test_thresholds_are_truncated():
    assert S.thresholds(S.LADDER_SIGMA2).tolist() == [9.0, 0.0, 1.0, 13.0, 39.0]


def test_the_ladder_straddles(oracle):
    c, o = S.case("ladder_n129"), oracle["ladder_n129"]
    rungs = c.extra["rungs"]
    recs = S.records_of(o)
    assert {(r.term, r.sigma2) for r in rungs} == {(t, s) for t in (1, 2) for s in S.LADDER_SIGMA2}
    inside = {(t, side): 0 for t in (1, 2) for side in (0, 1)}
    for h in np.flatnonzero(c.keep):
        e1, e2 = S.errors_f32(recs[h], c.X1, c.X2, c.K1, c.K2)
        for r in rungs:
            err, thr = (e1, c.thr1) if r.term == 1 else (e2, c.thr2)
            other_ok = (e2[r.index] < c.thr2[r.index]) if r.term == 1 else (e1[r.index] < c.thr1[r.index])
            is_in = bool(err[r.index] < thr[r.index])
            assert bool(o["inliers"][h][r.index]) == (is_in and bool(other_ok))
            if thr[r.index] == 0:
                assert not is_in and err[r.index] < 1e-6, "threshold 0: nothing is an inlier, even at (all but) zero error"
                continue
            assert other_ok, "the other term never decides a rung"
            if r.delta in (1e-1, 1e-2):
                assert not is_in, f"hypothesis {h}: rung {r} is inside"
            elif r.delta in (-1e-1, -1e-2):
                assert is_in, f"hypothesis {h}: rung {r} is outside"
            else:
                rel = abs(float(err[r.index]) - float(thr[r.index])) / float(thr[r.index])
                assert rel < 3e-3, f"rung {r} sits {rel:.1e} from the threshold"
                inside[(r.term, int(is_in))] += 1
    # rungs within 1e-3 of the threshold fall on both sides, for each of the two error terms
    assert all(v > 50 for v in inside.values()), inside
    # under the truth's own float32 rows the one-step pairs straddle as named
    rec = S.record_of(*c.truth)
    e1, e2 = S.errors_f32(rec, c.X1, c.X2, c.K1, c.K2)
    for r in rungs:
        if isinstance(r.delta, str):
            err, thr = (e1, c.thr1) if r.term == 1 else (e2, c.thr2)
            assert bool(err[r.index] < thr[r.index]) == (r.delta == "ulp-")


# ---- named outcomes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", [c.id for c in CASES if c.expect_valid is not None or c.expect_n or c.expect_mask])
def test_named_outcomes(oracle, id):
    c, o = S.case(id), oracle[id]
    if c.expect_valid is not None:
        assert np.array_equal(o["valid"], c.expect_valid), f"{id}: valid {o['valid'].astype(int)}"
    for h, n in c.expect_n.items():
        assert int(o["n_inliers"][h]) == n, f"{id}[{h}]: {o['n_inliers'][h]} inliers, stated {n}"
    for h, m in c.expect_mask.items():
        bad = np.flatnonzero(o["inliers"][h] != m)
        assert len(bad) == 0, f"{id}[{h}]: " + "; ".join(c.extra["why"][i] for i in bad)
    inv = ~o["valid"]
    assert (o["R"][inv] == np.eye(3, dtype=np.float32)).all() and (o["t"][inv] == 0).all() and (o["s"][inv] == 1).all()


def test_identity_traps_are_live(oracle):
    """The degenerate hypothesis would win if `valid` were ignored: it counts every correspondence."""
    c, o = S.case("trap_identity_triple"), oracle["trap_identity_triple"]
    assert not o["valid"][0] and o["n_inliers"][0] == c.n and o["valid"][2:].all()
    assert np.array_equal(c.X1[:3].view(np.uint32), c.X2[:3].view(np.uint32)) and not np.array_equal(c.X1[3:], c.X2[3:])
    p = S.case("trap_pure_scale")
    assert 3 <= (~p.expect_valid).sum() < p.H, "some, not all, of the exactly representable triples are flagged"


@pytest.mark.parametrize("id", ["skinny", "degenerate", "trap_pure_scale"])
def test_property_cases_on_the_oracle(oracle, id):
    c, o = S.case(id), oracle[id]
    assert c.props.any()
    for h in np.flatnonzero(c.props):
        assert o["valid"][h]
        S.check_properties(c, o, h)
    if id == "skinny":
        gaps = np.array([h.gap for h in c.horn])
        assert (gaps < S.G0).all() and len(gaps) >= 20


# ---- the paths of the rotation cases ---------------------------------------------------------------------------------------------------------
def test_small_angle_branch():
    for id in ("rot_3e-6", "rot_1e-6"):
        c = S.case(id)
        ang = np.array([h.angle for h in c.horn])
        assert (ang[c.keep] < 1e-5).all() and c.keep.sum() >= 50, f"{id}: SO3::exp's Taylor branch needs theta < 1e-5"
    assert min(h.angle for h in S.case("rot_1e-3").horn) > 1e-4
    # at 1e-5 rad the float32 rounding of the coordinates (a few 1e-7 rad) puts minimal sets on both sides of the switch
    c = S.case("rot_1e-5")
    ang = np.array([h.angle for h in c.horn])[c.keep]
    assert (ang < 1e-5).sum() >= 5 and (ang > 1e-5).sum() >= 5 and np.abs(ang - 1e-5).max() < 2e-6


def test_half_turns_reach_every_branch(oracle):
    """trace <= 0 with each diagonal entry the largest in turn, and eigenvectors with e0 of either sign next to 0."""
    for id, diag in (("rot_x180", 0), ("rot_y180", 1), ("rot_z180", 2), ("rot_623_150", 0), ("rot_263_150", 1), ("rot_326_150", 2)):
        o = oracle[id]
        R = o["R"][S.case(id).keep].astype(np.float64)
        tr = np.trace(R, axis1=1, axis2=2)
        assert (tr <= 0).sum() >= 10, f"{id}: {int((tr <= 0).sum())} hypotheses with trace <= 0"
        if "150" in id:          # half a turn about an axis leaves the branch's signs unseen (w and the off-axis components vanish); 150 deg does not
            assert (tr <= 0).all() and all(np.abs(S.quat_of(r)).min() > 0.1 for r in R)
        assert (np.argmax(np.diagonal(R, axis1=1, axis2=2), axis=1) == diag).all()
    e0 = np.array([h.e0 for id in ("rot_x180", "rot_y180", "rot_z180", "rot_skew180") for h, k in zip(S.case(id).horn, S.case(id).keep) if k])
    assert (np.abs(e0) < 1e-6).sum() >= 50
    e0 = np.array([h.e0 for h in S.case("rot_skew179_99").horn])
    assert np.allclose(np.abs(e0), np.sin(np.radians(0.005)), rtol=0.05)


@pytest.mark.parametrize("id", [c.id for c in CASES if c.score is not None])
def test_score_sets_keep_clear_of_their_thresholds(oracle, id):
    """Under the truth no key-point is closer than 1e-3 (relative) to a threshold, and inliers_num_f64 under the oracle's hypotheses gives the oracle's ratios."""
    c, o = S.case(id), oracle[id]
    sc = c.score
    assert len(sc["pair_start"]) == 3 and 36 <= sc["pair_start"][-1] <= 44
    truth = c.truth
    comp = lambda T: ([S.sim_mul(S.sim_Rts(a), T) for a in sc["S_c1w1"]], [S.sim_mul(S.sim_Rts(b), S.sim_inv(T)) for b in sc["S_c2w2"]])
    rest = (sc["K4_1"], sc["K4_2"], sc["X1"], sc["X2"], sc["kp1"], sc["kp2"], sc["sigma2_1"], sc["sigma2_2"], sc["edge1"], sc["edge2"])
    A, B = comp(truth)
    med, ratio, flags, rel = S.inliers_num_f64(sc["pair_start"], sc["pair_denominator"], A, B, *rest, margins=True)
    assert rel.min() > 1e-3 and 0.3 < med < 1.0 and 0 < flags.sum() < len(flags)
    for h in np.flatnonzero(c.keep if c.keep.any() else o["valid"])[:12]:
        T = (o["R"][h].astype(np.float64), o["t"][h].astype(np.float64), float(o["s"][h]))
        A, B = comp(T)
        med, ratio, flags, rel = S.inliers_num_f64(sc["pair_start"], sc["pair_denominator"], A, B, *rest, margins=True)
        if (rel > 1e-6).all():
            assert med == o["median"][h] and np.array_equal(ratio, o["ratio"][h]), f"{id}[{h}]"


# ---- ComputeInliersNum ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(S.inliers_num_cases())), ids=[c["id"] for c in S.inliers_num_cases()])
def test_inliers_num_equals_the_oracle(k):
    c = S.inliers_num_cases()[k]
    med, ratio, flags = S.inliers_num_f64(*S.inliers_args(c))
    omed, oratio, oflags = O.sim3_inliers(*S.inliers_args(c))
    bad = np.flatnonzero(flags != c["expect"])
    assert len(bad) == 0, f"{c['id']}: the restatement misses: " + "; ".join(c["why"][i] for i in bad)
    bad = np.flatnonzero(oflags != c["expect"])
    assert len(bad) == 0, f"{c['id']}: the oracle misses: " + "; ".join(c["why"][i] for i in bad)
    assert np.array_equal(ratio, oratio) and np.float32(med) == np.float32(omed), f"{c['id']}: ratios {ratio} / {oratio}, median {med} / {omed}"
    assert np.float32(med) == np.sort(ratio)[len(ratio) // 2]


def test_inliers_num_cases_cover_their_rules():
    cs = {c["id"]: c for c in S.inliers_num_cases()}
    assert [len(c["pair_start"]) - 1 for c in cs.values()] == [1, 2, 2, 4, 1]
    assert cs["empty_pair_only"]["pair_start"][-1] == 0
    two = cs["two_pairs_upper_middle"]
    med, ratio, _ = S.inliers_num_f64(*S.inliers_args(two))
    assert med == ratio.max() and ratio.min() < ratio.max(), "[n/2] of two ratios is the larger"
    four = cs["four_pairs"]
    med, ratio, _ = S.inliers_num_f64(*S.inliers_args(four))
    assert ratio[1] == 0 and ratio[2] == 0 and med == np.sort(ratio)[2] and med > 0
    why = " ".join(cs["ulp_two_pairs"]["why"])
    assert "under" in why and "over" in why and "pz < 0" in why and "pz == 0" in why


# ---- the host mirror over the identity trap ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,arrangement", [("plain", "first"), ("plain", "middle"), ("converge", "first"), ("converge", "middle"), ("rumination", "middle")])
def test_host_mirror_passes_the_identity_trap(mode, arrangement):
    s, tri, sc = S.trap_solver(OracleOptimizer(), arrangement)
    o = O.sim3_ransac(sc["X1"], sc["X2"], sc["s1"], sc["s2"], sc["K"], sc["K"], tri[:s.mRansacMaxIts], score=sc["score"])
    seq = S.SEQUENCES[arrangement]
    inv = np.array([k.startswith("I") for k in seq])
    assert np.array_equal(~o["valid"][:len(seq)], inv)
    assert (o["n_inliers"][:len(seq)][inv] > sc["min_inliers"]).all(), "the trap is live: the degenerate set's count alone would converge"
    want_it, want_total, want_calls, want_best, want_ratio = S.replay_upstream(o["valid"], o["n_inliers"], o["median"], sc["min_inliers"], s.mRansacMaxIts, 20, mode)
    assert want_it == len(seq) - 1, "the replay of upstream's loop returns at the first valid iteration above min_inliers"
    got = S.drive(s, mode, sc["score"])
    assert got["conv"] and got["calls"] == want_calls == 1 and s.mnIterations == want_it + 1 and s.mnBestInliers == want_best
    assert s.rng.state() == [3 * (want_it + 1)], "rand() stands after the draws of the returning iteration"
    assert np.array_equal(s.GetEstimatedRotation(), o["R"][want_it]) and s.GetEstimatedScale() == o["s"][want_it]
    if mode != "rumination":
        assert got["n_in"] == o["n_inliers"][want_it] and np.array_equal(got["vb"][0::2], o["inliers"][want_it]) and not got["vb"][1::2].any()
    else:
        assert got["ratio"] == pytest.approx(want_ratio) and want_ratio > 0.10


@pytest.mark.parametrize("arrangement", ["first", "middle", "identical"])
def test_batch_mirror_passes_the_identity_trap(arrangement):
    opt = OracleOptimizer()
    solvers, rng, used = S.trap_batch_solvers(opt, arrangement)
    want = reference_loop(solvers)
    next_word = rng.state()
    solvers, rng, _ = S.trap_batch_solvers(opt, arrangement)
    got, rounds = Sim3SolverBatch(opt, solvers, rng).run(40)
    assert_same_results(got, want)
    assert rng.state() == next_word == [3 * (1 + used + 1)]
    assert [g[0] for g in got] == [True, arrangement != "identical", True] and [g[4] for g in got] == [1, used, 1]


# ---- OptimizeSim3 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(S.optimize_cases())), ids=[c["id"] for c in S.optimize_cases()])
def test_optimize_cases_on_the_oracle(k):
    c = S.optimize_cases()[k]
    nin, nbad, early, Sout, status = O.optimize_sim3(*S.optimize_args(c), skip12=c["skip12"], skip21=c["skip21"])
    e = c["expect"]
    if e.get("unchanged"):
        assert (nin, nbad, int(early)) == e["res"] and np.abs(Sout - c["S0"]).max() <= 1e-12 and not status.any()
        return
    assert nbad == e["nBad"] and int(early) == e["early"], f"{c['id']}: nBad {nbad}, early {early}"
    if c["id"] == "nine_survivors":
        assert len(c["w1"]) - nbad == 9 and (status[:4] == 1).all() and not status[4:].any(), "n - nBad < 10: returns with the first pass's removals only"
    if "nIn" in e:
        assert nin == e["nIn"], f"{c['id']}: nIn {nin}"
    if c["id"] == "ten_survivors":
        assert len(c["w1"]) - nbad == 10 and nin >= 9
    if "status3" in e:
        assert np.flatnonzero(status == 3).tolist() == e["status3"]
    if not early:
        q, qt = Sout[:4], c["S_true"][:4]
        assert min(np.linalg.norm(q - qt), np.linalg.norm(q + qt)) < 2e-3 and abs(Sout[7] - c["S_true"][7]) < 5e-3 * c["S_true"][7]
    if c["id"] == "half_turn":
        assert abs(c["S_true"][3]) < 1e-9 and abs(c["S0"][3]) > 1e-3
