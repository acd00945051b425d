"""The constructed optimiser cases (opt_cases.py) checked on the CPU oracle alone: every case keeps its distance from every threshold, the
rough starts and hopeless frames survive one ulp on their observations, the cases reach the Levenberg-Marquardt decisions they were built
for, and the oracle itself does not care about the order of a graph."""
import numpy as np
import pytest

import opt_cases as C
import oracle_lib as O
from scene import K_TUM3, quat_rotate

EPS = float(np.finfo(np.float32).eps)


def test_trace_counts_what_the_call_did():
    p = C.pose_case(256)
    C.run_oracle(O, "pose", C.pose_args(p))
    tr = O.opt_last_trace()
    assert 4 <= tr["trials"] <= 400 and 0 <= tr["rejected"] < tr["trials"] and tr["rejected_run"] <= min(tr["rejected"], 10) and np.isfinite(tr["margin"])
    b = C.ba_case("batched")
    (its, _, _, _), tr = C.run_oracle(O, "local", C.ba_args(b))
    assert tr["trials"] >= its > 0 and tr["trials"] - tr["rejected"] <= its      # an iteration accepts at most one trial
    (_, _, _), tr = C.run_oracle(O, "global", C.ba_args(b))
    assert tr["margin"] == np.inf                                      # the global BA compares nothing with a threshold
    O.local_ba(*C.ba_args(b), stop=np.ones(1, np.uint8))               # every call resets the trace, one that returns at once too
    assert O.opt_last_trace() == dict(trials=0, rejected=0, ended_qmax=0, ended_rho0=0, rejected_run=0, margin=np.inf, gain=np.inf)


@pytest.mark.parametrize("n", sorted(set(C.POSE_SIZES + [n for n in C.BATCH_SIZES if n >= 3])))
def test_pose_sizes_keep_their_margin(n):
    p = C.pose_case(n)
    assert len(p["inv_sigma2"]) == n
    (ng, _, out), tr = C.check_margin(O, "pose", C.pose_args(p))
    assert ng == n - out.sum()
    if n >= 10:                                                        # chosen so: the exact ties that end an iteration are no part of a size test
        assert tr["ended_qmax"] == 0 and tr["ended_rho0"] == 0
        assert 0 < out.sum() < n                                       # inliers and outliers both


@pytest.mark.parametrize("n,seed,offset", C.ROUGH_POSE)
def test_rough_pose_starts_reject_trials_and_are_stable(n, seed, offset):
    a = C.pose_args(C.rough_start_pose(n, seed, offset))
    _, tr = C.check_margin(O, "pose", a)
    C.check_stable(O, "pose", a)
    assert tr["rejected"] >= 5, "at least 5 rejected trials in one pose call"


@pytest.mark.parametrize("n,seed", C.HOPELESS)
def test_hopeless_frames(n, seed):
    p = C.hopeless_frame(n, seed)
    a = C.pose_args(p)
    (ng, T, out), tr = C.check_margin(O, "pose", a)
    C.check_stable(O, "pose", a)
    assert ng == 0 and out.all()
    assert tr["trials"] >= 1                                           # the first round did optimise ...
    assert np.abs(T - p["T0"]).max() <= 2 * EPS                        # ... the later ones had no active edge: the pose is the (re-normalised) input


def test_a_hopeless_frame_rejects_five_trials():
    assert max(C.run_oracle(O, "pose", C.pose_args(C.hopeless_frame(n, s)))[1]["rejected"] for n, s in C.HOPELESS) >= 5


@pytest.mark.parametrize("n,seed", C.EXACT)
def test_exact_frames(n, seed):
    p = C.exact_frame(n, seed)
    (ng, T, out), _ = C.check_margin(O, "pose", C.pose_args(p))
    assert ng == n and not out.any() and np.abs(T - p["T0"]).max() <= 2e-7


@pytest.mark.parametrize("name,kind", C.BA_CASE_KINDS)
def test_ba_cases_keep_their_margin(name, kind):
    b = C.ba_case(name)
    assert (b["e_mp"][1:] >= b["e_mp"][:-1]).all(), "cases are built grouped by landmark; permuted() is what shuffles them"
    C.check_margin(O, kind, C.ba_args(b))


@pytest.mark.parametrize("name,kind", [nk for nk in C.BA_CASE_KINDS if nk[0] not in C.TIED])
def test_ba_cases_are_decisive(name, kind):
    """No accept / reject decision of the oracle within GAIN of a tie, no iteration ended on rho == 0: the iteration and trial counts of these
    cases do not depend on the order of a sum."""
    C.check_decisive(O, kind, C.ba_args(C.ba_case(name)))


def test_tiny_graphs_end_on_a_tie():
    """Why the counts of opt_cases.TIED are not compared: one landmark or one edge under five optimised key-frames leaves more unknowns than
    residuals, LM reaches the last bit of chi2 within its limit and the oracle's last decisions are ties (for every seed tried)."""
    for name in C.TIED:
        gains = [C.run_oracle(O, kind, C.ba_args(C.ba_case(name)))[1] for kind in ("local", "merge")]
        assert min(t["gain"] for t in gains) < 1e-12 and max(t["ended_rho0"] for t in gains) >= 1, name
    for seed in range(20):
        for w in (C.single_edge(seed), C.window(seed, 1)):
            assert min(C.run_oracle(O, kind, C.ba_args(w))[1]["gain"] for kind in ("local", "merge")) < C.GAIN


@pytest.mark.parametrize("name", C.ROUGH_BA)
@pytest.mark.parametrize("kind", ["local", "merge", "global"])
def test_rough_ba_starts_are_stable(name, kind):
    C.check_stable(O, kind, C.ba_args(C.ba_case(name)))


def test_rough_ba_starts_reach_the_lm_decisions():
    (its, _, _, _), tr = C.run_oracle(O, "local", C.ba_args(C.ba_case("rough early")))
    assert 0 < its < 10 and tr["ended_qmax"] == 0 and tr["ended_rho0"] == 0, "a BA call that ends before its iteration limit (three small gains in a row)"
    for kind in ("local", "merge", "global"):
        _, tr = C.run_oracle(O, kind, C.ba_args(C.ba_case("rough rejecting")))
        assert tr["rejected"] >= 2 and tr["rejected_run"] >= 2, f"{kind}: at least two rejected trials in a row, so that the growth of ni is used"


def test_degrees_and_counts_are_what_they_say():
    b = C.ba_case("degrees")
    assert np.count_nonzero(b["kf_fixed"] == 0) == 5 and np.count_nonzero(b["kf_fixed"]) == 30
    deg = np.bincount(b["e_mp"], minlength=len(b["mp_pos"]))
    assert tuple(deg[:len(C.DEGREES)]) == C.DEGREES
    for e in range(len(b["e_mp"]) - 1):                                # no landmark is observed twice by a key-frame
        assert b["e_mp"][e] != b["e_mp"][e + 1] or b["e_kf"][e] < b["e_kf"][e + 1]
    for n in C.COUNTS:
        w = C.ba_case(f"count {n}")
        assert len(w["mp_pos"]) == n and np.bincount(w["e_mp"], minlength=n).min() >= 3
    s = C.ba_case("single edge")
    assert len(s["e_mp"]) == 1 and len(s["mp_pos"]) == 1 and s["kf_fixed"][s["e_kf"][0]] == 0
    f = C.ba_case("fixed only")
    assert f["kf_fixed"][f["e_kf"][f["e_mp"] <= 1]].all() and np.count_nonzero(f["e_mp"] <= 1) == 3
    z = C.ba_case("no observation")
    assert z["kf_fixed"][30] == 0 and not (z["e_kf"] == 30).any()
    assert np.count_nonzero(C.ba_case("panel")["kf_fixed"] == 0) == 31 and np.count_nonzero(C.ba_case("large")["kf_fixed"] == 0) == 44
    assert len(C.ba_case("large")["kf_fixed"]) <= 64


@pytest.mark.parametrize("fixed", ["interleaved", "last"])
def test_permuted_is_the_same_graph(fixed):
    b = C.ba_case("batched")
    w, inv = C.permuted(b, np.random.default_rng(5), fixed)
    assert w["kf_fixed"][0] == 0 and (w["e_mp"][1:] < w["e_mp"][:-1]).any()
    if fixed == "last":
        assert w["kf_fixed"][-3:].all() and not w["kf_fixed"][:-3].any()
    else:
        assert not w["kf_fixed"][-3:].all()
    assert np.array_equal(w["kf_pose"][inv["kf"]], b["kf_pose"]) and np.array_equal(w["mp_pos"][inv["mp"]], b["mp_pos"])
    e = inv["edge"]
    assert np.array_equal(w["e_obs"][e], b["e_obs"]) and np.array_equal(w["e_w"][e], b["e_w"])
    assert np.array_equal(inv["mp"][b["e_mp"]], w["e_mp"][e]) and np.array_equal(inv["kf"][b["e_kf"]], w["e_kf"][e])


def _rounding(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.abs(a - b) <= 4 * EPS * np.maximum(1.0, np.abs(b))).all()


@pytest.mark.parametrize("name,kind", [("batched", "local"), ("batched", "merge"), ("panel", "global"), ("large", "local"), ("degrees", "merge"),
                                       ("rough rejecting", "local")])
def test_oracle_is_invariant_under_permutation(name, kind):
    """Sums in another order: the same decisions, the same values to float rounding, once mapped back."""
    b = C.ba_case(name)
    r0, t0 = C.run_oracle(O, kind, C.ba_args(b))
    for seed, fixed in ((1, "interleaved"), (2, "last")):
        w, inv = C.permuted(b, np.random.default_rng(seed), fixed)
        r1, t1 = C.run_oracle(O, kind, C.ba_args(w))
        assert np.array_equal(r0[0], r1[0]) and (t0["trials"], t0["rejected"]) == (t1["trials"], t1["rejected"])
        assert _rounding(r1[1][inv["kf"]], r0[1]) and _rounding(r1[2][inv["mp"]], r0[2])
        if kind != "global":
            assert np.array_equal(r1[3][inv["edge"]], r0[3])


@pytest.mark.parametrize("kind", ["local", "merge"])
def test_mirrored_landmark_is_erased_by_its_depth_alone(kind):
    b = C.ba_case("mirrored")
    (_, kp, mp, er), _ = C.check_margin(O, kind, C.ba_args(b))
    e = len(b["e_mp"]) - 1
    k, p = b["e_kf"][e], b["e_mp"][e]
    assert p == len(b["mp_pos"]) - 1 and b["kf_fixed"][k] == 1
    Xc, _ = quat_rotate(kp[k, :4].astype(np.float64), mp[p:p + 1].astype(np.float64))
    Xc = Xc[0] + kp[k, 4:]
    K = K_TUM3.astype(np.float64)
    r = b["e_obs"][e] - np.array([K[0] * Xc[0] / Xc[2] + K[2], K[1] * Xc[1] / Xc[2] + K[3]])
    assert Xc[2] < -1.0 and float(r @ r) * b["e_w"][e] < 1e-6 and er[e] == 1
    assert np.abs(mp[p] - b["mp_pos"][p]).max() <= 1e-6
    base = C.ba_case("degrees")                                        # the rest of the window does not notice the extra landmark
    assert np.array_equal(er[:e], C.run_oracle(O, kind, C.ba_args(base))[0][3])


def test_invalid_graphs_are_invalid():
    b = C.ba_case("batched")
    g = C.invalid_graphs(b)
    assert list(g) == ["e_mp == nMP", "e_kf == -1", "duplicated edge"]
    assert (g["e_mp == nMP"]["e_mp"] == len(b["mp_pos"])).sum() == 1 and (g["e_kf == -1"]["e_kf"] == -1).sum() == 1
    d = g["duplicated edge"]
    pairs = d["e_mp"].astype(np.int64) * 1000 + d["e_kf"]
    u, c = np.unique(pairs, return_counts=True)
    assert len(d["e_mp"]) == len(b["e_mp"]) + 1 and (c == 2).sum() == 1 and d["kf_fixed"][u[c == 2][0] % 1000] == 0
