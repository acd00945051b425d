"""The constructed relocalisation cases (reloc_cases.py) on the CPU: the oracle chain of Tracking.cc:3287-3345 reaches the intended statements
and counts on both sides of every boundary, the inputs satisfy the margin condition, and the round logic of rumi_slam_amd.tracker.relocalize
(Tracking.cc:3266-3348) over a fake refine."""
import numpy as np
import pytest

import reloc_cases as R
from rumi_slam_amd import tracker as TR

CASES, PTS = R.scene()
BITS = dict(P1=1, NULL1=2, S1=4, P2=8, S2=16, P3=32)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_chain_reaches_the_constructed_counts(name):
    case = CASES[name]
    got = R.oracle_result(name)
    if not case["constructed"]:
        assert got["ran"] == 1 | 2 | 4 and got["nadditional"][0] > 4, "the dense case searches once and finds a window full"
        return
    e = R.expected(case)
    for k in ("ran", "ngood", "nadditional", "ngood_final"):
        assert got[k] == e[k], (name, k, got[k], e[k])


def test_boundaries_from_both_sides():
    """Which statement each side of each boundary reaches (the constructed counts of reloc_cases.expected, spelled out)."""
    e = {n: R.expected(c) for n, c in CASES.items()}
    assert e["p1_two"]["ngood"][0] == 0 and e["p1_two"]["ran"] == 1 and e["p1_two"]["ngood_final"] == -1
    assert e["p1_9"]["ngood"][0] == 9 and e["p1_9"]["ran"] == 1 and e["p1_9"]["ngood_final"] == -1
    assert e["p1_10"]["ngood"][0] == 10 and e["p1_10"]["ran"] == 1 | 2 | 4 and e["p1_10"]["ngood_final"] == 10
    assert e["p1_49"]["ran"] == 1 | 2 | 4 and e["p1_49"]["ngood_final"] == 49
    assert e["p1_50"]["ran"] == 1 | 2 and e["p1_50"]["ngood_final"] == 50
    assert e["s1_49"]["nadditional"][0] + e["s1_49"]["ngood"][0] == 49 and not e["s1_49"]["ran"] & BITS["P2"]
    assert e["s1_50"]["nadditional"][0] + e["s1_50"]["ngood"][0] == 50 and e["s1_50"]["ran"] & BITS["P2"] and e["s1_50"]["ngood_final"] == 50
    assert e["p2_30"]["ngood"][1] == 30 and not e["p2_30"]["ran"] & BITS["S2"]
    assert e["p2_31"]["ngood"][1] == 31 and e["p2_31"]["ran"] & BITS["S2"] and not e["p2_31"]["ran"] & BITS["P3"]
    assert e["p2_49"]["ngood"][1] == 49 and e["p2_49"]["ran"] & BITS["S2"]
    assert e["p2_50"]["ngood"][1] == 50 and not e["p2_50"]["ran"] & BITS["S2"] and e["p2_50"]["ngood_final"] == 50
    assert e["s2_49"]["ngood"][1] + e["s2_49"]["nadditional"][1] == 49 and not e["s2_49"]["ran"] & BITS["P3"] and e["s2_49"]["ngood_final"] == 40
    assert e["s2_50"]["ngood"][1] + e["s2_50"]["nadditional"][1] == 50 and e["s2_50"]["ran"] & BITS["P3"] and e["s2_50"]["ngood_final"] == 50
    assert len(R.frame(True)["keys"]) == 0 and 600 <= len(R.frame()["keys"]) <= 1600


def test_p1_two_leaves_the_pose_untouched():
    got = R.oracle_result("p1_two")
    assert got["Tcw"].tobytes() == CASES["p1_two"]["Tcw7"].tobytes()
    f = CASES["p1_two"]["feats"]["a"]
    assert (got["outlier_last"][f] == 0).all() and (got["outlier_last"] != 255).sum() == 2      # the edges were added: mvbOutlier = false


def test_p2_50_nulls_nothing():
    """When P2 returns >= enough no nulling loop runs: P2's outliers are still in the frame, flagged."""
    got, case = R.oracle_result("p2_50"), CASES["p2_50"]
    g2 = case["feats"]["g2"]
    assert (got["frame_mp"][g2] >= 0).all() and (got["outlier_last"][g2] == 1).all()
    got49 = R.oracle_result("p2_49")
    assert (got49["frame_mp"][CASES["p2_49"]["feats"]["g2"]] >= 0).all(), "S2 found too little: P3 and its nulling did not run"


def test_p1_outliers_stay_in_sfound():
    got, case = R.oracle_result("sfound"), CASES["sfound"]
    g1 = case["feats"]["g1"]
    assert (got["frame_mp"][g1] == -1).all() and (got["outlier_last"][g1] == 1).all() and got["nadditional"][0] == 0
    # the same three key-frame points, were they not in sFound, are within reach of S1: searched alone they are all found
    import oracle_lib as O
    F = R.frame()
    T = got["Tcw"]
    cur = got["frame_mp"].copy()
    skip = np.ones(len(PTS["bad"]), np.uint8)
    skip[case["matches"][g1]] = 0
    n, cur2 = O.search_by_projection_reloc(F["keys"], F["desc"], R.W, R.H, F["sf"], R.LOG_SF, T, R.camera_centre(T), R.K_TUM3, case["kf_keys"], case["kf_mp"],
                                           dict(PTS, skip=skip), cur, 10.0, 100, True)
    assert n == 3 and np.array_equal(cur2[g1], case["matches"][g1])


def test_p2_outliers_block_in_s2_and_are_optimised_again():
    got, case = R.oracle_result("s2_50"), CASES["s2_50"]
    g2 = case["feats"]["g2"]
    assert got["ran"] == 63 and got["nadditional"] == [40, 10]
    assert (got["frame_mp"][g2] == -1).all() and (got["outlier_last"][g2] == 1).all()           # nulled at :3333 only
    T3, idx3, _ = got["solves"][2]
    assert set(g2) <= set(idx3.tolist()) and len(idx3) == 60                                      # P3 optimised them again
    twins = case["kf_mp"][-(case["spec"]["twin"] + case["spec"]["c"]):][:case["spec"]["twin"]]
    assert not np.isin(twins, got["frame_mp"]).any()                                              # their feature was blocked


def test_bad_point_and_empty_candidate_and_empty_frame():
    got = R.oracle_result("bad_point")
    assert got["nadditional"][0] == 15 and not np.isin(CASES["bad_point"]["kf_mp"][-4:], got["frame_mp"]).any()
    assert len(CASES["nkf_zero"]["kf_keys"]) == 0 and R.oracle_result("nkf_zero")["nadditional"] == [0, 0]
    F0 = R.frame(True)
    case = dict(CASES["p1_10"], matches=np.zeros(0, np.int32), inliers=np.zeros(0, np.uint8))

    def pose_opt(Xw, obs, w, K4, T):
        assert len(Xw) == 0
        return 0, T, np.zeros(0, np.uint8)
    r = R.run_chain(case, PTS, pose_opt, None, keys=F0["keys"], inv_sigma2=F0["inv_sigma2"])
    assert r["ran"] == 1 and r["ngood_final"] == -1 and len(r["frame_mp"]) == 0


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["constructed"]])
def test_margin_condition(name):
    """A condition on the inputs: at the oracle's final pose of every optimisation every correspondence reprojects within 0.1 px or beyond 10 px,
    so no decision can turn on the 1e-4 pose parity between the device and the oracle."""
    keys = R.frame()["keys"]
    for T, idx, mp in R.oracle_result(name)["solves"]:
        if len(idx) < 3:
            continue
        uv = R.project(T, PTS["pos"][mp])
        err = np.hypot(uv[:, 0] - keys["x"][idx], uv[:, 1] - keys["y"][idx])
        assert ((err < 0.1) | (err > 10.0)).all(), (name, np.sort(err[(err >= 0.1) & (err <= 10.0)])[:5])


# ---- the round loop over a fake refine --------------------------------------------------------------------------------------------------
class FakeTracker:
    """reloc_refine from a table: hypothesis pose tag (Tcw7[4]) -> ngood_final; records the calls."""

    def __init__(self, n, table):
        self.n, self.table, self.calls = n, table, []

    def reloc_refine(self, hyps, params=None):
        self.calls.append([h[0] for h in hyps])
        H = len(hyps)
        mp = np.full((H, self.n), -1, np.int32); ol = np.full((H, self.n), 255, np.uint8); res = np.zeros(H, TR.RELOC_RESULT_DTYPE)
        for h, (cand, T, inl) in enumerate(hyps):
            tag = int(T[4])
            mp[h, cand] = tag                                # every hypothesis leaves a mark of its own
            ol[h, (cand + 1) % self.n] = tag & 1
            final = self.table[tag]
            res[h]["ran"] = 1 if final < 0 else 3
            res[h]["ngood_final"] = final
            res[h]["Tcw"] = T
        return mp, ol, res


def scripted(script, n):
    """solver_step from a per-candidate list of (bTcw, bNoMore, tag)."""
    at = [0] * len(script)

    def step(i):
        b_tcw, b_no_more, tag = script[i][at[i]]
        at[i] += 1
        T = np.array([0, 0, 0, 1, tag, 0, 0], np.float32)
        return b_tcw, b_no_more, np.ones(n, np.uint8), T
    return step


def _both(script, table, cands=None, n=8):
    out = []
    for spec in (True, False):
        ft = FakeTracker(n, table)
        st = TR.relocalize(ft, cands if cands is not None else [{}] * len(script), None, scripted(script, n), speculate_round=spec)
        out.append((st, ft))
    (a, fa), (b, fb) = out
    assert a["matched"] == b["matched"] and a["winner"] == b["winner"]
    for k in ("frame_mp", "outlier", "Tcw"):
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k
    return a, fa, b, fb


def test_round_logic_first_winner_in_order():
    # round 1: candidate 0 no pose, 1 loses, 2 loses; round 2: 0 loses, 1 wins, 2 would win too
    script = [[(False, False, 0), (True, False, 3)], [(True, False, 1), (True, False, 4)], [(True, False, 2), (True, False, 5)]]
    table = {1: 20, 2: -1, 3: 49, 4: 50, 5: 60}
    a, fa, b, fb = _both(script, table)
    assert a["matched"] and a["winner"] == 1 and a["rounds"] == 2
    assert fa.calls == [[1, 2], [0, 1, 2]] and a["steps"] == [2, 2, 2]
    assert fb.calls == [[1], [2], [0], [1]] and b["steps"] == [2, 2, 1], "one hypothesis a call: the reference's solver calls exactly"
    assert a["frame_mp"][1] == 4 and a["Tcw"][4] == 4
    # mvbOutlier is layered: every replayed hypothesis wrote its flag, the one behind the winner did not
    assert a["outlier"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]


def test_round_logic_no_more_discards():
    # candidate 0 gives a losing pose and bNoMore in round 1 (its hypothesis still runs, :3281-3287); candidate 1 ends in round 2
    script = [[(True, True, 1)], [(False, False, 0), (True, True, 2)]]
    a, fa, b, fb = _both(script, {1: 30, 2: 12})
    assert not a["matched"] and a["winner"] == -1 and a["rounds"] == 2 and a["steps"] == [1, 2]
    assert a["frame_mp"][1] == 2 and a["frame_mp"][0] == -1, "the frame is left as the last hypothesis that ran left it"


def test_round_logic_all_discarded_from_the_start():
    a, fa, b, fb = _both([[], []], {}, cands=[None, None])
    assert not a["matched"] and a["rounds"] == 0 and fa.calls == [] and a["frame_mp"] is None
