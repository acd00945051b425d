"""Times rumi_track_reloc_refine (include/rumi_track.h) against what a caller had before it, in one process: per pose hypothesis the chain of
single C entries of Tracking.cc:3287-3345 -- three rumi_pose_optimization and two rumi_search_by_projection_reloc calls, each with its uploads, its
synchronisation and its results brought back for one `if` on the host.  Setup: a 2000-feature frame, K = 5 candidate key-frames of 1000 points,
H = 1, 3, 5, 10 hypotheses that all take the longest path (P1, S1, P2, S2, P3; tests/reloc_cases.py builds them).  (i) the chain per hypothesis
and (ii) one refine call alternate call by call; `rounds` rounds of `reps` calls after a warm-up, every number a median over a round, the
spread the range of the round medians.  Both sides are timed through their Python mirrors (a host clock around work that ends in a
synchronise); the results are compared before a time is printed.  Gate (DESIGN.md 4r form): at H >= 3 (ii) below (i) in every round by more than
the larger spread; at H = 1 (ii) not above (i) by more than that spread.
    python tools/reloc_probe.py [--hyps 1,3,5,10] [--reps 30] [--rounds 5] [--out profiles/reloc_probe.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hyps", default="1,3,5,10")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import reloc_cases as R
    R.NFEATURES = 2000                                       # before the first frame(): the probe's frame, not the tests'
    from rumi_slam_amd import tracker as TR
    from rumi_slam_amd.matcher import FrameView, ORBmatcher, SearchByProjection_Reloc
    from rumi_slam_amd.optimizer import Optimizer
    from scene import K_TUM3
    F = R.frame()
    n = len(F["keys"])
    K, NKF = 5, 1000
    tab = R._Table()
    cases = [R._make_case(tab, f"long{k}", a=10, b=(10, 10, 10), g2=10, c=10, T0=R.T_NEAR if k & 1 else R.T_TRUE, fill=NKF - 60) for k in range(K)]
    pts = tab.arrays()
    assert all(len(c["kf_mp"]) == NKF and R.expected(c)["ran"] == 63 for c in cases)
    t = TR.Tracker(R.NFEATURES, 1.2, R.NLEVELS, 20, 7, R.W, R.H, max_points=8192)
    _, keys, desc = t.extract(F["img"])
    assert keys.tobytes() == F["keys"].tobytes()
    t.reloc_begin(K_TUM3, [dict(kf_keys=c["kf_keys"], kf_mp=c["kf_mp"], matches=c["matches"]) for c in cases], pts)
    opt, m = Optimizer(), ORBmatcher(0.9, True, max_features=4096, max_queries=8192)
    cur = FrameView(F["keys"], F["desc"], R.W, R.H, F["sf"])

    def chain(case):
        def search(T, Ow, skip, cm, th, dist):
            return SearchByProjection_Reloc(m, cur, R.LOG_SF, T, Ow, K_TUM3, case["kf_keys"], case["kf_mp"], dict(pts, skip=skip), cm, th, dist)
        return R.run_chain(case, pts, opt.PoseOptimization, search)

    rows = []
    for H in [int(x) for x in a.hyps.split(",")]:
        hs = [cases[h % K] for h in range(H)]
        hyps = [(h % K, c["Tcw7"], c["inliers"]) for h, c in enumerate(hs)]
        mp, ol, res = t.reloc_refine(hyps)
        for h, c in enumerate(hs):                           # equal before any time counts
            ref = chain(c)
            assert int(res[h]["ran"]) == ref["ran"] == 63 and np.array_equal(mp[h], ref["frame_mp"]) and np.array_equal(ol[h], ref["outlier_last"])
            assert res[h]["Tcw"].tobytes() == ref["Tcw"].tobytes()
        med = {"chain": [], "refine": []}
        for rnd in range(a.rounds + 1):                      # round 0 warms up
            ts = {"chain": [], "refine": []}
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for c in hs:
                    chain(c)
                t1 = time.perf_counter()
                t.reloc_refine(hyps)
                t2 = time.perf_counter()
                ts["chain"].append(t1 - t0); ts["refine"].append(t2 - t1)
            if rnd:
                for k in med:
                    med[k].append(float(np.median(ts[k])) * 1e3)
        spread = max(max(v) - min(v) for v in med.values())
        ok = all(r < c - spread for c, r in zip(med["chain"], med["refine"])) if H >= 3 else all(r <= c + spread for c, r in zip(med["chain"], med["refine"]))
        row = dict(probe="reloc", H=H, K=K, nfeat=n, nkf=NKF, reps=a.reps, rounds=a.rounds, chain_ms=med["chain"], refine_ms=med["refine"],
                   chain_median_ms=float(np.median(med["chain"])), refine_median_ms=float(np.median(med["refine"])), spread_ms=spread,
                   launches_refine=17, calls_chain=5 * H, gate="below" if H >= 3 else "not above", gate_ok=bool(ok), attempts=t.reloc_attempts())
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
