"""Times rumi_track_reloc_refine (include/rumi_track.h) against what a caller had before it, in one process: per pose hypothesis the chain of
single C entries of Tracking.cc:3287-3345 -- three rumi_pose_optimization and two rumi_search_by_projection_reloc calls, each with its uploads, its
synchronisation and its results brought back for one `if` on the host.  Setup: a 2000-feature frame, K = 5 candidate key-frames of 1000 points,
H = 1, 3, 5, 10 hypotheses that all take the longest path (P1, S1, P2, S2, P3; tests/reloc_cases.py builds them).  (i) the chain per hypothesis
and (ii) one refine call alternate call by call; `rounds` rounds of `reps` calls after a warm-up, every number a median over a round, the
spread the range of the round medians.  Both sides are timed through their Python mirrors (a host clock around work that ends in a
synchronise); the results are compared before a time is printed.  Gate (DESIGN.md 4r form): at H >= 3 (ii) below (i) in every round by more than
the larger spread; at H = 1 (ii) not above (i) by more than that spread.
    python tools/reloc_probe.py [--hyps 1,3,5,10] [--reps 30] [--rounds 5] [--out profiles/reloc_probe.jsonl]
With --resident it times what opens the call instead -- the BoW walk and the session's begin, by host pointers against by slot (see resident()):
    python tools/reloc_probe.py --resident [--hyps 1,3,5,10] --out profiles/reloc_resident_probe.jsonl"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def resident(a):
    """--resident: what opens a Relocalization call, by host pointers and by slot, in one process on the same scene.
    (i) rumi_search_by_bow_batch + rumi_track_reloc_begin: the K key-frames and the point table packed and uploaded by the call;
    (ii) rumi_track_reloc_bow + rumi_track_reloc_begin_resident: the same key-frames and points read in a covisibility store.
    The two alternate call by call through their Python mirrors; medians of `reps` calls a round over `rounds` rounds after a warm-up, at
    K = 1, 3, 5, 10, once with the store current and once with 50 attribute edits staged before every (ii) call (their upload is inside its
    time).  Gate: (ii) not above (i) at K = 1, below it by more than the larger spread of the round medians at K >= 3.  compute_bow is timed
    and reported, not gated."""
    import reloc_cases as R
    R.NFEATURES = 2000
    import voc_scene
    from rumi_slam_amd import matcher as M
    from rumi_slam_amd import tracker as TR
    from rumi_slam_amd.covis import Covisibility
    from rumi_slam_amd.vocabulary import ORBVocabulary
    from scene import K_TUM3
    F = R.frame()
    n = len(F["keys"])
    KMAX, NKF, LEVELSUP = 10, 1000, 1
    tab = R._Table()
    cases = [R._make_case(tab, f"long{k}", a=10, b=(10, 10, 10), g2=10, c=10, T0=R.T_NEAR if k & 1 else R.T_TRUE, fill=NKF - 60) for k in range(KMAX)]
    pts = tab.arrays()
    npt = len(pts["bad"])
    voc = ORBVocabulary(*voc_scene.synthetic_vocabulary(3, 10, 3))
    t = TR.Tracker(R.NFEATURES, 1.2, R.NLEVELS, 20, 7, R.W, R.H, max_points=npt + 64)
    _, keys, desc = t.extract(F["img"])
    assert keys.tobytes() == F["keys"].tobytes()
    # a key-frame feature carries its point's descriptor (the frame feature it was built from, or its complement); mFeatVec is its transform
    cov = Covisibility(KMAX + 1, npt + 64)
    cov.set_keyframes(list(range(KMAX)), [3000 + k for k in range(KMAX)], [0] * KMAX, [0] * KMAX, [c["kf_mp"] for c in cases], [[]] * KMAX, [-1] * KMAX, [[]] * KMAX)
    cov.set_points(list(range(npt)), pts["bad"], [[]] * npt)
    zeros3 = np.zeros((npt, 3), np.float32)
    cov.set_point_attributes(list(range(npt)), pts["pos"], zeros3, pts["min_dist"], pts["max_dist"], pts["desc"])
    kfs, fvs = [], []
    for k, c in enumerate(cases):
        kd = pts["desc"][c["kf_mp"]]
        kfs.append(M.FrameView(c["kf_keys"], kd, R.W, R.H, F["sf"]))
        fvs.append(M.FeatureVector.from_csr(*voc.transform(kd, LEVELSUP)[1]))
        cov.set_keyframe_features(k, kfs[k], fvs[k], K_TUM3)
    m = M.ORBmatcher(0.75, True, max_features=4096, max_queries=8192)
    cur = M.FrameView(F["keys"], F["desc"], R.W, R.H, F["sf"])
    tb = []
    for _ in range(a.reps):
        b = t.compute_bow(voc, LEVELSUP)
        tb.append(t.last_call_s)
    f_fv = M.FeatureVector.from_csr(*voc.assemble(b["word_id"], b["word_weight"], b["node_id"])[1])
    edit = list(range(50))

    def host(K):
        nm, rows = M.SearchByBoW_batch(m, kfs[:K], fvs[:K], [c["kf_mp"] for c in cases[:K]], [pts["bad"]] * K, cur, f_fv)
        t.reloc_begin(K_TUM3, [dict(kf_keys=cases[k]["kf_keys"], kf_mp=cases[k]["kf_mp"], matches=rows[k]) if nm[k] >= 15 else None for k in range(K)
                               if nm[k] >= 15], pts)
        return nm, rows

    def store(K):
        nm, rows = t.reloc_bow(cov, list(range(K)), 0.75, True)
        ids = t.reloc_begin_resident(cov, K_TUM3, [k for k in range(K) if nm[k] >= 15])
        return nm, rows, ids

    out = [dict(probe="reloc_resident_compute_bow", nfeat=n, reps=a.reps, median_ms=float(np.median(tb)) * 1e3, gated=False)]
    print(json.dumps(out[0]), flush=True)
    for staged in (0, 50):
        for K in [int(x) for x in a.hyps.split(",")]:
            nm1, rows1 = host(K)
            keep = [k for k in range(K) if nm1[k] >= 15]
            hyp = [(j, cases[k]["Tcw7"], (rows1[k] >= 0).astype(np.uint8)) for j, k in enumerate(keep)]
            want = t.reloc_refine(hyp) if hyp else None
            nm2, rows2, ids = store(K)
            assert np.array_equal(nm1, nm2) and np.array_equal(rows1, rows2), "the two walks agree before any time counts"
            if hyp:
                mp, ol, res = t.reloc_refine(hyp)
                assert np.array_equal(np.stack([TR.rows_to_ids(r, ids) for r in mp]), want[0]) and np.array_equal(ol, want[1]) and res.tobytes() == want[2].tobytes()
            med = {"host": [], "store": []}
            for rnd in range(a.rounds + 1):                  # round 0 warms up
                ts = {"host": [], "store": []}
                for _ in range(a.reps):
                    if staged:
                        cov.set_point_attributes(edit, pts["pos"][:50], zeros3[:50], pts["min_dist"][:50], pts["max_dist"][:50], pts["desc"][:50])
                    t0 = time.perf_counter()
                    host(K)
                    t1 = time.perf_counter()
                    store(K)
                    t2 = time.perf_counter()
                    ts["host"].append(t1 - t0); ts["store"].append(t2 - t1)
                if rnd:
                    for k in med:
                        med[k].append(float(np.median(ts[k])) * 1e3)
            spread = max(max(v) - min(v) for v in med.values())
            ok = all(r < c - spread for c, r in zip(med["host"], med["store"])) if K >= 3 else all(r <= c for c, r in zip(med["host"], med["store"]))
            row = dict(probe="reloc_resident", K=K, live=len(keep), nfeat=n, nkf=NKF, table_rows=int(len(ids)), staged_attribute_edits=staged, reps=a.reps,
                       rounds=a.rounds, host_ms=med["host"], store_ms=med["store"], host_median_ms=float(np.median(med["host"])),
                       store_median_ms=float(np.median(med["store"])), spread_ms=spread, gate="below" if K >= 3 else "not above", gate_ok=bool(ok))
            out.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hyps", default="1,3,5,10")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resident", action="store_true", help="time the BoW walk and the session's begin by host pointers against by slot (--hyps: the K values)")
    a = ap.parse_args()
    if a.resident:
        return resident(a)
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
