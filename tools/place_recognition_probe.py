"""Times the Sim3 RANSAC and OptimizeSim3 stages of DetectCommonRegionsFromBoW (LoopClosing.cc:655-676, :728) for J candidates, in one process:
(a) what a caller had before: per candidate rumi_sim3_ransac in blocks of 20 iterations until the solver converges or runs out, and one
    rumi_optimize_sim3 per candidate;
(b) rumi_sim3_ransac_batch in rounds over a window of the shared iteration stream, and one rumi_optimize_sim3_batch call.
The times are those of the C entries alone, with their arguments marshalled, uploads, downloads and synchronisation included: the minimal sets are
drawn before the clock starts.  That host work is NOT in any figure; it is the same stream on both sides, but the batch side draws J x window sets a
round, so it grows with the window there and a comparison between windows by these figures is a comparison of the device entry only.  The two paths are alternated call by call, `rounds` rounds of `reps` calls after a
warm-up of every shape; every number is a median with the rounds' spread.  Both paths' results are compared before a time is printed.
    python tools/place_recognition_probe.py [--candidates 3,6] [--windows default,250,40] [--reps 100] [--out profiles/place_recognition_probe.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

# (seed, n_solver, outlier_frac, mRansacMinInliers): the scenes of tests/sim3_batch_scene.py and three more in the same range of N
EXTRA = [(10, 60, 0.45, 25), (11, 150, 0.50, 60), (12, 100, 0.50, 40)]
OPT_N = [100, 250, 400, 150, 300, 200]


class Recorder:
    """Forwards the two RANSAC entries of an Optimizer and keeps every call's arguments."""

    def __init__(self, opt):
        self.opt, self.single, self.batch = opt, [], []

    def Sim3Ransac(self, X1, X2, s1, s2, K1, K2, tri, fix_scale=False, score=None, want_inliers=True):
        self.single.append((X1, X2, s1, s2, K1, K2, np.ascontiguousarray(tri, np.int32), fix_scale))
        return self.opt.Sim3Ransac(X1, X2, s1, s2, K1, K2, tri, fix_scale=fix_scale)

    def Sim3RansacBatch(self, sol, X1, X2, s1, s2, tri, want_all=False):
        self.batch.append(tuple(np.ascontiguousarray(a) for a in (sol, X1, X2, s1, s2, tri)))
        return self.opt.Sim3RansacBatch(sol, X1, X2, s1, s2, tri)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="3,6")
    ap.add_argument("--windows", default="default,250,40")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401
    import sim3_batch_scene as B
    from rumi_slam_amd import capi
    from rumi_slam_amd.optimizer import SIM3_OPT_PROBLEM_DTYPE, SIM3_RANSAC_RESULT_DTYPE, Optimizer
    from rumi_slam_amd.sim3solver import GlibcRand, Sim3SolverBatch
    from sim3_scene import sim3_pair_problem
    opt = Optimizer()
    L, h, P = opt._lib, opt._h, capi.ptr
    for J in [int(x) for x in a.candidates.split(",")]:
        run = (B.RUN1 + EXTRA)[:J]
        # ---- (a) per candidate: the calls the reference's loop makes, recorded once
        rec = Recorder(opt)
        g = GlibcRand(0)
        want = B.reference_loop(B.make_solvers(rec, run, g))
        next_rand = g.rand()
        calls_a = []
        for X1, X2, s1, s2, K1, K2, tri, fix in rec.single:
            H, n = len(tri), len(X1)
            T, nin, inl = np.zeros((H, 16), np.float32), np.zeros(H, np.int32), np.zeros((H, n), np.uint8)
            calls_a.append(((h, n, P(X1), P(X2), P(s1), P(s2), P(K1), P(K2), int(fix), H, P(tri), None, P(T), P(nin), P(inl), None, None), (X1, X2, s1, s2, K1, K2, tri, T, nin, inl)))

        def ransac_a():
            for args, _ in calls_a:
                capi.check(L.rumi_sim3_ransac(*args))

        # ---- OptimizeSim3: one problem per candidate
        probs = [sim3_pair_problem(seed=20 + k, n=OPT_N[k]) for k in range(J)]
        opt_a_args, opt_a_keep = [], []
        for b in probs:
            n = len(b["w1"])
            arrs = [np.ascontiguousarray(b[k], np.float32) for k in ("P1c", "P2c", "obs1", "obs2", "w1", "w2")] + [np.ascontiguousarray(b["K"], np.float32)]
            S, st, r3 = np.ascontiguousarray(b["S0"], np.float64).copy(), np.zeros(n, np.uint8), np.zeros(3, np.int32)
            opt_a_keep.append((arrs, S, st, r3, np.ascontiguousarray(b["S0"], np.float64)))
            opt_a_args.append((h, n, None, 0, None, None, *[P(x) for x in arrs[:6]], None, None, P(arrs[6]), P(arrs[6]), C.c_float(10.0), 0, 1, P(S), P(st), P(r3)))

        def optimize_a():
            for args, keep in zip(opt_a_args, opt_a_keep):
                keep[1][:] = keep[4]
                capi.check(L.rumi_optimize_sim3(*args))

        pr = np.zeros(J, SIM3_OPT_PROBLEM_DTYPE)
        first = 0
        for r, b in zip(pr, probs):
            r["first"], r["n"], r["th2"], r["fix_scale"], r["robust_first_pass"], r["K4_1"], r["K4_2"] = first, len(b["w1"]), 10.0, 0, 1, b["K"], b["K"]
            first += len(b["w1"])
        cat = [np.ascontiguousarray(np.concatenate([k[0][i] for k in opt_a_keep])) for i in range(6)]
        S0 = np.stack([k[4] for k in opt_a_keep]); Sb = S0.copy(); stb = np.zeros(first, np.uint8); r3b = np.zeros((J, 3), np.int32)
        opt_b_args = (h, J, P(pr), first, *[P(x) for x in cat], P(Sb), P(stb), P(r3b))

        def optimize_b():
            Sb[:] = S0
            capi.check(L.rumi_optimize_sim3_batch(*opt_b_args))

        optimize_a(); optimize_b()
        opt_equal = bool(all(Sb[k].tobytes() == opt_a_keep[k][1].tobytes() and np.array_equal(r3b[k], opt_a_keep[k][3]) and
                             np.array_equal(stb[pr["first"][k]:pr["first"][k] + pr["n"][k]], opt_a_keep[k][2]) for k in range(J)))

        # ---- (b) rounds of the batch entry, per window
        for wname in a.windows.split(","):
            window = None if wname == "default" else int(wname)      # default: 20 for every solver still running, the reference's block
            rec_b = Recorder(opt)
            g = GlibcRand(0)
            got, rounds_used = Sim3SolverBatch(rec_b, B.make_solvers(rec_b, run, g), g).run(window)
            B.assert_same_results(got, want)
            equal = g.rand() == next_rand
            calls_b = []
            for sol, X1, X2, s1, s2, tri in rec_b.batch:
                res, inl = np.zeros(len(sol), SIM3_RANSAC_RESULT_DTYPE), np.zeros(len(X1), np.uint8)
                calls_b.append(((h, len(sol), P(sol), len(X1), P(X1), P(X2), P(s1), P(s2), tri.shape[1], P(tri), P(res), P(inl), None, None), (sol, X1, X2, s1, s2, tri, res, inl)))

            def ransac_b():
                for args, _ in calls_b:
                    capi.check(L.rumi_sim3_ransac_batch(*args))

            paths = {"ransac_per_candidate": ransac_a, "ransac_batch": ransac_b, "optimize_per_candidate": optimize_a, "optimize_batch": optimize_b}
            for _ in range(5):
                for fn in paths.values():
                    fn()
            per = {k: [] for k in paths}
            for _ in range(a.rounds):
                t = {k: [] for k in paths}
                for _ in range(a.reps):
                    for name, fn in paths.items():
                        t0 = time.perf_counter()
                        fn()
                        t[name].append((time.perf_counter() - t0) * 1e3)
                for k in t:
                    per[k].append(round(float(np.median(t[k])), 4))
            ms = {k: round(float(np.median(v)), 4) for k, v in per.items()}
            spread = {k: round(max(v) - min(v), 4) for k, v in per.items()}
            old, new = ms["ransac_per_candidate"] + ms["optimize_per_candidate"], ms["ransac_batch"] + ms["optimize_batch"]
            line = {"candidates": J, "N": [r[1] for r in run], "iterations": [w[4] for w in want], "converged": [bool(w[0]) for w in want],
                    "window": wname, "window_first_round": int(rec_b.batch[0][5].shape[1]), "rounds_used": rounds_used,
                    "hypotheses_evaluated": {"per_candidate": int(sum(len(c[1][6]) for c in calls_a)), "batch": int(sum(c[1][5].shape[0] * c[1][5].shape[1] for c in calls_b))},
                    "calls": {"ransac_per_candidate": len(calls_a), "ransac_batch": len(calls_b), "optimize_per_candidate": J, "optimize_batch": 1},
                    "optimize_n": OPT_N[:J], "equal_to_per_candidate": bool(equal and opt_equal), "reps": a.reps, "rounds": a.rounds,
                    "ms": ms, "round_median_ms": per, "spread_ms": spread, "per_candidate_total_ms": round(old, 4), "batch_total_ms": round(new, 4),
                    "gain_ms": round(old - new, 4), "larger_spread_ms": round(max(spread["ransac_per_candidate"] + spread["optimize_per_candidate"],
                                                                                  spread["ransac_batch"] + spread["optimize_batch"]), 4)}
            line["accepted"] = bool(line["gain_ms"] > line["larger_spread_ms"])
            print(json.dumps(line), flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            if not (equal and opt_equal):
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
