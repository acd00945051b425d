"""Times rumi_essential_graph (include/rumi_opt.h) on synthetic loop-closure graphs (tests/essential_scene.py, make_scene) of 100, 500 and
2560 key-frames and, where it is affordable, the scalar oracle (tests/cpp/essential_oracle.cc, g++ -O2, dense LL^T on one core) on the same
graph.  Per size one JSON line: vertices, edges, unknowns, LM iterations / trials, the wall time of the C entry (arguments marshalled; one
warm call, then the median of `--reps`), the wall time per trial, the device time of the last trial's factorisation and back-substitution
(HIP events, rumi_opt_stage_ms [3]) and what is left of a trial beside it (assembly, update, chi2, the host round trip).  The oracle runs the
full optimisation up to --oracle-full vertices and ONE iteration (a timing per trial) up to --oracle-max; above that it is skipped: its
factorisation is (7 n)^3 / 3 operations in scalar code.  Where both ran the same iterations the results are asserted to agree before a time
is reported.
    python tools/essential_probe.py [--sizes 100 500 2560] [--reps 3] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100, 500, 2560])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--oracle-full", type=int, default=100)
    ap.add_argument("--oracle-max", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import essential_scene as es
    from rumi_slam_amd import capi
    from rumi_slam_amd.optimizer import Optimizer

    opt = Optimizer(max_pose_edges=64, max_pose_batch=1, max_kf=max(a.sizes) + 8, max_mp=1024, max_edges=1 << 16)
    L = opt._lib
    out = open(a.out, "w") if a.out else None
    for n in a.sizes:
        sc = es.make_scene(n_free=n - 1, seed=1, isolated=False)

        def call(n_it):
            S = sc.S.copy(); stats = np.zeros(4, np.int32); trace = np.zeros(n_it + 1)
            t0 = time.perf_counter()
            rc = L.rumi_essential_graph(opt._h, sc.n_v, capi.ptr(S), capi.ptr(sc.fixed), capi.ptr(sc.fix_scale), sc.n_e, capi.ptr(sc.v0), capi.ptr(sc.v1),
                                        capi.ptr(sc.meas), n_it, None, capi.ptr(stats), capi.ptr(trace))
            dt = (time.perf_counter() - t0) * 1e3
            capi.check(rc)
            return dt, S, stats, trace

        call(a.iterations)                                        # warm: allocations, first launches
        runs = [call(a.iterations) for _ in range(a.reps)]
        ms = float(np.median([r[0] for r in runs]))
        _, S, stats, trace = runs[-1]
        solve_ms = float(opt.stage_ms()[3])
        trials = int(stats[1])
        rec = dict(vertices=sc.n_v, edges=sc.n_e, unknowns=7 * int(stats[2]), iterations=int(stats[0]), trials=trials, ended=int(stats[3]),
                   chi2_first=float(trace[0]), chi2_last=float(trace[stats[0]]), device_call_ms=round(ms, 3), device_ms_per_trial=round(ms / max(trials, 1), 3),
                   device_last_trial_solve_ms=round(solve_ms, 3), device_rest_of_trial_ms=round(ms / max(trials, 1) - solve_ms, 3))
        if n <= a.oracle_max:
            n_it = a.iterations if n <= a.oracle_full else 1
            t0 = time.perf_counter()
            ref = es.run_oracle(sc, n_it)
            oms = (time.perf_counter() - t0) * 1e3
            rec.update(oracle_iterations=n_it, oracle_trials=int(ref["stats"][1]), oracle_ms=round(oms, 1), oracle_ms_per_trial=round(oms / max(int(ref["stats"][1]), 1), 1))
            dS = call(n_it)[1] if n_it != a.iterations else S
            rec["pose_rel_diff_vs_oracle"] = float(np.abs(dS - ref["S"]).max() / np.abs(ref["S"]).max())
            assert rec["pose_rel_diff_vs_oracle"] < 1e-4, rec
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()
    opt.close()


if __name__ == "__main__":
    main()
