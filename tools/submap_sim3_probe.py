"""The sub-map alignment session (rumi_submap_sim3_begin + score + ransac + 2 x score + end) against the chain it replaces, in one process.

The chain is what ComputeSubmapSim3 runs through the per-call entries: per solver ``while (!bNoMore && !bConverge) iterate(20)`` as one
rumi_sim3_ransac of 20 hypotheses with the score set passed again every call, the sequential rule on the host between the calls, and three
rumi_sim3_inliers calls for the ComputeInliersNum at CloudMerging.cc:611, :748 and :809.  Both sides get the same pre-drawn minimal sets (the
drawing is host Python on either side and is not what is compared) and are checked to agree on every solver's outcome before anything is timed.

Shapes: 40 key-frame pairs x 300 matches and 10 x 150; cases: 15 solvers x 300 iterations with nothing converging, and a convergence inside
the first 20 iterations; chunk lengths 64, 256, 1024, the whole stream and the library's default (64, then doubling up to 1024).  One JSON line per (shape, case, chunk): medians over ``--rounds``
rounds of ``--calls`` calls by the host clock (every call ends in a device synchronise).

    python tools/submap_sim3_probe.py --out profiles/submap_sim3_probe.jsonl [--rounds 5] [--calls 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

N_SOLVERS, N_CORR, MAX_ITS = 15, 90, 300


def build(n_pairs, per_pair, seed=0):
    from sim3_scene import sim3_ransac_problem
    score = sim3_ransac_problem(seed, n_pairs=n_pairs, per_pair=per_pair)["score"]
    solvers = []
    for j in range(N_SOLVERS):
        pr = sim3_ransac_problem(seed + 100 + j, n_pairs=1, per_pair=20, n_solver=N_CORR)
        solvers.append(dict(X1=pr["X1"], X2=pr["X2"], s1=pr["sigma2_1"], s2=pr["sigma2_2"], K=pr["K"], S_kf1w=pr["score"]["S_kf1w"], S_kf2w=pr["score"]["S_kf2w"]))
    return score, solvers


def composed(score):
    """One pair of composed transform tables for the three ComputeInliersNum calls (the values do not matter to the time)."""
    import sim3_cases as S3
    Sw = (S3.rotvec([0.05, -0.2, 0.08]), np.array([0.4, -0.2, 0.3]), 1.25)
    A = np.stack([S3.sim8(*S3.sim_mul(S3.sim_Rts(a), Sw)) for a in score["S_c1w1"]])
    B = np.stack([S3.sim8(*S3.sim_mul(S3.sim_Rts(b), S3.sim_inv(Sw))) for b in score["S_c2w2"]])
    return A, B


def chain(opt, score, solvers, min_inliers, tri, AB):
    """The per-call path.  Returns (index of the converged solver or None, iterations consumed, best inliers per solver reached)."""
    inl = lambda: opt.ComputeInliersNum(score["pair_start"], score["pair_denominator"], AB[0], AB[1], score["K4_1"], score["K4_2"], score["X1"], score["X2"],
                                        score["kp1"], score["kp2"], score["sigma2_1"], score["sigma2_2"], score["edge1"], score["edge2"])
    inl()
    best_ratio, pos, conv_at, best = np.float32(0), 0, None, []
    for j, s in enumerate(solvers):
        sc = dict(score, S_kf1w=s["S_kf1w"], S_kf2w=s["S_kf2w"])
        best_n, last, used = 0, None, 0
        while used < MAX_ITS and conv_at is None:
            r = opt.Sim3Ransac(s["X1"], s["X2"], s["s1"], s["s2"], s["K"], s["K"], tri[pos + used:pos + min(used + 20, MAX_ITS)], score=sc, want_inliers=False)
            for h in range(len(r["n_inliers"])):
                if r["valid"][h]:
                    last = (int(r["n_inliers"][h]), r["median"][h])
                elif last is None:
                    last = (0, r["median"][h])
                used += 1
                if last[1] >= best_ratio and last[0] >= best_n:
                    best_n, best_ratio = last[0], last[1]
                    if float(last[1]) > 0.10 and last[0] > min_inliers:
                        conv_at = j
                        break
        best.append(best_n)
        pos += used
        if conv_at is not None:
            break
    inl(); inl()
    return conv_at, pos, best


def session(ses, score, prepared, tri, AB):
    ses.begin(score)
    ses.score([AB], want_inliers=True)
    rc, out = ses.ransac_status(prepared, tri)
    ses.score([AB], want_inliers=True); ses.score([AB], want_inliers=True)
    ses.end()
    assert rc == 0
    return out


def rounds_ms(fn, rounds, calls):
    fn(); fn()
    per = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        per.append((time.perf_counter() - t0) * 1e3 / calls)
    return float(np.median(per)), float(np.min(per)), float(np.max(per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    a = ap.parse_args()
    from rumi_slam_amd.optimizer import Optimizer, SIM3_CONVERGED
    from rumi_slam_amd.sim3solver import GlibcRand
    from rumi_slam_amd.submap import SUBMAP_SOLVER_DTYPE, SubmapSim3, SubmapSolver, draw_stream
    opt, opt_chain = Optimizer(), Optimizer()
    ses = SubmapSim3(opt)
    lines = []
    for n_pairs, per_pair in ((40, 300), (10, 150)):
        score, solvers = build(n_pairs, per_pair)
        AB = composed(score)
        for case, min_inliers in (("none_converges", N_CORR), ("converges_in_first_20", 40)):
            subs = [SubmapSolver(s["X1"], s["X2"], s["s1"], s["s2"], s["K"], s["K"], s["S_kf1w"], s["S_kf2w"], min_inliers, MAX_ITS) for s in solvers]
            tri = draw_stream(subs, GlibcRand(0))
            rec = np.zeros(len(subs), SUBMAP_SOLVER_DTYPE)
            for j, (r, s) in enumerate(zip(rec, subs)):
                r["first"], r["n"], r["min_inliers"], r["its"], r["K4_1"], r["K4_2"], r["S_kf1w"], r["S_kf2w"] = j * N_CORR, s.N, min_inliers, MAX_ITS, s.K1, s.K2, s.S_kf1w, s.S_kf2w
            cat = lambda name: np.concatenate([getattr(s, name) for s in subs])
            prepared = (rec, cat("X1"), cat("X2"), cat("s1"), cat("s2"))
            conv_at, used, best = chain(opt_chain, score, solvers, min_inliers, tri, AB)
            if case == "none_converges":
                assert conv_at is None and used == N_SOLVERS * MAX_ITS
            else:
                assert conv_at == 0 and used <= 20, (conv_at, used)
            chain_ms = rounds_ms(lambda: chain(opt_chain, score, solvers, min_inliers, tri, AB), a.rounds, a.calls)
            for chunk in (64, 256, 1024, None, 0):
                ses.set_chunk(chunk)
                out = session(ses, score, prepared, tri, AB)
                got = np.flatnonzero(out["state"] == SIM3_CONVERGED)
                assert out["its_consumed"] == used and (int(got[0]) if len(got) else None) == conv_at
                assert list(out["best_inliers"][:len(best)]) == best
                ses_ms = rounds_ms(lambda: session(ses, score, prepared, tri, AB), a.rounds, a.calls)
                line = dict(probe="submap_sim3", pairs=n_pairs, matches_per_pair=per_pair, total=int(score["pair_start"][-1]), solvers=N_SOLVERS, its=MAX_ITS, case=case,
                            iterations_consumed=int(used), chunk="all" if chunk is None else ("default" if chunk == 0 else chunk), rounds=a.rounds, calls=a.calls,
                            session_ms=round(ses_ms[0], 4), session_ms_min_max=[round(ses_ms[1], 4), round(ses_ms[2], 4)],
                            chain_ms=round(chain_ms[0], 4), chain_ms_min_max=[round(chain_ms[1], 4), round(chain_ms[2], 4)],
                            chain_over_session=round(chain_ms[0] / ses_ms[0], 3))
                print(json.dumps(line), flush=True)
                lines.append(line)
    ses.set_chunk(0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
