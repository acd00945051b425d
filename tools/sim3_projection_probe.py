"""Times rumi_search_by_projection_sim3_resident (include/rumi_mapping.h) against what a caller had before it for the same jobs, in one process:
one rumi_search_by_projection_sim3 call per job (the key-frame's key-points and descriptors and 72 bytes a point uploaded by every call, five
kernels and a synchronisation each).  Two shapes, each at 1000 and 2000 features: `stage` = 3 jobs on one slot x 4000 points, th 8 / 5 and both
projections (LoopClosing.cc:716, :738 for one candidate); `covis` = 30 jobs = 3 lists of 4000 x 10 slots, th 3 (the covisible check :773-795 of
three candidates).  The two paths are alternated call by call, `rounds` rounds of `reps` calls after a warm-up, every number a median with
the rounds' spread.  The C entries are timed with their arguments marshalled, so neither side is charged for Python, and the per-job side is
not charged for the host gather of the points' attributes.  The rows and counts are compared before a time is printed.
    python tools/sim3_projection_probe.py [--shapes stage:1000,stage:2000,covis:1000,covis:2000] [--reps 10] [--out profiles/sim3_projection_probe.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

LIST = 4000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="stage:1000,stage:2000,covis:1000,covis:2000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401
    import search_and_fuse_scene as F
    import search_in_neighbors_scene as S
    import sim3_projection_scene as P
    from search_and_fuse_probe import build_map
    from rumi_slam_amd import capi, mapping
    from rumi_slam_amd.matcher import ORBmatcher
    L = mapping._lib()
    for shape in a.shapes.split(","):
        kind, nf = shape.split(":")
        nf = int(nf)
        if kind == "stage":
            m = build_map(1, LIST, nf, 8100 + nf)
            p = m.poses[0]
            jobs = [P.Job(0, p, 0, LIST, P.STAGE_A, 0), P.Job(0, P.shifted(p, [0.02, -0.01, 0.03]), 0, LIST, P.STAGE_B, 1),
                    P.Job(0, P.shifted(p, [-0.03, 0.02, 0.0]), 0, LIST, P.STAGE_A, 1)]
        else:
            m = build_map(10, 3 * LIST, nf, 8200 + nf)
            jobs = [P.Job(k, m.poses[k], l * LIST, LIST, P.COVISIBLE, 0) for l in range(3) for k in range(10)]
        sc = P.Scene(m, np.arange(len(m.ids), dtype=np.int32), jobs)
        st = F.StoreScene(m)
        matcher = ORBmatcher(0.8, True, max_features=max(2048, nf), max_queries=16384)
        nj = len(jobs)

        # ---- the old path, marshalled: per job the listed points' attributes and the skip mask
        Kf = np.ascontiguousarray(S.K4, np.float32)
        old_args, old_rows, old_n = [], [], [C.c_int32() for _ in jobs]
        for j in jobs:
            pts = P.job_points(m, sc.ids[j.start:j.start + j.count])
            old_args.append([np.ascontiguousarray(j.pose[0], np.float32), np.ascontiguousarray(j.pose[1], np.float32)] +
                            [np.ascontiguousarray(pts[k]) for k in ("skip", "pos", "normal", "min_dist", "max_dist", "desc")])
            old_rows.append(np.full(m.kfs[j.k].n, -1, np.int32))

        def old():
            for jj, j in enumerate(jobs):
                x = old_args[jj]
                old_rows[jj][:] = -1
                capi.check(L.rumi_search_by_projection_sim3(matcher._h, C.byref(st.frames[j.k].c), C.c_float(S.LOG_SF), capi.ptr(x[0]), capi.ptr(x[1]), capi.ptr(Kf),
                                                            C.c_int32(j.count), *[capi.ptr(v) for v in x[2:]], C.c_int32(j.th), C.c_float(j.ratio),
                                                            C.c_int32(j.variant), capi.ptr(old_rows[jj]), C.byref(old_n[jj])))

        # ---- the new call, marshalled
        arr = sc.job_array()
        cap = sum(m.kfs[j.k].n for j in jobs)
        rows, start, nm = np.zeros(cap, np.int32), np.zeros(nj + 1, np.int32), np.zeros(nj, np.int32)

        def new():
            capi.check(L.rumi_search_by_projection_sim3_resident(matcher._h, st.store._h, capi.ptr(arr), nj, capi.ptr(sc.ids), len(sc.ids), capi.ptr(rows),
                                                                 capi.ptr(start), cap, capi.ptr(nm)))

        old(); new()
        equal = bool(all(rows[start[jj]:start[jj + 1]].tobytes() == old_rows[jj].tobytes() and nm[jj] == old_n[jj].value for jj in range(nj)))
        res_rounds = mapping.search_by_projection_sim3_rounds(matcher, nj)
        for _ in range(3):
            old(); new()
        per = {"per_job": [], "one_call": []}
        stage = []
        for _ in range(a.rounds):
            t = {"per_job": [], "one_call": []}
            for _ in range(a.reps):
                for name, fn in (("per_job", old), ("one_call", new)):
                    t0 = time.perf_counter()
                    fn()
                    t[name].append((time.perf_counter() - t0) * 1e3)
                stage.append(mapping.search_by_projection_sim3_stage_ms(matcher))
            for k in t:
                per[k].append(round(float(np.median(t[k])), 4))
        old_ms, new_ms = float(np.median(per["per_job"])), float(np.median(per["one_call"]))
        sm = np.median(np.stack(stage), 0)
        slots = len({j.k for j in jobs})
        line = {"shape": kind, "jobs": nj, "slots": slots, "list": LIST, "features": nf, "pairs": nj * LIST, "matches": int(nm.sum()),
                "equal_to_per_job": equal, "resolve_rounds": {"min": int(res_rounds.min()), "median": float(np.median(res_rounds)), "max": int(res_rounds.max())},
                "bytes_up_per_call": 128 * nj + 112 * slots + 4 * len(sc.ids), "bytes_up_per_job_loop": sum(73 * j.count + 60 * m.kfs[j.k].n for j in jobs),
                "bytes_back": 4 * (16 + 2 * nj + cap), "reps": a.reps, "rounds": a.rounds,
                "per_job": {"round_median_ms": per["per_job"], "ms": round(old_ms, 4)},
                "one_call": {"round_median_ms": per["one_call"], "ms": round(new_ms, 4), "stage_host_ms": round(float(sm[0]), 4),
                             "stage_device_ms": round(float(sm[1]), 4), "stage_write_out_ms": round(float(sm[2]), 4)},
                "ratio": round(old_ms / new_ms, 2)}
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        matcher.close()
        if not equal:
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
