"""Times rumi_search_in_neighbors_resident (include/rumi_mapping.h) against what a caller had before it for the same map, in one process: one
rumi_fuse_candidates call per target key-frame (its key-points, descriptors and the current key-frame's points uploaded by every call) and one
more the other way, with the candidate points of the targets' rows gathered on the host.  30 targets x 1000 features and 60 x 2000; the two
paths are alternated call by call, five rounds of `reps` calls after a warm-up, every number a median.  The C entries are timed with their
arguments marshalled, so neither side is charged for Python beyond the reverse pass's gather, which is the caller's work in the old path.
All outputs are compared (new call == per-target path, byte for byte) before a time is printed.
    python tools/search_in_neighbors_probe.py [--shapes 30x1000,60x2000] [--reps 20] [--out profiles/search_in_neighbors_probe.jsonl]"""
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
    ap.add_argument("--shapes", default="30x1000,60x2000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401
    import search_in_neighbors_scene as S
    from rumi_slam_amd import capi, mapping
    from rumi_slam_amd.matcher import ORBmatcher
    L = mapping._lib()
    for shape in a.shapes.split(","):
        nt, nf = (int(x) for x in shape.split("x"))
        m = S.seeded_map(1000 + nf, nt, n_extra=2, n_world=int(nf * 1.1), n_feat=nf)
        sc = S.StoreScene(m)
        matcher = ORBmatcher(0.6, True, max_features=max(2048, nf), max_queries=max(16384, nt * nf))
        obs = m.observations()
        cur = m.kfs[0]
        ids = np.asarray(cur.row, np.int64)
        safe = np.where(ids < 0, 0, ids)

        # ---- the old path, marshalled: per target the current key-frame's points with that target's skip flags
        def pts_of(idx, skip):
            return [np.ascontiguousarray(x) for x in (skip.astype(np.uint8), m.pos[idx], m.normal[idx], m.min_dist[idx], m.max_dist[idx], m.desc[idx])]
        fwd_args = []
        for t in range(nt):
            skip = np.array([p < 0 or m.bad[p] or (1 + t) in obs[p] for p in cur.row], bool)
            fwd_args.append(pts_of(safe, skip))
        Kf = np.ascontiguousarray(S.K4, np.float32)
        old_fwd = np.full((nt, cur.n), -1, np.int32)
        in_cur = np.array([0 in o for o in obs], bool)
        rows = [np.asarray(m.kfs[1 + t].row, np.int64) for t in range(nt)]
        state = {}

        def fuse(k, arrs, out):
            kf = m.kfs[k]
            capi.check(L.rumi_fuse_candidates(matcher._h, C.byref(sc.frames[k].c), float(S.LOG_SF), capi.ptr(kf.Tcw7), capi.ptr(kf.Ow), capi.ptr(Kf), len(arrs[0]),
                                              *[capi.ptr(x) for x in arrs], float(S.TH), 1, capi.ptr(out)))

        def old():
            for t in range(nt):
                fuse(1 + t, fwd_args[t], old_fwd[t])
            allp = np.concatenate(rows)                                   # LocalMapping.cc:706-727 on the host
            allp = allp[allp >= 0]
            allp = allp[~m.bad[allp] & ~in_cur[allp]]
            _, first = np.unique(allp, return_index=True)
            cand = allp[np.sort(first)]
            out = np.full(len(cand), -1, np.int32)
            if len(cand):
                fuse(0, pts_of(cand, np.zeros(len(cand), bool)), out)
            state["rev"] = (cand.astype(np.int32), out)

        # ---- the new call, marshalled
        slots = np.asarray([S.slot_of(k) for k in range(1, nt + 1)], np.int32)
        arr = (mapping.RumiFuseKF * nt)(*[sc.fuse_kf(k) for k in range(1, nt + 1)])
        c0 = sc.fuse_kf(0)
        cap = int(sum(len(r) for r in rows))
        fwd = np.full((nt, cur.n), -1, np.int32)
        rp, rb, n_rev = np.full(cap, -1, np.int32), np.full(cap, -1, np.int32), C.c_int32()

        def new():
            capi.check(L.rumi_search_in_neighbors_resident(matcher._h, sc.store._h, S.slot_of(0), C.byref(c0), capi.ptr(slots), C.byref(arr), nt, float(S.TH),
                                                           capi.ptr(fwd), capi.ptr(rp), capi.ptr(rb), cap, C.byref(n_rev)))

        old(); new()
        equal = bool(fwd.tobytes() == old_fwd.tobytes() and rp[:n_rev.value].tobytes() == state["rev"][0].tobytes()
                     and rb[:n_rev.value].tobytes() == state["rev"][1].tobytes())
        for _ in range(5):
            old(); new()
        rounds = {"per_target": [], "one_call": []}
        stage = []
        for _ in range(a.rounds):
            t = {"per_target": [], "one_call": []}
            for _ in range(a.reps):
                for name, fn in (("per_target", old), ("one_call", new)):
                    t0 = time.perf_counter()
                    fn()
                    t[name].append((time.perf_counter() - t0) * 1e3)
                stage.append(mapping.search_in_neighbors_stage_ms(matcher))
            for k in t:
                rounds[k].append(round(float(np.median(t[k])), 4))
        old_ms, new_ms = float(np.median(rounds["per_target"])), float(np.median(rounds["one_call"]))
        st = np.median(np.stack(stage), 0)
        line = {"targets": nt, "features": nf, "points": m.n_points, "forward_pairs": nt * cur.n, "forward_matches": int(np.count_nonzero(fwd >= 0)),
                "reverse_candidates": int(n_rev.value), "reverse_matches": int(np.count_nonzero(rb[:n_rev.value] >= 0)), "equal_to_per_target": equal,
                "reps": a.reps, "rounds": a.rounds, "per_target": {"round_median_ms": rounds["per_target"], "ms": round(old_ms, 4)},
                "one_call": {"round_median_ms": rounds["one_call"], "ms": round(new_ms, 4), "stage_host_ms": round(float(st[0]), 4),
                             "stage_device_ms": round(float(st[1]), 4), "stage_write_out_ms": round(float(st[2]), 4)},
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
