"""Times rumi_search_and_fuse_resident (include/rumi_mapping.h) against what a caller had before it for the same map, in one process: one
rumi_fuse_candidates call per corrected key-frame (check_reprojection = 0; its key-points, descriptors and the whole loop-point list with that
key-frame's skip mask uploaded by every call), which is what the facade's per-key-frame Fuse(pKF, Scw, ...) makes.  30 key-frames x 3000 loop
points and 100 x 8000, both at 1000 and 2000 features; the two paths are alternated call by call, five rounds of `reps` calls after a warm-up,
every number a median.  The C entries are timed with their arguments marshalled, so neither side is charged for Python, and the per-key-frame
side is not charged for the host gather of positions, normals and descriptors the facade repeats for every key-frame.  The outputs are compared
(hits == per-key-frame answers, pair for pair) before a time is printed.
    python tools/search_and_fuse_probe.py [--shapes 30x3000x1000,...] [--reps 10] [--out profiles/search_and_fuse_probe.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def build_map(nk, npts, nf, seed):
    """The loop points are points 0 .. npts - 1 in a wide box; nk corrected key-frames along the box each see the part of it in front of them,
    under a pose derived from a Sim3 with scale != 1.  A feature holds nothing (60 %), a point of the key-frame's own (30 %: the occupant a hit
    previews) or the loop point itself (10 %: a pair the key-frame lists)."""
    import search_and_fuse_scene as F
    import search_in_neighbors_scene as S
    rng = np.random.default_rng(seed)
    world = np.stack([rng.uniform(-12, 12, npts), rng.uniform(-2.2, 2.2, npts), rng.uniform(5.0, 9.0, npts)], 1).astype(np.float32)
    wdesc = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    level = rng.integers(1, 5, npts)
    dist = np.linalg.norm(world.astype(np.float64), axis=1)
    pos, normal = [world], [(world / dist[:, None]).astype(np.float32)]
    mx = [(dist * S.SF[level]).astype(np.float32)]
    desc = [wdesc]
    n_next = npts
    kfs, poses, sim3 = [], {}, {}
    for k in range(nk):
        q7, _ = S.pose_ry(rng.uniform(-0.03, 0.03), [rng.uniform(-9, 9), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])
        (T7, Ow), sim3[k] = F.corrected_pose(q7[:4], q7[4:], rng.uniform(0.8, 1.25))
        poses[k] = (T7, Ow)
        x, y, z, w = np.float64(T7[:4])
        R = np.float64([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        pc = world.astype(np.float64) @ R.T + np.float64(T7[4:])
        u, v = S.K4[0] * pc[:, 0] / pc[:, 2] + S.K4[2], S.K4[1] * pc[:, 1] / pc[:, 2] + S.K4[3]
        vis = np.nonzero((pc[:, 2] > 0.1) & (u > 6) & (u < S.W - 6) & (v > 6) & (v < S.H - 6))[0]
        seen = rng.permutation(vis)[:int(nf * 0.85)]
        ns, nc = len(seen), nf - len(seen)
        xy = np.concatenate([np.stack([u[seen], v[seen]], 1) + rng.uniform(-0.8, 0.8, (ns, 2)), rng.uniform([4, 4], [S.W - 4, S.H - 4], (nc, 2))])
        octs = np.concatenate([level[seen] - rng.integers(0, 2, ns), rng.integers(0, S.NLEVELS, nc)])
        noise = np.packbits(rng.random((ns, 256)) < 0.04, axis=1)                 # about ten bits a row
        ds = np.concatenate([wdesc[seen] ^ noise, rng.integers(0, 256, (nc, 32), dtype=np.uint8)])
        r = rng.random(ns)
        own = np.nonzero((r >= 0.6) & (r < 0.9))[0]
        row = np.full(nf, -1, np.int64)
        row[own] = n_next + np.arange(len(own))
        row[np.nonzero(r >= 0.9)[0]] = seen[r >= 0.9]
        n_next += len(own)
        pos.append(world[seen[own]]); normal.append(normal[0][seen[own]]); mx.append(mx[0][seen[own]]); desc.append(wdesc[seen[own]])
        kfs.append(S.KeyFrame(S.keypoints(np.float32(xy), octs), ds, *S.pose_t([0, 0, 0]), row.tolist()))
    mx = np.concatenate(mx)
    m = F.SafMap(kfs, list(range(nk)), poses, list(range(npts)), np.concatenate(pos), np.concatenate(normal), mx / float(S.SF[S.NLEVELS - 1]), mx,
                 np.concatenate(desc), sim3=sim3)
    m.bad[rng.choice(npts, npts // 50, replace=False)] = True                      # loop points that are bad at the call
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="30x3000x1000,30x3000x2000,100x8000x1000,100x8000x2000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401
    import search_and_fuse_scene as F
    import search_in_neighbors_scene as S
    from rumi_slam_amd import capi, mapping
    from rumi_slam_amd.matcher import ORBmatcher
    L = mapping._lib()
    for shape in a.shapes.split(","):
        nk, npts, nf = (int(x) for x in shape.split("x"))
        m = build_map(nk, npts, nf, 7000 + nf + nk)
        sc = F.StoreScene(m)
        matcher = ORBmatcher(0.8, True, max_features=max(2048, nf), max_queries=max(16384, npts))
        ids = np.arange(npts)
        Kf = np.ascontiguousarray(S.K4, np.float32)

        # ---- the old path, marshalled: per key-frame the loop points with that key-frame's skip mask
        old_args = []
        for k in range(nk):
            skip = m.bad[:npts].copy()
            row = np.asarray(m.kfs[k].row)
            skip[row[(row >= 0) & (row < npts)]] = True
            old_args.append([np.ascontiguousarray(x) for x in (skip.astype(np.uint8), m.pos[ids], m.normal[ids], m.min_dist[ids], m.max_dist[ids], m.desc[ids])])
        old_best = np.full((nk, npts), -1, np.int32)
        T7s = [np.ascontiguousarray(m.poses[k][0], np.float32) for k in range(nk)]
        Ows = [np.ascontiguousarray(m.poses[k][1], np.float32) for k in range(nk)]

        def old():
            for k in range(nk):
                capi.check(L.rumi_fuse_candidates(matcher._h, C.byref(sc.frames[k].c), float(S.LOG_SF), capi.ptr(T7s[k]), capi.ptr(Ows[k]), capi.ptr(Kf), npts,
                                                  *[capi.ptr(x) for x in old_args[k]], float(F.TH), 0, capi.ptr(old_best[k])))

        # ---- the new call, marshalled
        slots = np.asarray([S.slot_of(k) for k in range(nk)], np.int32)
        arr = (mapping.RumiFuseKF * nk)(*[sc.fuse_kf(k) for k in range(nk)])
        ids32 = np.ascontiguousarray(ids, np.int32)
        cap = min(nk * npts, 2 * nk * nf)
        hits, per, n_hits = np.zeros(cap, mapping.FUSE_HIT_DTYPE), np.zeros(nk, np.int32), C.c_int32()

        def new():
            capi.check(L.rumi_search_and_fuse_resident(matcher._h, sc.store._h, capi.ptr(slots), C.byref(arr), nk, capi.ptr(ids32), npts, float(F.TH),
                                                       capi.ptr(hits), cap, C.byref(n_hits), capi.ptr(per)))

        old(); new()
        h = hits[:n_hits.value]
        dense = np.full((nk, npts), -1, np.int32)
        dense[h["kf"], h["point"]] = h["feature"]
        rows = np.stack([np.asarray(kf.row) for kf in m.kfs])
        equal = bool(dense.tobytes() == old_best.tobytes() and (per == (old_best >= 0).sum(1)).all()
                     and (h["occupant"] == rows[h["kf"], h["feature"]]).all())
        for _ in range(3):
            old(); new()
        rounds = {"per_key_frame": [], "one_call": []}
        stage = []
        for _ in range(a.rounds):
            t = {"per_key_frame": [], "one_call": []}
            for _ in range(a.reps):
                for name, fn in (("per_key_frame", old), ("one_call", new)):
                    t0 = time.perf_counter()
                    fn()
                    t[name].append((time.perf_counter() - t0) * 1e3)
                stage.append(mapping.search_and_fuse_stage_ms(matcher))
            for k in t:
                rounds[k].append(round(float(np.median(t[k])), 4))
        old_ms, new_ms = float(np.median(rounds["per_key_frame"])), float(np.median(rounds["one_call"]))
        st = np.median(np.stack(stage), 0)
        line = {"key_frames": nk, "loop_points": npts, "features": nf, "pairs": nk * npts, "hits": int(n_hits.value),
                "hits_with_occupant": int(np.count_nonzero(h["occupant"] >= 0)), "equal_to_per_key_frame": equal,
                "bytes_back": 4 * (16 + ((nk + 3) & ~3)) + 16 * int(n_hits.value), "bytes_back_dense": 4 * nk * npts,
                "bytes_up_per_call": 112 * nk + 4 * npts, "bytes_up_per_key_frame_loop": nk * (73 * npts + 60 * nf),
                "reps": a.reps, "rounds": a.rounds, "per_key_frame": {"round_median_ms": rounds["per_key_frame"], "ms": round(old_ms, 4)},
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
