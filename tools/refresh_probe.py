"""Times rumi_refresh_map_points (include/rumi_mapping.h) against the path a user had before it: the scalar per-point loop of
MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (tests/cpp/refresh_oracle.cc, g++ -O2) on one core, in the same process.
Three workloads: (a) SearchInNeighbors-shaped, 1000 points of 2..30 observations, both modes; (b) the same with a long-session tail, 5 % of
the points with 100..400 observations; (c) post-BA-shaped, 3000 points of about 10 observations, normal and depth only.  The C entries are
timed with their arguments already marshalled; warm-up, then the median of repeated calls.  The outputs are asserted equal to the oracle's
before a time is reported.
    python tools/refresh_probe.py [--reps 30] [--only device] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def median_ms(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def workload(name, seed):
    """(key-frames, points, what) -- 200 key-frames of 1000 features (400 for the tail, so that a point can have 400 observers)."""
    from refresh_scene import SF, flip
    rng = np.random.default_rng(seed)
    n_kf = 420 if name == "b" else 200
    n_pts = 3000 if name == "c" else 1000
    counts = rng.integers(8, 13, n_pts) if name == "c" else rng.integers(2, 31, n_pts)
    if name == "b":
        tail = rng.choice(n_pts, n_pts // 20, replace=False)
        counts[tail] = rng.integers(100, 401, len(tail))
    nfeat = 1000
    desc = rng.integers(0, 256, (n_kf, nfeat, 32), dtype=np.uint8)
    octave = rng.integers(0, 8, (n_kf, nfeat))
    Ow = rng.uniform(-8, 8, (n_kf, 3)).astype(np.float32)
    bad = rng.random(n_kf) < 0.03
    rank = rng.permutation(n_kf)
    free = np.zeros(n_kf, np.int64)
    points = []
    for c in counts:
        kfs = sorted(rng.choice(n_kf, int(c), replace=False).tolist(), key=lambda k: rank[k])
        land = rng.integers(0, 256, 32, dtype=np.uint8)
        obs = []
        for k in kfs:
            f = int(free[k] % nfeat)
            free[k] += 1
            desc[k, f] = flip(rng, land, int(rng.integers(1, 40)))
            obs.append((k, f))
        ref_kf, ref_feature = obs[int(rng.integers(0, len(obs)))]
        points.append((rng.uniform(-5, 5, 3).astype(np.float32) + np.float32([0, 0, 8]), ref_kf, ref_feature, int(octave[ref_kf, ref_feature]), obs))
    what = 2 if name == "c" else 3
    return [(desc[k], SF, Ow[k], bad[k]) for k in range(n_kf)], points, what, counts


def occupancy(counts):
    """Share of busy lanes in the descriptor kernels' row loops: a group of G lanes runs max-N-of-its-wave rows with N lanes busy."""
    busy = total = 0
    for lo, hi, g in ((1, 16, 16), (17, 32, 32), (33, 64, 64)):
        c = [int(n) for n in counts if lo <= n <= hi]           # in list order, as the host bins them
        per = 64 // g
        for w in range(0, len(c), per):
            grp = c[w:w + per]
            busy += sum(n * max(grp) for n in grp)
            total += 64 * max(grp)
    for n in counts:
        if n > 64:
            cols = -(-int(n) // 64)
            busy += int(n) * int(n)
            total += int(n) * cols * 64
    return busy / total if total else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", default="", help="'device': time the device call alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401
    from refresh_scene import build_oracle, run_oracle, same_bytes
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import MapPointRefresher, RefreshBatch
    orc = build_oracle(tempfile.mkdtemp())
    r = MapPointRefresher()
    lines = []
    for name in "abc":
        kfs, points, what, counts = workload(name, 300 + ord(name))
        b = RefreshBatch(kfs, points)
        out, ref = b.outputs(), b.outputs()
        args_dev, args_ref = b.args(what, out), b.args(what, ref)

        def device_call():
            capi.check(r._lib.rumi_refresh_map_points(r._h, *args_dev))

        def oracle_loop():
            orc.rfo_refresh_map_points(*args_ref)
        device_call()
        oracle_loop()
        assert same_bytes(out, ref) == [], same_bytes(out, ref)
        good = [sum(not kfs[k][3] for k, _ in p[4]) for p in points]
        res = {"workload": name, "points": len(points), "observations": int(b.n_obs), "max_observations": int(counts.max()), "what": what,
               "equal_to_oracle": True}
        if what & 1:
            res["lane_occupancy"] = round(occupancy(good), 3)
        res["device_call_ms"], res["device_call_min_ms"] = [round(x, 4) for x in median_ms(device_call, a.reps)]
        stages = []
        for _ in range(a.reps):
            device_call()
            stages.append(r.stage_ms())
        g, d, w = np.median(np.array(stages), axis=0)
        res["host_gather_ms"], res["upload_kernels_download_ms"], res["write_out_ms"] = round(float(g), 4), round(float(d), 4), round(float(w), 4)
        if a.only != "device":
            res["oracle_loop_ms"], res["oracle_loop_min_ms"] = [round(x, 4) for x in median_ms(oracle_loop, max(5, a.reps // 3), 2)]
            res["speedup_vs_oracle_loop"] = round(res["oracle_loop_ms"] / res["device_call_ms"], 2)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    r.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
