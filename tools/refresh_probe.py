"""Times rumi_refresh_map_points (include/rumi_mapping.h) against the path a user had before it: the scalar per-point loop of
MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (tests/cpp/refresh_oracle.cc, g++ -O2) on one core, in the same process.
Three workloads: (a) SearchInNeighbors-shaped, 1000 points of 2..30 observations, both modes; (b) the same with a long-session tail, 5 % of
the points with 100..400 observations; (c) post-BA-shaped, 3000 points of about 10 observations, normal and depth only.  The C entries are
timed with their arguments already marshalled; warm-up, then the median of repeated calls.  The outputs are asserted equal to the oracle's
before a time is reported.
    python tools/refresh_probe.py [--reps 30] [--only device] [--out FILE]
--resident: the same three workloads through rumi_refresh_map_points_resident over a covisibility store that holds the map, against the block
entry in the same process with the same points: with nothing staged and with the edits a real step stages before its refresh (the observer
rows of the touched points and 25 camera centres, staged outside the timed call), as a query and with the write-back; the kernels the handle
launches itself (rumi_refresh_last_launches; the store's scatter of staged edits is not in that count); and what the write-back saves, the upload of the same points' attributes through rumi_covis_set_point_attributes (the resident
call with those edits staged minus the call with nothing staged).  Outputs are asserted equal to the block entry's before a time is printed.
    python tools/refresh_probe.py --resident [--reps 30] [--out profiles/refresh_resident_probe.jsonl]"""
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
    return [(desc[k], SF, Ow[k], bad[k]) for k in range(n_kf)], points, what, counts, octave


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


def resident_main(a):
    import refresh_resident_scene as rr
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import REFRESH_WRITE_BACK, MapPointRefresher, RefreshBatch, refresh_resident_outputs
    r = MapPointRefresher()
    lines = []
    for name in "abc":
        kfs, points, what, counts, octave = workload(name, 300 + ord(name))
        b = RefreshBatch(kfs, points)
        m = rr.ResidentMap(kfs, list(octave), [(p[0], p[1], p[4]) for p in points])
        store = m.store()
        ids = np.arange(m.n_pts, dtype=np.int32)
        blk, res = b.outputs(), refresh_resident_outputs(m.n_pts)
        args_blk = b.args(what, blk)
        attrs = m.initial_attributes(ids)
        centres = list(range(0, m.n_kf, max(1, m.n_kf // 25)))[:25]

        def block_call():
            capi.check(r._lib.rumi_refresh_map_points(r._h, *args_blk))

        def resident_call(flags):
            capi.check(r.status_resident(store, ids, what, flags, res))

        def stage_step():
            m.set_points(store, ids, attributes=False, references=False)
            m.set_centres(store, centres)

        def stage_attributes():
            store.set_point_attributes(ids, attrs["pos"], attrs["normal"], attrs["min_dist"], attrs["max_dist"], attrs["desc"])

        def timed(flags, stage, reps, warm=5):
            t, st = [], []
            for i in range(warm + reps):
                if stage:
                    stage()
                t0 = time.perf_counter()
                resident_call(flags)
                if i >= warm:
                    t.append((time.perf_counter() - t0) * 1e3)
                    st.append(r.stage_ms())
            return float(np.median(t)), [round(float(x), 4) for x in np.median(np.array(st), axis=0)]

        block_call()
        for flags in (0, REFRESH_WRITE_BACK):
            resident_call(flags)
            keys = (["best_obs", "best_median"] if what & 1 else []) + (["normal", "min_distance", "max_distance", "updated"] if what & 2 else [])
            diff = [k for k in keys if res[k].tobytes() != blk[k].tobytes()]
            assert diff == [], (name, flags, diff)
        out = {"workload": name, "points": m.n_pts, "observations": int(b.n_obs), "max_observations": int(counts.max()), "what": what,
               "equal_to_block_entry": True}
        out["block_call_ms"] = round(median_ms(block_call, a.reps)[0], 4)
        stages = []
        for _ in range(a.reps):
            block_call()
            stages.append(r.stage_ms())
        out["block_stages_ms"] = [round(float(x), 4) for x in np.median(np.array(stages), axis=0)]
        for label, flags, stage in (("query_nothing_staged", 0, None), ("write_back_nothing_staged", REFRESH_WRITE_BACK, None),
                                    ("query_step_staged", 0, stage_step), ("write_back_step_staged", REFRESH_WRITE_BACK, stage_step),
                                    ("query_attributes_staged", 0, stage_attributes)):
            ms, st = timed(flags, stage, a.reps)
            out[label + "_ms"], out[label + "_stages_ms"] = round(ms, 4), st
            out[label + "_launches"] = r.last_launches()      # the handle's own kernels; what the store launches for its staged edits shows in a kernel trace
            out[label + "_upload_bytes"] = store.stats()["last_upload_bytes"]
        out["attribute_upload_ms"] = round(out["query_attributes_staged_ms"] - out["query_nothing_staged_ms"], 4)
        out["block_plus_attribute_upload_ms"] = round(out["block_call_ms"] + out["attribute_upload_ms"], 4)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        store.close()
    r.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", default="", help="'device': time the device call alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--resident", action="store_true", help="time rumi_refresh_map_points_resident against the block entry")
    a = ap.parse_args()
    import torch  # noqa: F401
    if a.resident:
        return resident_main(a)
    from refresh_scene import build_oracle, run_oracle, same_bytes
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import MapPointRefresher, RefreshBatch
    orc = build_oracle(tempfile.mkdtemp())
    r = MapPointRefresher()
    lines = []
    for name in "abc":
        kfs, points, what, counts, _ = workload(name, 300 + ord(name))
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
