"""Times Tracking::UpdateLocalMap + TrackLocalMap per frame, two ways, in the same process and alternating:
  (a) two_calls     Covisibility.local_map -> the point table gathered on the host from flat numpy arrays indexed by point id (no MapPoint
                    objects, no mutex: a FASTER baseline than the reference's walk) -> Tracker.local, which uploads the table
  (b) one_call      Tracker.local_map (rumi_track_local_map): the table is built on the device from the store's attribute records;
                    with 0 and with 50 attribute edits (rumi_covis_set_point_attributes) staged before every frame
The map is tests/covis_scene.py's probe_world (300 key-frames x 1000 features, a frame with 400 matched points) joined with a point table: every
point lies on the plane of the synthetic frame behind one of its key-points and carries that key-point's descriptor with a few bits flipped, so
the local search has real candidates.  Both ways are checked to give the same frame vector and the same pose bytes before anything is timed.
Warm-up, then `reps` rounds of (a), (b0), (b50) in turn; median, minimum and the 10th..90th percentile of each are reported, (a) also split into
its three parts, (b) with rumi_covis_stage_ms of the store's half.
    python tools/local_map_probe.py [--reps 300] [--out profiles/local_map_probe.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def stats(t):
    t = np.asarray(t) * 1e3
    return dict(median_ms=round(float(np.median(t)), 4), min_ms=round(float(t.min()), 4), p10_ms=round(float(np.percentile(t, 10)), 4),
                p90_ms=round(float(np.percentile(t, 90)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401
    from covis_scene import probe_world
    from rumi_slam_amd.synth import synth_frame
    from rumi_slam_amd.tracker import Tracker
    from scene import K_TUM3
    from test_tracking_loop_gpu import PLANE_D
    w, frame = probe_world()
    cov = w.handle()
    npts = w.max_points
    trk = Tracker(1000, 1.2, 8, 20, 7, 640, 480, 16384)
    _, keys, desc = trk.extract(synth_frame(4242))
    n = len(keys)
    # ---- the point table by id: behind key-point p % n, its descriptor with up to three bits flipped
    rng = np.random.default_rng(0)
    fx, fy, cx, cy = K_TUM3.astype(np.float64)
    src = np.arange(npts) % n
    jitter = rng.normal(0, 0.3, (npts, 2))
    pos = np.stack([(keys["x"][src] + jitter[:, 0] - cx) / fx * PLANE_D, (keys["y"][src] + jitter[:, 1] - cy) / fy * PLANE_D, np.full(npts, PLANE_D)], 1).astype(np.float32)
    dist = np.linalg.norm(pos, axis=1).astype(np.float32)
    sf = np.float32(1.2) ** np.arange(8, dtype=np.float32)
    lvl = keys["octave"][src]
    attr = dict(pos=pos, normal=(pos / dist[:, None]).astype(np.float32), max_dist=(dist * sf[lvl]).astype(np.float32),
                min_dist=(dist * sf[lvl] / sf[7]).astype(np.float32), desc=desc[src].copy())
    flip = rng.integers(0, 256, (npts, 3))
    for j in range(3):
        attr["desc"][np.arange(npts), flip[:, j] // 8] ^= (1 << (flip[:, j] % 8)).astype(np.uint8)
    bad_id = np.zeros(npts, np.uint8)
    obs_id = np.zeros(npts, np.int32)
    for p, d in w.pt.items():
        bad_id[p], obs_id[p] = d["bad"], len(d["obs"])
    ids_all = np.arange(npts, dtype=np.int32)
    cov.set_point_attributes(ids_all, attr["pos"], attr["normal"], attr["min_dist"], attr["max_dist"], attr["desc"])
    fp = np.full(n, -1, np.int32)
    fp[:len(frame)] = frame
    T = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    row_of = np.full(npts, -1, np.int32)
    parts = {"local_map": [], "host_gather": [], "track_local": []}

    def two_calls(record=True):
        t0 = time.perf_counter()
        lm = cov.local_map(fp)
        t1 = time.perf_counter()
        local = lm["local_points"]
        row_of[local] = np.arange(len(local), dtype=np.int32)
        held = fp[fp >= 0]
        held = held[bad_id[held] == 0]
        extra = held[row_of[held] < 0]
        _, first = np.unique(extra, return_index=True)
        extra = extra[np.sort(first)]
        table = np.concatenate([local, extra])
        row_of[extra] = len(local) + np.arange(len(extra), dtype=np.int32)
        fin = np.where((fp >= 0) & (bad_id[np.maximum(fp, 0)] == 0), row_of[np.maximum(fp, 0)], -1).astype(np.int32)
        local_flag = np.zeros(len(table), np.uint8)
        local_flag[:len(local)] = 1
        points = dict(pos=attr["pos"][table], normal=attr["normal"][table], min_dist=attr["min_dist"][table], max_dist=attr["max_dist"][table],
                      desc=attr["desc"][table], obs=obs_id[table], bad=bad_id[table], local=local_flag)
        row_of[table] = -1
        t2 = time.perf_counter()
        r = trk.local(K_TUM3, T, fin, points, None, 1.0)
        t3 = time.perf_counter()
        if record:
            parts["local_map"].append(t1 - t0); parts["host_gather"].append(t2 - t1); parts["track_local"].append(t3 - t2)
        return table, r, t3 - t0

    edit_ids = np.ascontiguousarray(rng.choice(npts, 50, replace=False), np.int32)
    edit = [np.ascontiguousarray(attr[k][edit_ids]) for k in ("pos", "normal", "min_dist", "max_dist", "desc")]
    cov_ms = {0: [], 50: []}
    up = {}

    def one_call(n_edits, record=True):
        t0 = time.perf_counter()
        if n_edits:
            cov.set_point_attributes(edit_ids, *edit)
        r = trk.local_map(cov, K_TUM3, T, fp, table_cap=16384)
        dt = time.perf_counter() - t0
        if record:
            cov_ms[n_edits].append(cov.stage_ms())
            up[n_edits] = cov.stats()["last_upload_bytes"]
        return r, dt

    # ---- the same answer, then warm-up
    table, ra, _ = two_calls(False)
    rb, _ = one_call(0, False)
    ids = np.where(ra["frame_mp"] >= 0, table[np.maximum(ra["frame_mp"], 0)], -1)
    assert np.array_equal(rb["table_ids"], table) and np.array_equal(rb["frame_mp"], ids) and rb["Tcw"].tobytes() == ra["Tcw"].tobytes()
    assert np.array_equal(rb["in_view"], ra["in_view"]) and rb["matches_inliers"] == ra["matches_inliers"]
    for _ in range(20):
        two_calls(False); one_call(0, False); one_call(50, False)
    ta, tb0, tb50 = [], [], []
    for _ in range(a.reps):
        ta.append(two_calls()[2]); tb0.append(one_call(0)[1]); tb50.append(one_call(50)[1])
    shape = dict(key_frames=w.n_live(), points=len(w.pt), frame_features=n, frame_points=int((fp >= 0).sum()), local_points=int(len(rb["local_points"])),
                 table_rows=int(len(table)), in_view=int((rb["in_view"] == 1).sum()), nmatches_local=rb["nmatches_local"], matches_inliers=rb["matches_inliers"], reps=a.reps)
    lines = [json.dumps(dict(workload="two_calls", **shape, **stats(ta), parts={k: stats(v) for k, v in parts.items()},
                             table_upload_bytes=int(len(table)) * (12 + 12 + 4 + 4 + 32 + 4 + 1 + 1)))]
    for k, t in ((0, tb0), (50, tb50)):
        g, d, wr = np.median(np.array(cov_ms[k]), axis=0)
        lines.append(json.dumps(dict(workload=f"one_call_{k}_edits", **shape, **stats(t), store_upload_bytes=up[k],
                                     store_validate_stage_ms=round(float(g), 4), store_upload_kernels_read_ms=round(float(d), 4),
                                     speedup_vs_two_calls=round(float(np.median(ta) / np.median(t)), 3))))
    for l in lines:
        print(l, flush=True)
    cov.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
