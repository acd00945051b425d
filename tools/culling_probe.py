"""Times rumi_keyframe_culling (include/rumi_mapping.h) against the scalar loop of LocalMapping::KeyFrameCulling on flat arrays
(tests/cpp/culling_oracle.cc, g++ -O2) on one core, in the same process.  The flat-array loop is a FASTER baseline than the reference's
member, which copies a std::map per point.  Two workloads (tests/culling_scene.py, probe_batch): (a) 30 candidates x 1000 features, 4..15
observations a point; (b) 100 candidates x 2000 features, 4..40 observations, a handful of culls.  The C entries are timed with their
arguments already marshalled; warm-up, then the median of repeated calls.  The outputs are asserted equal to the oracle's before a time is
reported.
--resident times rumi_keyframe_culling_resident on the same two maps, loaded once into a covisibility store (tests/culling_resident_scene.py),
next to the block entry in the same process: on a steady state with nothing staged, and with the edits of one culled key-frame (its record,
its row, the observer rows of its points) staged before every call.  Each line carries the three-way split of both entries.
    python tools/culling_probe.py [--reps 30] [--only device] [--resident] [--workloads ab] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

WORKLOADS = {"a": (30, 1000, (4, 15), 0), "b": (100, 2000, (4, 40), 1)}


def median_ms(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def walk_stats(b):
    """The first pass's observation walks, counted on the host: over every candidate slot whose point is walked (not bad, Observations() > 3),
    the mean number of entries read before the fourth qualifying observer (or the end of the list), the mean list length, and the share of
    walks that run to the end."""
    octave, mp = b._keep[0::2], b._keep[1::2]
    okf, ofe = b.obs_kf.tolist(), b.obs_feature.tolist()
    octl = [o.tolist() for o in octave]
    steps = lists = full = walks = 0
    for k in b.cand[:b.n_cand].tolist():
        for i, p in enumerate(mp[k].tolist()):
            if p < 0 or b.pts["is_bad"][p] or b.pts["n_obs_count"][p] <= 3:
                continue
            lo, hi = int(b.pts["obs_begin"][p]), int(b.pts["obs_end"][p])
            n, o = 0, lo
            while o < hi:
                kk = okf[o]
                o += 1
                if kk != k and octl[kk][ofe[o - 1]] <= octl[k][i] + 1:
                    n += 1
                    if n > 3:
                        break
            walks += 1
            steps += o - lo
            lists += hi - lo
            full += n <= 3
    return {"walks": walks, "mean_walk": round(steps / max(walks, 1), 2), "mean_list": round(lists / max(walks, 1), 2),
            "walks_to_the_end": round(full / max(walks, 1), 3)}


def resident_times(r, b, block_out, reps):
    """The resident entry on the map of batch ``b``: outputs equal to the block entry's (already equal to the oracle's), then the medians."""
    import culling_resident_scene as rs
    from culling_scene import same_bytes
    from rumi_slam_amd import capi
    from rumi_slam_amd.covis import Covisibility
    from rumi_slam_amd.mapping import CULL_CULLED, cull_candidates, cull_outputs
    m = rs.MapMirror.from_batch(b)
    store = Covisibility(m.n_kf, m.n_pts + 8)
    t0 = time.perf_counter()
    m.load(store)
    load_ms = (time.perf_counter() - t0) * 1e3
    cand = b.cand[:b.n_cand].tolist()
    rec = cull_candidates(m.candidates(cand))
    out = cull_outputs(len(rec))
    args = (r._h, store._h, capi.ptr(rec), len(rec), 0, capi.ptr(out["status"]), capi.ptr(out["n_mps"]), capi.ptr(out["n_redundant"]),
            capi.ptr(out["culled"]), capi.ptr(out["n_culled"]))

    def resident_call():
        capi.check(r._lib.rumi_keyframe_culling_resident(*args))
    resident_call()
    first_upload = store.stats()["last_upload_bytes"] + store.feature_stats()["last_upload_bytes"]
    assert same_bytes(out, block_out) == [], same_bytes(out, block_out)

    def split(call, before=lambda: None):
        total, stages = [], []
        for i in range(reps + 5):
            before()
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= 5:
                total.append(dt)
                stages.append(r.stage_ms())
        return [round(float(x), 4) for x in (np.median(total), np.min(total), *np.median(np.array(stages), axis=0))]

    res = {"resident_equal_to_block": True, "store_load_ms": round(load_ms, 2), "first_upload_bytes": int(first_upload)}
    res["resident_steady_ms"], res["resident_steady_min_ms"], *res["resident_steady_split_ms"] = split(resident_call)
    res["resident_steady_upload_bytes"] = store.stats()["last_upload_bytes"]
    # what SetBadFlag() of one culled key-frame touches, staged again with the values the map holds: the same bytes travel, the state stays
    hit = np.nonzero(out["status"][:len(cand)] == CULL_CULLED)[0]
    k = cand[int(hit[0]) if len(hit) else 0]
    pts = sorted({int(p) for p in m.mp[k] if p >= 0})
    stage_ms = []

    def stage():
        t0 = time.perf_counter()
        m.set_keyframes(store, [k])
        m.set_points(store, pts)
        stage_ms.append((time.perf_counter() - t0) * 1e3)
    res["resident_staged_ms"], res["resident_staged_min_ms"], *res["resident_staged_split_ms"] = split(resident_call, stage)
    res["resident_staged_upload_bytes"] = store.stats()["last_upload_bytes"]
    res["staged_points"], res["staging_python_ms"] = len(pts), round(float(np.median(stage_ms)), 4)
    assert same_bytes(out, block_out) == []
    block_args = b.args(0, block_out)

    def block_call():
        capi.check(r._lib.rumi_keyframe_culling(r._h, *block_args))
    res["block_again_ms"], res["block_again_min_ms"], *res["block_again_split_ms"] = split(block_call)
    store.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", default="", help="'device': time the device call alone (for a kernel trace)")
    ap.add_argument("--resident", action="store_true", help="also time rumi_keyframe_culling_resident on the same maps")
    ap.add_argument("--workloads", default="ab")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401
    from culling_scene import build_oracle, probe_batch, same_bytes
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import CULL_CULLED, KeyFrameCuller
    orc = build_oracle(tempfile.mkdtemp())
    r = KeyFrameCuller()
    lines = []
    for name, (n_cand, n_feat, obs_range, seed) in WORKLOADS.items():
        if name not in a.workloads:
            continue
        b = probe_batch(n_cand, n_feat, obs_range, seed)
        out, ref = b.outputs(), b.outputs()
        args_dev, args_ref = b.args(0, out), b.args(0, ref) + (None,) * 6

        def device_call():
            capi.check(r._lib.rumi_keyframe_culling(r._h, *args_dev))

        def oracle_loop():
            orc.cuo_keyframe_culling(*args_ref)
        device_call()
        oracle_loop()
        assert same_bytes(out, ref) == [], same_bytes(out, ref)
        res = {"workload": name, "candidates": b.n_cand, "key_frames": b.n_kf, "features": n_feat, "points": b.n_pts, "observations": int(b.n_obs),
               "culled": int(out["n_culled"][0]), "equal_to_oracle": True}
        res.update(walk_stats(b))
        assert res["culled"] == int((out["status"][:b.n_cand] == CULL_CULLED).sum())
        res["device_call_ms"], res["device_call_min_ms"] = [round(x, 4) for x in median_ms(device_call, a.reps)]
        stages = []
        for _ in range(a.reps):
            device_call()
            stages.append(r.stage_ms())
        g, d, w = np.median(np.array(stages), axis=0)
        res["host_validate_pack_ms"], res["upload_kernels_download_ms"], res["write_out_ms"] = round(float(g), 4), round(float(d), 4), round(float(w), 4)
        if a.only != "device":
            res["oracle_loop_ms"], res["oracle_loop_min_ms"] = [round(x, 4) for x in median_ms(oracle_loop, a.reps, 2)]
            res["speedup_vs_oracle_loop"] = round(res["oracle_loop_ms"] / res["device_call_ms"], 2)
        if a.resident:
            res.update(resident_times(r, b, out, a.reps))
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    r.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
