"""Times the covisibility store (include/rumi_covis.h) against the scalar loops of tests/cpp/covis_oracle.cc (g++ -O2) on one core, in the
same process.  The flat-array loops are a FASTER baseline than the reference's members, which copy a std::map per point.  One resident map
(tests/covis_scene.py, probe_world): 300 key-frames x 1000 features, 4..15 observers a point, a frame with 400 matched points.
  local_map            no edits between calls
  local_map_edits      50 point edits and 1 key-frame edit staged before every call (the per-frame steady state); the edits re-send the
                       objects as they are, so the answer stays the oracle's while the staging and the upload are those of real edits
  connections_B1/B480  update_connections for one key-frame and for a welding window of 40 x 6 x 2
The C entries are timed with their arguments already marshalled; warm-up, then the median of repeated calls, each split by
rumi_covis_stage_ms into validate + stage | upload + kernels + download | write-out.  The outputs are asserted equal to the oracle's before
a time is reported.
    python tools/covis_probe.py [--reps 30] [--out FILE]"""
import argparse
import ctypes as C
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
    return round(float(np.median(t)), 4), round(float(np.min(t)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401
    from covis_scene import _ptr, build_oracle, differing, oracle_connections, oracle_local_map, probe_world
    from rumi_slam_amd import capi
    from rumi_slam_amd.covis import Covisibility, _csr
    orc = build_oracle(tempfile.mkdtemp())
    w, frame = probe_world()
    flat = w.flat()
    h = w.handle()
    L = h._lib
    n_live = w.n_live()
    lines = []

    def report(name, device_call, oracle_call, extra, after=None):
        res = {"workload": name, "key_frames": n_live, "points": len(w.pt), "observations": int(len(flat["obs"])), "equal_to_oracle": True}
        res.update(extra)
        res["device_call_ms"], res["device_call_min_ms"] = median_ms(device_call, a.reps)
        stages = []
        for _ in range(a.reps):
            device_call()
            stages.append(h.stage_ms())
        g, d, wr = np.median(np.array(stages), axis=0)
        res["validate_stage_ms"], res["upload_kernels_download_ms"], res["write_out_ms"] = round(float(g), 4), round(float(d), 4), round(float(wr), 4)
        res["upload_bytes"] = h.stats()["last_upload_bytes"]
        res["oracle_loop_ms"], res["oracle_loop_min_ms"] = median_ms(oracle_call, a.reps, 2)
        res["speedup_vs_oracle_loop"] = round(res["oracle_loop_ms"] / res["device_call_ms"], 3)
        if after:
            res.update(after())
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

    # ---- (a) local_map
    fp = np.ascontiguousarray(frame, np.int32)
    out = Covisibility.local_map_outputs(len(fp), w.max_kf, w.max_points)
    lm_args = (h._h, len(fp), _ptr(fp), _ptr(out["frame_point_bad"]), _ptr(out["local_kf"]), w.max_kf, _ptr(out["n_k1"]), _ptr(out["n_local_kf"]),
               _ptr(out["ref_kf"]), _ptr(out["local_points"]), w.max_points, _ptr(out["n_local_points"]))
    want = oracle_local_map(orc, w, frame, flat)

    def lm_equal():
        got = dict(frame_point_bad=out["frame_point_bad"][:len(fp)], local_kf=out["local_kf"][:int(out["n_local_kf"][0])], n_k1=int(out["n_k1"][0]),
                   ref_kf=int(out["ref_kf"][0]), local_points=out["local_points"][:int(out["n_local_points"][0])])
        assert differing(got, want) == [], differing(got, want)

    o_bad, o_kf, o_pt = np.zeros(len(fp), np.uint8), np.zeros(w.max_kf, np.int32), np.zeros(w.max_points, np.int32)
    o_s = [np.zeros(1, np.int32) for _ in range(4)]
    lm_oracle_args = (w.max_kf, _ptr(flat["key"]), _ptr(flat["kf_bad"]), _ptr(flat["mp_off"]), _ptr(flat["mp"]), _ptr(flat["best"]), _ptr(flat["parent"]),
                      _ptr(flat["child_off"]), _ptr(flat["children"]), w.max_points, _ptr(flat["pt_bad"]), _ptr(flat["obs_off"]), _ptr(flat["obs"]),
                      len(fp), _ptr(fp), _ptr(o_bad), _ptr(o_kf), _ptr(o_s[0]), _ptr(o_s[1]), _ptr(o_s[2]), _ptr(o_pt), _ptr(o_s[3]))

    def lm_device():
        capi.check(L.rumi_covis_local_map(*lm_args))

    def lm_oracle():
        orc.cvo_local_map(*lm_oracle_args)
    lm_device()
    lm_equal()
    shape = {"frame_points": int((fp >= 0).sum()), "k1": want["n_k1"], "local_key_frames": int(len(want["local_kf"])), "local_points": int(len(want["local_points"]))}
    report("local_map", lm_device, lm_oracle, shape)

    rng = np.random.default_rng(1)
    ids = np.ascontiguousarray(rng.choice(sorted(w.pt), 50, replace=False), np.int32)
    p_bad = np.array([w.pt[int(p)]["bad"] for p in ids], np.uint8)
    p_off, p_obs = _csr([w.pt[int(p)]["obs"] for p in ids])
    s = int(rng.choice(sorted(w.kf)))
    d = w.kf[s]
    k_slot, k_key, k_map, k_bad = np.array([s], np.int32), np.array([d["key"]], np.uint64), np.array([d["map"]], np.int32), np.array([d["bad"]], np.uint8)
    k_mo, k_mp = _csr([d["mp"]]); k_co, k_ch = _csr([d["children"]])
    k_best = np.full(10, -1, np.int32); k_best[:len(d["best"])] = d["best"]
    k_par = np.array([d["parent"]], np.int32)
    edit_ms = []

    def lm_device_edits():
        t0 = time.perf_counter()
        capi.check(L.rumi_covis_set_points(h._h, 50, _ptr(ids), _ptr(p_bad), _ptr(p_off), _ptr(p_obs)))
        capi.check(L.rumi_covis_set_keyframes(h._h, 1, _ptr(k_slot), _ptr(k_key), _ptr(k_map), _ptr(k_bad), _ptr(k_mo), _ptr(k_mp), _ptr(k_best), _ptr(k_par),
                                              _ptr(k_co), _ptr(k_ch)))
        edit_ms.append((time.perf_counter() - t0) * 1e3)
        capi.check(L.rumi_covis_local_map(*lm_args))
    lm_device_edits()
    lm_equal()
    report("local_map_edits", lm_device_edits, lm_oracle, dict(shape, point_edits=50, key_frame_edits=1),
           after=lambda: {"edit_calls_ms": round(float(np.median(edit_ms)), 4)})      # the share of device_call_ms spent in the two set_ calls

    # ---- (b) update_connections
    for B in (1, 480):
        batch = np.ascontiguousarray(np.random.default_rng(B).choice(sorted(w.kf), B, replace=B > n_live), np.int32)
        cap = B * n_live
        o = Covisibility.connection_outputs(B, cap, cap)
        uc_args = (h._h, B, _ptr(batch), _ptr(o["status"]), _ptr(o["conn_off"]), _ptr(o["conn_slot"]), _ptr(o["conn_count"]), cap, _ptr(o["ord_off"]),
                   _ptr(o["ord_slot"]), _ptr(o["ord_weight"]), cap)
        r = Covisibility.connection_outputs(B, cap, cap)
        uc_oracle_args = (_ptr(flat["key"]), _ptr(flat["map"]), _ptr(flat["kf_bad"]), _ptr(flat["mp_off"]), _ptr(flat["mp"]), _ptr(flat["pt_bad"]),
                          _ptr(flat["obs_off"]), _ptr(flat["obs"]), B, _ptr(batch), _ptr(r["status"]), _ptr(r["conn_off"]), _ptr(r["conn_slot"]),
                          _ptr(r["conn_count"]), _ptr(r["ord_off"]), _ptr(r["ord_slot"]), _ptr(r["ord_weight"]))

        def uc_device():
            capi.check(L.rumi_covis_update_connections(*uc_args))

        def uc_oracle():
            orc.cvo_update_connections(*uc_oracle_args)
        uc_device()
        uc_oracle()
        nc, no = int(r["conn_off"][B]), int(r["ord_off"][B])
        assert differing({k: (v[:nc] if k.startswith("conn_s") or k == "conn_count" else v[:no] if k in ("ord_slot", "ord_weight") else v) for k, v in o.items()},
                         {k: (v[:nc] if k.startswith("conn_s") or k == "conn_count" else v[:no] if k in ("ord_slot", "ord_weight") else v) for k, v in r.items()}) == []
        report(f"connections_B{B}", uc_device, uc_oracle, {"batch": B, "connections": nc, "ordered": no})
    h.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
