"""Times rumi_create_new_map_points (include/rumi_mapping.h) against the path a user had before it, in one process and on one scene: one
rumi_search_for_triangulation call per neighbour (with the flags the reference's loop reaches) and the scalar triangulation loop on the host
(tests/cpp/newpoints_oracle.cc).  30 neighbours x 1000 and x 2000 features; warm-up, then the median of repeated calls.  The C entries are
timed with their arguments already marshalled, so neither side is charged for Python.
    python tools/newpoints_probe.py [--features 1000,2000] [--reps 30] [--only new] [--out FILE]
With --resident: the block entry against rumi_create_new_map_points_resident over a covisibility store filled from the same scene (see resident()).
    python tools/newpoints_probe.py --resident --out profiles/newpts_resident_probe.jsonl"""
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
    return float(np.median(t)), float(np.min(t))


def resident(a):
    """--resident: rumi_create_new_map_points (i) against rumi_create_new_map_points_resident with everything resident (ii), with one
    rumi_covis_set_keyframe_features of the current key-frame before it (iii: what a new key-frame costs), and (iii) with 600 point edits and
    600 attribute edits staged as well (iv).  The four are alternated call by call in one process; five rounds of `reps` calls each after a
    warm-up; every number is a median, every path's stage split comes from rumi_newpts_stage_ms, and all outputs are compared with the
    oracle's before a time is printed."""
    import torch  # noqa: F401
    from newpoints_scene import NewPointsScene, build_oracle, params, run_oracle
    from resident_scene import ResidentScene, slot_of, view_pose
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import NEWPOINT_DTYPE, _lib, pack, pack_poses
    from rumi_slam_amd.matcher import ORBmatcher
    orc = build_oracle(tempfile.mkdtemp())
    L = _lib()
    CL = capi.covis_lib()
    lines = []
    for nf in (int(x) for x in a.features.split(",")):
        s = NewPointsScene(100 + nf, a.neighbours, nf)
        nn, n1 = len(s.neigh), s.cur.frame.n
        prm = params(0, 0, 0, 0.0)
        want = run_oracle(orc, s.cur, s.neigh, prm)
        m = ORBmatcher(0.6, False)
        rs = ResidentScene(s)
        c, arr = pack(s.cur, s.neigh)
        cp, parr = pack_poses(view_pose(rs.views[0]), [view_pose(v) for v in rs.views[1:]])
        slots = np.int32([slot_of(k) for k in range(1, nn + 1)])
        out = np.zeros(n1, NEWPOINT_DTYPE)
        per, sk, n_out = np.zeros(nn, np.int32), np.zeros(nn, np.uint8), C.c_int32()
        ms3 = np.zeros(3, np.float32)
        # 600 edits that change nothing: points of the last neighbours, set again as they are
        ids = np.concatenate([r[r >= 0] for r in rs.rows[1:]])[-600:].astype(np.int32)
        owner = np.concatenate([np.full((r >= 0).sum(), slot_of(1 + k), np.int32) for k, r in enumerate(rs.rows[1:])])[-600:]
        pos = np.concatenate([v.mp_pos[v.kf_mp >= 0] for v in s.neigh])[-600:].astype(np.float32)
        zeros8, obs_off = np.zeros(600, np.uint8), np.arange(601, dtype=np.int32)
        nrm, mn, mx, dsc = np.tile(np.float32([0, 0, 1]), (600, 1)), np.full(600, 0.5, np.float32), np.full(600, 50.0, np.float32), np.full((600, 32), 0x5A, np.uint8)
        cur, curK = rs.views[0], np.ascontiguousarray(rs.views[0].K4, np.float32)

        def block():
            capi.check(L.rumi_create_new_map_points(m._h, C.byref(c), C.byref(arr), nn, C.byref(prm), capi.ptr(out), n1, C.byref(n_out), capi.ptr(per),
                                                    capi.ptr(sk)))

        def res():
            capi.check(L.rumi_create_new_map_points_resident(m._h, rs.store._h, slot_of(0), C.byref(cp), capi.ptr(slots), C.byref(parr), nn, C.byref(prm),
                                                             capi.ptr(out), n1, C.byref(n_out), capi.ptr(per), capi.ptr(sk)))

        def set_cur():
            capi.check(CL.rumi_covis_set_keyframe_features(rs.store._h, slot_of(0), C.byref(cur.frame.c), C.byref(cur.fv.c), capi.ptr(curK)))

        def edits():
            capi.check(CL.rumi_covis_set_points(rs.store._h, 600, capi.ptr(ids), capi.ptr(zeros8), capi.ptr(obs_off), capi.ptr(owner)))
            capi.check(CL.rumi_covis_set_point_attributes(rs.store._h, 600, capi.ptr(ids), capi.ptr(pos), capi.ptr(nrm), capi.ptr(mn), capi.ptr(mx),
                                                          capi.ptr(dsc)))

        paths = {"block": (None, block), "resident": (None, res), "set_cur_then_resident": (set_cur, res),
                 "set_cur_and_600_edits_then_resident": (lambda: (set_cur(), edits()), res)}

        def equal():
            return (n_out.value == len(want["points"]) and out[:n_out.value].tobytes() == want["points"].tobytes() and
                    np.array_equal(per, want["per_neigh"]) and np.array_equal(sk, want["skipped"]))

        def once(name, t):
            pre, call = paths[name]
            t0 = time.perf_counter()
            if pre:
                pre()
            t1 = time.perf_counter()
            call()
            t2 = time.perf_counter()
            capi.check(L.rumi_newpts_stage_ms(m._h, capi.ptr(ms3)))
            if t is not None:
                t.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3) + tuple(float(x) for x in ms3))

        ok = True
        for name in paths:                               # warm-up, and the outputs of every path against the oracle
            for _ in range(5):
                out[:] = 0
                once(name, None)
                ok = ok and equal()
        assert ok, "a path's output differs from the oracle's"
        rounds = {name: [] for name in paths}
        for _ in range(5):
            t = {name: [] for name in paths}
            for _ in range(a.reps):
                for name in paths:
                    once(name, t[name])
            for name in paths:
                rounds[name].append(np.median(np.array(t[name]), axis=0))
        res_line = {"neighbours": nn, "features": n1, "points": int(n_out.value), "equal_to_oracle": bool(ok and equal()), "reps": a.reps, "rounds": 5,
                    "feature_bytes_resident": rs.store.feature_stats()["used"]}
        for name in paths:
            r = np.array(rounds[name])                   # [round][total, before the call, host, upload + kernels + download, write-out]
            res_line[name] = {"round_median_ms": [round(float(x), 4) for x in r[:, 0]], "ms": round(float(np.median(r[:, 0])), 4),
                              "spread_ms": round(float(r[:, 0].max() - r[:, 0].min()), 4), "set_and_edit_calls_ms": round(float(np.median(r[:, 1])), 4),
                              "stage_host_ms": round(float(np.median(r[:, 2])), 4), "stage_device_ms": round(float(np.median(r[:, 3])), 4),
                              "stage_write_out_ms": round(float(np.median(r[:, 4])), 4)}
        b, g = np.array(rounds["block"])[:, 0], np.array(rounds["set_cur_then_resident"])[:, 0]
        gap = float(np.median(b) - np.median(g))
        res_line["gate"] = {"below_in_every_round": bool((g < b).all()), "gap_ms": round(gap, 4),
                            "larger_spread_ms": round(float(max(b.max() - b.min(), g.max() - g.min())), 4),
                            "passed": bool((g < b).all() and gap > max(b.max() - b.min(), g.max() - g.min()))}
        m.close()
        lines.append(json.dumps(res_line))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", default="1000,2000")
    ap.add_argument("--neighbours", type=int, default=30)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", default="", help="'new': time the new call alone (for a kernel trace)")
    ap.add_argument("--resident", action="store_true", help="the block entry against rumi_create_new_map_points_resident (appends to --out)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.resident:
        return resident(a)
    import torch  # noqa: F401
    import oracle_lib as O
    from newpoints_scene import RATIO_FACTOR, SF, NewPointsScene, build_oracle, params, run_oracle
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import NEWPOINT_DTYPE, _lib, pack
    from rumi_slam_amd.matcher import ORBmatcher
    orc = build_oracle(tempfile.mkdtemp())
    L = _lib()
    lines = []
    for nf in (int(x) for x in a.features.split(",")):
        s = NewPointsScene(100 + nf, a.neighbours, nf)
        nn, n1 = len(s.neigh), s.cur.frame.n
        prm = params(0, 0, 0, 0.0)
        want = run_oracle(orc, s.cur, s.neigh, prm)
        m = ORBmatcher(0.6, False)
        c, arr = pack(s.cur, s.neigh)
        out = np.zeros(n1, NEWPOINT_DTYPE)
        per, sk, n_out = np.zeros(nn, np.int32), np.zeros(nn, np.uint8), C.c_int32()

        def new_call():
            capi.check(L.rumi_create_new_map_points(m._h, C.byref(c), C.byref(arr), nn, C.byref(prm), capi.ptr(out), n1, C.byref(n_out), capi.ptr(per),
                                                    capi.ptr(sk)))
        new_call()
        equal = (n_out.value == len(want["points"]) and out[:n_out.value].tobytes() == want["points"].tobytes() and
                 np.array_equal(per, want["per_neigh"]) and np.array_equal(sk, want["skipped"]))
        res = {"neighbours": nn, "features": n1, "points": int(n_out.value), "equal_to_oracle": bool(equal)}
        res["new_call_ms"], res["new_call_min_ms"] = [round(x, 4) for x in median_ms(new_call, a.reps)]
        if a.only != "new":
            # the path of before: one blocking search per searched neighbour, flags as the loop leaves them
            flags = [np.ascontiguousarray(want["flags_before"][k]) for k in range(nn)]
            m12, nm = np.zeros(n1, np.int32), C.c_int32()
            live = [k for k in range(nn) if not want["skipped"][k]]

            def old_search():
                for k in live:
                    nb = s.neigh[k]
                    capi.check(m._lib.rumi_search_for_triangulation(m._h, C.byref(s.cur.frame.c), C.byref(s.cur.fv.c), capi.ptr(flags[k]), C.byref(nb.frame.c),
                                                                    C.byref(nb.fv.c), capi.ptr(nb.kf_mp), capi.ptr(nb.F12), capi.ptr(nb.epipole2), 0, 0, 0,
                                                                    capi.ptr(m12), C.byref(nm)))
            res["old_search_calls"] = len(live)
            res["old_search_ms"], res["old_search_min_ms"] = [round(x, 4) for x in median_ms(old_search, a.reps)]
            # the host side of before: the oracle's whole loop minus its own (CPU) searches = the scalar triangulation loop
            v0 = s.views[0]

            def cpu_search():
                for k in live:
                    v = s.views[1 + k]
                    O.search_for_triangulation(v0["keys"], v0["desc"], flags[k], v0["fv"], v["keys"], v["desc"], v["kf_mp"], v["fv"], SF, v["F12"], v["ep"], False, False, False)
            full, _ = median_ms(lambda: run_oracle(orc, s.cur, s.neigh, prm), max(5, a.reps // 3), 2)
            srch, _ = median_ms(cpu_search, max(5, a.reps // 3), 2)
            res["oracle_loop_ms"] = round(full, 4)
            res["oracle_search_part_ms"] = round(srch, 4)
            res["host_triangulation_loop_ms"] = round(max(full - srch, 0.0), 4)
            res["old_path_ms"] = round(res["old_search_ms"] + res["host_triangulation_loop_ms"], 4)
            res["speedup_vs_old_search_alone"] = round(res["old_search_ms"] / res["new_call_ms"], 2)
            res["speedup_vs_old_path"] = round(res["old_path_ms"] / res["new_call_ms"], 2)
        m.close()
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
