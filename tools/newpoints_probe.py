"""Times rumi_create_new_map_points (include/rumi_mapping.h) against the path a user had before it, in one process and on one scene: one
rumi_search_for_triangulation call per neighbour (with the flags the reference's loop reaches) and the scalar triangulation loop on the host
(tests/cpp/newpoints_oracle.cc).  30 neighbours x 1000 and x 2000 features; warm-up, then the median of repeated calls.  The C entries are
timed with their arguments already marshalled, so neither side is charged for Python.
    python tools/newpoints_probe.py [--features 1000,2000] [--reps 30] [--only new] [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", default="1000,2000")
    ap.add_argument("--neighbours", type=int, default=30)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", default="", help="'new': time the new call alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
