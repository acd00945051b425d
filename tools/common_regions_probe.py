#!/usr/bin/env python3
"""Measurements behind rumi_common_regions_bow, one JSON record per line on standard output and, with --out FILE, appended
to that file (the quoted copy lives in profiles/).

Workload: the BoW stage of DetectCommonRegionsFromBoW for one new key-frame -- 6 groups (3 loop + 3 merge candidates) x 11 members of 1000-feature
key-frames, about 40 distinct member key-frames (covisibles shared between candidates), FeatureVectors from a synthetic tree of ORBvoc.txt's geometry
(k = 10, L = 6, levelsup = 4), ORBmatcher(0.9, true).

  call     the new entry through the C ABI (arguments marshalled once, outside the clock)
  loop     what the parent commit does: 66 rumi_search_by_bow_kf calls through the C ABI, then the union of LoopClosing.cc:635-651 on the host
           (vectorised numpy, timed apart)
           --repeats calls a round, --rounds rounds, the two alternated call by call; medians per round and their spread
  stages   the new entry's own event times (rumi_common_regions_bow_profile): host pack, upload + clears, match kernel, finish + union kernels,
           copy back; taken in calls of their own, not in the timed rounds
  --trace  only runs both paths a few times (for a separate rocprofv3 --kernel-trace --stats pass; nothing is timed or written)

  --resident  rumi_common_regions_bow_resident against rumi_common_regions_bow in the same process: the workload above
           and 1 group x 1 member, both put into a covisibility store; the two entries alternate call by call (arguments marshalled once,
           outside the clock), medians of --repeats calls in each of --rounds rounds, the six arrays compared before a time counts.  Rows: the
           by-slot entry with matches12 = NULL (as the facade calls it), with matches12 copied back, and with 50 point edits staged before
           each call (set_bad outside the clock, their flush inside).  The gate of the section is evaluated and written into the record.

Both paths must return the same six arrays before anything is timed.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, GROUPS, MEMBERS, DISTINCT = 1000, 6, 11, 40


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(float(np.median(xs)), 3), "max": round(xs[-1], 3)}


def flip(desc, k, rng):
    """Each row with k random bits flipped (a bit drawn twice flips back)."""
    d = desc.copy()
    rows = np.arange(len(d))
    for _ in range(k):
        b = rng.integers(0, 256, len(d))
        d[rows, b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    return d


def workload(seed=5):
    from rumi_slam_amd import matcher as M
    from rumi_slam_amd.vocabulary import ORBVocabulary
    from voc_scene import synthetic_vocabulary_fast
    rng = np.random.default_rng(seed)
    parent, leaf, vdesc, weight = synthetic_vocabulary_fast(21, 10, 6)
    voc = ORBVocabulary(parent, leaf, vdesc, weight)
    P = 8 * N
    base = flip(vdesc[11 + rng.integers(0, 100, P)], 20, rng)            # map points scattered around the 100 level-2 nodes
    angle = rng.uniform(0, 360, P).astype(np.float32)
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)

    def observe(points, turn):
        desc = flip(base[points], 8, rng)
        keys = np.zeros(len(points), M.KP_DTYPE)
        keys["x"], keys["y"] = rng.uniform(0, 640, len(points)), rng.uniform(0, 480, len(points))
        keys["angle"] = np.mod(angle[points] + turn + rng.normal(0, 6, len(points)), 360)
        (_, _), (fn, fo, fi) = voc.transform(desc, 4)
        return M.FrameView(keys, desc, 640, 480, sf), M.FeatureVector.from_csr(fn, fo, fi)

    cur = observe(np.arange(N), 0.0)
    kfs = []
    for k in range(DISTINCT):
        share = [N // 2, N // 4, N // 8, 20][k % 4]
        pts = np.concatenate([rng.choice(N, share, replace=False), N + rng.choice(P - N, N - share, replace=False)])
        rng.shuffle(pts)
        F, fv = observe(pts, 30.0 * (k % 5))
        kfs.append((F, fv, np.where(rng.random(N) < 0.1, -1, pts).astype(np.int32)))
    groups = []
    for g in range(GROUPS):                                              # neighbouring candidates share covisibles: 66 members over 40 key-frames
        first = (g * DISTINCT) // GROUPS
        groups.append([(first + j) % DISTINCT for j in range(MEMBERS)])
    mp_bad = (rng.random(P) < 0.03).astype(np.uint8)
    cur_good = (rng.random(N) < 0.9).astype(np.uint8)
    assert len({k for g in groups for k in g}) == DISTINCT
    return M, cur, cur_good, kfs, mp_bad, groups


def host_union(n, groups, kfs, m12, nm):
    """LoopClosing.cc:622-651 from the per-member results, vectorised: first occurrences in (j, k) order, later writes to a slot overwrite."""
    G = len(groups)
    point, member = np.full((G, n), -1, np.int32), np.full((G, n), -1, np.int32)
    num, most = np.zeros(G, np.int32), np.zeros((G, 2), np.int32)
    row = 0
    for g, grp in enumerate(groups):
        f = m12[row:row + len(grp)]
        pts = np.stack([np.where(f[j] >= 0, kfs[k][2][np.maximum(f[j], 0)], -1) for j, k in enumerate(grp)]).ravel()
        live = np.nonzero(pts >= 0)[0]
        _, firsts = np.unique(pts[live], return_index=True)
        at = np.sort(live[firsts])                                       # flat j * n + k of every insertion, ascending
        point[g][at % n] = pts[at]                                       # repeated slots: the last assignment stands
        member[g][at % n] = at // n
        num[g] = len(at)
        c = nm[row:row + len(grp)]
        j = int(np.argmax(c)) if c.max(initial=0) > 0 else 0            # argmax returns the first maximum
        most[g] = (j, c[j] if len(c) else 0)
        row += len(grp)
    return point, member, num, most


def resident(a):
    """The --resident mode: one record per workload."""
    import torch
    from rumi_slam_amd import capi, mapping as MP
    from rumi_slam_amd.covis import Covisibility
    M, cur, cur_good, kfs, mp_bad, groups_full = workload()
    h = M.ORBmatcher(0.9, True)
    L, LM = h._lib, MP._lib()
    n, nmp = cur[0].n, len(mp_bad)
    # the store: the current key-frame in slot 0, table entry k in slot k + 1; a good current feature holds a fresh point, the others none
    cov = Covisibility(len(kfs) + 1, nmp + n)
    cur_row = np.where(cur_good != 0, nmp + np.arange(n), -1).astype(np.int32)
    slots = list(range(len(kfs) + 1))
    cov.set_keyframes(slots, [100 + s for s in slots], [0] * len(slots), [0] * len(slots), [cur_row] + [k[2] for k in kfs], [[]] * len(slots), [-1] * len(slots),
                      [[]] * len(slots))
    cov.set_points(np.arange(nmp + n, dtype=np.int32), np.concatenate([mp_bad, np.zeros(n, np.uint8)]), [[]] * (nmp + n))
    for s_, (F, fv) in zip(slots, [cur] + [(k[0], k[1]) for k in kfs]):
        cov.set_keyframe_features(s_, F, fv, [500.0, 500.0, 320.0, 240.0])
    dev = torch.cuda.get_device_name(0)
    edit_ids = np.arange(50, dtype=np.int32) * 7
    edit_bad = mp_bad[edit_ids].copy()                                   # the values they have: staged edits that change no result
    for name, groups in (("6x11", groups_full), ("1x1", [[0]])):
        G, members = len(groups), [k for g in groups for k in g]
        start = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
        used = sorted(set(members))                                      # the host-pointer entry gets the key-frames of this workload only
        table = (M.RumiBowKeyFrame * len(used))()
        for t, k in zip(table, used):
            t.feat, t.fv, t.mp = kfs[k][0].c, kfs[k][1].c, kfs[k][2].ctypes.data
        member = np.array([used.index(k) for k in members], np.int32)
        member_slot = np.array(members, np.int32) + 1
        shapes = [(len(members), n), (len(members),), (G, n), (G, n), (G,), (G, 2)]
        outP, outS = [np.zeros(sh, np.int32) for sh in shapes], [np.zeros(sh, np.int32) for sh in shapes]
        argsP = (h._h, C.addressof(cur[0].c), C.addressof(cur[1].c), capi.ptr(cur_good), len(used), C.addressof(table), nmp, capi.ptr(mp_bad), G, capi.ptr(start),
                 capi.ptr(member), 0.9, 1, *[capi.ptr(o) for o in outP])
        argsS = (h._h, cov._h, 0, G, capi.ptr(start), capi.ptr(member_slot), 0.9, 1, *[capi.ptr(o) for o in outS])
        argsN = argsS[:8] + (None,) + argsS[9:]

        def timed(fn, args):
            t0 = time.perf_counter()
            rc = fn(*args)
            t = time.perf_counter() - t0
            assert rc == 0, capi.lib().rumi_last_error()
            return t * 1e3

        def same():
            return all(np.array_equal(x, y) for x, y in zip(outP, outS))

        for o in outS:
            o[...] = -9
        timed(L.rumi_common_regions_bow, argsP); timed(LM.rumi_common_regions_bow_resident, argsS)
        assert same(), "the by-slot entry differs from the host-pointer entry"
        keep = outS[0].copy()
        timed(LM.rumi_common_regions_bow_resident, argsN)
        assert same() and np.array_equal(keep, outS[0]), "matches12 = NULL changed another array"
        for _ in range(5):
            timed(L.rumi_common_regions_bow, argsP); timed(LM.rumi_common_regions_bow_resident, argsS); timed(LM.rumi_common_regions_bow_resident, argsN)
        rounds = {"pointer": [], "slot_null": [], "slot_rows": [], "slot_null_50_edits": []}
        for _ in range(a.rounds):
            t = {k: [] for k in rounds}
            for _ in range(a.repeats):
                t["pointer"].append(timed(L.rumi_common_regions_bow, argsP))
                t["slot_null"].append(timed(LM.rumi_common_regions_bow_resident, argsN))
                t["slot_rows"].append(timed(LM.rumi_common_regions_bow_resident, argsS))
                cov.set_bad(pt_ids=edit_ids, pt_bad=edit_bad)
                t["slot_null_50_edits"].append(timed(LM.rumi_common_regions_bow_resident, argsN))
                assert same(), "results changed inside the timed rounds"
            for k in rounds:
                rounds[k].append(float(np.median(t[k])))
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        spread = {k: max(v) - min(v) for k, v in rounds.items()}           # ms, of the round medians
        gate = {}
        for k in ("slot_null", "slot_rows"):
            if name == "1x1":
                gate[k] = med[k] <= med["pointer"]
            else:
                gate[k] = med["pointer"] - med[k] > max(spread[k], spread["pointer"])
        rec = {"device": dev, "probe": "common_regions_resident", "workload": name, "groups": G, "members": len(members), "distinct_keyframes": len(used), "features": n,
               "repeats": a.repeats, "rounds": a.rounds, "num_bow_matches": outS[4].tolist(),
               "rumi_common_regions_bow_ms": stats(rounds["pointer"]), "resident_matches12_null_ms": stats(rounds["slot_null"]),
               "resident_matches12_back_ms": stats(rounds["slot_rows"]), "resident_null_after_50_staged_edits_ms": stats(rounds["slot_null_50_edits"]),
               "spread_of_round_medians_ms": {k: round(v, 4) for k, v in spread.items()},
               "resident_stage_ms_last_call": [round(float(x), 4) for x in MP.common_regions_bow_resident_stage_ms(h)],
               "gate": ("not above the host-pointer entry" if name == "1x1" else "below the host-pointer entry by more than the larger spread of the round medians"),
               "gate_held": gate}
        recs = [rec]
        if name == "6x11":
            recs.append(dict(device=dev, **facade_stages(a, M, cur, cur_good, kfs, mp_bad, groups)))
        for r_ in recs:
            line = json.dumps(r_)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


def facade_stages(a, M, cur, cur_good, kfs, mp_bad, groups):
    """The two facade stages over the same workload (tests/cpp/test_common_regions_resident_facade.cc, mode lc with repeats and rounds): the
    whole stage by the wall clock, marshalling included.  The binary is built into a temporary directory."""
    import subprocess
    import tempfile
    from common_regions_scene import KF, Scene
    from test_common_regions_facade_gpu import write_scene
    from test_common_regions_resident_facade_gpu import build_facade_test
    as_kf = lambda F, fv, mp=None: KF(F.keys["angle"], F.desc, (fv.node_ids, fv.offsets, fv.indices), mp)
    scene = Scene("probe", as_kf(*cur), cur_good, [as_kf(*k) for k in kfs], mp_bad, groups, 0.9, True)
    cov = {k: [] for k in range(len(kfs) + 1)}
    for g in groups:                                                     # the candidate, then its covisibles: vpCovKFi has the group's members
        cov[g[0] + 1] = [k + 1 for k in g[1:]]
    with tempfile.TemporaryDirectory() as tmp:
        exe, path = os.path.join(tmp, "facade"), os.path.join(tmp, "scene.bin")
        build_facade_test(exe)
        write_scene(path, scene, [g[0] + 1 for g in groups], cov, [], set())
        r = subprocess.run([exe, "lc", path, "-1", str(a.repeats), str(a.rounds)], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    lines = [l.split() for l in r.stdout.splitlines()]
    assert lines[0] == ["E", "with", "equal"] and lines[1] == ["E", "without", "equal"], lines[:2]
    t = {l[1]: [float(x) for x in l[2:]] for l in lines if l[0] == "T"}
    return {"probe": "common_regions_resident_facade", "workload": f"{len(groups)}x{len(groups[0])}", "repeats": a.repeats, "rounds": a.rounds,
            "CommonRegionsBoWStage_ms": stats(t["pointer"]), "CommonRegionsBoWStageResident_ms": stats(t["slot"]),
            "spread_of_round_medians_ms": {k: round(max(v) - min(v), 4) for k, v in t.items()},
            "note": "whole stage by the wall clock: groups, marshalling, the C entry, back to pointers; the by-slot stage without member matches"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    assert a.repeats >= 20
    if a.resident:
        return resident(a)
    import torch
    from rumi_slam_amd import capi
    M, cur, cur_good, kfs, mp_bad, groups = workload()
    h = M.ORBmatcher(0.9, True)
    L = h._lib
    n, nmp = cur[0].n, len(mp_bad)
    members = [k for g in groups for k in g]

    # ---- the new call: arguments marshalled once ----
    table = (M.RumiBowKeyFrame * len(kfs))()
    for t, (F, fv, mp) in zip(table, kfs):
        t.feat, t.fv, t.mp = F.c, fv.c, mp.ctypes.data
    start = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    member = np.array(members, np.int32)
    out = [np.zeros((len(members), n), np.int32), np.zeros(len(members), np.int32), np.zeros((GROUPS, n), np.int32), np.zeros((GROUPS, n), np.int32),
           np.zeros(GROUPS, np.int32), np.zeros((GROUPS, 2), np.int32)]
    args_new = (h._h, C.addressof(cur[0].c), C.addressof(cur[1].c), capi.ptr(cur_good), len(kfs), C.addressof(table), nmp, capi.ptr(mp_bad), GROUPS,
                capi.ptr(start), capi.ptr(member), 0.9, 1, *[capi.ptr(o) for o in out])

    def call():
        t0 = time.perf_counter()
        rc = L.rumi_common_regions_bow(*args_new)
        t = time.perf_counter() - t0
        assert rc == 0
        return t * 1e3

    # ---- the loop: 66 single searches, then the union on the host ----
    cur_mp = np.where(cur_good != 0, nmp, -1).astype(np.int32)
    bad1 = np.concatenate([mp_bad, [0]]).astype(np.uint8)
    m12 = np.zeros((len(members), n), np.int32)
    nm = [C.c_int32() for _ in members]
    rows = [(C.byref(kfs[k][0].c), C.byref(kfs[k][1].c), capi.ptr(kfs[k][2]), C.c_void_p(m12[i].ctypes.data), C.byref(nm[i])) for i, k in enumerate(members)]
    curF, curV, curM, badp = C.byref(cur[0].c), C.byref(cur[1].c), capi.ptr(cur_mp), capi.ptr(bad1)

    def loop():
        t0 = time.perf_counter()
        for F2, fv2, mp2, o, c in rows:
            rc = L.rumi_search_by_bow_kf(h._h, curF, curV, curM, F2, fv2, mp2, nmp + 1, badp, 0.9, 1, o, c)
            assert rc == 0
        t1 = time.perf_counter()
        u = host_union(n, groups, kfs, m12, np.fromiter((c.value for c in nm), np.int32, len(nm)))
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, u

    call()
    _, _, u = loop()
    nm_loop = np.array([c.value for c in nm], np.int32)
    got = [o.copy() for o in out]
    assert np.array_equal(got[0], m12) and np.array_equal(got[1], nm_loop), "the batch differs from the 66 single searches"
    for x, y in zip(got[2:], u):
        assert np.array_equal(x, y), "the device union differs from the host union"
    if a.trace:
        for _ in range(5):
            call(); loop()
        return
    for _ in range(5):
        call(); loop()
    dev = torch.cuda.get_device_name(0)
    recs = []
    per_round = {"call": [], "loop_calls": [], "loop_union": [], "loop": []}
    for _ in range(a.rounds):
        tc, tl, tu = [], [], []
        for _ in range(a.repeats):
            tc.append(call())
            l, un, _ = loop()
            tl.append(l); tu.append(un)
        per_round["call"].append(float(np.median(tc))); per_round["loop_calls"].append(float(np.median(tl)))
        per_round["loop_union"].append(float(np.median(tu))); per_round["loop"].append(float(np.median(np.add(tl, tu))))
    spread = {k: (max(v) - min(v)) / float(np.median(v)) for k, v in per_round.items()}
    c_med, l_med = float(np.median(per_round["call"])), float(np.median(per_round["loop"]))
    recs.append({"device": dev, "probe": "common_regions", "workload": f"{GROUPS} groups x {MEMBERS} members, {len(kfs)} distinct key-frames of {N} features, "
                 "k = 10, L = 6 tree at levelsup = 4, nnratio 0.9, orientation check on", "repeats": a.repeats, "rounds": a.rounds,
                 "nodes_current": int(cur[1].c.n_nodes), "num_bow_matches": got[4].tolist(), "nmatches_sum": int(got[1].sum()),
                 "rumi_common_regions_bow_ms": stats(per_round["call"]), "loop_66_calls_ms": stats(per_round["loop_calls"]),
                 "loop_host_union_ms": stats(per_round["loop_union"]), "loop_total_ms": stats(per_round["loop"]),
                 "relative_range_of_round_medians": {k: round(v, 4) for k, v in spread.items()}, "loop_over_call": round(l_med / c_med, 2)})
    M.CommonRegionsBoW_times(h, True)
    stages = []
    for _ in range(a.repeats):
        call()
        stages.append(M.CommonRegionsBoW_times(h).copy())
    M.CommonRegionsBoW_times(h, False)
    st = np.array(stages)
    names = ["host_pack_ms", "upload_and_clears_ms", "match_kernel_ms", "finish_and_union_kernels_ms", "copy_back_ms"]
    recs.append({"device": dev, "probe": "common_regions_stages", "source": "device events inside the entry (host clock for the pack), calls of their own",
                 "repeats": a.repeats, **{nm_: stats(st[:, i].tolist()) for i, nm_ in enumerate(names)},
                 "upload_bytes": int(sum(F.n * 41 + fv.c.n_nodes * 8 + F.n * 4 for F, fv, _ in kfs) + n * 41), "result_bytes": int(sum(o.nbytes for o in out))})
    for r in recs:
        line = json.dumps(r)
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
