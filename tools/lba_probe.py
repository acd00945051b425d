"""Local BA of BASELINE configs[3] (20 + 5 key-frames x 3000 points): wall / device ms per call, then batches of windows through
rumi_local_ba_batch."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
from ba_scene import ba_problem
from rumi_slam_amd.optimizer import Optimizer


def resident_probe(argv):
    """--resident [--out FILE]: rumi_local_ba_resident against a compiled scalar flatten of the same window from flat host arrays plus
    rumi_local_ba, in one process: medians of five rounds of 30 calls at 20 + 5 key-frames x 3000 points and at 8 + 3 x 800.  The flatten
    (tools/lba_flatten.cc, g++ -O2, one core) is timed apart from the solve.  Before every resident call the pose edits of the previous
    window and 50 attribute edits are staged; the map itself is put back to its first state outside the timed part, so that every call
    solves the same window.  Left out: the facade's walk of the live objects, which is slower than flat arrays, and the replay of the
    results on them."""
    import ctypes as C, json, subprocess
    import lba_resident_cases as LC
    from rumi_slam_amd import capi
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "lba_resident_probe.jsonl")
    so = os.path.join(ROOT, "tools", "bin", "liblba_flatten.so")
    if not os.path.exists(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tools", "lba_flatten.cc"), "-o", so])
    F = C.CDLL(so).lba_flatten
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    opt, ref = Optimizer(), Optimizer()
    lines = []
    for n_opt, n_fixed, n_points in ((20, 5, 3000), (8, 3, 800)):
        b = ba_problem(seed=0, n_opt=n_opt, n_fixed=n_fixed, n_points=n_points)
        nkf = n_opt + n_fixed
        S = LC.Scene(0)
        per_kf = np.bincount(b["e_kf"], minlength=nkf)
        octs = np.rint(np.log(1.0 / b["e_w"].astype(np.float64)) / (2 * np.log(1.2))).astype(np.int32)
        for k in range(nkf):
            S.add_kf(k, k + 1, int(per_kf[k]))
            S.kfs[k]["pose7"] = b["kf_pose"][k].copy()
        for p in range(n_points):
            S.add_point(p)
            S.pts[p]["pos"] = b["mp_pos"][p].copy()
        used = [0] * nkf
        for e in range(len(b["e_mp"])):
            k, p = int(b["e_kf"][e]), int(b["e_mp"][e])
            f = used[k]; used[k] += 1
            kf = S.kfs[k]
            kf["keys"]["x"][f], kf["keys"]["y"][f], kf["keys"]["octave"][f] = b["e_obs"][e][0], b["e_obs"][e][1], octs[e]
            kf["row"][f] = p
            S.pts[p]["obs"].append((k, f))
        cur, neigh, init = n_fixed, list(range(n_fixed + 1, nkf)), -1
        w = LC.window(S, cur, neigh, init)
        a = w["args"]
        # ---- flat arrays of the same map for the scalar loop
        slots, ids = sorted(S.kfs), sorted(S.pts)
        key = np.array([S.kfs[s]["key"] for s in slots], np.uint64); kmap = np.zeros(nkf, np.int32); kbad = np.zeros(nkf, np.uint8)
        row_off = np.concatenate([[0], np.cumsum([len(S.kfs[s]["row"]) for s in slots])]).astype(np.int32)
        row = np.concatenate([np.array(S.kfs[s]["row"], np.int32) for s in slots])
        keys = np.concatenate([S.kfs[s]["keys"] for s in slots])
        kx, ky, ko = (np.ascontiguousarray(keys[n]) for n in ("x", "y", "octave"))
        sf = np.concatenate([S.kfs[s]["sf"] for s in slots]).astype(np.float32)
        pose7 = np.stack([S.kfs[s]["pose7"] for s in slots]).astype(np.float32)
        pbad = np.zeros(n_points, np.uint8); pmap = np.zeros(n_points, np.int32); pos = np.stack([S.pts[p]["pos"] for p in ids]).astype(np.float32)
        obs_off = np.concatenate([[0], np.cumsum([len(S.pts[p]["obs"]) for p in ids])]).astype(np.int32)
        obs_slot = np.array([o[0] for p in ids for o in S.pts[p]["obs"]], np.int32); obs_feat = np.array([o[1] for p in ids for o in S.pts[p]["obs"]], np.int32)
        nE = len(obs_slot)
        ng = np.array(neigh, np.int32)
        o_slots = np.zeros(nkf, np.int32); o_pose = np.zeros((nkf, 7), np.float32); o_fixed = np.zeros(nkf, np.uint8); o_ids = np.zeros(n_points, np.int32)
        o_pos = np.zeros((n_points, 3), np.float32); o_emp = np.zeros(nE, np.int32); o_ekf = np.zeros(nE, np.int32); o_obs = np.zeros((nE, 2), np.float32)
        o_w = np.zeros(nE, np.float32); counts = np.zeros(5, np.int32)
        def flat():
            return F(nkf, P(key), P(kmap), P(kbad), P(row_off), P(row), P(kx), P(ky), P(ko), P(sf), 8, P(pose7), n_points, P(pbad), P(pmap), P(pos), P(obs_off),
                     P(obs_slot), P(obs_feat), cur, P(ng), len(ng), init, P(o_slots), P(o_pose), P(o_fixed), P(o_ids), P(o_pos), P(o_emp), P(o_ekf), P(o_obs), P(o_w), P(counts))
        assert flat() == 0 and counts.tolist() == [len(a[1]), w["num_OptKF"], w["num_fixedKF"], len(w["mp_ids"]), len(w["edges"])]
        n_e = int(counts[4])
        flat_args = (o_pose[:counts[0]], o_fixed[:counts[0]], o_pos[:counts[3]], o_emp[:n_e], o_ekf[:n_e], o_obs[:n_e], o_w[:n_e], S.K4)
        assert all(np.array_equal(x, y) for x, y in zip(flat_args, a)), "the compiled flatten and the Python restatement agree"
        store = LC.to_store(S)
        local = [cur] + neigh
        first_pose = np.stack([S.kfs[s]["pose7"] for s in local]); first_pos = np.stack([S.pts[p]["pos"] for p in ids])
        zeros = dict(normal=np.tile(np.float32([0, 0, 1]), (n_points, 1)), mn=np.full(n_points, 0.5, np.float32), mx=np.full(n_points, 40.0, np.float32),
                     desc=np.zeros((n_points, 32), np.uint8))
        def restore():          # outside the timed part: the first state again, uploaded by a query of the store
            store.set_keyframe_poses(local, first_pose)
            store.set_point_attributes(ids, first_pos, zeros["normal"], zeros["mn"], zeros["mx"], zeros["desc"])
            store.update_connections([cur])
        def stage_edits():      # the pose edits of the previous window and 50 attribute edits, staged before the call
            store.set_keyframe_poses(local, first_pose)
            store.set_point_attributes(ids[:50], first_pos[:50], zeros["normal"][:50], zeros["mn"][:50], zeros["mx"][:50], zeros["desc"][:50])
        want = ref.LocalBundleAdjustment(*a)
        restore(); stage_edits()
        got = opt.LocalBundleAdjustmentResident(store, cur, neigh, init)
        same = bool(np.array_equal(got["mp_pos3"], want[2]) and np.array_equal(got["kf_pose7"], want[1][:w["num_OptKF"]]) and np.array_equal(got["stats"], want[0]))
        med = {"flatten_ms": [], "local_ba_ms": [], "resident_ms": []}
        for _ in range(5):
            tf, tb, tr = [], [], []
            for _ in range(30):
                t0 = time.perf_counter(); flat(); tf.append((time.perf_counter() - t0) * 1e3)
                ref.LocalBundleAdjustment(*flat_args); tb.append(ref.last_call_s * 1e3)
                restore(); stage_edits()
                opt.LocalBundleAdjustmentResident(store, cur, neigh, init); tr.append(opt.last_call_s * 1e3)
            med["flatten_ms"].append(float(np.median(tf))); med["local_ba_ms"].append(float(np.median(tb))); med["resident_ms"].append(float(np.median(tr)))
        rec = dict(window="%d + %d key-frames x %d points" % (n_opt, n_fixed, n_points), edges=n_e, equal_to_local_ba=same,
                   flatten_ms=float(np.median(med["flatten_ms"])), local_ba_ms=float(np.median(med["local_ba_ms"])), resident_ms=float(np.median(med["resident_ms"])),
                   rounds=med, staged_upload_bytes=store.stats()["last_upload_bytes"])
        rec["host_path_ms"] = rec["flatten_ms"] + rec["local_ba_ms"]
        lines.append(rec)
        print(json.dumps(rec))
        store.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if "--resident" in sys.argv:
    resident_probe(sys.argv)
    sys.exit(0)
opt = Optimizer()
for n_opt in (int(x) for x in (sys.argv[1:] or ["20"])):
    b = ba_problem(seed=0, n_opt=n_opt, n_fixed=5, n_points=3000)
    a = (b["kf_pose"], b["kf_fixed"], b["mp_pos"], b["e_mp"], b["e_kf"], b["e_obs"], b["e_w"], b["K"])
    for _ in range(3): opt.LocalBundleAdjustment(*a)
    ts = []
    for _ in range(20):
        t0 = time.perf_counter(); stats, *_ = opt.LocalBundleAdjustment(*a); ts.append((time.perf_counter() - t0) * 1e3)
    dev = opt.stage_ms()[5]
    print("n_opt %d  wall ms median %.3f min %.3f  device %.3f  stats %s" % (n_opt, float(np.median(ts)), min(ts), dev, [int(x) for x in stats]))

# R windows through rumi_local_ba_batch
b = ba_problem(seed=0, n_opt=20, n_fixed=5, n_points=3000)
w = (b["kf_pose"], b["kf_fixed"], b["mp_pos"], b["e_mp"], b["e_kf"], b["e_obs"], b["e_w"], b["K"])
for R, workers in ((16, 1), (32, 1), (4, 1)):
    opt.LocalBundleAdjustmentBatch([w] * R, workers)
    dts, cpu = [], []
    for _ in range(5):
        c0, t0 = time.process_time(), time.perf_counter(); opt.LocalBundleAdjustmentBatch([w] * R, workers); dts.append(time.perf_counter() - t0); cpu.append(time.process_time() - c0)
    print("batch of %d windows (20 + 5 key-frames x 3000 points), %d workers: %.3f ms per window (best of 5; median %.3f); host cores busy %.2f (process CPU time / wall time)" % (
        R, workers, min(dts) * 1e3 / R, float(np.median(dts)) * 1e3 / R, float(np.median(cpu)) / float(np.median(dts))))
