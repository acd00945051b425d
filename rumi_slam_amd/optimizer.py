"""Host-side mirror of the two hot members of the all-static ``ORB_SLAM3::Optimizer``
(R/include/cloud_edge_slam_lib/Optimizer.h:53,55) over the C ABI in include/rumi_opt.h."""
import ctypes as C

import numpy as np

from . import capi


class RumiSim3ScoreSet(C.Structure):
    """include/rumi_opt.h RumiSim3ScoreSet"""
    _fields_ = [("n_pairs", C.c_int32)] + [(k, C.c_void_p) for k in ("pair_start", "pair_denominator", "S_c1w1", "S_c2w2", "S_kf1w", "S_kf2w", "K4_1", "K4_2",
                                                                   "X1", "X2", "kp1", "kp2", "sigma2_1", "sigma2_2", "edge1", "edge2")]


OPT_SYMBOLS = capi.OPT_SYMBOLS          # one list: every entry of include/rumi_opt.h

# include/rumi_opt.h: RumiSim3RansacSolver, RumiSim3RansacResult, RumiSim3OptProblem
SIM3_RANSAC_SOLVER_DTYPE = np.dtype([("first", "<i4"), ("n", "<i4"), ("min_inliers", "<i4"), ("its_left", "<i4"), ("fix_scale", "<i4"),
                                     ("K4_1", "<f4", 4), ("K4_2", "<f4", 4)])
SIM3_RANSAC_RESULT_DTYPE = np.dtype([("state", "<i4"), ("its", "<i4"), ("hyp", "<i4"), ("n_inliers", "<i4"), ("T12", "<f4", 16)])
SIM3_OPT_PROBLEM_DTYPE = np.dtype([("first", "<i4"), ("n", "<i4"), ("th2", "<f4"), ("fix_scale", "<i4"), ("robust_first_pass", "<i4"),
                                   ("K4_1", "<f4", 4), ("K4_2", "<f4", 4)])
assert SIM3_RANSAC_SOLVER_DTYPE.itemsize == 52 and SIM3_RANSAC_RESULT_DTYPE.itemsize == 80 and SIM3_OPT_PROBLEM_DTYPE.itemsize == 52
SIM3_NOT_REACHED, SIM3_CONVERGED, SIM3_EXHAUSTED, SIM3_WINDOW_ENDED = 0, 1, 2, 3


class RumiLbaResidentOut(C.Structure):
    """include/rumi_opt.h RumiLbaResidentOut"""
    _fields_ = [("kf_cap", C.c_int32), ("mp_cap", C.c_int32), ("erase_cap", C.c_int32), ("kf_slots", C.c_void_p), ("kf_pose7", C.c_void_p),
                ("mp_ids", C.c_void_p), ("mp_pos3", C.c_void_p), ("erased", C.c_void_p), ("n_kf", C.c_int32), ("num_OptKF", C.c_int32),
                ("num_fixedKF", C.c_int32), ("num_MPs", C.c_int32), ("num_edges", C.c_int32), ("n_erased", C.c_int32), ("stats", C.c_int32 * 4)]


def _lib():
    L = capi.lib()
    if getattr(L, "_opt_ready", False):
        return L
    vp, i32 = C.c_void_p, C.c_int32
    L.rumi_opt_create.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.rumi_opt_destroy.argtypes = [vp]
    L.rumi_opt_destroy.restype = None
    L.rumi_pose_optimization.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, C.POINTER(i32)]
    L.rumi_pose_optimization_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rumi_local_ba.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rumi_local_ba_batch.argtypes = [vp, i32, vp, i32]
    L.rumi_local_ba_resident.argtypes = [vp, vp, i32, vp, i32, i32, vp, C.POINTER(RumiLbaResidentOut)]
    L.rumi_bundle_adjustment.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp]
    L.rumi_sim3_inliers.argtypes = [vp, i32] + [vp] * 17
    L.rumi_merge_ba.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rumi_opt_stage_ms.argtypes = [vp, vp]
    L.rumi_opt_set_profiling.argtypes = [vp, i32]
    L.rumi_opt_kernel_ms.argtypes = [vp, vp]
    L.rumi_opt_footprint.argtypes = [vp, vp]
    L.rumi_sim3_ransac.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.rumi_optimize_sim3.argtypes = [vp, i32, vp, i32] + [vp] * 12 + [C.c_float, i32, i32, vp, vp, vp]
    L.rumi_essential_graph.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp]
    L.rumi_sim3_correct_points.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp]
    L.rumi_sim3_ransac_batch.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.rumi_optimize_sim3_batch.argtypes = [vp, i32, vp, i32] + [vp] * 9
    L._opt_ready = True
    return L


class RumiBaWindow(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("kf_pose7", C.c_void_p), ("kf_fixed", C.c_void_p), ("n_mp", C.c_int32), ("mp_pos3", C.c_void_p),
                ("n_edges", C.c_int32), ("e_mp", C.c_void_p), ("e_kf", C.c_void_p), ("e_obs", C.c_void_p), ("e_inv_sigma2", C.c_void_p),
                ("K4", C.c_void_p), ("stop_flag", C.c_void_p), ("erase_out", C.c_void_p), ("stats", C.c_int32 * 4), ("status", C.c_int32)]


class Optimizer:
    def __init__(self, max_pose_edges=1 << 18, max_pose_batch=1024, max_kf=64, max_mp=16384, max_edges=1 << 18, device=-1):
        self._lib = _lib()
        self._h = C.c_void_p()
        capi.check(self._lib.rumi_opt_create(max_pose_edges, max_pose_batch, max_kf, max_mp, max_edges, device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.rumi_opt_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def PoseOptimization(self, Xw, obs, inv_sigma2, K4, Tcw7):
        """Returns (nInitialCorrespondences - nBad, Tcw7, outlier[n])."""
        Xw = np.ascontiguousarray(Xw, np.float32); obs = np.ascontiguousarray(obs, np.float32)
        w = np.ascontiguousarray(inv_sigma2, np.float32); K4 = np.ascontiguousarray(K4, np.float32)
        T = np.ascontiguousarray(Tcw7, np.float32).copy()
        out = np.zeros(max(len(w), 1), np.uint8)
        ng = C.c_int32()
        capi.check(self._lib.rumi_pose_optimization(self._h, capi.ptr(Xw), capi.ptr(obs), capi.ptr(w), len(w), capi.ptr(K4), capi.ptr(T),
                                                    capi.ptr(out), C.byref(ng)))
        return ng.value, T, out[:len(w)]

    def PoseOptimizationBatch(self, start, Xw, obs, inv_sigma2, K4, Tcw7):
        start = np.ascontiguousarray(start, np.int32)
        Xw = np.ascontiguousarray(Xw, np.float32); obs = np.ascontiguousarray(obs, np.float32)
        w = np.ascontiguousarray(inv_sigma2, np.float32); K4 = np.ascontiguousarray(K4, np.float32)
        T = np.ascontiguousarray(Tcw7, np.float32).copy()
        B = len(start) - 1
        out = np.zeros(max(len(w), 1), np.uint8)
        ng = np.zeros(B, np.int32)
        capi.check(self._lib.rumi_pose_optimization_batch(self._h, B, capi.ptr(start), capi.ptr(Xw), capi.ptr(obs), capi.ptr(w), capi.ptr(K4),
                                                          capi.ptr(T), capi.ptr(out), capi.ptr(ng)))
        return ng, T, out[:len(w)]

    def LocalBundleAdjustment(self, kf_pose, kf_fixed, mp_pos, e_mp, e_kf, e_obs, e_inv_sigma2, K4, stop_flag=None, merge=False):
        """Returns (stats[4], kf_pose, mp_pos, erase[nE])."""
        kp = np.ascontiguousarray(kf_pose, np.float32).copy(); kfix = np.ascontiguousarray(kf_fixed, np.uint8)
        mp = np.ascontiguousarray(mp_pos, np.float32).copy(); em = np.ascontiguousarray(e_mp, np.int32)
        ek = np.ascontiguousarray(e_kf, np.int32); eo = np.ascontiguousarray(e_obs, np.float32)
        ew = np.ascontiguousarray(e_inv_sigma2, np.float32); K4 = np.ascontiguousarray(K4, np.float32)
        erase = np.zeros(max(len(em), 1), np.uint8)
        stats = np.zeros(4, np.int32)
        sp = capi.ptr(stop_flag) if stop_flag is not None else None
        fn = self._lib.rumi_merge_ba if merge else self._lib.rumi_local_ba
        import time
        t0 = time.perf_counter()
        rc = fn(self._h, len(kfix), capi.ptr(kp), capi.ptr(kfix), len(mp), capi.ptr(mp), len(em), capi.ptr(em),
                capi.ptr(ek), capi.ptr(eo), capi.ptr(ew), capi.ptr(K4), sp, capi.ptr(erase), capi.ptr(stats))
        self.last_call_s = time.perf_counter() - t0
        capi.check(rc)
        return stats, kp, mp, erase[:len(em)]

    def LocalBundleAdjustmentResident(self, covis, cur_slot, neigh_slots, init_slot, stop_flag=None, kf_cap=None, mp_cap=None, erase_cap=None,
                                      fill=0, check=True):
        """rumi_local_ba_resident: Optimizer::LocalBundleAdjustment with the window assembled on the device from the store ``covis``.
        Returns dict(kf_slots [n_kf], num_OptKF, num_fixedKF, kf_pose7 [num_OptKF, 7], mp_ids [num_MPs], mp_pos3 [num_MPs, 3], num_edges,
        erased [n_erased, 3] = (slot, point id, feature), stats [4], status, raw = the untrimmed output arrays).  The capacities default to
        the store's and the handle's sizes; every output byte starts as ``fill``; with check=False a refusal comes back as status."""
        neigh = np.ascontiguousarray(neigh_slots, np.int32).reshape(-1)
        kf_cap = covis.max_kf if kf_cap is None else int(kf_cap)
        mp_cap = covis.max_points if mp_cap is None else int(mp_cap)
        erase_cap = (1 << 18) if erase_cap is None else int(erase_cap)
        f = lambda n, dt: np.frombuffer(bytes([fill]) * (max(int(n), 1) * np.dtype(dt).itemsize), dt).copy()
        raw = dict(kf_slots=f(kf_cap, np.int32), kf_pose7=f(kf_cap * 7, np.float32), mp_ids=f(mp_cap, np.int32), mp_pos3=f(mp_cap * 3, np.float32),
                   erased=f(erase_cap * 3, np.int32))
        out = RumiLbaResidentOut.from_buffer_copy(bytes([fill]) * C.sizeof(RumiLbaResidentOut))
        out.kf_cap, out.mp_cap, out.erase_cap = kf_cap, mp_cap, erase_cap
        for k, v in raw.items():
            setattr(out, k, v.ctypes.data)
        sp = capi.ptr(stop_flag) if stop_flag is not None else None
        import time
        t0 = time.perf_counter()
        rc = self._lib.rumi_local_ba_resident(self._h, covis._h, int(cur_slot), capi.ptr(neigh), len(neigh), int(init_slot), sp, C.byref(out))
        self.last_call_s = time.perf_counter() - t0
        if check:
            capi.check(rc)
        res = dict(status=int(rc), raw=raw, stats=np.array(out.stats, np.int32), header=bytes(out))
        if rc == capi.RUMI_OK and not res["stats"][3]:
            nk, no, nm, ne = out.n_kf, out.num_OptKF, out.num_MPs, out.n_erased
            res.update(kf_slots=raw["kf_slots"][:nk], num_OptKF=no, num_fixedKF=out.num_fixedKF, kf_pose7=raw["kf_pose7"][:no * 7].reshape(no, 7),
                       mp_ids=raw["mp_ids"][:nm], mp_pos3=raw["mp_pos3"][:nm * 3].reshape(nm, 3), num_edges=out.num_edges,
                       erased=raw["erased"][:ne * 3].reshape(ne, 3))
        return res

    def LocalBundleAdjustmentBatch(self, windows, n_workers=4, return_status=False):
        """rumi_local_ba_batch: `windows` = list of (kf_pose, kf_fixed, mp_pos, e_mp, e_kf, e_obs, e_inv_sigma2, K4) tuples; returns one
        (stats[4], kf_pose, mp_pos, erase[nE]) per window, as LocalBundleAdjustment does.  Any failure raises, unless return_status: then the
        call returns (results, the batch's status, the status of every window) and a failed window's arrays are what the C entry left of them."""
        arr = (RumiBaWindow * len(windows))()
        keep = []
        for W, w in zip(arr, windows):
            kp = np.ascontiguousarray(w[0], np.float32).copy(); kfix = np.ascontiguousarray(w[1], np.uint8)
            mp = np.ascontiguousarray(w[2], np.float32).copy(); em = np.ascontiguousarray(w[3], np.int32)
            ek = np.ascontiguousarray(w[4], np.int32); eo = np.ascontiguousarray(w[5], np.float32)
            ew = np.ascontiguousarray(w[6], np.float32); K4 = np.ascontiguousarray(w[7], np.float32)
            erase = np.zeros(max(len(em), 1), np.uint8)
            keep.append((kp, kfix, mp, em, ek, eo, ew, K4, erase))
            W.n_kf, W.kf_pose7, W.kf_fixed, W.n_mp, W.mp_pos3 = len(kfix), kp.ctypes.data, kfix.ctypes.data, len(mp), mp.ctypes.data
            W.n_edges, W.e_mp, W.e_kf, W.e_obs, W.e_inv_sigma2 = len(em), em.ctypes.data, ek.ctypes.data, eo.ctypes.data, ew.ctypes.data
            W.K4, W.stop_flag, W.erase_out = K4.ctypes.data, None, erase.ctypes.data
        import time
        t0 = time.perf_counter()
        rc = self._lib.rumi_local_ba_batch(self._h, len(windows), C.cast(arr, C.c_void_p), int(n_workers))
        self.last_call_s = time.perf_counter() - t0         # the C entry alone (the mirror above copies every array of every window)
        if not return_status:
            capi.check(rc)
        res = [(np.array(W.stats, np.int32), k[0], k[2], k[8][:len(k[3])]) for W, k in zip(arr, keep)]
        return (res, int(rc), [int(W.status) for W in arr]) if return_status else res

    def BundleAdjustment(self, kf_pose, kf_fixed, mp_pos, e_mp, e_kf, e_obs, e_inv_sigma2, K4, n_iterations=5, robust=True, stop_flag=None):
        """Optimizer::BundleAdjustment (global BA): returns (stats[4], kf_pose, mp_pos)."""
        kp = np.ascontiguousarray(kf_pose, np.float32).copy(); kfix = np.ascontiguousarray(kf_fixed, np.uint8)
        mp = np.ascontiguousarray(mp_pos, np.float32).copy(); em = np.ascontiguousarray(e_mp, np.int32)
        ek = np.ascontiguousarray(e_kf, np.int32); eo = np.ascontiguousarray(e_obs, np.float32)
        ew = np.ascontiguousarray(e_inv_sigma2, np.float32); K4 = np.ascontiguousarray(K4, np.float32)
        stats = np.zeros(4, np.int32)
        sp = capi.ptr(stop_flag) if stop_flag is not None else None
        capi.check(self._lib.rumi_bundle_adjustment(self._h, len(kfix), capi.ptr(kp), capi.ptr(kfix), len(mp), capi.ptr(mp), len(em), capi.ptr(em),
                                                    capi.ptr(ek), capi.ptr(eo), capi.ptr(ew), capi.ptr(K4), sp, int(n_iterations), int(robust), capi.ptr(stats)))
        return stats, kp, mp

    def MergeBundleAdjustment(self, *args, **kw):
        """Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag): the two-pass merge-window BA."""
        return self.LocalBundleAdjustment(*args, merge=True, **kw)

    def ComputeInliersNum(self, pair_start, pair_denominator, S_c1w2, S_c2w1, K4_1, K4_2, X1, X2, kp1, kp2, sigma2_1, sigma2_2, edge1, edge2):
        """Sim3Solver::ComputeInliersNum on flat arrays (include/rumi_opt.h).  Returns (median ratio, ratio per pair, inlier flags)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        ps = np.ascontiguousarray(pair_start, np.int32); pd = np.ascontiguousarray(pair_denominator, np.int32)
        A = np.ascontiguousarray(S_c1w2, np.float64); B = np.ascontiguousarray(S_c2w1, np.float64)
        arrs = [f32(K4_1), f32(K4_2), f32(X1), f32(X2), f32(kp1), f32(kp2), f32(sigma2_1), f32(sigma2_2), np.ascontiguousarray(edge1, np.uint8),
                np.ascontiguousarray(edge2, np.uint8)]
        n_pairs, total = len(ps) - 1, int(ps[-1])
        inl = np.zeros(max(total, 1), np.uint8); ratio = np.zeros(max(n_pairs, 1), np.float32); med = C.c_float()
        capi.check(self._lib.rumi_sim3_inliers(self._h, n_pairs, capi.ptr(ps), capi.ptr(pd), capi.ptr(A), capi.ptr(B), *[capi.ptr(a) for a in arrs],
                                               capi.ptr(inl), capi.ptr(ratio), C.byref(med)))
        return med.value, ratio[:n_pairs], inl[:total]

    def Sim3Ransac(self, X3Dc1, X3Dc2, sigma2_1, sigma2_2, K4_1, K4_2, triples, fix_scale=False, score=None, want_inliers=True):
        """The hypotheses of one block of Sim3Solver::iterate (R/lib_src/Sim3Solver.cc:159-404; include/rumi_opt.h, rumi_sim3_ransac).
        triples [n_hyp,3] = the minimal sets.  score: None or a dict with the ComputeInliersNum data (pair_start, pair_denominator, S_c1w1, S_c2w2,
        S_kf1w, S_kf2w, K4_1, K4_2, X1, X2, kp1, kp2, sigma2_1, sigma2_2, edge1, edge2).
        Returns dict(R [h,3,3], t [h,3], s [h], valid [h], n_inliers [h], inliers [h,n] or None, ratio [h,n_pairs] or None, median [h] or None)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        X1, X2, s1, s2, K1, K2 = f32(X3Dc1).reshape(-1, 3), f32(X3Dc2).reshape(-1, 3), f32(sigma2_1), f32(sigma2_2), f32(K4_1), f32(K4_2)
        tri = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
        n, H = len(X1), len(tri)
        T = np.zeros((max(H, 1), 16), np.float32); nin = np.zeros(max(H, 1), np.int32)
        inl = np.zeros((max(H, 1), n), np.uint8) if want_inliers else None
        sc, keep, ratio, med = None, [], None, None
        if score is not None:
            f64 = lambda a: np.ascontiguousarray(a, np.float64)
            u8 = lambda a: np.ascontiguousarray(a, np.uint8)
            ps, pd = np.ascontiguousarray(score["pair_start"], np.int32), np.ascontiguousarray(score["pair_denominator"], np.int32)
            keep = [ps, pd, f64(score["S_c1w1"]), f64(score["S_c2w2"]), f64(score["S_kf1w"]), f64(score["S_kf2w"]), f32(score["K4_1"]), f32(score["K4_2"]),
                    f32(score["X1"]), f32(score["X2"]), f32(score["kp1"]), f32(score["kp2"]), f32(score["sigma2_1"]), f32(score["sigma2_2"]),
                    u8(score["edge1"]), u8(score["edge2"])]
            sc = RumiSim3ScoreSet(len(ps) - 1, *[a.ctypes.data_as(C.c_void_p) for a in keep])
            ratio = np.zeros((max(H, 1), len(ps) - 1), np.float32); med = np.zeros(max(H, 1), np.float32)
        P = capi.ptr
        capi.check(self._lib.rumi_sim3_ransac(self._h, n, P(X1), P(X2), P(s1), P(s2), P(K1), P(K2), int(bool(fix_scale)), H, P(tri),
                                              C.byref(sc) if sc is not None else None, P(T), P(nin), P(inl) if inl is not None else None,
                                              P(ratio) if ratio is not None else None, P(med) if med is not None else None))
        T = T[:H]
        return dict(R=T[:, :9].reshape(-1, 3, 3).copy(), t=T[:, 9:12].copy(), s=T[:, 12].copy(), valid=T[:, 13] != 0, n_inliers=nin[:H].copy(),
                    inliers=inl[:H].astype(bool) if inl is not None else None, ratio=ratio[:H] if ratio is not None else None,
                    median=med[:H] if med is not None else None)

    def OptimizeSim3(self, S8, P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K4_1, K4_2, th2=10.0, fix_scale=False, robust_first_pass=True,
                     pair_of=None, S_c1w=None, S_c2w=None, skip12=None, skip21=None):
        """Optimizer::OptimizeSim3 (robust first pass, no key-frame transforms) and, with pair_of / S_c1w / S_c2w and
        robust_first_pass=False, Optimizer::OptimizeCloudSim3, on flat arrays (include/rumi_opt.h).
        Returns (nIn, nBad, early, S8, status[n])."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8)
        P1c, P2c, obs1, obs2, w1, w2, K1, K2 = (f32(a) for a in (P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K4_1, K4_2))
        n = len(w1)
        S = np.ascontiguousarray(S8, np.float64).copy()
        world = S_c1w is not None
        po = np.ascontiguousarray(pair_of, np.int32) if world else None
        A = np.ascontiguousarray(S_c1w, np.float64).reshape(-1, 8) if world else None
        B = np.ascontiguousarray(S_c2w, np.float64).reshape(-1, 8) if world else None
        s12, s21 = u8(skip12), u8(skip21)
        status = np.zeros(max(n, 1), np.uint8); res = np.zeros(3, np.int32)
        P = lambda a: None if a is None else capi.ptr(a)
        capi.check(self._lib.rumi_optimize_sim3(self._h, n, P(po), len(A) if world else 0, P(A), P(B), P(P1c), P(P2c), P(obs1), P(obs2), P(w1), P(w2),
                                                P(s12), P(s21), P(K1), P(K2), float(th2), int(fix_scale), int(robust_first_pass), P(S), P(status), P(res)))
        return int(res[0]), int(res[1]), bool(res[2]), S, status[:n]

    def Sim3RansacBatch(self, solvers, X3Dc1, X3Dc2, sigma2_1, sigma2_2, triples, want_all=False):
        """One window of the shared iteration stream over J solvers of Sim3Solver::iterate(..., bConverge) (include/rumi_opt.h,
        rumi_sim3_ransac_batch).  solvers: records of SIM3_RANSAC_SOLVER_DTYPE over the concatenated correspondences; triples [J, R, 3] = the
        window drawn with every solver's own N (GlibcRand.draw_window), indices relative to the solver's first.
        Returns dict(state [J], its [J], hyp [J], n_inliers [J], T12 [J,16], inliers [n_total] bool, and with want_all n_inliers_all [J,R],
        T12_all [J,R,16])."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        sol = np.ascontiguousarray(solvers, SIM3_RANSAC_SOLVER_DTYPE)
        X1, X2, s1, s2 = f32(X3Dc1).reshape(-1, 3), f32(X3Dc2).reshape(-1, 3), f32(sigma2_1), f32(sigma2_2)
        J, n = len(sol), len(X1)
        tri = np.ascontiguousarray(triples, np.int32).reshape(J, -1, 3)
        R = tri.shape[1]
        if not (len(X2) == len(s1) == len(s2) == n):
            raise ValueError("Sim3RansacBatch: array lengths disagree")
        res = np.zeros(max(J, 1), SIM3_RANSAC_RESULT_DTYPE); inl = np.zeros(max(n, 1), np.uint8)
        nall = np.zeros((max(J, 1), max(R, 1)), np.int32) if want_all else None
        Tall = np.zeros((max(J, 1), max(R, 1), 16), np.float32) if want_all else None
        P = lambda a: None if a is None else capi.ptr(a)
        capi.check(self._lib.rumi_sim3_ransac_batch(self._h, J, P(sol), n, P(X1), P(X2), P(s1), P(s2), R, P(tri), P(res), P(inl), P(nall), P(Tall)))
        res = res[:J]
        out = dict(state=res["state"].copy(), its=res["its"].copy(), hyp=res["hyp"].copy(), n_inliers=res["n_inliers"].copy(), T12=res["T12"].copy(),
                   inliers=inl[:n].astype(bool))
        if want_all:
            out.update(n_inliers_all=nall[:J, :R], T12_all=Tall[:J, :R])
        return out

    def OptimizeSim3Batch(self, problems, S8, P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2):
        """Optimizer::OptimizeSim3 of J candidates in one call (include/rumi_opt.h, rumi_optimize_sim3_batch).  problems: records of
        SIM3_OPT_PROBLEM_DTYPE over the concatenated correspondences; S8 [J,8] the initial estimates.
        Returns (result3 [J,3] = nIn, nBad, early; S8 [J,8]; status [n_total])."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        pr = np.ascontiguousarray(problems, SIM3_OPT_PROBLEM_DTYPE)
        P1c, P2c, obs1, obs2, w1, w2 = f32(P1c).reshape(-1, 3), f32(P2c).reshape(-1, 3), f32(obs1).reshape(-1, 2), f32(obs2).reshape(-1, 2), f32(inv_sigma2_1), f32(inv_sigma2_2)
        J, n = len(pr), len(w1)
        S = np.ascontiguousarray(S8, np.float64).reshape(-1, 8).copy()
        if len(S) != J or not (len(P1c) == len(P2c) == len(obs1) == len(obs2) == len(w2) == n):
            raise ValueError("OptimizeSim3Batch: array lengths disagree")
        status = np.zeros(max(n, 1), np.uint8); res = np.zeros((max(J, 1), 3), np.int32)
        P = capi.ptr
        capi.check(self._lib.rumi_optimize_sim3_batch(self._h, J, P(pr), n, P(P1c), P(P2c), P(obs1), P(obs2), P(w1), P(w2), P(S), P(status), P(res)))
        return res[:J], S, status[:n]

    def essential_graph(self, S8, fixed, fix_scale, e_v0, e_v1, meas8, n_iterations=20, stop_flag=None):
        """Optimizer::OptimizeEssentialGraph on the flattened Sim3 pose graph (include/rumi_opt.h, rumi_essential_graph).
        Returns (S8 [n_v,8], stats[4], chi2_trace[n_iterations + 1])."""
        S = np.ascontiguousarray(S8, np.float64).reshape(-1, 8).copy()
        fx = np.ascontiguousarray(fixed, np.uint8); fs = np.ascontiguousarray(fix_scale, np.uint8)
        v0 = np.ascontiguousarray(e_v0, np.int32); v1 = np.ascontiguousarray(e_v1, np.int32)
        M = np.ascontiguousarray(meas8, np.float64).reshape(-1, 8)
        if len(fx) != len(S) or len(fs) != len(S) or len(v1) != len(v0) or len(M) != len(v0):
            raise ValueError("essential_graph: array lengths disagree")
        stats = np.zeros(4, np.int32); trace = np.full(max(int(n_iterations), 0) + 1, np.nan)
        sp = capi.ptr(stop_flag) if stop_flag is not None else None
        rc = self._lib.rumi_essential_graph(self._h, len(S), capi.ptr(S), capi.ptr(fx), capi.ptr(fs), len(v0), capi.ptr(v0), capi.ptr(v1), capi.ptr(M),
                                            int(n_iterations), sp, capi.ptr(stats), capi.ptr(trace))
        capi.check(rc)
        return S, stats, trace

    def correct_points(self, X, ref, tab_a, tab_b, mode=0):
        """The point correction that ends both overloads (rumi_sim3_correct_points).  mode 0: Sim3 tables [n_v,8] double (Srw, correctedSwr);
        mode 1: SE(3) tables [n_v,7] float (Twr, TNonCorrectedwr).  Returns X [n,3] float32."""
        X = np.ascontiguousarray(X, np.float32).reshape(-1, 3).copy(); ref = np.ascontiguousarray(ref, np.int32)
        dt, w = (np.float64, 8) if mode == 0 else (np.float32, 7)
        A = np.ascontiguousarray(tab_a, dt).reshape(-1, w); B = np.ascontiguousarray(tab_b, dt).reshape(-1, w)
        if len(ref) != len(X) or len(A) != len(B):
            raise ValueError("correct_points: array lengths disagree")
        capi.check(self._lib.rumi_sim3_correct_points(self._h, int(mode), len(X), capi.ptr(X), capi.ptr(ref), len(A), capi.ptr(A), capi.ptr(B)))
        return X

    def set_profiling(self, on=True):
        capi.check(self._lib.rumi_opt_set_profiling(self._h, int(on)))

    def kernel_ms(self):
        """Per-kernel device time of the last bundle adjustment run with profiling on: dict(hpp, syrk, solve in ms over the call, trials)."""
        ms = np.zeros(4, np.float32)
        capi.check(self._lib.rumi_opt_kernel_ms(self._h, capi.ptr(ms)))
        return dict(hpp=float(ms[0]), syrk=float(ms[1]), solve=float(ms[2]), trials=int(ms[3]))

    def footprint(self):
        """(device bytes, pinned host bytes) the handle owns right now: the sum over its buffers (include/rumi_opt.h states the expressions)."""
        out = np.zeros(2, np.int64)
        capi.check(self._lib.rumi_opt_footprint(self._h, capi.ptr(out)))
        return int(out[0]), int(out[1])

    def stage_ms(self):
        ms = np.zeros(8, np.float32)
        capi.check(self._lib.rumi_opt_stage_ms(self._h, capi.ptr(ms)))
        return ms
