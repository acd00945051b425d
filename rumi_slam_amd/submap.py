"""Host-side mirror of the key-point match of ``CloudMerging::ComputeSubmapSim3`` (R/lib_src/CloudMerging.cc:503-551) over
``rumi_submap_match`` (include/rumi_match.h): every matched key-frame pair of the two sub-maps in one call.

A key-frame is a ``SubmapFrame``: ``mvKeys`` and ``mvKeysUn`` as [n, 2] float arrays, one flag per slot (does it hold a map point), and the
grid's origin and inverse cell sizes.  The arrays are numpy arrays, or torch tensors on the GPU that the call then reads in place, for example
``record_views(records, cap)[0][f, :n, :2].contiguous()`` of the queue's gathered records."""
import ctypes as C

import numpy as np

from . import capi

GRID_COLS, GRID_ROWS, MAX_KEYPOINTS = 64, 48, 16384


class RumiSubmapFrame(C.Structure):
    _fields_ = [("n", C.c_int32), ("keys_xy", C.c_void_p), ("keys_un_xy", C.c_void_p), ("has_mp", C.c_void_p), ("min_x", C.c_float),
                ("min_y", C.c_float), ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float), ("on_device", C.c_int32)]


def _lib():
    L = capi.lib()
    if getattr(L, "_submap_ready", False):
        return L
    vp, i32 = C.c_void_p, C.c_int32
    L.rumi_match_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
    L.rumi_match_destroy.argtypes = [vp]
    L.rumi_match_destroy.restype = None
    L.rumi_submap_match.argtypes = [vp, i32, vp, i32, vp, vp, C.c_float, vp, vp, vp]
    L._submap_ready = True
    return L


def grid_inverse(min_x, min_y, max_x, max_y):
    """mfGridElementWidthInv, mfGridElementHeightInv as Frame.cc:322-323 forms them: float(cols) / float(max - min)."""
    return (float(np.float32(GRID_COLS) / np.float32(np.float32(max_x) - np.float32(min_x))),
            float(np.float32(GRID_ROWS) / np.float32(np.float32(max_y) - np.float32(min_y))))


def _is_tensor(a):
    return hasattr(a, "data_ptr")


class SubmapFrame:
    """What the match reads of one key-frame (keeps the arrays alive).  keys_un_xy None: the key-points are not distorted, mvKeysUn = mvKeys."""

    def __init__(self, keys_xy, has_mp, keys_un_xy=None, min_x=0.0, min_y=0.0, max_x=640.0, max_y=480.0, grid_inv=None):
        self.on_device = _is_tensor(keys_xy)
        if self.on_device:
            import torch
            arrays = [keys_xy, has_mp] + ([keys_un_xy] if keys_un_xy is not None else [])
            assert all(_is_tensor(a) and a.is_cuda and a.is_contiguous() for a in arrays), "device form: every array is a contiguous tensor on the GPU"
            assert keys_xy.dtype == torch.float32 and has_mp.dtype in (torch.uint8, torch.bool) and (keys_un_xy is None or keys_un_xy.dtype == torch.float32)
            self.keys, self.un, self.mp = keys_xy, keys_un_xy, has_mp
            self.n = int(keys_xy.shape[0])
            assert tuple(keys_xy.shape) == (self.n, 2) and has_mp.numel() == self.n and (keys_un_xy is None or tuple(keys_un_xy.shape) == (self.n, 2))
            p = lambda a: a.data_ptr() if a is not None and a.numel() else None
        else:
            self.keys = np.ascontiguousarray(keys_xy, np.float32).reshape(-1, 2)
            self.un = None if keys_un_xy is None else np.ascontiguousarray(keys_un_xy, np.float32).reshape(-1, 2)
            self.mp = np.ascontiguousarray(np.asarray(has_mp) != 0, np.uint8)
            self.n = len(self.keys)
            assert len(self.mp) == self.n and (self.un is None or len(self.un) == self.n)
            p = lambda a: a.ctypes.data if a is not None and a.size else None
        self.min_x, self.min_y = float(min_x), float(min_y)
        self.grid_inv = tuple(float(v) for v in (grid_inv if grid_inv is not None else grid_inverse(min_x, min_y, max_x, max_y)))
        self.c = RumiSubmapFrame(self.n, p(self.keys), p(self.un), p(self.mp), self.min_x, self.min_y, self.grid_inv[0], self.grid_inv[1], int(self.on_device))


class SubmapResult:
    """best2[p]: per key-point of pair p's key-frame 1, the key-point of key-frame 2 it keeps (-1 none); matches[p]: [k, 2] (i1, i2) in ascending
    i1 (vpMatchedKeyPoints12 = vpValidMatchedKeyPoints12); counts[p] = matchNum; total = matchMapPointNum."""

    def __init__(self, best2, matches, counts, pair_start):
        self.best2, self.matches, self.counts, self.pair_start = best2, matches, counts, pair_start
        self.total = int(pair_start[-1])


class SubmapMatcher:
    def __init__(self, device=-1):
        self._lib = _lib()
        self._h = C.c_void_p()
        capi.check(self._lib.rumi_match_create(1, 1, device, C.byref(self._h)))       # the call's own arenas grow on demand

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.rumi_match_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def match(self, frames, pairs, tolerance=3.0):
        """frames: the table of SubmapFrame; pairs: (index of key-frame 1, index of key-frame 2) in the order of mKfMatch12."""
        rc, best2, pair_start, matches = submap_status(self._h, frames, pairs, tolerance)
        capi.check(rc)
        q = np.concatenate([[0], np.cumsum([frames[a].n for a, _ in pairs])]).astype(np.int64)
        return SubmapResult([best2[q[p]:q[p + 1]] for p in range(len(pairs))],
                            [matches[pair_start[p]:pair_start[p + 1]] for p in range(len(pairs))], np.diff(pair_start).astype(np.int32), pair_start)


def submap_status(handle, frames, pairs, tolerance, fill=0x77):
    """The raw call: (status, best2, pair_start, matches) over output arrays that held ``fill`` in every byte.  ``handle`` may be None: the
    validation comes before anything that needs the matcher."""
    L = _lib()
    n = len(frames)
    table = (RumiSubmapFrame * max(n, 1))(*[f.c for f in frames])
    f1 = np.array([a for a, _ in pairs], np.int32)
    f2 = np.array([b for _, b in pairs], np.int32)
    q = sum(max(frames[a].n, 0) for a, _ in pairs if 0 <= a < n)
    fillv = np.uint8(fill)
    best2 = np.full(q + 1, fillv, np.uint8).repeat(4).view(np.int32)
    pair_start = np.full(len(pairs) + 1, fillv, np.uint8).repeat(4).view(np.int32)
    matches = np.full(2 * q + 2, fillv, np.uint8).repeat(4).view(np.int32).reshape(-1, 2)
    rc = L.rumi_submap_match(handle, n, C.cast(table, C.c_void_p), len(pairs), capi.ptr(f1), capi.ptr(f2), float(tolerance),
                             capi.ptr(best2), capi.ptr(pair_start), capi.ptr(matches))
    return rc, best2[:q] if rc == capi.RUMI_OK else best2, pair_start, matches


# ---- the alignment session of ComputeSubmapSim3: resident score set, every RANSAC solver in one call (include/rumi_opt.h) ----------------
SUBMAP_SOLVER_DTYPE = np.dtype([("first", "<i4"), ("n", "<i4"), ("min_inliers", "<i4"), ("its", "<i4"), ("fix_scale", "<i4"), ("K4_1", "<f4", 4),
                                ("K4_2", "<f4", 4), ("pad", "<i4"), ("S_kf1w", "<f8", 8), ("S_kf2w", "<f8", 8)])
SUBMAP_RESULT_DTYPE = np.dtype([("state", "<i4"), ("its", "<i4"), ("best_hyp", "<i4"), ("best_inliers", "<i4"), ("best_ratio_after", "<f4"),
                                ("T12", "<f4", 16)])
assert SUBMAP_SOLVER_DTYPE.itemsize == 184 and SUBMAP_RESULT_DTYPE.itemsize == 84
SCORE_KEYS = ("pair_start", "pair_denominator", "S_c1w1", "S_c2w2", "S_kf1w", "S_kf2w", "K4_1", "K4_2", "X1", "X2", "kp1", "kp2", "sigma2_1", "sigma2_2",
              "edge1", "edge2")


class SubmapSolver:
    """One Sim3Solver of CloudMerging.cc:663-741 as the session takes it: the correspondences its constructor keeps (as rumi_slam_amd.sim3solver.Sim3Solver),
    g2o::Sim3(R, t, 1.0) of its two key-frames as 8 doubles, mRansacMinInliers and mRansacMaxIts after SetRansacParameters."""

    def __init__(self, X3Dc1, X3Dc2, sigma2_1, sigma2_2, K4_1, K4_2, S_kf1w, S_kf2w, min_inliers, its, fix_scale=False):
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        self.X1, self.X2, self.s1, self.s2 = f32(X3Dc1).reshape(-1, 3), f32(X3Dc2).reshape(-1, 3), f32(sigma2_1), f32(sigma2_2)
        self.K1, self.K2 = f32(K4_1), f32(K4_2)
        self.S_kf1w, self.S_kf2w = np.ascontiguousarray(S_kf1w, np.float64), np.ascontiguousarray(S_kf2w, np.float64)
        self.N, self.min_inliers, self.its, self.fix_scale = len(self.X1), int(min_inliers), int(its), bool(fix_scale)


def draw_stream(solvers, rng):
    """The minimal sets of every solver's iterations, flat in solver order, drawn from the one generator exactly as Sim3Solver.cc:321-331 (the
    generator ends after the last solver's last draw)."""
    tri = np.zeros((sum(s.its for s in solvers), 3), np.int32)
    h = 0
    for s in solvers:
        for _ in range(s.its):
            avail = list(range(s.N))
            for i in range(3):
                r = rng.RandomInt(0, len(avail) - 1)
                tri[h, i] = avail[r]
                avail[r] = avail[-1]
                avail.pop()
            h += 1
    return tri


class SubmapSim3:
    """begin(score) once, then score(S_list) and ransac(solvers, rng) on the resident set, end().  ``optimizer``: a rumi_slam_amd.optimizer.Optimizer."""

    def __init__(self, optimizer):
        from .optimizer import RumiSim3ScoreSet, _lib as opt_lib
        self._opt, self._lib, self._Set = optimizer, opt_lib(), RumiSim3ScoreSet
        vp, i32 = C.c_void_p, C.c_int32
        self._lib.rumi_submap_sim3_begin.argtypes = [vp, vp]
        self._lib.rumi_submap_sim3_end.argtypes = [vp]
        self._lib.rumi_submap_sim3_score.argtypes = [vp, i32, vp, vp, vp, vp, vp]
        self._lib.rumi_submap_sim3_ransac.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp]
        self.n_pairs = self.total = 0

    def set_chunk(self, chunk):
        """Test hook: iterations between two read-backs of the rule's state (0: the default; None: the whole stream as one chunk)."""
        capi.check(capi.hooks().rumi_hook_submap_sim3_set_chunk(self._opt._h, (1 << 30) if chunk is None else int(chunk)))

    def begin(self, score):
        """score: the dict Optimizer.Sim3Ransac takes (S_kf1w / S_kf2w are not read and may be absent)."""
        dt = dict(pair_start=np.int32, pair_denominator=np.int32, S_c1w1=np.float64, S_c2w2=np.float64, S_kf1w=np.float64, S_kf2w=np.float64, edge1=np.uint8,
                  edge2=np.uint8)
        keep = [np.ascontiguousarray(score[k], dt.get(k, np.float32)) if score.get(k) is not None else None for k in SCORE_KEYS]
        sc = self._Set(len(keep[0]) - 1, *[a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None for a in keep])
        capi.check(self._lib.rumi_submap_sim3_begin(self._opt._h, C.byref(sc)))
        self.n_pairs, self.total = len(keep[0]) - 1, int(keep[0][-1])

    def end(self):
        capi.check(self._lib.rumi_submap_sim3_end(self._opt._h))

    def score(self, S_list, want_inliers=True):
        """ComputeInliersNum of every (S_c1w2 [n_pairs, 8], S_c2w1 [n_pairs, 8]) of S_list.  Returns (median [n_S], ratio [n_S, n_pairs],
        inliers [n_S, total] uint8 or None)."""
        A = np.ascontiguousarray([a for a, _ in S_list], np.float64).reshape(len(S_list), -1, 8)
        B = np.ascontiguousarray([b for _, b in S_list], np.float64).reshape(len(S_list), -1, 8)
        n_S = len(S_list)
        if n_S and (A.shape[1] != self.n_pairs or B.shape[1] != self.n_pairs):
            raise ValueError("SubmapSim3.score: one composed transform per key-frame pair and side")
        med = np.zeros(max(n_S, 1), np.float32); ratio = np.zeros((max(n_S, 1), max(self.n_pairs, 1)), np.float32)
        inl = np.zeros((max(n_S, 1), max(self.total, 1)), np.uint8) if want_inliers else None
        P = lambda a: None if a is None else capi.ptr(a)
        capi.check(self._lib.rumi_submap_sim3_score(self._opt._h, n_S, P(A), P(B), P(inl), P(ratio), P(med)))
        return med[:n_S], ratio[:n_S, :self.n_pairs], None if inl is None else inl[:n_S, :self.total]

    def ransac_status(self, solvers, triples, best_ratio=0.0, want_all=False, fill=0):
        """The raw call over output arrays that held ``fill`` in every byte: (status, dict).  ``solvers``: SubmapSolver objects or a prepared
        (records, X1, X2, s1, s2) tuple."""
        if isinstance(solvers, tuple):
            rec, X1, X2, s1, s2 = solvers
        else:
            rec = np.zeros(len(solvers), SUBMAP_SOLVER_DTYPE)
            first = 0
            for r, s in zip(rec, solvers):
                r["first"], r["n"], r["min_inliers"], r["its"], r["fix_scale"] = first, s.N, s.min_inliers, s.its, int(s.fix_scale)
                r["K4_1"], r["K4_2"], r["S_kf1w"], r["S_kf2w"] = s.K1, s.K2, s.S_kf1w, s.S_kf2w
                first += s.N
            cat = lambda name, w: (np.concatenate([getattr(s, name) for s in solvers]) if solvers else np.zeros((0,) + w, np.float32))
            X1, X2, s1, s2 = cat("X1", (3,)), cat("X2", (3,)), cat("s1", ()), cat("s2", ())
        tri = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
        J, H = len(rec), len(tri)
        f = lambda n, dt: np.frombuffer(bytes([fill]) * (max(int(n), 1) * np.dtype(dt).itemsize), dt).copy()
        res = f(J, SUBMAP_RESULT_DTYPE); used = f(1, np.int32)
        nall, mall, Tall = (f(H, np.int32), f(H, np.float32), f(H * 16, np.float32)) if want_all else (None, None, None)
        P = lambda a: None if a is None else capi.ptr(a)
        rc = self._lib.rumi_submap_sim3_ransac(self._opt._h, J, P(rec), len(X1), P(X1), P(X2), P(s1), P(s2), P(tri), float(best_ratio), P(res), P(used),
                                               P(nall), P(mall), P(Tall))
        out = dict(results=res[:J], its_consumed=int(used[0]), raw_used=used)
        for k in SUBMAP_RESULT_DTYPE.names:
            out[k] = res[k][:J]
        if want_all:
            out.update(n_inliers_all=nall[:H], median_all=mall[:H], T12_all=Tall[:H * 16].reshape(H, 16))
        return rc, out

    def ransac(self, solvers, rng, best_ratio=0.0, want_all=False):
        """The loop of CloudMerging.cc:643-741 over ``solvers`` (SubmapSolver, in the order upstream visits them; the caller leaves out those with
        N < min_inliers).  Draws every solver's minimal sets from ``rng`` and leaves it where upstream's loop leaves rand(): after the draws of
        the last consumed iteration.  Returns the result dict: per solver state, its, best_hyp, best_inliers, best_ratio_after, T12; its_consumed;
        converged = index of the solver that converged or None; best_ratio = the shared ratio at the end."""
        from .optimizer import SIM3_CONVERGED
        start = rng.state()
        tri = draw_stream(solvers, rng)
        rc, out = self.ransac_status(solvers, tri, best_ratio, want_all)
        rng.set_state(start)
        capi.check(rc)
        rng.advance(out["its_consumed"])
        conv = np.flatnonzero(out["state"] == SIM3_CONVERGED)
        out["converged"] = int(conv[0]) if len(conv) else None
        out["best_ratio"] = float(out["best_ratio_after"][-1]) if len(solvers) else float(best_ratio)
        out["triples"] = tri
        return out
