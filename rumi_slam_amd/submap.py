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
