"""Host-side mirror of ``LocalMapping::CreateNewMapPoints`` (R/lib_src/LocalMapping.cc:354-647, monocular pinhole) over the C ABI in
include/rumi_mapping.h: one call for the current key-frame and all of its neighbours."""
import ctypes as C

import numpy as np

from . import capi
from .matcher import FeatureVector, FrameView, RumiFeatureVector, RumiFrameFeatures

MAX_NEIGH = 64

NEWPOINT_DTYPE = np.dtype([("neigh", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("x3D", "<f4", 3)])
assert NEWPOINT_DTYPE.itemsize == 24


class RumiNewPointsKF(C.Structure):
    _fields_ = [("feat", RumiFrameFeatures), ("fv", RumiFeatureVector), ("kf_mp", C.c_void_p), ("mp_pos", C.c_void_p), ("K4", C.c_float * 4),
                ("Tcw", C.c_float * 12), ("Ow", C.c_float * 3), ("F12", C.c_float * 9), ("epipole2", C.c_float * 2)]


class RumiNewPointsParams(C.Structure):
    _fields_ = [("coarse", C.c_int32), ("check_orientation", C.c_int32), ("far_points", C.c_int32), ("th_far_points", C.c_float),
                ("ratio_factor", C.c_float)]


def _lib():
    L = capi.lib()
    if getattr(L, "_mapping_ready", False):
        return L
    vp, i32 = C.c_void_p, C.c_int32
    L.rumi_create_new_map_points.argtypes = [vp, vp, vp, i32, vp, vp, i32, C.POINTER(i32), vp, vp]
    L.rumi_hook_newpts_matches.argtypes = [vp, i32, i32, vp]
    L._mapping_ready = True
    return L


class KeyFrameView:
    """What CreateNewMapPoints reads of a KeyFrame (keeps the arrays alive).  ``Tcw`` is the 3x4 pose, ``Ow`` the camera centre; a neighbour
    also carries ``mp_pos`` ([n, 3] world position of each feature's map point, read where ``kf_mp >= 0``), ``F12`` and ``epipole2``."""

    def __init__(self, frame: FrameView, fv: FeatureVector, kf_mp, K4, Tcw, Ow, mp_pos=None, F12=None, epipole2=None):
        self.frame, self.fv = frame, fv
        self.kf_mp = np.ascontiguousarray(kf_mp, np.int32)
        self.mp_pos = None if mp_pos is None else np.ascontiguousarray(mp_pos, np.float32).reshape(-1, 3)
        assert len(self.kf_mp) == frame.n and (self.mp_pos is None or len(self.mp_pos) == frame.n)
        self.K4 = np.ascontiguousarray(K4, np.float32).reshape(4)
        self.Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(12)
        self.Ow = np.ascontiguousarray(Ow, np.float32).reshape(3)
        self.F12 = np.zeros(9, np.float32) if F12 is None else np.ascontiguousarray(F12, np.float32).reshape(9)
        self.epipole2 = np.zeros(2, np.float32) if epipole2 is None else np.ascontiguousarray(epipole2, np.float32).reshape(2)

    def fill(self, c):
        c.feat, c.fv = self.frame.c, self.fv.c
        c.kf_mp = self.kf_mp.ctypes.data
        c.mp_pos = None if self.mp_pos is None else self.mp_pos.ctypes.data
        c.K4[:], c.Tcw[:], c.Ow[:], c.F12[:], c.epipole2[:] = self.K4.tolist(), self.Tcw.tolist(), self.Ow.tolist(), self.F12.tolist(), self.epipole2.tolist()
        return c


def pack(cur, neighbours):
    """(RumiNewPointsKF, array of RumiNewPointsKF) for the C entry (and for the test oracle, which takes the same structs)."""
    c = cur.fill(RumiNewPointsKF())
    arr = (RumiNewPointsKF * max(len(neighbours), 1))()
    for k, nb in enumerate(neighbours):
        nb.fill(arr[k])
    return c, arr


def CreateNewMapPoints(matcher, cur, neighbours, ratio_factor, coarse=False, far_points=False, th_far_points=0.0, cap=None):
    """Returns (points as NEWPOINT_DTYPE in creation order, count per neighbour, baseline-skip flag per neighbour).  ``matcher`` is an
    ``ORBmatcher`` (its mbCheckOrientation is used; the reference constructs this member's matcher with False)."""
    L = _lib()
    c, arr = pack(cur, neighbours)
    n = len(neighbours)
    prm = RumiNewPointsParams(int(coarse), int(matcher.mbCheckOrientation), int(far_points), float(th_far_points), float(ratio_factor))
    cap = cur.frame.n if cap is None else int(cap)
    out = np.zeros(max(cap, 1), NEWPOINT_DTYPE)
    per = np.zeros(max(n, 1), np.int32)
    skipped = np.zeros(max(n, 1), np.uint8)
    n_out = C.c_int32()
    capi.check(L.rumi_create_new_map_points(matcher._h, C.byref(c), C.byref(arr) if n else None, n, C.byref(prm), capi.ptr(out), cap, C.byref(n_out),
                                            capi.ptr(per), capi.ptr(skipped)))
    return out[:n_out.value], per[:n], skipped[:n]


def last_matches(matcher, n_neigh, n1):
    """Test hook: [n_neigh, n1] the neighbour feature each current feature was paired with when the loop reached that neighbour (-1 none)."""
    out = np.full((n_neigh, n1), -1, np.int32)
    capi.check(_lib().rumi_hook_newpts_matches(matcher._h, n_neigh, n1, capi.ptr(out)))
    return out
