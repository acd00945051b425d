"""Host-side mirror of the reference's ``KFDSample`` (R/include/cloud_edge_slam_lib/KFDSample.h:55-84) over the C ABI (include/rumi_kfd.h): the PD
frame selector that decides, while tracking is lost, which camera frames enter the rumination queue.  One ``step`` per frame: pyramidal LK flow of the
last selection's key-points, mean flow magnitude, PD threshold, and the ORB extraction of a selected frame, all on the device."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi
from .capi import KP_DTYPE, RumiKfdStep


@dataclass
class KFDStep:
    selected: bool
    n_tracked: int
    n_good: int
    moptf: float            # numpy float32 scalars: the bits the C entry returned
    pd_out: float
    th: float
    next: np.ndarray        # [n_tracked, 2] f32
    status: np.ndarray      # [n_tracked] u8
    mono: int               # selected frames: what ORBextractor.__call__(frame, None, (0, 0)) returns ...
    keypoints: np.ndarray   # ... [n] KP_DTYPE
    descriptors: np.ndarray  # ... [n, 32] u8


def _frame_args(img):
    assert img.dtype == np.uint8 and (img.ndim == 2 or img.ndim == 3), "CV_8UC1 or CV_8UC3 expected"
    ch = 1 if img.ndim == 2 else img.shape[2]
    if img.strides[-1] != 1 or (img.ndim == 3 and img.strides[1] != ch):
        img = np.ascontiguousarray(img)
    return img, img.shape[1], img.shape[0], img.strides[0], ch


def _view(p, dt, shape):
    n = int(np.prod(shape)) * np.dtype(dt).itemsize
    if n == 0:
        return np.zeros(shape, dt)
    return np.ctypeslib.as_array((C.c_uint8 * n).from_address(p)).view(dt).reshape(shape).copy()


class KFDSampler:
    """KFDSample on extractor ``extractor`` (the reference builds ORBextractor(2000, 1.2, 8, 20, 7)); Kp, Kd, th start at its 0.8, 0.005, 10."""

    def __init__(self, extractor, Kp=0.8, Kd=0.005, th=10.0):
        self._ext = extractor                     # the sampler lives on the extractor's handle: keep it alive
        self._lib = capi.kfd_lib()
        self._s = C.c_void_p()
        capi.check(self._lib.rumi_kfd_create(extractor._h, C.byref(self._s)))
        self.set_pd(Kp, Kd, th)

    def close(self):
        if getattr(self, "_s", None) is not None and self._s.value:
            if self._ext._h.value:
                self._lib.rumi_kfd_destroy(self._s)
            self._s = C.c_void_p()

    __del__ = close

    def set_pd(self, Kp, Kd, th):
        """KFDSample::SetPDKFselectorParams"""
        capi.check(self._lib.rumi_kfd_set_pd(self._s, float(Kp), float(Kd), float(th)))

    def reset(self):
        """KFDSample::Reset: the next step is a first step; the controller keeps its previous input."""
        capi.check(self._lib.rumi_kfd_reset(self._s))

    def step(self, img, timestamp):
        """KFDSample::Step.  img: [H, W] u8 grey or [H, W, 3] u8 BGR.  Returns a KFDStep (copies).  Raises RumiError (RUMI_E_EMPTY for an empty image,
        RUMI_E_INVALID for a wrong size or channel count) and then leaves the sampler as it was."""
        out = RumiKfdStep()
        if img is None or img.size == 0:
            capi.check(self._lib.rumi_kfd_step(self._s, None, 0, 0, 0, 1, float(timestamp), C.byref(out)))
        img, w, h, stride, ch = _frame_args(img)
        capi.check(self._lib.rumi_kfd_step(self._s, capi.ptr(img), w, h, stride, ch, float(timestamp), C.byref(out)))
        nt, n = out.n_tracked, out.n if out.selected else 0
        f32 = lambda v: np.float32(v)
        return KFDStep(bool(out.selected), nt, out.n_good, f32(out.moptf), f32(out.pd_out), f32(out.th), _view(out.next, np.float32, (nt, 2)),
                       _view(out.status, np.uint8, (nt,)), out.mono, _view(out.kp, KP_DTYPE, (n,)), _view(out.desc, np.uint8, (n, 32)))

    @staticmethod
    def track(prev, cur, pts, dumps=False, device=-1):
        """rumi_kfd_track: the flow alone.  pts [n, 2] f32 followed from frame `prev` into `cur` -> (next [n, 2] f32, status [n] u8), and with dumps
        also the three LK levels of `prev` (list of [h, w] u8) and their Scharr derivatives (list of [h, w, 2] i16)."""
        lib = capi.kfd_lib()
        prev, w, h, stride, ch = _frame_args(prev)
        cur, w2, h2, stride2, ch2 = _frame_args(cur)
        assert (w, h, ch) == (w2, h2, ch2), "two frames of one size"
        if stride2 != stride:
            prev, cur = np.ascontiguousarray(prev), np.ascontiguousarray(cur)
            stride = prev.strides[0]
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = len(pts)
        nxt, status = np.zeros((max(n, 1), 2), np.float32), np.zeros(max(n, 1), np.uint8)
        sizes = [(h, w)]
        for _ in range(2):
            sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
        total = sum(a * b for a, b in sizes)
        pyr = np.zeros(total if dumps else 1, np.uint8)
        der = np.zeros(2 * total if dumps else 1, np.int16)
        capi.check(lib.rumi_kfd_track(int(device), capi.ptr(prev), capi.ptr(cur), w, h, stride, ch, capi.ptr(pts), n, capi.ptr(nxt), capi.ptr(status),
                                      capi.ptr(pyr) if dumps else None, capi.ptr(der) if dumps else None))
        if not dumps:
            return nxt[:n], status[:n]
        levels, derivs, o = [], [], 0
        for a, b in sizes:
            levels.append(pyr[o:o + a * b].reshape(a, b))
            derivs.append(der[2 * o:2 * (o + a * b)].reshape(a, b, 2))
            o += a * b
        return nxt[:n], status[:n], levels, derivs
