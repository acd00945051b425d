"""Streaming front-end over the C ABI (include/rumi_orb.h, RumiOrbStream): one call per camera frame that extracts it and brute-force
matches it against the previous frame, which stays resident on the device."""
import ctypes as C

import numpy as np

from . import capi
from .capi import KP_DTYPE, RumiStreamFrame


class FrameStream:
    def __init__(self, extractor):
        self._ext = extractor                 # the stream lives on the extractor's handle: keep it alive
        self._lib = extractor._lib
        self.cap = extractor.nfeatures + 4 * extractor.nlevels + 64
        self._s = C.c_void_p()
        capi.check(self._lib.rumi_orb_stream_create(extractor._h, C.byref(self._s)))
        self.n_prev = 0

    def close(self):
        if getattr(self, "_s", None) is not None and self._s.value:
            if self._ext._h.value:            # (an extractor closed first has taken the device arenas' context with it; the stream's blocks are freed here all the same)
                self._lib.rumi_orb_stream_destroy(self._s)
            self._s = C.c_void_p()

    __del__ = close

    def push(self, img, lap=(0, 1000)):
        """Returns (monoIndex, keypoints[KP_DTYPE], descriptors [n,32] u8, best_idx, best_dist, second_dist [n] i32) as copies: the frame's
        features and their matches in the previous frame (self.n_prev of its key-points; 0: no previous frame, every best_idx is -1).
        An empty image raises RumiError with code RUMI_E_EMPTY and leaves the previous frame in place."""
        f = RumiStreamFrame()
        if img is None or img.size == 0:
            capi.check(self._lib.rumi_orb_stream_push(self._s, None, 0, 0, 0, int(lap[0]), int(lap[1]), C.byref(f)))
        assert img.dtype == np.uint8 and img.ndim == 2, "CV_8UC1 expected"
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        h, w = img.shape
        capi.check(self._lib.rumi_orb_stream_push(self._s, capi.ptr(img), w, h, img.strides[0], int(lap[0]), int(lap[1]), C.byref(f)))
        n = f.n
        self.n_prev = f.n_prev

        def view(p, dt, shape):
            return np.ctypeslib.as_array((C.c_uint8 * (int(np.prod(shape)) * np.dtype(dt).itemsize)).from_address(p)).view(dt).reshape(shape).copy()
        if n == 0:
            z = np.zeros(0, np.int32)
            return f.mono, np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8), z, z.copy(), z.copy()
        return (f.mono, view(f.kp, KP_DTYPE, (n,)), view(f.desc, np.uint8, (n, 32)), view(f.best_idx, np.int32, (n,)),
                view(f.best_dist, np.int32, (n,)), view(f.second_dist, np.int32, (n,)))

    def reset(self):
        """Forget the previous frame: the next push behaves as a first one."""
        capi.check(self._lib.rumi_orb_stream_reset(self._s))

    def resident(self):
        """The current frame where it lies on the device, as torch views (no copy): kp [cap,7] f32 (the 28-byte records), desc [cap,32] u8,
        counts [2] i32 = (n, monoIndex).  Valid until the push after the next one overwrites the slot."""
        import torch
        kp, desc, counts = C.c_void_p(), C.c_void_p(), C.c_void_p()
        capi.check(self._lib.rumi_orb_stream_resident(self._s, C.byref(kp), C.byref(desc), C.byref(counts)))
        dev = torch.device("cuda", torch.cuda.current_device())

        def tensor(p, nbytes, dt, shape):
            iface = {"shape": (nbytes,), "typestr": "|u1", "data": (p, False), "version": 3}
            holder = type("_DevBlock", (), {"__cuda_array_interface__": iface})()
            return torch.as_tensor(holder, device=dev).view(dt).reshape(shape)
        return (tensor(kp.value, self.cap * 28, torch.float32, (self.cap, 7)), tensor(desc.value, self.cap * 32, torch.uint8, (self.cap, 32)),
                tensor(counts.value, 8, torch.int32, (2,)))
