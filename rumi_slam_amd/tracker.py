"""Host-side mirror of include/rumi_track.h: one device-resident Tracking step (TrackWithMotionModel + TrackLocalMap data path,
R/lib_src/Tracking.cc:2441-2607, 2996-3055) behind one call."""
import ctypes as C

import time

import numpy as np

from . import capi
from .capi import KP_DTYPE, RumiOrbConfig


class RumiTrackPoints(C.Structure):
    _fields_ = [("n", C.c_int32), ("pos", C.c_void_p), ("normal", C.c_void_p), ("min_dist", C.c_void_p), ("max_dist", C.c_void_p),
                ("desc", C.c_void_p), ("obs", C.c_void_p), ("bad", C.c_void_p), ("local", C.c_void_p),
                ("stale_in_view", C.c_void_p), ("stale_proj", C.c_void_p)]       # optional: points["stale_in_view"] [n] u8, points["stale_proj"] [n,5] f32


def _stale(points, a):
    """The optional stale-mbTrackInView arrays of include/rumi_track.h (RumiTrackPoints.stale_in_view / stale_proj) as two pointers (None, None when absent)."""
    if points.get("stale_in_view") is None:
        return None, None
    a["stale_in"] = np.ascontiguousarray(points["stale_in_view"], np.uint8)
    a["stale_proj"] = np.ascontiguousarray(points["stale_proj"], np.float32).reshape(-1, 5)
    assert len(a["stale_in"]) == len(a["stale_proj"]) == len(points["obs"])
    return capi.ptr(a["stale_in"]), capi.ptr(a["stale_proj"])


class RumiTrackResult(C.Structure):
    _fields_ = [("n", C.c_int32), ("mono_index", C.c_int32), ("th_motion", C.c_int32), ("nmatches_motion", C.c_int32), ("ngood_motion", C.c_int32),
                ("nmatches_map", C.c_int32), ("n_to_match", C.c_int32), ("nmatches_local", C.c_int32), ("ngood_local", C.c_int32),
                ("matches_inliers", C.c_int32), ("Tcw_motion", C.c_float * 7), ("Tcw", C.c_float * 7), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3),
                ("Ow", C.c_float * 3)]


class RumiRelocCandidate(C.Structure):
    _fields_ = [("nkf", C.c_int32), ("kf_keys", C.c_void_p), ("kf_mp", C.c_void_p), ("matches", C.c_void_p)]


class RumiRelocParams(C.Structure):
    _fields_ = [("min_good", C.c_int32), ("enough", C.c_int32), ("retry_above", C.c_int32), ("th_coarse", C.c_float), ("dist_coarse", C.c_int32),
                ("th_fine", C.c_float), ("dist_fine", C.c_int32), ("check_orientation", C.c_int32)]


class RumiRelocHypothesis(C.Structure):
    _fields_ = [("cand", C.c_int32), ("Tcw7", C.c_float * 7), ("inliers", C.c_void_p)]


class RumiRelocResult(C.Structure):
    _fields_ = [("ran", C.c_int32), ("ngood", C.c_int32 * 3), ("nadditional", C.c_int32 * 2), ("ngood_final", C.c_int32), ("Tcw", C.c_float * 7)]


RELOC_MAX_HYPOTHESES = 256          # RUMI_RELOC_MAX_HYPOTHESES of include/rumi_track.h
RELOC_RESULT_DTYPE = np.dtype([("ran", "<i4"), ("ngood", "<i4", 3), ("nadditional", "<i4", 2), ("ngood_final", "<i4"), ("Tcw", "<f4", 7)])
assert RELOC_RESULT_DTYPE.itemsize == C.sizeof(RumiRelocResult)


def _bind(L):
    if getattr(L, "_track_ready", False):
        return L
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    L.rumi_track_create.argtypes = [C.POINTER(RumiOrbConfig), i32, i32, C.POINTER(vp)]
    L.rumi_track_destroy.argtypes = [vp]
    L.rumi_track_destroy.restype = None
    L.rumi_track_frame.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, C.POINTER(RumiTrackPoints), f32, f32, i32, f32,
                                   vp, vp, i32, vp, vp, vp, vp, C.POINTER(RumiTrackResult)]
    L.rumi_track_extract.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.rumi_track_motion.argtypes = [vp, vp, vp, vp, i32, vp, vp, C.POINTER(RumiTrackPoints), f32, vp, vp, C.POINTER(RumiTrackResult)]
    L.rumi_track_reference_keyframe.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, C.POINTER(RumiTrackPoints), f32, i32, vp, vp, vp, vp, vp,
                                                C.POINTER(RumiTrackResult)]
    L.rumi_track_local.argtypes = [vp, vp, vp, vp, C.POINTER(RumiTrackPoints), vp, f32, i32, f32, vp, vp, vp, C.POINTER(RumiTrackResult)]
    L.rumi_track_local_map.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, f32, i32, f32, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp,
                                       C.POINTER(RumiTrackResult)]
    L.rumi_track_last_projections.argtypes = [vp, i32, vp]
    L.rumi_track_set_distortion.argtypes = [vp, vp, vp]
    L.rumi_track_undistorted.argtypes = [vp, vp, i32, vp]
    L.rumi_track_image_buffer.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(i32)]
    L.rumi_reloc_default_params.argtypes = [C.POINTER(RumiRelocParams)]
    L.rumi_reloc_default_params.restype = None
    L.rumi_track_reloc_begin.argtypes = [vp, vp, i32, vp, C.POINTER(RumiTrackPoints)]
    L.rumi_track_reloc_refine.argtypes = [vp, C.POINTER(RumiRelocParams), i32, vp, vp, vp, vp]
    L.rumi_track_reloc_attempts.argtypes = [vp, C.POINTER(i32)]
    L.rumi_track_compute_bow.argtypes = [vp, vp, i32, vp, vp, vp]
    L.rumi_track_reloc_bow.argtypes = [vp, vp, i32, vp, f32, i32, vp, vp]
    L.rumi_track_reloc_begin_resident.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp]
    L._track_ready = True
    return L


class Tracker:
    """rumi_track_create / rumi_track_frame.  `points` of track(): dict pos, normal [n,3], min_dist, max_dist [n], desc [n,32], obs [n], bad [n], local [n]."""

    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, max_width=640, max_height=480, max_points=8192, device=-1,
                 blur_variant=0):
        self._lib = _bind(capi.lib())
        self.cfg = RumiOrbConfig(nfeatures, scale_factor, nlevels, ini_th, min_th, max_width, max_height, 1, device, 0, blur_variant)
        self.cap = nfeatures + 4 * nlevels + 64
        self.max_points = int(max_points)
        self._h = C.c_void_p()
        capi.check(self._lib.rumi_track_create(C.byref(self.cfg), int(max_points), int(device), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.rumi_track_destroy(self._h)
            self._h = C.c_void_p()

    def track(self, img, K4, Tcw_pred7, last_keys, last_mp, last_outlier, points, th_motion=15.0, th_local=1.0, far_points=False, th_far_points=50.0):
        img = np.asarray(img, np.uint8)                      # rows may be strided (a view into a wider buffer); pixels of a row are contiguous
        assert img.ndim == 2 and img.strides[1] == 1
        h, w = img.shape
        K4 = np.ascontiguousarray(K4, np.float32); T = np.ascontiguousarray(Tcw_pred7, np.float32)
        lk = np.ascontiguousarray(last_keys, KP_DTYPE); lm = np.ascontiguousarray(last_mp, np.int32); lo = np.ascontiguousarray(last_outlier, np.uint8)
        n = len(points["obs"])
        a = dict(pos=np.ascontiguousarray(points["pos"], np.float32), normal=np.ascontiguousarray(points["normal"], np.float32),
                 mn=np.ascontiguousarray(points["min_dist"], np.float32), mx=np.ascontiguousarray(points["max_dist"], np.float32),
                 desc=np.ascontiguousarray(points["desc"], np.uint8), obs=np.ascontiguousarray(points["obs"], np.int32),
                 bad=np.ascontiguousarray(points["bad"], np.uint8), local=np.ascontiguousarray(points["local"], np.uint8))
        P = RumiTrackPoints(n, *(capi.ptr(a[k]) for k in ("pos", "normal", "mn", "mx", "desc", "obs", "bad", "local")), *_stale(points, a))
        keys = np.zeros(self.cap, KP_DTYPE); desc = np.zeros((self.cap, 32), np.uint8)
        mp_motion = np.full(self.cap, -1, np.int32); mp = np.full(self.cap, -1, np.int32); outl = np.zeros(self.cap, np.uint8)
        in_view = np.zeros(max(n, 1), np.uint8)
        res = RumiTrackResult()
        capi.check(self._lib.rumi_track_frame(self._h, capi.ptr(img), w, h, img.strides[0], capi.ptr(K4), capi.ptr(T), capi.ptr(lk), len(lk), capi.ptr(lm),
                                              capi.ptr(lo), C.byref(P), float(th_motion), float(th_local), int(far_points), float(th_far_points),
                                              capi.ptr(keys), capi.ptr(desc), self.cap, capi.ptr(mp_motion), capi.ptr(mp), capi.ptr(outl), capi.ptr(in_view),
                                              C.byref(res)))
        k = res.n
        out = {f: getattr(res, f) for f in ("n", "mono_index", "th_motion", "nmatches_motion", "ngood_motion", "nmatches_map", "n_to_match",
                                            "nmatches_local", "ngood_local", "matches_inliers")}
        for f in ("Tcw_motion", "Tcw", "Rcw", "tcw", "Ow"):
            out[f] = np.array(getattr(res, f), np.float32)
        out.update(keys=keys[:k].copy(), desc=desc[:k].copy(), frame_mp_motion=mp_motion[:k].copy(), frame_mp=mp[:k].copy(), outlier=outl[:k].copy(),
                   in_view=in_view[:n].copy())
        return out

    def image_buffer(self, w, h):
        """rumi_track_image_buffer: an [h, w] uint8 view of the tracker's pinned staging memory; a frame written there and passed to track() /
        extract() is uploaded without the staging copy."""
        buf, stride = C.c_void_p(), C.c_int32()
        capi.check(self._lib.rumi_track_image_buffer(self._h, int(w), int(h), C.byref(buf), C.byref(stride)))
        flat = np.ctypeslib.as_array((C.c_uint8 * (stride.value * h)).from_address(buf.value))
        return flat.reshape(h, stride.value)[:, :w]

    # ---- step-wise entries: one member function of Tracking per call, the frame resident in between (include/rumi_track.h) ----
    @staticmethod
    def _points(points, need_frustum):
        n = len(points["obs"])
        z3, z1 = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        a = dict(pos=np.ascontiguousarray(points["pos"], np.float32), normal=np.ascontiguousarray(points.get("normal", z3), np.float32),
                 mn=np.ascontiguousarray(points.get("min_dist", z1), np.float32), mx=np.ascontiguousarray(points.get("max_dist", z1), np.float32),
                 desc=np.ascontiguousarray(points["desc"], np.uint8), obs=np.ascontiguousarray(points["obs"], np.int32),
                 bad=np.ascontiguousarray(points["bad"], np.uint8), local=np.ascontiguousarray(points.get("local", np.zeros(n, np.uint8)), np.uint8))
        return n, a, RumiTrackPoints(n, *(capi.ptr(a[k]) for k in ("pos", "normal", "mn", "mx", "desc", "obs", "bad", "local")), *_stale(points, a))

    def set_distortion(self, K4, dist5):
        """rumi_track_set_distortion: mK and mDistCoef (k1, k2, p1, p2, k3); dist5 None / k1 == 0 switches undistortion off."""
        K = np.ascontiguousarray(K4, np.float32)
        d = np.ascontiguousarray(dist5, np.float32) if dist5 is not None else None
        capi.check(self._lib.rumi_track_set_distortion(self._h, capi.ptr(K), capi.ptr(d) if d is not None else None))

    def undistorted(self):
        """(mvKeysUn of the resident frame, (mnMinX, mnMinY, mnMaxX, mnMaxY))."""
        keys = np.zeros(self.cap, KP_DTYPE); b = np.zeros(4, np.float32)
        capi.check(self._lib.rumi_track_undistorted(self._h, capi.ptr(keys), self.cap, capi.ptr(b)))
        return keys[:self._n].copy(), b

    def last_projections(self, n_points):
        """rumi_track_last_projections: [n_points, 5] f32 = mTrackProjX, mTrackProjY, mnTrackScaleLevel, mTrackViewCos, mTrackDepth of the last SearchLocalPoints."""
        out = np.zeros((int(n_points), 5), np.float32)
        capi.check(self._lib.rumi_track_last_projections(self._h, int(n_points), capi.ptr(out)))
        return out

    @staticmethod
    def _result(res, fields):
        out = {f: getattr(res, f) for f in fields if f not in ("Tcw_motion", "Tcw", "Rcw", "tcw", "Ow")}
        for f in ("Tcw_motion", "Tcw", "Rcw", "tcw", "Ow"):
            if f in fields:
                out[f] = np.array(getattr(res, f), np.float32)
        return out

    def extract(self, img):
        """rumi_track_extract: Frame::ExtractORB; returns (monoIndex, keys, desc) and keeps the frame on the device."""
        img = np.asarray(img, np.uint8)
        assert img.ndim == 2 and img.strides[1] == 1
        h, w = img.shape
        keys = np.zeros(self.cap, KP_DTYPE); desc = np.zeros((self.cap, 32), np.uint8)
        n, mono = C.c_int32(), C.c_int32()
        capi.check(self._lib.rumi_track_extract(self._h, capi.ptr(img), w, h, img.strides[0], capi.ptr(keys), capi.ptr(desc), self.cap, C.byref(n), C.byref(mono)))
        self._n = n.value
        return mono.value, keys[:n.value].copy(), desc[:n.value].copy()

    def motion(self, K4, Tcw_pred7, last_keys, last_mp, last_outlier, points, th_motion=15.0):
        """rumi_track_motion: Tracking::TrackWithMotionModel on the resident frame."""
        K4 = np.ascontiguousarray(K4, np.float32); T = np.ascontiguousarray(Tcw_pred7, np.float32)
        lk = np.ascontiguousarray(last_keys, KP_DTYPE); lm = np.ascontiguousarray(last_mp, np.int32); lo = np.ascontiguousarray(last_outlier, np.uint8)
        _, keep, P = self._points(points, False)
        assert len(lm) >= len(lk) and len(lo) >= len(lk), "last_mp / last_outlier must cover every last-frame key-point (the C entry reads nlast of each)"
        mp = np.full(self.cap, -1, np.int32); dis = np.full(self.cap, -1, np.int32)
        res = RumiTrackResult()
        capi.check(self._lib.rumi_track_motion(self._h, capi.ptr(K4), capi.ptr(T), capi.ptr(lk), len(lk), capi.ptr(lm), capi.ptr(lo), C.byref(P), float(th_motion),
                                               capi.ptr(mp), capi.ptr(dis), C.byref(res)))
        out = self._result(res, ("n", "mono_index", "th_motion", "nmatches_motion", "ngood_motion", "nmatches_map", "Tcw_motion"))
        out.update(frame_mp=mp[:res.n].copy(), discarded=dis[:res.n].copy())
        return out

    def reference_keyframe(self, voc, K4, Tcw_init7, kf_view, kf_fv, kf_mp, points, levelsup=4, nnratio=0.7, check_orientation=True):
        """rumi_track_reference_keyframe: Tracking::TrackReferenceKeyFrame on the resident frame.  voc: rumi_slam_amd.vocabulary.Vocabulary;
        kf_view: matcher.FrameView of the key-frame; kf_fv: matcher.FeatureVectorView (CSR); kf_mp: indices into `points`."""
        K4 = np.ascontiguousarray(K4, np.float32); T = np.ascontiguousarray(Tcw_init7, np.float32)
        km = np.ascontiguousarray(kf_mp, np.int32)
        _, keep, P = self._points(points, False)
        mp = np.full(self.cap, -1, np.int32); dis = np.full(self.cap, -1, np.int32)
        word = np.zeros(self.cap, np.uint32); node = np.zeros(self.cap, np.uint32); wgt = np.zeros(self.cap, np.float64)
        res = RumiTrackResult()
        t0 = time.perf_counter()
        rc = self._lib.rumi_track_reference_keyframe(self._h, voc._h, int(levelsup), capi.ptr(K4), capi.ptr(T), C.byref(kf_view.c), C.byref(kf_fv.c),
                                                     capi.ptr(km), C.byref(P), float(nnratio), int(check_orientation), capi.ptr(word), capi.ptr(wgt),
                                                     capi.ptr(node), capi.ptr(mp), capi.ptr(dis), C.byref(res))
        self.last_call_s = time.perf_counter() - t0                    # the C entry alone (probes)
        capi.check(rc)
        out = self._result(res, ("n", "mono_index", "nmatches_motion", "ngood_motion", "nmatches_map", "Tcw_motion"))
        k = res.n
        out.update(frame_mp=mp[:k].copy(), discarded=dis[:k].copy(), word_id=word[:k].copy(), word_weight=wgt[:k].copy(), node_id=node[:k].copy())
        return out

    def local(self, K4, Tcw7, frame_mp_in, points, seen_in=None, th_local=1.0, far_points=False, th_far_points=50.0):
        """rumi_track_local: Tracking::TrackLocalMap after UpdateLocalMap on the resident frame."""
        K4 = np.ascontiguousarray(K4, np.float32); T = np.ascontiguousarray(Tcw7, np.float32)
        fin = np.ascontiguousarray(frame_mp_in, np.int32)
        n, keep, P = self._points(points, True)
        si = np.ascontiguousarray(seen_in, np.uint8) if seen_in is not None else None
        # the C entry reads frame_mp_in[0 .. n of the resident frame) and seen_in[0 .. points): shorter arrays would be host out-of-bounds reads
        assert getattr(self, "_n", None) is None or len(fin) >= self._n, f"frame_mp_in has {len(fin)} entries, the resident frame {self._n} features"
        assert si is None or len(si) >= n, f"seen_in has {len(si)} entries for {n} points"
        mp = np.full(self.cap, -1, np.int32); outl = np.zeros(self.cap, np.uint8); in_view = np.zeros(max(n, 1), np.uint8)
        res = RumiTrackResult()
        capi.check(self._lib.rumi_track_local(self._h, capi.ptr(K4), capi.ptr(T), capi.ptr(fin), C.byref(P), capi.ptr(si) if si is not None else None,
                                              float(th_local), int(far_points), float(th_far_points), capi.ptr(mp), capi.ptr(outl), capi.ptr(in_view), C.byref(res)))
        out = self._result(res, ("n", "n_to_match", "nmatches_local", "ngood_local", "matches_inliers", "Tcw", "Rcw", "tcw", "Ow"))
        out.update(frame_mp=mp[:res.n].copy(), outlier=outl[:res.n].copy(), in_view=in_view[:n].copy())
        return out

    @staticmethod
    def local_map_outputs(n, kf_cap, table_cap, fill=0):
        """The output arrays of local_map_into, every byte = fill."""
        f = lambda m, dt=np.int32: np.frombuffer(bytes([fill]) * (max(int(m), 1) * np.dtype(dt).itemsize), dt).copy()
        return dict(frame_point_bad=f(n, np.uint8), local_kf=f(kf_cap), n_k1=f(1), n_local_kf=f(1), ref_kf=f(1), table_ids=f(table_cap), n_local_points=f(1),
                    n_table=f(1), frame_mp=f(n), outlier=f(n, np.uint8), in_view=f(table_cap, np.uint8), res=f(C.sizeof(RumiTrackResult), np.uint8))

    def local_map_into(self, cov, K4, Tcw7, frame_points, out, kf_cap, table_cap, discarded=None, discarded_in_view=None, discarded_proj=None, th_local=1.0,
                       far_points=False, th_far_points=50.0):
        """The raw rumi_track_local_map call: status code; results in `out` (local_map_outputs)."""
        K4 = np.ascontiguousarray(K4, np.float32); T = np.ascontiguousarray(Tcw7, np.float32)
        fp = np.ascontiguousarray(frame_points, np.int32)
        assert getattr(self, "_n", None) is None or len(fp) >= self._n, f"frame_points has {len(fp)} entries, the resident frame {self._n} features"
        di = np.ascontiguousarray(discarded if discarded is not None else [], np.int32)
        dv = np.ascontiguousarray(discarded_in_view, np.uint8) if discarded_in_view is not None else None
        dp = np.ascontiguousarray(discarded_proj, np.float32).reshape(-1, 5) if discarded_proj is not None else None
        assert (dv is None) == (dp is None) and (dv is None or len(dv) == len(dp) == len(di))
        o = out
        return self._lib.rumi_track_local_map(self._h, cov._h, capi.ptr(K4), capi.ptr(T), capi.ptr(fp), len(di), capi.ptr(di), capi.ptr(dv) if dv is not None else None,
                                              capi.ptr(dp) if dp is not None else None, float(th_local), int(far_points), float(th_far_points),
                                              capi.ptr(o["frame_point_bad"]), capi.ptr(o["local_kf"]), int(kf_cap), capi.ptr(o["n_k1"]), capi.ptr(o["n_local_kf"]),
                                              capi.ptr(o["ref_kf"]), capi.ptr(o["table_ids"]), int(table_cap), capi.ptr(o["n_local_points"]), capi.ptr(o["n_table"]),
                                              capi.ptr(o["frame_mp"]), capi.ptr(o["outlier"]), capi.ptr(o["in_view"]),
                                              C.cast(capi.ptr(o["res"]), C.POINTER(RumiTrackResult)))

    def local_map(self, cov, K4, Tcw7, frame_points, discarded=None, discarded_in_view=None, discarded_proj=None, th_local=1.0, far_points=False,
                  th_far_points=50.0, kf_cap=None, table_cap=None):
        """rumi_track_local_map: Tracking::UpdateLocalMap + TrackLocalMap on the resident frame and the covisibility store `cov`
        (rumi_slam_amd.covis.Covisibility, its points carrying attributes).  frame_points: point ids, -1 = NULL; discarded: the ids the previous
        function discarded as outliers, discarded_in_view / discarded_proj their stale mbTrackInView and projections.
        -> the dict of Covisibility.local_map (local_points = the first rows of the table) and of Tracker.local (frame_mp in point ids,
        in_view per table row), plus table_ids."""
        kf_cap = cov.max_kf if kf_cap is None else kf_cap
        table_cap = min(cov.max_points, self.max_points) if table_cap is None else table_cap
        n = len(frame_points)
        o = self.local_map_outputs(n, kf_cap, table_cap)
        capi.check(self.local_map_into(cov, K4, Tcw7, frame_points, o, kf_cap, table_cap, discarded, discarded_in_view, discarded_proj, th_local, far_points,
                                       th_far_points))
        res = RumiTrackResult.from_buffer_copy(o["res"].tobytes())
        nt, nl = int(o["n_table"][0]), int(o["n_local_points"][0])
        out = self._result(res, ("n", "n_to_match", "nmatches_local", "ngood_local", "matches_inliers", "Tcw", "Rcw", "tcw", "Ow"))
        out.update(frame_point_bad=o["frame_point_bad"][:n], local_kf=o["local_kf"][:int(o["n_local_kf"][0])], n_k1=int(o["n_k1"][0]), ref_kf=int(o["ref_kf"][0]),
                   local_points=o["table_ids"][:nl].copy(), table_ids=o["table_ids"][:nt], frame_mp=o["frame_mp"][:res.n], outlier=o["outlier"][:res.n],
                   in_view=o["in_view"][:nt])
        return out

    # ---- Tracking::Relocalization: the refine chain of every pose hypothesis of a round in one call (include/rumi_track.h) ----
    def reloc_default_params(self):
        p = RumiRelocParams()
        self._lib.rumi_reloc_default_params(C.byref(p))
        return p

    def reloc_begin_status(self, K4, cands, pts):
        """The raw rumi_track_reloc_begin call: its status code.  cands: list of dicts kf_keys (KP_DTYPE [nkf]), kf_mp [nkf], matches [n]
        (ids into pts, -1 NULL); pts: dict pos, min_dist, max_dist, desc, bad."""
        K4 = np.ascontiguousarray(K4, np.float32)
        keep = []
        arr = (RumiRelocCandidate * max(len(cands), 1))()
        for k, c in enumerate(cands):
            kk = np.ascontiguousarray(c["kf_keys"], KP_DTYPE); km = np.ascontiguousarray(c["kf_mp"], np.int32); mt = np.ascontiguousarray(c["matches"], np.int32)
            assert len(km) == len(kk) and len(mt) >= getattr(self, "_n", 0), "kf_mp covers the key-frame, matches the resident frame"
            keep += [kk, km, mt]
            arr[k] = RumiRelocCandidate(len(kk), capi.ptr(kk), capi.ptr(km), capi.ptr(mt))
        n = len(pts["bad"])
        a = dict(pos=np.ascontiguousarray(pts["pos"], np.float32).reshape(-1, 3), mn=np.ascontiguousarray(pts["min_dist"], np.float32),
                 mx=np.ascontiguousarray(pts["max_dist"], np.float32), desc=np.ascontiguousarray(pts["desc"], np.uint8).reshape(-1, 32),
                 bad=np.ascontiguousarray(pts["bad"], np.uint8))
        assert len(a["pos"]) == len(a["mn"]) == len(a["mx"]) == len(a["desc"]) == n
        P = RumiTrackPoints(n, capi.ptr(a["pos"]), None, capi.ptr(a["mn"]), capi.ptr(a["mx"]), capi.ptr(a["desc"]), None, capi.ptr(a["bad"]), None, None, None)
        rc = self._lib.rumi_track_reloc_begin(self._h, capi.ptr(K4), len(cands), C.cast(arr, C.c_void_p), C.byref(P))
        if rc == 0:
            self._reloc_K = len(cands)
        return rc

    def reloc_begin(self, K4, cands, pts):
        capi.check(self.reloc_begin_status(K4, cands, pts))

    def reloc_refine_into(self, hyps, params, frame_mp, outlier_last, results):
        """The raw rumi_track_reloc_refine call: its status code; outputs written in place.  hyps: list of (cand, Tcw7, inliers [n] u8; None = NULL)."""
        H = len(hyps)
        arr = (RumiRelocHypothesis * max(H, 1))()
        keep = []
        for h, (cand, T, inl) in enumerate(hyps):
            if inl is not None:
                inl = np.ascontiguousarray(inl, np.uint8)
                assert len(inl) >= getattr(self, "_n", 0), "vbInliers covers the resident frame"
                keep.append(inl)
            arr[h] = RumiRelocHypothesis(int(cand), (C.c_float * 7)(*[float(x) for x in np.asarray(T, np.float32)]), capi.ptr(inl) if inl is not None else None)
        return self._lib.rumi_track_reloc_refine(self._h, C.byref(params) if params is not None else None, H, C.cast(arr, C.c_void_p), capi.ptr(frame_mp),
                                                 capi.ptr(outlier_last), capi.ptr(results))

    def reloc_refine(self, hyps, params=None):
        """rumi_track_reloc_refine -> (frame_mp [H, n] i32, outlier_last [H, n] u8 (255: never written), results [H] RELOC_RESULT_DTYPE)."""
        H = len(hyps)
        mp = np.full((max(H, 1), self.cap), -1, np.int32); ol = np.full((max(H, 1), self.cap), 255, np.uint8)
        res = np.zeros(max(H, 1), RELOC_RESULT_DTYPE)
        capi.check(self.reloc_refine_into(hyps, params, mp, ol, res))
        n = self._n
        return mp[:H, :n].copy(), ol[:H, :n].copy(), res[:H].copy()

    def reloc_attempts(self):
        """How often the last reloc_refine ran its chain (1: the candidate lists fitted their arena at once)."""
        a = C.c_int32()
        capi.check(self._lib.rumi_track_reloc_attempts(self._h, C.byref(a)))
        return a.value

    # ---- Tracking::Relocalization by slot: the BoW walk and the refine session read the covisibility store (include/rumi_track.h) ----
    def compute_bow_into(self, voc, levelsup, word, wgt, node):
        """The raw rumi_track_compute_bow call: its status code.  voc None / an output None goes in as NULL."""
        return self._lib.rumi_track_compute_bow(self._h, voc._h if voc is not None else None, int(levelsup), capi.ptr(word) if word is not None else None,
                                                capi.ptr(wgt) if wgt is not None else None, capi.ptr(node) if node is not None else None)

    def compute_bow(self, voc, levelsup=4):
        """rumi_track_compute_bow: Frame::ComputeBoW on the resident frame -> dict word_id, word_weight, node_id [n] (the per-feature transform,
        for Vocabulary.assemble); the frame's FeatureVector stays on the device for reloc_bow."""
        word = np.zeros(self.cap, np.uint32); node = np.zeros(self.cap, np.uint32); wgt = np.zeros(self.cap, np.float64)
        t0 = time.perf_counter()
        rc = self.compute_bow_into(voc, levelsup, word, wgt, node)
        self.last_call_s = time.perf_counter() - t0
        capi.check(rc)
        n = self._n
        return dict(word_id=word[:n].copy(), word_weight=wgt[:n].copy(), node_id=node[:n].copy())

    def reloc_bow_into(self, cov, slots, nnratio, check_orientation, matches, nmatches):
        """The raw rumi_track_reloc_bow call: its status code; outputs written in place (matches [K, n] i32, nmatches [K] i32)."""
        s = np.ascontiguousarray(slots, np.int32).reshape(-1)
        return self._lib.rumi_track_reloc_bow(self._h, cov._h, len(s), capi.ptr(s) if len(s) else None, float(nnratio), int(check_orientation),
                                              capi.ptr(matches) if matches is not None and matches.size else None, capi.ptr(nmatches))

    def reloc_bow(self, cov, slots, nnratio=0.75, check_orientation=True):
        """rumi_track_reloc_bow: SearchByBoW of the key-frames in `slots` of the covisibility store `cov` against the resident frame (after
        compute_bow) -> (nmatches [K] (-1: a bad key-frame, not searched), matches [K, n] store point ids, -1 = NULL)."""
        K = len(slots)
        matches = np.full((K, self._n), -1, np.int32); nm = np.zeros(max(K, 1), np.int32)
        capi.check(self.reloc_bow_into(cov, slots, nnratio, check_orientation, matches, nm))
        return nm[:K].copy(), matches

    def reloc_begin_resident_into(self, cov, K4, cand, table_ids, table_cap, n_table):
        """The raw rumi_track_reloc_begin_resident call: its status code; table_ids [table_cap] i32 and n_table [1] i32 written in place."""
        K4 = np.ascontiguousarray(K4, np.float32)
        cd = np.ascontiguousarray(cand, np.int32).reshape(-1)
        return self._lib.rumi_track_reloc_begin_resident(self._h, cov._h, capi.ptr(K4), len(cd), capi.ptr(cd) if len(cd) else None, capi.ptr(table_ids),
                                                         int(table_cap), capi.ptr(n_table))

    def reloc_begin_resident(self, cov, K4, cand, table_cap=None):
        """rumi_track_reloc_begin_resident: the session of reloc_refine from the store, for the candidates `cand` (indices into the slots of the
        preceding reloc_bow) -> table_ids [n_table]: the store point id of every table row (reloc_refine's frame_mp holds rows)."""
        table_cap = min(cov.max_points, self.max_points) if table_cap is None else int(table_cap)
        ids = np.full(max(table_cap, 1), -1, np.int32); nt = np.zeros(1, np.int32)
        capi.check(self.reloc_begin_resident_into(cov, K4, cand, ids, table_cap, nt))
        self._reloc_K = len(cand)
        return ids[:int(nt[0])].copy()


def relocalize(tracker, cands, pts, solver_step, speculate_round=True, K4=None, params=None, frame_mp=None, outlier=None, Tcw=None):
    """The round loop of Tracking::Relocalization (R/lib_src/Tracking.cc:3266-3348) over tracker.reloc_refine.  cands [K]: the candidates of
    reloc_begin, None for one that is discarded from the start (isBad, or fewer than 15 BoW matches); with K4 the session is begun here,
    otherwise the caller has begun it.  solver_step(i) -> (bTcw, bNoMore, inliers, Tcw7) is one `pSolver->iterate(5, ...)` of candidate i.
    frame_mp / outlier / Tcw: the frame's mvpMapPoints, mvbOutlier and pose before the call (None: all NULL / false / None).

    speculate_round: every live candidate of a round iterates, the round's hypotheses go to the device in ONE refine call, and the results are
    replayed in candidate order up to and including the first that wins (ran & 2 and ngood_final >= enough) -- the reference's sequential rule;
    the candidates behind the winner have then iterated once more than in the reference.  False: one hypothesis a call in the reference's
    order, exactly its solver calls.  Both leave the same frame.
    -> dict(matched, frame_mp, outlier, Tcw, winner (candidate or -1), rounds, steps [K] solver calls, refines)."""
    K = len(cands)
    if K4 is not None:
        tracker.reloc_begin(K4, [c if c is not None else dict(kf_keys=np.zeros(0, KP_DTYPE), kf_mp=[], matches=np.full(getattr(tracker, "_n", 0), -1, np.int32))
                                 for c in cands], pts)
    return _relocalize_rounds(tracker, [c is None for c in cands], lambda i: i, lambda mp: mp.copy(), solver_step, speculate_round, params, frame_mp, outlier, Tcw)


def _relocalize_rounds(tracker, discarded, cand_of, map_mp, solver_step, speculate_round, params, frame_mp, outlier, Tcw):
    """The rounds of relocalize / relocalize_resident on an open session.  discarded [K]: the candidates that are out from the start;
    cand_of(i): candidate i's index in the session; map_mp(row): a hypothesis' frame_mp as the caller numbers its points."""
    K = len(discarded)
    discarded = list(discarded)
    enough = params.enough if params is not None else 50
    n_cand = discarded.count(False)
    st = dict(matched=False, frame_mp=None if frame_mp is None else np.array(frame_mp, np.int32), outlier=None if outlier is None else np.array(outlier, np.uint8),
              Tcw=None if Tcw is None else np.array(Tcw, np.float32), winner=-1, rounds=0, steps=[0] * K, refines=0)

    def replay(cand, mp, ol, r):
        """What the body of `for (i ...)` leaves in the frame for one hypothesis; True when it wins (:3342)."""
        if st["outlier"] is None:
            st["outlier"] = np.zeros(len(ol), np.uint8)
        w = ol != 255
        st["outlier"][w] = ol[w]
        st["frame_mp"] = map_mp(mp); st["Tcw"] = np.array(r["Tcw"], np.float32)
        if (int(r["ran"]) & 2) and int(r["ngood_final"]) >= enough:
            st["matched"] = True; st["winner"] = cand
            return True
        return False

    def step(i):
        st["steps"][i] += 1
        b_tcw, b_no_more, inl, T = solver_step(i)
        return b_tcw, b_no_more, inl, T

    while n_cand > 0 and not st["matched"]:
        st["rounds"] += 1
        if speculate_round:
            hyps = []
            for i in range(K):
                if discarded[i]:
                    continue
                b_tcw, b_no_more, inl, T = step(i)
                if b_no_more:
                    discarded[i] = True; n_cand -= 1
                if b_tcw:
                    hyps.append((i, T, inl))
            if hyps:
                mp, ol, res = tracker.reloc_refine([(cand_of(i), T, inl) for i, T, inl in hyps], params)
                st["refines"] += 1
                for h, (i, _, _) in enumerate(hyps):
                    if replay(i, mp[h], ol[h], res[h]):
                        break
        else:
            for i in range(K):
                if discarded[i]:
                    continue
                b_tcw, b_no_more, inl, T = step(i)
                if b_no_more:
                    discarded[i] = True; n_cand -= 1
                if b_tcw:
                    mp, ol, res = tracker.reloc_refine([(cand_of(i), T, inl)], params)
                    st["refines"] += 1
                    if replay(i, mp[0], ol[0], res[0]):
                        break
    return st


def relocalize_resident(tracker, cov, slots, solver_step, K4, make=None, nnratio=0.75, check_orientation=True, min_matches=15, speculate_round=True, params=None,
                        frame_mp=None, outlier=None, Tcw=None):
    """Tracking::Relocalization (R/lib_src/Tracking.cc:3226-3348) by slot, after tracker.compute_bow on the resident frame: one reloc_bow over
    the candidate slots of the covisibility store `cov`, make(k, matches_k) for every candidate that keeps at least min_matches (:3253: the
    caller sets up its solver from the matches, store point ids), one reloc_begin_resident over those, then the rounds of relocalize.
    solver_step(k) as in relocalize, k an index into `slots`.  -> the dict of relocalize, frame_mp in store point ids, plus nmatches [K],
    matches [K, n] and table_ids."""
    nm, matches = tracker.reloc_bow(cov, slots, nnratio, check_orientation)
    keep = [k for k in range(len(slots)) if nm[k] >= min_matches]
    if make is not None:
        for k in keep:
            make(k, matches[k])
    ids = tracker.reloc_begin_resident(cov, K4, keep)
    place = {k: j for j, k in enumerate(keep)}
    st = _relocalize_rounds(tracker, [k not in place for k in range(len(slots))], lambda k: place[k], lambda mp: rows_to_ids(mp, ids), solver_step, speculate_round,
                            params, frame_mp, outlier, Tcw)
    st.update(nmatches=nm, matches=matches, table_ids=ids)
    return st


def rows_to_ids(rows, table_ids):
    """Table rows (-1 = NULL) as the store's point ids."""
    rows = np.asarray(rows, np.int32)
    ids = np.asarray(table_ids, np.int32)
    return np.where(rows >= 0, ids[np.clip(rows, 0, max(len(ids) - 1, 0))] if len(ids) else -1, -1).astype(np.int32)
