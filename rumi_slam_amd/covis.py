"""The covisibility store over the C ABI of include/rumi_covis.h (ctypes; host logic only): key-frame and observation tables resident on
the GPU, KeyFrame::UpdateConnections for a batch of key-frames and Tracking::UpdateLocalMap for a frame."""
import ctypes as C

import numpy as np

from . import capi

MAX_KEYFRAMES, MAX_FEATURES, NBEST, TH, LOCAL_LIMIT = 8192, 65536, 10, 15, 80
CONNECTED, EMPTY = 0, 1

_i32, _u8, _u64 = np.int32, np.uint8, np.uint64


def _csr(rows):
    """list of int sequences -> (offsets [n + 1], flat) as int32"""
    off = np.zeros(len(rows) + 1, _i32)
    for i, r in enumerate(rows):
        off[i + 1] = off[i] + len(r)
    flat = np.concatenate([np.asarray(r, _i32).reshape(-1) for r in rows]) if rows else np.zeros(0, _i32)
    return off, np.ascontiguousarray(flat, _i32)


def _p(a):
    return None if a is None else capi.ptr(a)


class Covisibility:
    """Device-resident covisibility store.  Key-frames are slots 0..max_kf-1, points ids 0..max_points-1; order_key restates pointer order."""

    def __init__(self, max_kf, max_points, arena_entries=0, device=-1):
        self._lib = capi.covis_lib()
        self._h = C.c_void_p()
        self.max_kf, self.max_points = int(max_kf), int(max_points)
        capi.check(self._lib.rumi_covis_create(int(max_kf), int(max_points), int(arena_entries), int(device), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.rumi_covis_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    # ---- edits: each returns the status code when check=False ----
    def _ret(self, rc, check):
        if check:
            capi.check(rc)
        return rc

    def set_keyframes(self, slots, keys, maps, bad, mp_rows, best, parents, children, check=True):
        """mp_rows[i]: point ids (-1 = NULL); best[i]: up to 10 slots; parents[i]: slot or -1; children[i]: slots."""
        slots = np.ascontiguousarray(slots, _i32); keys = np.ascontiguousarray(keys, _u64); maps = np.ascontiguousarray(maps, _i32)
        bad = np.ascontiguousarray(bad, _u8); parents = np.ascontiguousarray(parents, _i32)
        n = len(slots)
        b = np.full((n, NBEST), -1, _i32)
        for i, r in enumerate(best):
            r = list(r)[:NBEST]
            b[i, :len(r)] = r
        mo, mp = _csr(list(mp_rows)); co, ch = _csr(list(children))
        return self._ret(self._lib.rumi_covis_set_keyframes(self._h, n, _p(slots), _p(keys), _p(maps), _p(bad), _p(mo), _p(mp), _p(b), _p(parents),
                                                            _p(co), _p(ch)), check)

    def row_length(self, slot):
        """Length of a live slot's map-point row as the store holds it; -1 for a slot that is not live."""
        return int(self._lib.rumi_covis_row_length(self._h, int(slot)))

    def set_points(self, ids, bad, observers, check=True):
        ids = np.ascontiguousarray(ids, _i32); bad = np.ascontiguousarray(bad, _u8)
        oo, ob = _csr(list(observers))
        return self._ret(self._lib.rumi_covis_set_points(self._h, len(ids), _p(ids), _p(bad), _p(oo), _p(ob)), check)

    def set_point_observations(self, ids, bad, observations, check=True):
        """set_points with the feature index of every observer: observations[i] = [(slot, feature), ...] of point ids[i]."""
        ids = np.ascontiguousarray(ids, _i32); bad = np.ascontiguousarray(bad, _u8)
        oo, ob = _csr([[o[0] for o in r] for r in observations])
        _, of = _csr([[o[1] for o in r] for r in observations])
        return self._ret(self._lib.rumi_covis_set_point_observations(self._h, len(ids), _p(ids), _p(bad), _p(oo), _p(ob), _p(of)), check)

    def set_point_attributes(self, ids, pos, normal, min_dist, max_dist, desc, check=True):
        """GetWorldPos / GetNormal [n, 3], mfMinDistance / mfMaxDistance [n] (raw), GetDescriptor [n, 32] of the points `ids`."""
        ids = np.ascontiguousarray(ids, _i32); n = len(ids)
        pos = np.ascontiguousarray(pos, np.float32).reshape(n, 3); normal = np.ascontiguousarray(normal, np.float32).reshape(n, 3)
        mn = np.ascontiguousarray(min_dist, np.float32).reshape(n); mx = np.ascontiguousarray(max_dist, np.float32).reshape(n)
        desc = np.ascontiguousarray(desc, _u8).reshape(n, 32)
        return self._ret(self._lib.rumi_covis_set_point_attributes(self._h, n, _p(ids), _p(pos), _p(normal), _p(mn), _p(mx), _p(desc)), check)

    def set_keyframe_centres(self, slots, Ow, check=True):
        """GetCameraCenter() [n, 3] of the live slots ``slots`` (where the reference calls SetPose); read by mapping.RefreshMapPointsResident."""
        s = np.ascontiguousarray(slots, _i32).reshape(-1)
        Ow = np.ascontiguousarray(Ow, np.float32).reshape(len(s), 3)
        return self._ret(self._lib.rumi_covis_set_keyframe_centres(self._h, len(s), _p(s), _p(Ow)), check)

    def set_point_reference(self, ids, ref_slots, check=True):
        """GetReferenceKeyFrame() of the points ``ids`` as live slots; -1 clears it."""
        ids = np.ascontiguousarray(ids, _i32).reshape(-1); ref = np.ascontiguousarray(ref_slots, _i32).reshape(-1)
        assert len(ids) == len(ref)
        return self._ret(self._lib.rumi_covis_set_point_reference(self._h, len(ids), _p(ids), _p(ref)), check)

    def set_keyframe_poses(self, slots, pose7, check=True):
        """GetPose() [n, 7] (qx qy qz qw tx ty tz) of the live slots ``slots`` (where the reference calls SetPose, beside set_keyframe_centres);
        read by optimizer.LocalBundleAdjustmentResident."""
        s = np.ascontiguousarray(slots, _i32).reshape(-1)
        T = np.ascontiguousarray(pose7, np.float32).reshape(len(s), 7)
        return self._ret(self._lib.rumi_covis_set_keyframe_poses(self._h, len(s), _p(s), _p(T)), check)

    def set_point_maps(self, ids, map_ids, check=True):
        """MapPoint::GetMap() of the points ``ids`` in the key-frames' map_id numbering."""
        ids = np.ascontiguousarray(ids, _i32).reshape(-1); m = np.ascontiguousarray(map_ids, _i32).reshape(-1)
        assert len(ids) == len(m)
        return self._ret(self._lib.rumi_covis_set_point_maps(self._h, len(ids), _p(ids), _p(m)), check)

    def read_attributes(self, ids, from_device=False, check=True):
        """Test hook: the 64-byte attribute records [n, 64] of ``ids`` from the device copy or the host mirror; uploads nothing.  With
        check=False -> (status, records)."""
        ids = np.ascontiguousarray(ids, _i32).reshape(-1)
        out = np.zeros((len(ids), 64), _u8)
        rc = capi.hooks().rumi_hook_covis_read_attributes(self._h, len(ids), _p(ids), _p(out), int(bool(from_device)))
        if check:
            capi.check(rc)
            return out
        return rc, out

    def read_poses(self, slots=(), ids=(), from_device=False):
        """Test hook: (pose8 [n_kf, 8] float64, has_pose [n_kf], map_id [n_pt], has_map [n_pt]) from the device copy or the host mirror."""
        s = np.ascontiguousarray(slots, _i32).reshape(-1); p = np.ascontiguousarray(ids, _i32).reshape(-1)
        T, hp = np.zeros((max(len(s), 1), 8), np.float64), np.zeros(max(len(s), 1), _i32)
        m, hm = np.zeros(max(len(p), 1), _i32), np.zeros(max(len(p), 1), _i32)
        capi.check(capi.hooks().rumi_hook_covis_read_poses(self._h, len(s), _p(s), _p(T), _p(hp), len(p), _p(p), _p(m), _p(hm), int(bool(from_device))))
        return T[:len(s)], hp[:len(s)], m[:len(p)], hm[:len(p)]

    def read_row(self, slot):
        """Test hook: what the host mirror holds for a live slot -> (map-point row, bad bit of each entry's point, the key-frame's bad bit)."""
        n = max(self.row_length(slot), 0)
        row, bad, kf = np.zeros(max(n, 1), _i32), np.zeros(max(n, 1), _u8), np.zeros(1, _i32)
        capi.check(capi.hooks().rumi_hook_covis_read_row(self._h, int(slot), n, _p(row), _p(bad), _p(kf)))
        return row[:n], bad[:n], int(kf[0])

    def set_bad(self, kf_slots=(), kf_bad=(), pt_ids=(), pt_bad=(), check=True):
        ks = np.ascontiguousarray(kf_slots, _i32); kb = np.ascontiguousarray(kf_bad, _u8)
        ps = np.ascontiguousarray(pt_ids, _i32); pb = np.ascontiguousarray(pt_bad, _u8)
        return self._ret(self._lib.rumi_covis_set_bad(self._h, len(ks), _p(ks), _p(kb), len(ps), _p(ps), _p(pb)), check)

    def set_maps(self, slots, maps, check=True):
        s = np.ascontiguousarray(slots, _i32); m = np.ascontiguousarray(maps, _i32)
        return self._ret(self._lib.rumi_covis_set_maps(self._h, len(s), _p(s), _p(m)), check)

    # ---- key-frame features: uploaded once per key-frame, read in place by mapping.CreateNewMapPointsResident ----
    def set_keyframe_features(self, slot, frame, fv, K4, check=True):
        """mvKeysUn, mDescriptors, mvScaleFactors (``frame``: a matcher.FrameView), mFeatVec (``fv``: a matcher.FeatureVector) and fx fy cx cy
        of a live slot; setting a slot again replaces them.  Staged: the next consumer uploads them."""
        K4 = np.ascontiguousarray(K4, np.float32).reshape(4)
        return self._ret(self._lib.rumi_covis_set_keyframe_features(self._h, int(slot), C.byref(frame.c), C.byref(fv.c), _p(K4)), check)

    def drop_keyframe_features(self, slots, check=True):
        s = np.ascontiguousarray(slots, _i32).reshape(-1)
        return self._ret(self._lib.rumi_covis_drop_keyframe_features(self._h, len(s), _p(s)), check)

    def reserve_features(self, nbytes, check=True):
        """First size of the feature arena (0: the default); before the first set_keyframe_features."""
        return self._ret(self._lib.rumi_covis_reserve_features(self._h, int(nbytes)), check)

    def feature_stats(self):
        v = np.zeros(6, np.int64)
        capi.check(self._lib.rumi_covis_feature_stats(self._h, _p(v)))
        return dict(zip(("capacity", "used", "slots", "growths", "compactions", "last_upload_bytes"), (int(x) for x in v)))

    # ---- queries ----
    @staticmethod
    def connection_outputs(B, conn_cap, ord_cap, fill=0):
        """The output arrays of update_connections, every byte = fill."""
        f = lambda n, dt=_i32: np.frombuffer(bytes([fill]) * (max(int(n), 1) * np.dtype(dt).itemsize), dt).copy()
        return dict(status=f(B), conn_off=f(B + 1), conn_slot=f(conn_cap), conn_count=f(conn_cap), ord_off=f(B + 1), ord_slot=f(ord_cap),
                    ord_weight=f(ord_cap))

    def update_connections_into(self, batch, out, conn_cap, ord_cap):
        """The raw call: status code; results in `out` (connection_outputs)."""
        batch = np.ascontiguousarray(batch, _i32)
        return self._lib.rumi_covis_update_connections(self._h, len(batch), _p(batch), _p(out["status"]), _p(out["conn_off"]), _p(out["conn_slot"]),
                                                       _p(out["conn_count"]), int(conn_cap), _p(out["ord_off"]), _p(out["ord_slot"]),
                                                       _p(out["ord_weight"]), int(ord_cap))

    def update_connections(self, batch, n_live=None):
        """-> dict of status [B], conn_off, conn_slot, conn_count, ord_off, ord_slot, ord_weight, trimmed to their lengths."""
        B = len(batch)
        cap = B * (self.max_kf if n_live is None else int(n_live))
        out = self.connection_outputs(B, cap, cap)
        capi.check(self.update_connections_into(batch, out, cap, cap))
        nc, no = int(out["conn_off"][B]), int(out["ord_off"][B])
        return dict(status=out["status"][:B], conn_off=out["conn_off"][:B + 1], conn_slot=out["conn_slot"][:nc], conn_count=out["conn_count"][:nc],
                    ord_off=out["ord_off"][:B + 1], ord_slot=out["ord_slot"][:no], ord_weight=out["ord_weight"][:no])

    @staticmethod
    def local_map_outputs(n, kf_cap, pt_cap, fill=0):
        f = lambda m, dt=_i32: np.frombuffer(bytes([fill]) * (max(int(m), 1) * np.dtype(dt).itemsize), dt).copy()
        return dict(frame_point_bad=f(n, _u8), local_kf=f(kf_cap), n_k1=f(1), n_local_kf=f(1), ref_kf=f(1), local_points=f(pt_cap), n_local_points=f(1))

    def local_map_into(self, frame_points, out, kf_cap, pt_cap):
        fp = np.ascontiguousarray(frame_points, _i32)
        return self._lib.rumi_covis_local_map(self._h, len(fp), _p(fp), _p(out["frame_point_bad"]), _p(out["local_kf"]), int(kf_cap), _p(out["n_k1"]),
                                              _p(out["n_local_kf"]), _p(out["ref_kf"]), _p(out["local_points"]), int(pt_cap), _p(out["n_local_points"]))

    def local_map(self, frame_points, kf_cap=None, pt_cap=None):
        """-> dict of frame_point_bad [n], local_kf, n_k1, ref_kf, local_points (trimmed)."""
        kf_cap = self.max_kf if kf_cap is None else kf_cap
        pt_cap = self.max_points if pt_cap is None else pt_cap
        n = len(frame_points)
        out = self.local_map_outputs(n, kf_cap, pt_cap)
        capi.check(self.local_map_into(frame_points, out, kf_cap, pt_cap))
        return dict(frame_point_bad=out["frame_point_bad"][:n], local_kf=out["local_kf"][:int(out["n_local_kf"][0])], n_k1=int(out["n_k1"][0]),
                    ref_kf=int(out["ref_kf"][0]), local_points=out["local_points"][:int(out["n_local_points"][0])])

    def stage_ms(self):
        ms = np.zeros(3, np.float32)
        capi.check(self._lib.rumi_covis_stage_ms(self._h, _p(ms)))
        return ms

    def stats(self):
        v = np.zeros(7, np.int64)
        capi.check(self._lib.rumi_covis_stats(self._h, _p(v)))
        return dict(zip(("capacity", "tail", "live", "replaced", "compactions", "growths", "last_upload_bytes"), (int(x) for x in v)))
