"""Host-side mirror of ``LocalMapping::CreateNewMapPoints`` (R/lib_src/LocalMapping.cc:354-647, monocular pinhole) over the C ABI in
include/rumi_mapping.h: one call for the current key-frame and all of its neighbours; of the map-point refresh
(``MapPoint::ComputeDistinctiveDescriptors`` / ``UpdateNormalAndDepth``, R/lib_src/MapPoint.cc:353-427, 450-518) for a batch of points; and of
``LocalMapping::KeyFrameCulling`` / ``CloudKeyFrameCulling`` (R/lib_src/LocalMapping.cc:953-1079, 820-951) for the whole covisible list; and of
the searches of ``LocalMapping::SearchInNeighbors`` (R/lib_src/LocalMapping.cc:649-743) for every target key-frame in one call; and of those of
``LoopClosing::SearchAndFuse`` (R/lib_src/LoopClosing.cc:1996-2065) for every corrected key-frame in one call."""
import ctypes as C

import numpy as np

from . import capi
from .matcher import FeatureVector, FrameView, RumiFeatureVector, RumiFrameFeatures

MAX_NEIGH = 64
MAX_FEATURES = 16384

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
    L.rumi_create_new_map_points_resident.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, C.POINTER(i32), vp, vp]
    L.rumi_newpts_stage_ms.argtypes = [vp, vp]
    L.rumi_search_in_neighbors_resident.argtypes = [vp, vp, i32, vp, vp, vp, i32, C.c_float, vp, vp, vp, i32, C.POINTER(i32)]
    L.rumi_search_in_neighbors_stage_ms.argtypes = [vp, vp]
    L.rumi_search_and_fuse_resident.argtypes = [vp, vp, vp, vp, i32, vp, i32, C.c_float, vp, i32, C.POINTER(i32), vp]
    L.rumi_search_and_fuse_stage_ms.argtypes = [vp, vp]
    L.rumi_search_by_projection_sim3_resident.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, i32, vp]
    L.rumi_search_by_projection_sim3_stage_ms.argtypes = [vp, vp]
    L.rumi_search_by_projection_sim3_rounds.argtypes = [vp, vp, i32]
    L.rumi_common_regions_bow_resident.argtypes = [vp, vp, i32, i32, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp, vp]
    L.rumi_common_regions_bow_resident_stage_ms.argtypes = [vp, vp]
    L.rumi_hook_newpts_matches.argtypes = [vp, i32, i32, vp]
    L.rumi_refresh_create.argtypes = [i32, C.POINTER(vp)]
    L.rumi_refresh_destroy.argtypes = [vp]
    L.rumi_refresh_destroy.restype = None
    L.rumi_refresh_map_points.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.rumi_refresh_stage_ms.argtypes = [vp, vp]
    L.rumi_refresh_map_points_resident.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.rumi_refresh_last_launches.argtypes = [vp]
    L.rumi_cull_create.argtypes = [i32, C.POINTER(vp)]
    L.rumi_cull_destroy.argtypes = [vp]
    L.rumi_cull_destroy.restype = None
    L.rumi_keyframe_culling.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.rumi_cull_stage_ms.argtypes = [vp, vp]
    L.rumi_keyframe_culling_resident.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]
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


class RumiNewPointsPose(C.Structure):
    _fields_ = [("Tcw", C.c_float * 12), ("Ow", C.c_float * 3), ("F12", C.c_float * 9), ("epipole2", C.c_float * 2)]


assert C.sizeof(RumiNewPointsPose) == 104


def pose(Tcw, Ow, F12=None, epipole2=None):
    """What changes with every bundle adjustment, by value: a KeyFrameView's Tcw / Ow / F12 / epipole2 as one RumiNewPointsPose."""
    p = RumiNewPointsPose()
    p.Tcw[:] = np.asarray(Tcw, np.float32).reshape(12).tolist()
    p.Ow[:] = np.asarray(Ow, np.float32).reshape(3).tolist()
    if F12 is not None:
        p.F12[:] = np.asarray(F12, np.float32).reshape(9).tolist()
    if epipole2 is not None:
        p.epipole2[:] = np.asarray(epipole2, np.float32).reshape(2).tolist()
    return p


def pack_poses(cur_pose, neigh_poses):
    """(RumiNewPointsPose, array of RumiNewPointsPose) for the C entry."""
    arr = (RumiNewPointsPose * max(len(neigh_poses), 1))(*neigh_poses)
    return cur_pose, arr


def CreateNewMapPointsResident(matcher, store, cur_slot, cur_pose, neigh_slots, neigh_poses, ratio_factor, coarse=False, far_points=False,
                               th_far_points=0.0, cap=None):
    """CreateNewMapPoints over key-frames resident in ``store`` (a covis.Covisibility whose slots hold features, map-point rows and point
    attributes).  ``cur_pose`` / ``neigh_poses``: RumiNewPointsPose (see ``pose``).  Returns what CreateNewMapPoints returns."""
    L = _lib()
    n = len(neigh_slots)
    assert len(neigh_poses) == n
    slots = np.ascontiguousarray(neigh_slots, np.int32).reshape(-1)
    cp, arr = pack_poses(cur_pose, list(neigh_poses))
    prm = RumiNewPointsParams(int(coarse), int(matcher.mbCheckOrientation), int(far_points), float(th_far_points), float(ratio_factor))
    cap = MAX_FEATURES if cap is None else int(cap)          # a list never needs more entries than the current key-frame has features
    out = np.zeros(max(cap, 1), NEWPOINT_DTYPE)
    per = np.zeros(max(n, 1), np.int32)
    skipped = np.zeros(max(n, 1), np.uint8)
    n_out = C.c_int32()
    capi.check(L.rumi_create_new_map_points_resident(matcher._h, store._h, int(cur_slot), C.byref(cp), capi.ptr(slots) if n else None,
                                                     C.byref(arr) if n else None, n, C.byref(prm), capi.ptr(out), cap, C.byref(n_out),
                                                     capi.ptr(per), capi.ptr(skipped)))
    return out[:n_out.value], per[:n], skipped[:n]


def stage_ms(matcher):
    """(validation + packing, upload + kernels + download, write-out) of the matcher's last CreateNewMapPoints call of either kind, ms."""
    out = np.zeros(3, np.float32)
    capi.check(_lib().rumi_newpts_stage_ms(matcher._h, capi.ptr(out)))
    return out


def last_matches(matcher, n_neigh, n1):
    """Test hook: [n_neigh, n1] the neighbour feature each current feature was paired with when the loop reached that neighbour (-1 none)."""
    out = np.full((n_neigh, n1), -1, np.int32)
    capi.check(_lib().rumi_hook_newpts_matches(matcher._h, n_neigh, n1, capi.ptr(out)))
    return out


# ---- SearchInNeighbors ----
FUSE_MAX_TARGETS = 640


class RumiFuseKF(C.Structure):
    _fields_ = [("Tcw7", C.c_float * 7), ("Ow", C.c_float * 3), ("bounds", C.c_float * 4), ("log_scale_factor", C.c_float)]


assert C.sizeof(RumiFuseKF) == 60


def fuse_kf(Tcw7, Ow, bounds, log_sf):
    """What SearchInNeighbors needs of a key-frame besides what the store keeps: the pose as qx qy qz qw tx ty tz, the camera centre, the image
    bounds (mnMinX, mnMinY, mnMaxX, mnMaxY) and mfLogScaleFactor, as one RumiFuseKF."""
    k = RumiFuseKF()
    k.Tcw7[:] = np.asarray(Tcw7, np.float32).reshape(7).tolist()
    k.Ow[:] = np.asarray(Ow, np.float32).reshape(3).tolist()
    k.bounds[:] = np.asarray(bounds, np.float32).reshape(4).tolist()
    k.log_scale_factor = float(log_sf)
    return k


def SearchInNeighborsResident(matcher, store, cur_slot, cur, target_slots, targets, th=3.0, rev_cap=None):
    """The search half of LocalMapping::SearchInNeighbors over key-frames and points resident in ``store``: one device call for every target.
    ``cur`` / ``targets``: RumiFuseKF (see ``fuse_kf``).  Returns (fwd_best [n_targets, n_cur], rev_point, rev_best): the target feature each
    point of the current key-frame fuses with, and for every distinct point of the targets' rows that is not bad and not in the current
    key-frame its id and the current key-frame's feature (-1: none).  ``rev_cap``: entries of the reverse lists (default: all that can occur)."""
    L = _lib()
    n = len(target_slots)
    assert len(targets) == n
    slots = np.ascontiguousarray(target_slots, np.int32).reshape(-1)
    arr = (RumiFuseKF * max(n, 1))(*targets)
    lengths = [store.row_length(int(s)) for s in [cur_slot] + slots.tolist()]
    if min(lengths) < 0:
        raise ValueError("SearchInNeighborsResident: slot %d is not live in the store" % ([cur_slot] + slots.tolist())[lengths.index(min(lengths))])
    n_cur = lengths[0]
    if rev_cap is None:
        rev_cap = sum(lengths[1:])
    rev_cap = int(rev_cap)
    fwd = np.full((n, max(n_cur, 0)), -1, np.int32)
    rev_point = np.full(max(rev_cap, 1), -1, np.int32)
    rev_best = np.full(max(rev_cap, 1), -1, np.int32)
    n_rev = C.c_int32()
    capi.check(L.rumi_search_in_neighbors_resident(matcher._h, store._h, int(cur_slot), C.byref(cur), capi.ptr(slots) if n else None,
                                                   C.byref(arr) if n else None, n, float(th), capi.ptr(fwd if fwd.size else np.zeros(1, np.int32)),
                                                   capi.ptr(rev_point), capi.ptr(rev_best), rev_cap, C.byref(n_rev)))
    return fwd, rev_point[:n_rev.value], rev_best[:n_rev.value]


def search_in_neighbors_stage_ms(matcher):
    """(validation + table, upload + kernels + download, write-out) of the matcher's last SearchInNeighborsResident call, ms."""
    out = np.zeros(3, np.float32)
    capi.check(_lib().rumi_search_in_neighbors_stage_ms(matcher._h, capi.ptr(out)))
    return out


# ---- SearchAndFuse ----
FUSE_HIT_DTYPE = np.dtype([("kf", "<i4"), ("point", "<i4"), ("feature", "<i4"), ("occupant", "<i4")])
assert FUSE_HIT_DTYPE.itemsize == 16


def SearchAndFuseResident(matcher, store, kf_slots, kfs, point_ids, th=4.0, hit_cap=None):
    """The searches of LoopClosing::SearchAndFuse over key-frames and points resident in ``store``: one device call for every corrected key-frame.
    ``kfs``: one RumiFuseKF per slot (see ``fuse_kf``) carrying the pose derived from the corrected Sim3, ORBmatcher.cc:1190-1191; ``point_ids``:
    the loop points (an id < 0 is passed over).  Returns (hits as FUSE_HIT_DTYPE in ascending (kf, point) order, hits per key-frame): only the
    pairs that found a feature travel back.  ``hit_cap``: first size of the hit list (default: 4 hits per list entry, 1024 at least); when the
    call answers RUMI_E_CAPACITY the list is grown once to the count it reported and the call is made again."""
    L = _lib()
    n = len(kf_slots)
    assert len(kfs) == n
    slots = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
    ids = np.ascontiguousarray(point_ids, np.int32).reshape(-1)
    arr = (RumiFuseKF * max(n, 1))(*kfs)
    cap = max(1024, 4 * len(ids)) if hit_cap is None else int(hit_cap)
    per = np.zeros(max(n, 1), np.int32)
    n_hits = C.c_int32()
    for attempt in range(2):
        hits = np.zeros(max(cap, 1), FUSE_HIT_DTYPE)
        rc = L.rumi_search_and_fuse_resident(matcher._h, store._h, capi.ptr(slots) if n else None, C.byref(arr) if n else None, n,
                                             capi.ptr(ids) if len(ids) else None, len(ids), float(th), capi.ptr(hits), cap, C.byref(n_hits), capi.ptr(per))
        if rc != capi.RUMI_E_CAPACITY or attempt or n_hits.value <= cap:
            break
        cap = n_hits.value
    capi.check(rc)
    return hits[:n_hits.value], per[:n]


def search_and_fuse_stage_ms(matcher):
    """(validation + table, upload + kernels + download, write-out) of the matcher's last SearchAndFuseResident call, ms."""
    out = np.zeros(3, np.float32)
    capi.check(_lib().rumi_search_and_fuse_stage_ms(matcher._h, capi.ptr(out)))
    return out


# ---- SearchByProjection(KeyFrame*, Sim3f&, points, ...) of place recognition ----
SIM3_PROJ_JOB_DTYPE = np.dtype([("kf_slot", "<i4"), ("Tcw7", "<f4", 7), ("Ow", "<f4", 3), ("bounds", "<f4", 4), ("log_scale_factor", "<f4"),
                                ("point_start", "<i4"), ("point_count", "<i4"), ("th", "<i4"), ("ratio_hamming", "<f4"), ("explicit_invz", "<i4")])
assert SIM3_PROJ_JOB_DTYPE.itemsize == 84          # RumiSim3ProjJob


def sim3_proj_job(kf_slot, Tcw7, Ow, bounds, log_sf, point_start, point_count, th, ratio_hamming, explicit_invz=False):
    """One RumiSim3ProjJob as a record of SIM3_PROJ_JOB_DTYPE: the key-frame's slot, the pose derived from Scw (ORBmatcher.cc:380-381), its bounds and
    mfLogScaleFactor, the job's range of the call's point ids, th, the Hamming ratio and which overload's projection to use."""
    j = np.zeros((), SIM3_PROJ_JOB_DTYPE)
    j["kf_slot"], j["Tcw7"], j["Ow"], j["bounds"], j["log_scale_factor"] = kf_slot, np.float32(Tcw7), np.float32(Ow), np.float32(bounds), log_sf
    j["point_start"], j["point_count"], j["th"], j["ratio_hamming"], j["explicit_invz"] = point_start, point_count, th, ratio_hamming, int(explicit_invz)
    return j


def SearchByProjectionSim3Resident(matcher, store, jobs, point_ids):
    """Every SearchByProjection(KeyFrame*, Sim3f&, ...) call of a place-recognition stage over key-frames and points resident in ``store``: one
    device call.  ``jobs``: a structured array of SIM3_PROJ_JOB_DTYPE (see ``sim3_proj_job``); ``point_ids``: the ids the jobs' ranges index.
    Returns (matched_rows, nmatches): matched_rows[j][f] is the position inside job j's list of the point left in vpMatched[f], or -1; every job
    starts from an all-NULL vpMatched."""
    L = _lib()
    jobs = np.ascontiguousarray(jobs, SIM3_PROJ_JOB_DTYPE).reshape(-1)
    ids = np.ascontiguousarray(point_ids, np.int32).reshape(-1)
    n = len(jobs)
    start = np.zeros(n + 1, np.int32)
    nm = np.zeros(max(n, 1), np.int32)
    lengths = [store.row_length(int(s)) for s in jobs["kf_slot"]]
    cap = sum(max(x, 0) for x in lengths)
    for attempt in range(2):
        rows = np.full(max(cap, 1), -1, np.int32)
        rc = L.rumi_search_by_projection_sim3_resident(matcher._h, store._h, capi.ptr(jobs) if n else None, n, capi.ptr(ids) if len(ids) else None,
                                                       len(ids), capi.ptr(rows), capi.ptr(start), cap, capi.ptr(nm))
        if rc != capi.RUMI_E_CAPACITY or attempt or int(start[n]) <= cap:
            break
        cap = int(start[n])
    capi.check(rc)
    return [rows[start[j]:start[j + 1]] for j in range(n)], nm[:n]


def search_by_projection_sim3_stage_ms(matcher):
    """(validation + table, upload + kernels + download, write-out) of the matcher's last SearchByProjectionSim3Resident call, ms."""
    out = np.zeros(3, np.float32)
    capi.check(_lib().rumi_search_by_projection_sim3_stage_ms(matcher._h, capi.ptr(out)))
    return out


def search_by_projection_sim3_rounds(matcher, n_jobs):
    """Rounds the ordered resolve took for each job of the matcher's last SearchByProjectionSim3Resident call."""
    out = np.zeros(max(int(n_jobs), 1), np.int32)
    capi.check(_lib().rumi_search_by_projection_sim3_rounds(matcher._h, capi.ptr(out), int(n_jobs)))
    return out[:int(n_jobs)]


# ---- the BoW stage of DetectCommonRegionsFromBoW by slot ----
def CommonRegionsBoWResident_status(matcher, store, cur_slot, groups, nnratio=None, check_ori=None, want_matches12=True, fill=-1, n=None, null_out=None):
    """``rumi_common_regions_bow_resident`` with its status code instead of an exception.  matcher / store may be None (a NULL handle);
    ``groups``: one list of slots per candidate, None (a NULL group_start), or a tuple (group_start, member_slot) that goes in as given, for a
    caller that wants them malformed.  The outputs start out filled with ``fill``; ``n``: the row width when the current slot cannot tell;
    ``null_out``: which of the six outputs goes in as NULL (1 .. 5; 0 is want_matches12=False).
    Returns (rc, matches12 or None, nmatches, matched_point, matched_member, num_bow_matches, most_matches)."""
    L = _lib()
    if n is None:
        n = max(store.row_length(int(cur_slot)), 0) if store is not None else 0
    start = member = None
    if groups is not None:
        if isinstance(groups, tuple):
            start = np.ascontiguousarray(groups[0], np.int32)
            member = None if groups[1] is None else np.ascontiguousarray(groups[1], np.int32)
        else:
            start = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
            member = np.array([k for g in groups for k in g], np.int32)
    G = 0 if start is None else len(start) - 1
    M = 0 if member is None else len(member)
    out = [np.full((M, n), fill, np.int32) if want_matches12 else None, np.full(M, fill, np.int32), np.full((G, n), fill, np.int32),
           np.full((G, n), fill, np.int32), np.full(G, fill, np.int32), np.full((G, 2), fill, np.int32)]
    p = lambda a: None if a is None else capi.ptr(a)
    ratio = nnratio if nnratio is not None else (matcher.mfNNratio if matcher is not None else 0.9)
    ori = check_ori if check_ori is not None else (matcher.mbCheckOrientation if matcher is not None else True)
    rc = L.rumi_common_regions_bow_resident(matcher._h if matcher is not None else None, store._h if store is not None else None, int(cur_slot), G, p(start),
                                            p(member), float(ratio), int(ori),
                                            *[None if i == null_out else p(a) for i, a in enumerate(out)])
    return (rc, *out)


def CommonRegionsBoWResident(matcher, store, cur_slot, groups, nnratio=None, check_ori=None, want_matches12=False):
    """The BoW stage of LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:576-651) for every candidate in one call, over key-frames
    resident in ``store`` (a covis.Covisibility): the current key-frame's slot and one list of member slots per candidate, in vpCovKFi order.
    nnratio / check_ori default to the handle's.  Returns (matches12 [M, n] or None when not asked for, nmatches [M], matched_point [G, n] as
    store point ids, matched_member [G, n], num_bow_matches [G], most_matches [G, 2])."""
    r = CommonRegionsBoWResident_status(matcher, store, cur_slot, groups, nnratio, check_ori, want_matches12)
    capi.check(r[0])
    return r[1:]


def common_regions_bow_resident_stage_ms(matcher):
    """(validation + table, store flush + upload + kernels + download, write-out) of the matcher's last CommonRegionsBoWResident call, ms."""
    out = np.zeros(3, np.float32)
    capi.check(_lib().rumi_common_regions_bow_resident_stage_ms(matcher._h, capi.ptr(out)))
    return out


# ---- map-point refresh ----
REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH = 1, 2
REFRESH_MAX_OBS = 2048

REFRESH_POINT_DTYPE = np.dtype([("pos", "<f4", 3), ("ref_kf", "<i4"), ("ref_feature", "<i4"), ("ref_level", "<i4"), ("obs_begin", "<i4"),
                                ("obs_end", "<i4")])
assert REFRESH_POINT_DTYPE.itemsize == 32


class RumiRefreshKF(C.Structure):
    _fields_ = [("desc", C.c_void_p), ("n", C.c_int32), ("nlevels", C.c_int32), ("scale_factors", C.c_void_p), ("Ow", C.c_float * 3),
                ("is_bad", C.c_uint8), ("pad_", C.c_uint8 * 3)]


assert C.sizeof(RumiRefreshKF) == 40


class RefreshBatch:
    """The arguments of one rumi_refresh_map_points call, marshalled (keeps the arrays alive).  ``keyframes``: (mDescriptors [n, 32] uint8,
    mvScaleFactors, camera centre, isBad) per key-frame; ``points``: (world position, reference key-frame index, ref_feature, ref_level,
    [(key-frame index, feature index), ...] in the order the map iterates them) per point."""

    def __init__(self, keyframes, points):
        self._keep = []
        self.n_kf = len(keyframes)
        self.kf = (RumiRefreshKF * max(self.n_kf, 1))()
        for k, (desc, sf, Ow, bad) in enumerate(keyframes):
            desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
            sf = np.ascontiguousarray(sf, np.float32)
            self._keep += [desc, sf]
            c = self.kf[k]
            c.desc, c.n, c.nlevels, c.scale_factors, c.is_bad = desc.ctypes.data, len(desc), len(sf), sf.ctypes.data, int(bool(bad))
            c.Ow[:] = np.asarray(Ow, np.float32).tolist()
        self.pts = np.zeros(max(len(points), 1), REFRESH_POINT_DTYPE)
        self.n_pts = len(points)
        okf, ofeat = [], []
        for i, (pos, ref_kf, ref_feature, ref_level, obs) in enumerate(points):
            self.pts[i] = (np.asarray(pos, np.float32), ref_kf, ref_feature, ref_level, len(okf), len(okf) + len(obs))
            okf += [o[0] for o in obs]
            ofeat += [o[1] for o in obs]
        self.n_obs = len(okf)
        self.obs_kf = np.array(okf + [0], np.int32)
        self.obs_feature = np.array(ofeat + [0], np.int32)

    def outputs(self, fill=0):
        """Fresh output arrays, every byte ``fill``."""
        n = max(self.n_pts, 1)
        shapes = dict(best_obs=(n, np.int32), best_median=(n, np.int32), normal=((n, 3), np.float32), min_distance=(n, np.float32),
                      max_distance=(n, np.float32), updated=(n, np.uint8))
        out = {}
        for k, (shape, dt) in shapes.items():
            a = np.empty(shape, dt)
            a.view(np.uint8).fill(fill)
            out[k] = a
        return out

    def args(self, what, out):
        """The argument tuple after the handle (the oracle of the tests takes the same)."""
        return (C.byref(self.kf), self.n_kf, capi.ptr(self.pts), self.n_pts, capi.ptr(self.obs_kf), capi.ptr(self.obs_feature), self.n_obs, int(what),
                capi.ptr(out["best_obs"]), capi.ptr(out["best_median"]), capi.ptr(out["normal"]), capi.ptr(out["min_distance"]),
                capi.ptr(out["max_distance"]), capi.ptr(out["updated"]))


class MapPointRefresher:
    """A rumi_refresh handle (the blocks of its calls); one per calling thread."""

    def __init__(self, device=-1):
        self._lib = _lib()
        h = C.c_void_p()
        capi.check(self._lib.rumi_refresh_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            self._lib.rumi_refresh_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def stage_ms(self):
        """(validation + gather, upload + kernels + download, write-out) of the last call, host wall-clock ms."""
        out = np.zeros(3, np.float32)
        capi.check(self._lib.rumi_refresh_stage_ms(self._h, capi.ptr(out)))
        return out

    def status(self, batch, what, out):
        """The raw status of one call (outputs in ``out``)."""
        return self._lib.rumi_refresh_map_points(self._h, *batch.args(what, out))


    def status_resident(self, store, ids, what, flags, out):
        """The raw status of one rumi_refresh_map_points_resident call (outputs in ``out``, see refresh_resident_outputs)."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        return self._lib.rumi_refresh_map_points_resident(self._h, store._h, capi.ptr(ids), len(ids), int(what), int(flags), capi.ptr(out["best_obs"]),
                                                          capi.ptr(out["best_median"]), capi.ptr(out["desc"]), capi.ptr(out["normal"]),
                                                          capi.ptr(out["min_distance"]), capi.ptr(out["max_distance"]), capi.ptr(out["updated"]))

    def last_launches(self):
        """Kernels the last resident call launched itself."""
        return int(self._lib.rumi_refresh_last_launches(self._h))


REFRESH_WRITE_BACK = 1


def refresh_resident_outputs(n_pts, fill=0):
    """Fresh output arrays of the resident entry, every byte ``fill``: those of RefreshBatch.outputs and desc [n, 32]."""
    n = max(int(n_pts), 1)
    shapes = dict(best_obs=(n, np.int32), best_median=(n, np.int32), desc=((n, 32), np.uint8), normal=((n, 3), np.float32),
                  min_distance=(n, np.float32), max_distance=(n, np.float32), updated=(n, np.uint8))
    out = {}
    for k, (shape, dt) in shapes.items():
        a = np.empty(shape, dt)
        a.view(np.uint8).fill(fill)
        out[k] = a
    return out


def RefreshMapPointsResident(refresher, store, ids, what=REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH, write_back=True, out=None):
    """ComputeDistinctiveDescriptors and / or UpdateNormalAndDepth of the points ``ids`` of a covis.Covisibility store, read where the store
    keeps them; with ``write_back`` the store's attribute records take the results.  Returns the dict of RefreshMapPoints plus desc [n, 32]
    (the winning row where best_obs >= 0)."""
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    out = refresh_resident_outputs(len(ids)) if out is None else out
    capi.check(refresher.status_resident(store, ids, what, REFRESH_WRITE_BACK if write_back else 0, out))
    return {k: v[:len(ids)] for k, v in out.items()}


_refresher = None


def RefreshMapPoints(batch, what=REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH, refresher=None, out=None):
    """ComputeDistinctiveDescriptors and / or UpdateNormalAndDepth for every point of ``batch`` in one device call.  Returns a dict of
    best_obs, best_median (position in the point's own observation list of the descriptor to clone, -1 = leave the descriptor; its median),
    normal [n, 3], min_distance, max_distance, updated; the arrays of a mode not asked for keep what ``out`` (or zeros) held."""
    global _refresher
    if refresher is None:
        if _refresher is None:
            _refresher = MapPointRefresher()
        refresher = _refresher
    out = batch.outputs() if out is None else out
    capi.check(refresher.status(batch, what, out))
    return {k: v[:batch.n_pts] for k, v in out.items()}


# ---- key-frame culling ----
CULL_CLOUD, CULL_ABORT_BA = 1, 2
CULL_NOT_REACHED, CULL_SKIPPED_CLOUD, CULL_SKIPPED_INIT, CULL_SKIPPED_BAD, CULL_KEPT, CULL_CULLED, CULL_TO_BE_ERASED = range(7)
CULL_MAX_KEYFRAMES = 65536

CULL_POINT_DTYPE = np.dtype([("obs_begin", "<i4"), ("obs_end", "<i4"), ("n_obs_count", "<i4"), ("is_bad", "u1"), ("pad_", "u1", 3)])
assert CULL_POINT_DTYPE.itemsize == 16


class RumiCullKF(C.Structure):
    _fields_ = [("octave", C.c_void_p), ("mp", C.c_void_p), ("n", C.c_int32), ("is_bad", C.c_uint8), ("is_init", C.c_uint8),
                ("not_erase", C.c_uint8), ("is_cloud", C.c_uint8)]


assert C.sizeof(RumiCullKF) == 24


class CullBatch:
    """The arguments of one rumi_keyframe_culling call, marshalled (keeps the arrays alive).  ``keyframes``: (octave [n], mp [n] as indices
    into ``points`` or -1, isBad, is the initial key-frame, mbNotErase, isCloud) per key-frame; ``cand``: the covisible list as indices into
    ``keyframes``; ``points``: (isBad, Observations(), [(key-frame index, feature index), ...]) per point."""

    def __init__(self, keyframes, cand, points):
        self._keep = []
        self.n_kf = len(keyframes)
        self.kf = (RumiCullKF * max(self.n_kf, 1))()
        for k, (octave, mp, bad, init, not_erase, cloud) in enumerate(keyframes):
            octave = np.ascontiguousarray(octave, np.int32)
            mp = np.ascontiguousarray(mp, np.int32)
            assert len(octave) == len(mp)
            self._keep += [octave, mp]
            c = self.kf[k]
            c.octave, c.mp, c.n = octave.ctypes.data, mp.ctypes.data, len(mp)
            c.is_bad, c.is_init, c.not_erase, c.is_cloud = int(bool(bad)), int(bool(init)), int(bool(not_erase)), int(bool(cloud))
        self.n_cand = len(cand)
        self.cand = np.array(list(cand) + [0], np.int32)
        self.n_pts = len(points)
        self.pts = np.zeros(max(self.n_pts, 1), CULL_POINT_DTYPE)
        okf, ofeat = [], []
        for i, (bad, n_obs_count, obs) in enumerate(points):
            self.pts[i] = (len(okf), len(okf) + len(obs), n_obs_count, int(bool(bad)), 0)
            okf += [o[0] for o in obs]
            ofeat += [o[1] for o in obs]
        self.n_obs = len(okf)
        self.obs_kf = np.array(okf + [0], np.int32)
        self.obs_feature = np.array(ofeat + [0], np.int32)

    def outputs(self, fill=0):
        """Fresh output arrays, every byte ``fill``."""
        n = max(self.n_cand, 1)
        out = {}
        for k, m in (("status", n), ("n_mps", n), ("n_redundant", n), ("culled", n), ("n_culled", 1)):
            a = np.empty(m, np.int32)
            a.view(np.uint8).fill(fill)
            out[k] = a
        return out

    def args(self, flags, out):
        """The argument tuple after the handle (the oracle of the tests takes the same, and more)."""
        return (C.byref(self.kf), self.n_kf, capi.ptr(self.cand), self.n_cand, capi.ptr(self.pts), self.n_pts, capi.ptr(self.obs_kf),
                capi.ptr(self.obs_feature), self.n_obs, int(flags), capi.ptr(out["status"]), capi.ptr(out["n_mps"]), capi.ptr(out["n_redundant"]),
                capi.ptr(out["culled"]), capi.ptr(out["n_culled"]))


class KeyFrameCuller:
    """A rumi_cull handle (the blocks of its calls); one per calling thread."""

    def __init__(self, device=-1):
        self._lib = _lib()
        h = C.c_void_p()
        capi.check(self._lib.rumi_cull_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            self._lib.rumi_cull_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def stage_ms(self):
        """(validation + pack, upload + kernels + download, write-out) of the last call, host wall-clock ms."""
        out = np.zeros(3, np.float32)
        capi.check(self._lib.rumi_cull_stage_ms(self._h, capi.ptr(out)))
        return out

    def status(self, batch, flags, out):
        """The raw status of one call (outputs in ``out``)."""
        return self._lib.rumi_keyframe_culling(self._h, *batch.args(flags, out))


    def status_resident(self, store, candidates, flags, out):
        """The raw status of one rumi_keyframe_culling_resident call (outputs in ``out``)."""
        return cull_resident_status(self, store, candidates, flags, out)


CULL_CANDIDATE_DTYPE = np.dtype([("slot", "<i4"), ("is_init", "u1"), ("not_erase", "u1"), ("is_cloud", "u1"), ("pad_", "u1")])
assert CULL_CANDIDATE_DTYPE.itemsize == 8


def cull_candidates(candidates):
    """(slot, is_init, not_erase, is_cloud) tuples, or an array of CULL_CANDIDATE_DTYPE -> the records of one call."""
    if isinstance(candidates, np.ndarray) and candidates.dtype == CULL_CANDIDATE_DTYPE:
        return np.ascontiguousarray(candidates)
    rec = np.zeros(len(candidates), CULL_CANDIDATE_DTYPE)
    for i, (slot, init, not_erase, cloud) in enumerate(candidates):
        rec[i] = (int(slot), int(bool(init)), int(bool(not_erase)), int(bool(cloud)), 0)
    return rec


def cull_outputs(n_cand, fill=0):
    """Fresh output arrays of a culling call over n_cand candidates, every byte ``fill``."""
    out = {}
    for k, m in (("status", max(n_cand, 1)), ("n_mps", max(n_cand, 1)), ("n_redundant", max(n_cand, 1)), ("culled", max(n_cand, 1)), ("n_culled", 1)):
        a = np.empty(m, np.int32)
        a.view(np.uint8).fill(fill)
        out[k] = a
    return out


def cull_resident_status(cull, store, candidates, flags, out):
    """The raw call; ``cull`` a KeyFrameCuller or None, ``store`` a covis.Covisibility or None (a missing handle is the library's to refuse)."""
    rec = cull_candidates(candidates)
    h = cull._h if cull is not None else None
    s = store._h if store is not None else None
    return _lib().rumi_keyframe_culling_resident(h, s, capi.ptr(rec) if len(rec) else None, len(rec), int(flags), capi.ptr(out["status"]),
                                                 capi.ptr(out["n_mps"]), capi.ptr(out["n_redundant"]), capi.ptr(out["culled"]), capi.ptr(out["n_culled"]))


def KeyFrameCullingResident(cull, store, candidates, flags=0):
    """KeyFrameCulling (flags & CULL_CLOUD: CloudKeyFrameCulling) over the key-frames ``candidates`` names by slot in ``store`` (a
    covis.Covisibility whose points were set through set_point_observations and whose key-frames hold features): only the store's staged
    edits and the candidate records travel.  Returns what keyframe_culling returns."""
    rec = cull_candidates(candidates)
    out = cull_outputs(len(rec))
    capi.check(cull_resident_status(cull, store, rec, flags, out))
    n = int(out["n_culled"][0])
    return dict(status=out["status"][:len(rec)], n_mps=out["n_mps"][:len(rec)], n_redundant=out["n_redundant"][:len(rec)], culled=out["culled"][:n])


_culler = None


def trim(batch, out):
    """The outputs cut to their lengths: status, n_mps, n_redundant [n_cand], culled [n_culled]."""
    n = int(out["n_culled"][0])
    return dict(status=out["status"][:batch.n_cand], n_mps=out["n_mps"][:batch.n_cand], n_redundant=out["n_redundant"][:batch.n_cand],
                culled=out["culled"][:n])


def keyframe_culling(batch, cloud=False, abort_ba=False, culler=None, out=None):
    """KeyFrameCulling (``cloud``: CloudKeyFrameCulling) over ``batch`` in one device call.  Returns a dict of status (CULL_*), n_mps,
    n_redundant per candidate and culled, the positions in the covisible list to call SetBadFlag() on, in order."""
    global _culler
    if culler is None:
        if _culler is None:
            _culler = KeyFrameCuller()
        culler = _culler
    out = batch.outputs() if out is None else out
    capi.check(culler.status(batch, (CULL_CLOUD if cloud else 0) | (CULL_ABORT_BA if abort_ba else 0), out))
    return trim(batch, out)
