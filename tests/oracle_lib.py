"""ctypes binding of oracle/liboracle.so — the CPU restatement used as the parity checker.
TEST INFRASTRUCTURE ONLY: nothing under rumi_slam_amd/ may import this."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28

_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", ORACLE_DIR])


def lib():
    global _lib
    if _lib is None:
        so = os.environ.get("RUMI_ORACLE_SO") or os.path.join(ORACLE_DIR, "liboracle.so")   # override: a sanitizer build of the same sources
        if not os.path.exists(so):
            build()
        _lib = C.CDLL(so)
        _lib.orc_orb_create.restype = C.c_void_p
        _lib.orc_orb_create.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]
        _lib.orc_orb_destroy.argtypes = [C.c_void_p]
        _lib.orc_orb_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        _lib.orc_orb_tables.argtypes = [C.c_void_p] + [C.c_void_p] * 6
        _lib.orc_orb_level_size.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _lib.orc_orb_get_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib.orc_orb_get_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        _lib.orc_cv_round.argtypes = [C.c_double]
        _lib.orc_fast_atan2.restype = C.c_float
        _lib.orc_fast_atan2.argtypes = [C.c_float, C.c_float]
        _lib.orc_resize_linear.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
        _lib.orc_gaussian_blur.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib.orc_gaussian_blur_variant.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        _lib.orc_orb_set_blur_variant.argtypes = [C.c_void_p, C.c_int]
        _lib.orc_fast_score.argtypes = [C.c_void_p, C.c_int]
        _lib.orc_fast_cell.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        _lib.orc_octree.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class OracleExtractor:
    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, blur_variant=0):
        self.L = lib()
        self.nlevels = nlevels
        self.nfeatures = nfeatures
        self.h = C.c_void_p(self.L.orc_orb_create(nfeatures, scale_factor, nlevels, ini_th, min_th))
        if blur_variant:
            self.L.orc_orb_set_blur_variant(self.h, int(blur_variant))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.orc_orb_destroy(self.h)
            self.h = None

    def tables(self):
        n = self.nlevels
        f = [np.zeros(n, np.float32) for _ in range(4)]
        per = np.zeros(n, np.int32)
        umax = np.zeros(16, np.int32)
        self.L.orc_orb_tables(self.h, *[_p(a) for a in f], _p(per), _p(umax))
        return dict(scale=f[0], inv_scale=f[1], sigma2=f[2], inv_sigma2=f[3], per_level=per, umax=umax)

    def extract(self, img, lap=(0, 1000)):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        cap = self.nfeatures * 4 + 4096
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        mono = self.L.orc_orb_extract(self.h, _p(img), w, h, w, lap[0], lap[1], _p(kps), _p(desc), cap, C.byref(n))
        assert mono != -2, "oracle capacity"
        return mono, kps[:n.value].copy(), desc[:n.value].copy()

    def level(self, l, blurred=False):
        w, h = C.c_int(), C.c_int()
        self.L.orc_orb_level_size(self.h, l, C.byref(w), C.byref(h))
        out = np.zeros((h.value, w.value), np.uint8)
        got = self.L.orc_orb_get_level(self.h, l, 1 if blurred else 0, _p(out))
        return out if got else None

    def keypoints(self, l, selected):
        n = self.L.orc_orb_get_keypoints(self.h, l, 1 if selected else 0, None, 0)
        out = np.zeros(max(n, 1), KP_DTYPE)
        self.L.orc_orb_get_keypoints(self.h, l, 1 if selected else 0, _p(out), n)
        return out[:n]


def fast_atan2(y, x):
    return float(lib().orc_fast_atan2(float(y), float(x)))


def resize_linear(src, dw, dh):
    src = np.ascontiguousarray(src, np.uint8)
    dst = np.zeros((dh, dw), np.uint8)
    lib().orc_resize_linear(_p(src), src.shape[1], src.shape[0], _p(dst), dw, dh)
    return dst


def gaussian_blur(src, variant=0):
    src = np.ascontiguousarray(src, np.uint8)
    dst = np.zeros_like(src)
    lib().orc_gaussian_blur_variant(_p(src), src.shape[1], src.shape[0], _p(dst), int(variant))
    return dst


def fast_cell(img, threshold):
    img = np.ascontiguousarray(img, np.uint8)
    cap = img.size
    out = np.zeros(max(cap, 1), KP_DTYPE)
    n = lib().orc_fast_cell(_p(img), img.shape[1], img.shape[1], img.shape[0], threshold, _p(out), cap)
    return out[:n].copy()


def octree(cand, min_x, max_x, min_y, max_y, n_want):
    cand = np.ascontiguousarray(cand, KP_DTYPE)
    out = np.zeros(len(cand) + 1, KP_DTYPE)
    m = lib().orc_octree(_p(cand), len(cand), min_x, max_x, min_y, max_y, n_want, _p(out), len(out))
    return out[:m].copy()


# ---------------------------------------------------------------------------------------------------------
# matchers (oracle/match_oracle.cc)
# ---------------------------------------------------------------------------------------------------------
def _mlib():
    L = lib()
    if getattr(L, "_m_ready", False):
        return L
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.orc_descriptor_distance.argtypes = [vp, vp]
    L.orc_features_in_area.argtypes = [vp, i32, f32, f32, f32, f32, f32, f32, f32, i32, i32, vp, i32]
    L.orc_search_by_projection_mappoints.argtypes = [vp, vp, i32, f32, f32, f32, f32, vp, i32] + [vp] * 9 + [f32, i32, f32, f32, vp]
    L.orc_search_by_projection_frame.argtypes = [vp, vp, i32, f32, f32, f32, f32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, f32, i32, vp]
    L.orc_search_by_bow.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, f32, i32, vp]
    L.orc_undistort_points.argtypes = [vp, i32, vp, vp, vp]
    L.orc_undistort_points.restype = None
    L.orc_image_bounds.argtypes = [i32, i32, vp, vp, vp]
    L.orc_image_bounds.restype = None
    L.orc_bruteforce_match.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    L.orc_search_for_initialization.argtypes = [vp, vp, i32, vp, vp, i32, f32, f32, f32, f32, vp, i32, f32, i32, vp]
    L.orc_search_for_initialization.restype = i32
    L.orc_search_for_triangulation.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, vp]
    L.orc_search_for_triangulation.restype = i32
    L.orc_fuse_candidates.argtypes = [vp, vp, i32, f32, f32, f32, f32, vp, i32, f32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, f32, i32, vp]
    L.orc_search_by_sim3.argtypes = [vp, vp, i32, vp, vp, i32, f32, f32, f32, f32, vp, i32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, vp]
    L.orc_search_by_sim3.restype = i32
    L.orc_is_in_frustum.argtypes = [vp, vp, vp, vp, f32, f32, f32, f32, f32, i32, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orc_search_by_bow_kf.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, i32, vp, f32, i32, vp]
    L.orc_search_by_projection_sim3.argtypes = [vp, vp, i32, f32, f32, f32, f32, vp, i32, f32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, f32, i32, vp]
    L.orc_search_by_projection_reloc.argtypes = [vp, vp, i32, f32, f32, f32, f32, vp, i32, f32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, f32, i32, i32, vp]
    L._m_ready = True
    return L


def descriptor_distance(a, b):
    a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
    return _mlib().orc_descriptor_distance(_p(a), _p(b))


def features_in_area(keys, w, h, x, y, r, min_level, max_level):
    keys = np.ascontiguousarray(keys, KP_DTYPE)
    out = np.zeros(len(keys) + 1, np.int32)
    n = _mlib().orc_features_in_area(_p(keys), len(keys), 0.0, 0.0, float(w), float(h), x, y, r, min_level, max_level, _p(out), len(out))
    return out[:n]


def search_by_projection_mappoints(keys, desc, w, h, sf, mp, frame_mp, th, far, th_far, nnratio):
    keys = np.ascontiguousarray(keys, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8); sf = np.ascontiguousarray(sf, np.float32)
    a = {k: np.ascontiguousarray(mp[k], t) for k, t in [("track_in_view", np.uint8), ("proj_x", np.float32), ("proj_y", np.float32),
                                                         ("scale_level", np.int32), ("view_cos", np.float32), ("track_depth", np.float32),
                                                         ("is_bad", np.uint8), ("desc", np.uint8), ("obs", np.int32)]}
    fm = np.ascontiguousarray(frame_mp, np.int32).copy()
    n = _mlib().orc_search_by_projection_mappoints(_p(keys), _p(desc), len(keys), *_bounds(w, h), _p(sf), len(a["proj_x"]),
                                                  _p(a["track_in_view"]), _p(a["proj_x"]), _p(a["proj_y"]), _p(a["scale_level"]),
                                                  _p(a["view_cos"]), _p(a["track_depth"]), _p(a["is_bad"]), _p(a["desc"]), _p(a["obs"]),
                                                  th, int(far), th_far, nnratio, _p(fm))
    return n, fm


def undistort_points(xy, K4, dist5):
    """Frame::UndistortKeyPoints' cv::undistortPoints(mat, mat, K, mDistCoef, cv::Mat(), mK) (oracle/frame_oracle.cc): [n,2] f32 -> [n,2] f32."""
    a = np.ascontiguousarray(xy, np.float32).reshape(-1, 2); K = np.ascontiguousarray(K4, np.float32); d = np.ascontiguousarray(dist5, np.float32)
    out = np.zeros_like(a)
    _mlib().orc_undistort_points(_p(a), len(a), _p(K), _p(d), _p(out))
    return out


def undistort_keys(keys, K4, dist5):
    """mvKeysUn from mvKeys (Frame.cc:770-797): copies of the key-points with pt replaced; mvKeysUn = mvKeys when mDistCoef[0] == 0."""
    out = np.ascontiguousarray(keys, KP_DTYPE).copy()
    if float(np.float32(dist5[0])) == 0.0:
        return out
    u = undistort_points(np.stack([out["x"], out["y"]], 1), K4, dist5)
    out["x"], out["y"] = u[:, 0], u[:, 1]
    return out


def image_bounds(w, h, K4, dist5):
    """Frame::ComputeImageBounds (Frame.cc:799-826): (mnMinX, mnMinY, mnMaxX, mnMaxY) f32."""
    K = np.ascontiguousarray(K4, np.float32); d = np.ascontiguousarray(dist5, np.float32)
    b = np.zeros(4, np.float32)
    _mlib().orc_image_bounds(int(w), int(h), _p(K), _p(d), _p(b))
    return b


def _bounds(w, h):
    """(w, h) of an undistorted camera, or w = (minX, minY, maxX, maxY) with h ignored."""
    if np.ndim(w) > 0:
        return tuple(float(x) for x in w)
    return 0.0, 0.0, float(w), float(h)


def search_by_projection_frame(cur_keys, cur_desc, w, h, sf, Tcw7, K4, last_keys, last_mp, last_outlier, mp_pos, mp_desc, mp_obs, cur_mp,
                               th, check_ori):
    arrs = [np.ascontiguousarray(cur_keys, KP_DTYPE), np.ascontiguousarray(cur_desc, np.uint8), np.ascontiguousarray(sf, np.float32),
            np.ascontiguousarray(Tcw7, np.float32), np.ascontiguousarray(K4, np.float32), np.ascontiguousarray(last_keys, KP_DTYPE),
            np.ascontiguousarray(last_mp, np.int32), np.ascontiguousarray(last_outlier, np.uint8), np.ascontiguousarray(mp_pos, np.float32),
            np.ascontiguousarray(mp_desc, np.uint8), np.ascontiguousarray(mp_obs, np.int32)]
    cm = np.ascontiguousarray(cur_mp, np.int32).copy()
    n = _mlib().orc_search_by_projection_frame(_p(arrs[0]), _p(arrs[1]), len(arrs[0]), *_bounds(w, h), _p(arrs[2]), _p(arrs[3]),
                                              _p(arrs[4]), _p(arrs[5]), len(arrs[5]), _p(arrs[6]), _p(arrs[7]), _p(arrs[8]), _p(arrs[9]),
                                              _p(arrs[10]), th, int(check_ori), _p(cm))
    return n, cm


def search_by_bow(kf_keys, kf_desc, kf_mp, mp_bad, kf_fv, f_keys, f_desc, f_fv, nnratio, check_ori):
    """kf_fv / f_fv: (node_ids u32, offsets i32, indices u32)."""
    kk = np.ascontiguousarray(kf_keys, KP_DTYPE); kd = np.ascontiguousarray(kf_desc, np.uint8); km = np.ascontiguousarray(kf_mp, np.int32)
    mb = np.ascontiguousarray(mp_bad, np.uint8); fk = np.ascontiguousarray(f_keys, KP_DTYPE); fd = np.ascontiguousarray(f_desc, np.uint8)
    out = np.full(len(fk), -1, np.int32)
    n = _mlib().orc_search_by_bow(_p(kk), _p(kd), len(kk), _p(km), _p(mb), _p(kf_fv[0]), _p(kf_fv[1]), _p(kf_fv[2]), len(kf_fv[0]),
                                  _p(fk), _p(fd), len(fk), _p(f_fv[0]), _p(f_fv[1]), _p(f_fv[2]), len(f_fv[0]), nnratio, int(check_ori), _p(out))
    return n, out


def bruteforce_match(q, t):
    q = np.ascontiguousarray(q, np.uint8); t = np.ascontiguousarray(t, np.uint8)
    bi, bd, sd = (np.zeros(len(q), np.int32) for _ in range(3))
    _mlib().orc_bruteforce_match(_p(q), len(q), _p(t), len(t), _p(bi), _p(bd), _p(sd))
    return bi, bd, sd


# ---------------------------------------------------------------------------------------------------------
# optimiser (oracle/opt_oracle.cc)
# ---------------------------------------------------------------------------------------------------------
def _olib():
    L = lib()
    if getattr(L, "_o_ready", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.orc_pose_optimization.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    L.orc_local_ba.argtypes = [i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L._o_ready = True
    return L


def pose_optimization(Xw, obs, inv_sigma2, K4, Tcw7):
    Xw = np.ascontiguousarray(Xw, np.float32); obs = np.ascontiguousarray(obs, np.float32)
    w = np.ascontiguousarray(inv_sigma2, np.float32); K4 = np.ascontiguousarray(K4, np.float32)
    T = np.ascontiguousarray(Tcw7, np.float32).copy()
    out = np.zeros(len(w), np.uint8)
    ngood = _olib().orc_pose_optimization(_p(Xw), _p(obs), _p(w), len(w), _p(K4), _p(T), _p(out))
    return ngood, T, out


def local_ba(kf_pose, kf_fixed, mp_pos, e_mp, e_kf, e_obs, e_inv_sigma2, K4, stop=None):
    kp = np.ascontiguousarray(kf_pose, np.float32).copy(); kfix = np.ascontiguousarray(kf_fixed, np.uint8)
    mp = np.ascontiguousarray(mp_pos, np.float32).copy(); em = np.ascontiguousarray(e_mp, np.int32); ek = np.ascontiguousarray(e_kf, np.int32)
    eo = np.ascontiguousarray(e_obs, np.float32); ew = np.ascontiguousarray(e_inv_sigma2, np.float32); K4 = np.ascontiguousarray(K4, np.float32)
    erase = np.zeros(len(em), np.uint8)
    sp = _p(stop) if stop is not None else None
    its = _olib().orc_local_ba(len(kfix), _p(kp), _p(kfix), len(mp), _p(mp), len(em), _p(em), _p(ek), _p(eo), _p(ew), _p(K4), sp, _p(erase))
    return its, kp, mp, erase


def bundle_adjustment(kf_pose, kf_fixed, mp_pos, e_mp, e_kf, e_obs, e_inv_sigma2, K4, n_iterations, robust):
    kp = np.ascontiguousarray(kf_pose, np.float32).copy(); kfix = np.ascontiguousarray(kf_fixed, np.uint8)
    mp = np.ascontiguousarray(mp_pos, np.float32).copy(); em = np.ascontiguousarray(e_mp, np.int32); ek = np.ascontiguousarray(e_kf, np.int32)
    eo = np.ascontiguousarray(e_obs, np.float32); ew = np.ascontiguousarray(e_inv_sigma2, np.float32); K4 = np.ascontiguousarray(K4, np.float32)
    L = _olib()
    L.orc_bundle_adjustment.restype = C.c_int32
    L.orc_bundle_adjustment.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_int32]
    its = L.orc_bundle_adjustment(len(kfix), _p(kp), _p(kfix), len(mp), _p(mp), len(em), _p(em), _p(ek), _p(eo), _p(ew), _p(K4), None, int(n_iterations), int(robust))
    return its, kp, mp


def merge_ba(kf_pose, kf_fixed, mp_pos, e_mp, e_kf, e_obs, e_inv_sigma2, K4, stop=None):
    """Returns (its of the two optimize() calls, kf_pose, mp_pos, erase)."""
    kp = np.ascontiguousarray(kf_pose, np.float32).copy(); kfix = np.ascontiguousarray(kf_fixed, np.uint8)
    mp = np.ascontiguousarray(mp_pos, np.float32).copy(); em = np.ascontiguousarray(e_mp, np.int32); ek = np.ascontiguousarray(e_kf, np.int32)
    eo = np.ascontiguousarray(e_obs, np.float32); ew = np.ascontiguousarray(e_inv_sigma2, np.float32); K4 = np.ascontiguousarray(K4, np.float32)
    erase = np.zeros(len(em), np.uint8)
    its2 = np.zeros(2, np.int32)
    sp = _p(stop) if stop is not None else None
    L = _olib()
    L.orc_merge_ba.restype = C.c_int32
    L.orc_merge_ba.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 8
    L.orc_merge_ba(len(kfix), _p(kp), _p(kfix), len(mp), _p(mp), len(em), _p(em), _p(ek), _p(eo), _p(ew), _p(K4), sp, _p(erase), _p(its2))
    return its2, kp, mp, erase


def opt_last_trace():
    """What the last pose_optimization / local_ba / merge_ba / bundle_adjustment call on this thread decided: dict(trials, rejected, ended_qmax,
    ended_rho0, rejected_run, margin) -- LM trials run, rejected trials, iterations that ended by qmax == 10 and by rho == 0, the most rejections in a
    row inside one iteration, the smallest
    |chi2 - th| / th over every threshold comparison the call made (inf when it made none), and as `gain` the smallest relative change of chi2 any
    trial made: how far the closest accept / reject decision was from a tie."""
    L = _olib()
    L.orc_opt_last_trace.restype = None
    L.orc_opt_last_trace.argtypes = [C.c_void_p, C.c_void_p]
    counts = np.zeros(5, np.int32); margin = np.zeros(2, np.float64)
    L.orc_opt_last_trace(_p(counts), _p(margin))
    return dict(trials=int(counts[0]), rejected=int(counts[1]), ended_qmax=int(counts[2]), ended_rho0=int(counts[3]), rejected_run=int(counts[4]), margin=float(margin[0]), gain=float(margin[1]))


def search_by_bow_kf(k1, d1, mp1, fv1, k2, d2, mp2, fv2, mp_bad, nnratio, check_ori):
    k1 = np.ascontiguousarray(k1, KP_DTYPE); d1 = np.ascontiguousarray(d1, np.uint8); m1 = np.ascontiguousarray(mp1, np.int32)
    k2 = np.ascontiguousarray(k2, KP_DTYPE); d2 = np.ascontiguousarray(d2, np.uint8); m2 = np.ascontiguousarray(mp2, np.int32)
    mb = np.ascontiguousarray(mp_bad, np.uint8)
    out = np.full(len(k1), -1, np.int32)
    n = _mlib().orc_search_by_bow_kf(_p(k1), _p(d1), len(k1), _p(m1), _p(fv1[0]), _p(fv1[1]), _p(fv1[2]), len(fv1[0]), _p(k2), _p(d2), len(k2),
                                     _p(m2), _p(fv2[0]), _p(fv2[1]), _p(fv2[2]), len(fv2[0]), _p(mb), nnratio, int(check_ori), _p(out))
    return n, out


def search_by_projection_sim3(keys, desc, w, h, sf, log_sf, Tcw7, Ow3, K4, pts, matched, th, ratio, variant):
    keys = np.ascontiguousarray(keys, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8); sf = np.ascontiguousarray(sf, np.float32)
    a = [np.ascontiguousarray(pts["skip"], np.uint8), np.ascontiguousarray(pts["pos"], np.float32), np.ascontiguousarray(pts["normal"], np.float32),
         np.ascontiguousarray(pts["min_dist"], np.float32), np.ascontiguousarray(pts["max_dist"], np.float32), np.ascontiguousarray(pts["desc"], np.uint8)]
    T = np.ascontiguousarray(Tcw7, np.float32); Ow = np.ascontiguousarray(Ow3, np.float32); K = np.ascontiguousarray(K4, np.float32)
    m = np.ascontiguousarray(matched, np.int32).copy()
    n = _mlib().orc_search_by_projection_sim3(_p(keys), _p(desc), len(keys), 0.0, 0.0, float(w), float(h), _p(sf), len(sf), float(log_sf), _p(T), _p(Ow),
                                              _p(K), len(a[0]), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), _p(a[5]), int(th), float(ratio),
                                              int(variant), _p(m))
    return n, m


def search_by_projection_reloc(cur_keys, cur_desc, w, h, sf, log_sf, Tcw7, Ow3, K4, kf_keys, kf_mp, pts, cur_mp, th, orb_dist, check_ori):
    ck = np.ascontiguousarray(cur_keys, KP_DTYPE); cd = np.ascontiguousarray(cur_desc, np.uint8); sf = np.ascontiguousarray(sf, np.float32)
    kk = np.ascontiguousarray(kf_keys, KP_DTYPE); km = np.ascontiguousarray(kf_mp, np.int32)
    a = [np.ascontiguousarray(pts["skip"], np.uint8), np.ascontiguousarray(pts["pos"], np.float32), np.ascontiguousarray(pts["min_dist"], np.float32),
         np.ascontiguousarray(pts["max_dist"], np.float32), np.ascontiguousarray(pts["desc"], np.uint8)]
    T = np.ascontiguousarray(Tcw7, np.float32); Ow = np.ascontiguousarray(Ow3, np.float32); K = np.ascontiguousarray(K4, np.float32)
    cm = np.ascontiguousarray(cur_mp, np.int32).copy()
    n = _mlib().orc_search_by_projection_reloc(_p(ck), _p(cd), len(ck), 0.0, 0.0, float(w), float(h), _p(sf), len(sf), float(log_sf), _p(T), _p(Ow), _p(K),
                                               _p(kk), len(kk), _p(km), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), float(th), int(orb_dist),
                                               int(check_ori), _p(cm))
    return n, cm


def is_in_frustum(Rcw9, tcw3, Ow3, K4, w, h, log_sf, nlevels, cos_limit, pts):
    n = len(pts["max_dist"])
    f = lambda a: np.ascontiguousarray(a, np.float32)
    R, t, Ow, K, pos, nrm, mn, mx = f(Rcw9), f(tcw3), f(Ow3), f(K4), f(pts["pos"]), f(pts["normal"]), f(pts["min_dist"]), f(pts["max_dist"])
    out = dict(track_in_view=np.zeros(n, np.uint8), proj_x=np.zeros(n, np.float32), proj_y=np.zeros(n, np.float32),
               scale_level=np.zeros(n, np.int32), view_cos=np.zeros(n, np.float32), track_depth=np.zeros(n, np.float32))
    _mlib().orc_is_in_frustum(_p(R), _p(t), _p(Ow), _p(K), *_bounds(w, h), float(log_sf), int(nlevels), float(cos_limit), n, _p(pos), _p(nrm),
                              _p(mn), _p(mx), _p(out["track_in_view"]), _p(out["proj_x"]), _p(out["proj_y"]), _p(out["scale_level"]), _p(out["view_cos"]),
                              _p(out["track_depth"]))
    return out


def search_for_initialization(keys1, desc1, keys2, desc2, w, h, prev_matched, window, nnratio, check_ori):
    k1 = np.ascontiguousarray(keys1, KP_DTYPE); d1 = np.ascontiguousarray(desc1, np.uint8)
    k2 = np.ascontiguousarray(keys2, KP_DTYPE); d2 = np.ascontiguousarray(desc2, np.uint8)
    pm = np.ascontiguousarray(prev_matched, np.float32).copy()
    m12 = np.full(len(k1), -1, np.int32)
    n = _mlib().orc_search_for_initialization(_p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2), 0.0, 0.0, float(w), float(h), _p(pm), int(window),
                                              float(nnratio), int(check_ori), _p(m12))
    return n, m12, pm


def search_for_triangulation(k1, d1, mp1, fv1, k2, d2, mp2, fv2, sf2, F12, ep, only_stereo, coarse, check_ori):
    k1 = np.ascontiguousarray(k1, KP_DTYPE); d1 = np.ascontiguousarray(d1, np.uint8); m1 = np.ascontiguousarray(mp1, np.int32)
    k2 = np.ascontiguousarray(k2, KP_DTYPE); d2 = np.ascontiguousarray(d2, np.uint8); m2 = np.ascontiguousarray(mp2, np.int32)
    sf2 = np.ascontiguousarray(sf2, np.float32); F = np.ascontiguousarray(F12, np.float32).ravel(); e = np.ascontiguousarray(ep, np.float32)
    out = np.full(len(k1), -1, np.int32)
    n = _mlib().orc_search_for_triangulation(_p(k1), _p(d1), len(k1), _p(m1), _p(fv1[0]), _p(fv1[1]), _p(fv1[2]), len(fv1[0]), _p(k2), _p(d2), len(k2),
                                             _p(m2), _p(fv2[0]), _p(fv2[1]), _p(fv2[2]), len(fv2[0]), _p(sf2), _p(F), _p(e), int(only_stereo),
                                             int(coarse), int(check_ori), _p(out))
    idx = np.nonzero(out >= 0)[0]
    return n, np.stack([idx, out[idx]], 1).astype(np.int64)


def fuse_candidates(keys, desc, w, h, sf, log_sf, Tcw7, Ow3, K4, pts, th, check_reproj):
    keys = np.ascontiguousarray(keys, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8); sf = np.ascontiguousarray(sf, np.float32)
    a = [np.ascontiguousarray(pts["skip"], np.uint8), np.ascontiguousarray(pts["pos"], np.float32), np.ascontiguousarray(pts["normal"], np.float32),
         np.ascontiguousarray(pts["min_dist"], np.float32), np.ascontiguousarray(pts["max_dist"], np.float32), np.ascontiguousarray(pts["desc"], np.uint8)]
    T = np.ascontiguousarray(Tcw7, np.float32); Ow = np.ascontiguousarray(Ow3, np.float32); K = np.ascontiguousarray(K4, np.float32)
    out = np.full(len(a[0]), -1, np.int32)
    _mlib().orc_fuse_candidates(_p(keys), _p(desc), len(keys), 0.0, 0.0, float(w), float(h), _p(sf), len(sf), float(log_sf), _p(T), _p(Ow), _p(K),
                                len(a[0]), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), _p(a[5]), float(th), int(check_reproj), _p(out))
    return out


def search_by_sim3(k1, d1, k2, d2, w, h, sf, log_sf, K4, side1, side2, th):
    k1 = np.ascontiguousarray(k1, KP_DTYPE); d1 = np.ascontiguousarray(d1, np.uint8); k2 = np.ascontiguousarray(k2, KP_DTYPE); d2 = np.ascontiguousarray(d2, np.uint8)
    sf = np.ascontiguousarray(sf, np.float32); K = np.ascontiguousarray(K4, np.float32)
    def prep(d):
        return [np.ascontiguousarray(d["skip"], np.uint8), np.ascontiguousarray(d["pc"], np.float32), np.ascontiguousarray(d["min_dist"], np.float32),
                np.ascontiguousarray(d["max_dist"], np.float32), np.ascontiguousarray(d["desc"], np.uint8)]
    a, b = prep(side1), prep(side2)
    out = np.full(len(k1), -1, np.int32)
    n = _mlib().orc_search_by_sim3(_p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2), 0.0, 0.0, float(w), float(h), _p(sf), len(sf), float(log_sf), _p(K),
                                   *[_p(x) for x in a], *[_p(x) for x in b], float(th), _p(out))
    return n, out


class OracleVocabulary:
    """DBoW2 vocabulary tree + transform restated on the CPU (oracle/voc_oracle.cc)."""

    def __init__(self, parent, is_leaf, desc, weight, weighting=0, scoring=0):
        L = lib()
        vp, i32 = C.c_void_p, C.c_int32
        L.orc_voc_create.restype = vp
        L.orc_voc_create.argtypes = [i32, vp, vp, vp, vp, i32, i32]
        L.orc_voc_destroy.argtypes = [vp]
        L.orc_voc_transform_features.argtypes = [vp, vp, i32, i32, vp, vp, vp]
        L.orc_voc_transform.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        self._L = L
        a = [np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(is_leaf, np.uint8), np.ascontiguousarray(desc, np.uint8),
             np.ascontiguousarray(weight, np.float64)]
        self._h = L.orc_voc_create(len(a[0]), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), int(weighting), int(scoring))
        L.orc_voc_set_levels.argtypes = [vp, i32]

    def set_levels(self, levels):
        self._L.orc_voc_set_levels(self._h, int(levels))

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.orc_voc_destroy(self._h)
            self._h = None

    def transform_features(self, desc, levelsup=4):
        d = np.ascontiguousarray(desc, np.uint8)
        n = len(d)
        word, node, w = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float64)
        self._L.orc_voc_transform_features(self._h, _p(d), n, int(levelsup), _p(word), _p(w), _p(node))
        return word, w, node

    def transform(self, desc, levelsup=4):
        d = np.ascontiguousarray(desc, np.uint8)
        n = len(d)
        bi, bv = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float64)
        fn, fo, fi = np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.int32), np.zeros(max(n, 1), np.uint32)
        nw, nn = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._L.orc_voc_transform(self._h, _p(d), n, int(levelsup), _p(bi), _p(bv), _p(nw), _p(fn), _p(fo), _p(fi), _p(nn))
        return (bi[:nw[0]].copy(), bv[:nw[0]].copy()), (fn[:nn[0]].copy(), fo[:nn[0] + 1].copy(), fi[:fo[nn[0]]].copy())


def sim3_inliers(pair_start, pair_denominator, S_c1w2, S_c2w1, K4_1, K4_2, X1, X2, kp1, kp2, sigma2_1, sigma2_2, edge1, edge2):
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    ps = np.ascontiguousarray(pair_start, np.int32); pd = np.ascontiguousarray(pair_denominator, np.int32)
    A = np.ascontiguousarray(S_c1w2, np.float64); B = np.ascontiguousarray(S_c2w1, np.float64)
    arrs = [f32(K4_1), f32(K4_2), f32(X1), f32(X2), f32(kp1), f32(kp2), f32(sigma2_1), f32(sigma2_2), np.ascontiguousarray(edge1, np.uint8),
            np.ascontiguousarray(edge2, np.uint8)]
    n_pairs, total = len(ps) - 1, int(ps[-1])
    inl = np.zeros(max(total, 1), np.uint8); ratio = np.zeros(max(n_pairs, 1), np.float32)
    L = _olib()
    L.orc_sim3_inliers.restype = C.c_float
    L.orc_sim3_inliers.argtypes = [C.c_int32] + [C.c_void_p] * 16
    med = L.orc_sim3_inliers(n_pairs, _p(ps), _p(pd), _p(A), _p(B), *[_p(a) for a in arrs], _p(inl), _p(ratio))
    return med, ratio[:n_pairs], inl[:total]


def libc_srand(seed):
    """srand() of the C library this process (and liboracle's rand()) uses."""
    C.CDLL(None).srand(C.c_uint(int(seed)))


def libc_rand():
    return int(C.CDLL(None).rand())


def sim3_draw_triples(seed, n, n_hyp):
    """srand(seed), then the minimal sets of n_hyp Sim3Solver iterations (orc_sim3_draw_triples)."""
    L = _olib()
    L.orc_sim3_draw_triples.restype = None
    L.orc_sim3_draw_triples.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
    tri = np.zeros((n_hyp, 3), np.int32)
    libc_srand(seed)
    L.orc_sim3_draw_triples(n, n_hyp, _p(tri))
    return tri


def sim3_ransac(X1, X2, sigma2_1, sigma2_2, K4_1, K4_2, triples, fix_scale=False, score=None):
    """orc_sim3_ransac: per hypothesis ComputeSim3 + CheckInliers (+ ComputeInliersNum).  Same result dict as Optimizer.Sim3Ransac."""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    f64 = lambda a: np.ascontiguousarray(a, np.float64)
    u8 = lambda a: np.ascontiguousarray(a, np.uint8)
    X1, X2 = f32(X1).reshape(-1, 3), f32(X2).reshape(-1, 3)
    tri = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
    n, H = len(X1), len(tri)
    T = np.zeros((max(H, 1), 16), np.float32); nin = np.zeros(max(H, 1), np.int32); inl = np.zeros((max(H, 1), n), np.uint8)
    if score is not None:
        ps, pd = np.ascontiguousarray(score["pair_start"], np.int32), np.ascontiguousarray(score["pair_denominator"], np.int32)
        sc = [ps, pd, f64(score["S_c1w1"]), f64(score["S_c2w2"]), f64(score["S_kf1w"]), f64(score["S_kf2w"]), f32(score["K4_1"]), f32(score["K4_2"]),
              f32(score["X1"]), f32(score["X2"]), f32(score["kp1"]), f32(score["kp2"]), f32(score["sigma2_1"]), f32(score["sigma2_2"]), u8(score["edge1"]),
              u8(score["edge2"])]
        npairs = len(ps) - 1
        ratio = np.zeros((max(H, 1), npairs), np.float32); med = np.zeros(max(H, 1), np.float32)
    else:
        sc, npairs, ratio, med = [None] * 16, 0, None, None
    L = _olib()
    L.orc_sim3_ransac.restype = None
    L.orc_sim3_ransac.argtypes = [C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 16 + [C.c_void_p] * 5
    arrs = [X1, X2, f32(sigma2_1), f32(sigma2_2), f32(K4_1), f32(K4_2)]
    L.orc_sim3_ransac(n, *[_p(a) for a in arrs], int(bool(fix_scale)), H, _p(tri), npairs, *[_p(a) if a is not None else None for a in sc],
                      _p(T), _p(nin), _p(inl), _p(ratio) if ratio is not None else None, _p(med) if med is not None else None)
    T = T[:H]
    return dict(R=T[:, :9].reshape(-1, 3, 3).copy(), t=T[:, 9:12].copy(), s=T[:, 12].copy(), valid=T[:, 13] != 0, n_inliers=nin[:H].copy(),
                inliers=inl[:H].astype(bool), ratio=ratio[:H] if ratio is not None else None, median=med[:H] if med is not None else None)


def optimize_sim3(S8, P1c, P2c, obs1, obs2, w1, w2, K4_1, K4_2, th2=10.0, fix_scale=False, robust_first_pass=True, pair_of=None, S_c1w=None,
                  S_c2w=None, skip12=None, skip21=None):
    """orc_optimize_sim3: Optimizer::OptimizeSim3 / OptimizeCloudSim3.  Returns (nIn, nBad, early, S8, status)."""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    P1c, P2c, obs1, obs2, w1, w2, K1, K2 = (f32(a) for a in (P1c, P2c, obs1, obs2, w1, w2, K4_1, K4_2))
    n = len(w1)
    S = np.ascontiguousarray(S8, np.float64).copy()
    world = S_c1w is not None
    po = np.ascontiguousarray(pair_of, np.int32) if world else None
    A = np.ascontiguousarray(S_c1w, np.float64) if world else None
    B = np.ascontiguousarray(S_c2w, np.float64) if world else None
    s12 = None if skip12 is None else np.ascontiguousarray(skip12, np.uint8)
    s21 = None if skip21 is None else np.ascontiguousarray(skip21, np.uint8)
    status = np.zeros(max(n, 1), np.uint8); res = np.zeros(3, np.int32)
    L = _olib()
    L.orc_optimize_sim3.argtypes = [C.c_int32] + [C.c_void_p] * 13 + [C.c_float, C.c_int32, C.c_int32] + [C.c_void_p] * 3
    P = lambda a: None if a is None else _p(a)
    L.orc_optimize_sim3(n, P(po), P(A), P(B), P(P1c), P(P2c), P(obs1), P(obs2), P(w1), P(w2), P(s12), P(s21), P(K1), P(K2), float(th2), int(fix_scale),
                        int(robust_first_pass), P(S), P(status), P(res))
    return int(res[0]), int(res[1]), bool(res[2]), S, status[:n]
