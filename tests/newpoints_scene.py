"""Synthetic LocalMapping scenes for the tests of include/rumi_mapping.h (CreateNewMapPoints), and the binding of their C++ oracle
(tests/cpp/newpoints_oracle.cc).  TEST INFRASTRUCTURE.

A current key-frame and up to 30 neighbours stand on an arc and look at a seeded point cloud.  A feature is the projection of a landmark plus
pixel noise of sigma = 1.2^octave; its descriptor is the landmark's up to a few flipped bits; landmarks are noisy copies of the words of a
synthetic vocabulary (tests/voc_scene.py), so that a vocabulary node holds several look-alikes and the search has something to reject; the
FeatureVectors are the oracle vocabulary's transform of the descriptors.  Part of the features already hold map points."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O
from rumi_slam_amd import capi
from rumi_slam_amd.mapping import NEWPOINT_DTYPE, KeyFrameView, RumiNewPointsParams, pack
from rumi_slam_amd.matcher import FeatureVector, FrameView
from voc_scene import synthetic_vocabulary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_TUM3 = np.array([535.4, 539.2, 320.1, 247.6], np.float32)
W, H, NLEVELS = 640, 480, 8
SF = (np.float32(1.2) ** np.arange(NLEVELS)).astype(np.float32)
RATIO_FACTOR = float(np.float32(1.5) * np.float32(1.2))            # LocalMapping.cc:391
CENTRE = np.array([0.0, 0.0, 8.0])
GATES = ["ok", "parallax", "w0", "z1", "z2", "reproj1", "reproj2", "dist0", "far", "scale"]

TRACE_DTYPE = np.dtype([("neigh", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("gate", "<i4"), ("x3D", "<f4", 3), ("A", "<f4", 16)])

# (seed, neighbours, features, coarse, check_orientation, far points): what the CPU tests assert the scene conditions on and the GPU tests compare
SCENES = [(0, 30, 1000, 0, 0, 0), (1, 30, 1000, 0, 1, 1), (2, 7, 500, 0, 1, 0), (3, 30, 2000, 1, 0, 1), (4, 7, 1000, 1, 1, 0), (5, 1, 500, 0, 0, 0),
          (6, 30, 500, 1, 1, 1), (7, 7, 2000, 0, 0, 1), (8, 1, 1000, 1, 1, 1)]
TH_FAR = 10.0          # inside the cloud (3 .. 14 deep), and below the ~12 where the nearest neighbour's rays stop passing the parallax test


_voc = None


def _vocabulary():
    global _voc
    if _voc is None:
        tree = synthetic_vocabulary(7, 10, 3)
        _voc = (tree, O.OracleVocabulary(*tree))
    return _voc


def look_at(pos):
    """(Rcw, tcw) of a camera at pos looking at the cloud's centre, image y pointing down the world's y."""
    z = CENTRE - pos
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ pos


def arc_angles(n_neigh):
    """Angles (rad) of the neighbours on the arc around the current key-frame at 0.  Index 3 stands almost on the current key-frame (the baseline
    test skips it), index 5 a little further (searched, but the rays are nearly parallel), index 6 has
    stepped forward towards the cloud (NewPointsScene: a wrong pair can then lie in front of one camera and behind the other); the rest alternate sides with growing baselines."""
    a = []
    for k in range(n_neigh):
        mag = 0.03 + 0.011 * k
        if k == 3:
            mag = 0.004
        elif k == 5:
            mag = 0.014
        a.append(mag if k % 2 == 0 else -mag)
    return a


class NewPointsScene:
    def __init__(self, seed, n_neigh=30, nfeat=1000, mp_frac_cur=0.4, mp_frac_neigh=0.5, empty_neigh=(), levelsup=1):
        rng = np.random.default_rng(seed)
        (parent, leaf, vdesc, _), voc = _vocabulary()
        n_land = 4 * nfeat
        self.land = np.stack([rng.uniform(-5, 5, n_land), rng.uniform(-3.5, 3.5, n_land), rng.uniform(3, 14, n_land)], 1)
        words = np.nonzero(leaf)[0]
        ldesc = vdesc[rng.choice(words, n_land)].copy()
        self._flip(rng, ldesc, np.full(n_land, 12))
        langle = rng.uniform(0, 360, n_land)
        saliency = rng.random(n_land)
        fx, fy, cx, cy = K_TUM3.astype(np.float64)
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
        Kinv = np.linalg.inv(K)

        poses = []
        for k, a in enumerate([0.0] + arc_angles(n_neigh)):
            pos = CENTRE + (5.0 if k == 7 else 8.0) * np.array([np.sin(a), 0.0, -np.cos(a)]) + (rng.normal(size=3) * [0.002, 0.02, 0.002] if a else 0.0)
            poses.append((pos,) + look_at(pos))
        self.views = []
        for k, (pos, R, t) in enumerate(poses):
            Xc = self.land @ R.T + t
            u, v = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
            vis = (Xc[:, 2] > 0.5) & (u > 8) & (u < W - 8) & (v > 8) & (v < H - 8)
            prio = np.where(vis, saliency + rng.uniform(0, 0.3, n_land), -1.0)
            ids = np.sort(np.argsort(-prio)[:min(nfeat, int(vis.sum()))])
            rng.shuffle(ids)
            n = len(ids)
            depth = np.linalg.norm(self.land[ids] - pos, axis=1)
            octave = np.round(np.log(14.0 / depth) / np.log(1.2)).astype(np.int64)
            jit = rng.random(n)
            octave += np.where(jit < 0.2, rng.integers(-1, 2, n), 0) + np.where(jit > 0.95, rng.choice([-5, -4, 4, 5], n), 0)
            octave = np.clip(octave, 0, NLEVELS - 1)
            keys = np.zeros(n, capi.KP_DTYPE)
            sig = 1.2 ** octave
            keys["x"] = u[ids] + rng.normal(size=n) * sig
            keys["y"] = v[ids] + rng.normal(size=n) * sig
            ang = langle[ids] + rng.normal(size=n) * 4.0
            ang = np.where(rng.random(n) < 0.08, rng.uniform(0, 360, n), ang) % 360.0
            keys["angle"] = ang
            keys["octave"] = octave
            keys["size"] = 31.0 * sig
            keys["class_id"] = -1
            desc = ldesc[ids].copy()
            self._flip(rng, desc, rng.integers(0, 11, n))
            frac = mp_frac_cur if k == 0 else (0.0 if (k - 1) in empty_neigh else mp_frac_neigh)
            kf_mp = np.where(rng.random(n) < frac, ids, -1).astype(np.int32)
            mp_pos = (self.land[ids] + rng.normal(size=(n, 3)) * 0.02).astype(np.float32)
            _, (fn, fo, fi) = voc.transform(desc, levelsup)
            Tcw = np.concatenate([R, t[:, None]], 1).astype(np.float32)
            self.views.append(dict(keys=keys, desc=desc, kf_mp=kf_mp, mp_pos=mp_pos, fv=(fn, fo, fi), Tcw=Tcw, Ow=pos.astype(np.float32),
                                   R=R, t=t, land=ids))
        # F12 and the epipole per neighbour: K1^-T [t12]x R12 K2^-1 (GeometricTools::ComputeF12 is what Pinhole::epipolarConstrain rebuilds),
        # project2(T2w * Ow1) (ORBmatcher.cc:815-818); formed in double from the float poses the key-frames carry, handed over in float
        T1 = self.views[0]["Tcw"].astype(np.float64)
        R1, t1 = T1[:, :3], T1[:, 3]
        Ow1 = self.views[0]["Ow"].astype(np.float64)
        for v in self.views[1:]:
            T2 = v["Tcw"].astype(np.float64)
            R2, t2 = T2[:, :3], T2[:, 3]
            R12 = R1 @ R2.T
            t12 = -R12 @ t2 + t1
            tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
            v["F12"] = (Kinv.T @ tx @ R12 @ Kinv).astype(np.float32).ravel()
            c = R2 @ Ow1 + t2
            v["ep"] = np.array([fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy], np.float32)
        self.n_neigh = n_neigh
        self.cur = self._view(self.views[0], False)
        self.neigh = [self._view(v, True) for v in self.views[1:]]

    @staticmethod
    def _flip(rng, desc, count):
        n = len(desc)
        rows = np.arange(n)
        for j in range(int(count.max()) if n else 0):
            b = rng.integers(0, 256, n)
            m = (count > j).astype(np.uint8)
            desc[rows, b >> 3] ^= ((1 << (b & 7)).astype(np.uint8) * m)

    @staticmethod
    def _view(v, neighbour):
        return KeyFrameView(FrameView(v["keys"], v["desc"], W, H, SF), FeatureVector.from_csr(*v["fv"]), v["kf_mp"], K_TUM3, v["Tcw"], v["Ow"],
                            v["mp_pos"] if neighbour else None, v.get("F12"), v.get("ep"))

    def truncated(self, n):
        """The same scene with the first n neighbours only."""
        return self.neigh[:n]


# The rotation histogram ON its first cut: one neighbour, one FeatureVector node of at most 40 features a side.  13 of the pairs the search finds
# (distinct features on both sides) get the angles of match_cases.HISTOGRAMS["cut_kept"], bins 2 / 5 / 8 / 10 with 10 / 1 / 1 / 1 pairs; the
# other features of the current key-frame receive a map point and leave the search (the queries are independent: vbMatched2 is never set).
# 1 < 0.1f * 10 is false in float, so bins 5 and 8 stay and bin 10 goes for being the fourth.
CUT_KEPT = [(60.0, 0.0, 2)] * 10 + [(155.0, 5.0, 5), (250.0, 10.0, 8), (300.0, 0.0, 10)]


def cut_kept_scene(L):
    """-> (scene, pairs [13, 2], bins [13]) with the pairs in CUT_KEPT's order."""
    s = NewPointsScene(70, 1, 40, mp_frac_cur=0.0, mp_frac_neigh=0.3, levelsup=3)
    cur, nb = s.views[0], s.views[1]
    assert len(cur["fv"][0]) == 1 and len(nb["fv"][0]) == 1 and len(cur["keys"]) <= 40 and len(nb["keys"]) <= 40
    m = run_oracle(L, s.cur, s.neigh, params(0, 0, 0, TH_FAR))["matches"][0]
    pairs, used = [], set()
    for i1 in np.nonzero(m >= 0)[0]:
        if int(m[i1]) not in used and len(pairs) < len(CUT_KEPT):
            used.add(int(m[i1])); pairs.append((int(i1), int(m[i1])))
    assert len(pairs) == len(CUT_KEPT), "the scene's search finds too few pairs"
    cur["kf_mp"][:] = cur["land"]
    for (i1, i2), (a1, a2, _) in zip(pairs, CUT_KEPT):
        cur["kf_mp"][i1] = -1
        cur["keys"]["angle"][i1] = a1; nb["keys"]["angle"][i2] = a2
    s.cur, s.neigh = s._view(cur, False), [s._view(nb, True)]
    return s, np.array(pairs, np.int32), np.array([b for _, _, b in CUT_KEPT])


# ---- the C++ oracle ----
def build_oracle(out_dir):
    O.lib()                                                    # builds oracle/liboracle.so when it is missing
    so = os.path.join(str(out_dir), "libnewpoints_oracle.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "newpoints_oracle.cc"), "-o", so, "-L", O.ORACLE_DIR, "-loracle",
                           "-Wl,-rpath," + O.ORACLE_DIR])
    L = C.CDLL(so)
    vp, i32 = C.c_void_p, C.c_int32
    L.npo_median_depth.restype = C.c_float
    L.npo_median_depth.argtypes = [vp]
    L.npo_triangulate.argtypes = [vp] * 6
    L.npo_create_new_map_points.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp]
    return L


def params(coarse=False, check_ori=False, far_points=False, th_far=0.0, ratio_factor=RATIO_FACTOR):
    return RumiNewPointsParams(int(coarse), int(check_ori), int(far_points), float(th_far), float(ratio_factor))


def run_oracle(L, cur, neighbours, prm):
    """dict(points, per_neigh, skipped, matches [n_neigh, n1], flags_before [n_neigh, n1], hist_removed, trace) of the reference's loop."""
    c, arr = pack(cur, neighbours)
    n, n1 = len(neighbours), cur.frame.n
    out = np.zeros(max(n1, 1), NEWPOINT_DTYPE)
    per, skipped, removed = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32)
    matches = np.full((max(n, 1), max(n1, 1)), -1, np.int32)
    flags = np.full((max(n, 1), max(n1, 1)), -1, np.int32)
    trace = np.zeros(max(n * n1, 1), TRACE_DTYPE)
    ntr = C.c_int32()
    cnt = L.npo_create_new_map_points(C.byref(c), C.byref(arr), n, C.byref(prm), capi.ptr(out), len(out), capi.ptr(per), capi.ptr(skipped),
                                      capi.ptr(matches), capi.ptr(flags), capi.ptr(removed), capi.ptr(trace), len(trace), C.byref(ntr))
    assert cnt <= len(out) and ntr.value <= len(trace)
    return dict(points=out[:cnt], per_neigh=per[:n], skipped=skipped[:n], matches=matches[:n, :n1], flags_before=flags[:n, :n1],
                hist_removed=removed[:n], trace=trace[:ntr.value])


def median_depth(L, view):
    c, _ = pack(view, [])
    return float(L.npo_median_depth(C.byref(c)))
