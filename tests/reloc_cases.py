"""Constructed scenes for Tracking::Relocalization's refine chain (R/lib_src/Tracking.cc:3287-3345): rumi_track_reloc_begin / _refine.

One synthetic frame (the extractor's own key-points and descriptors of a synthetic image: 1504 features), noise-free geometry around one true
pose.  A map point is the back-projection of a frame feature: a CLEAN one reprojects onto its feature exactly, a GROSS one is the back-projection
of a pixel 12 px beside a feature of octave 2-4 -- beyond 10 px, an outlier of every optimisation, yet inside the coarse search window
(10 * 1.2^octave >= 14.4 px) of its own feature, whose descriptor it carries.  So every nGood is the number of clean correspondences and every
nadditional the number of planted points the search can reach: the counts are constructed, not found.

A case is one pose hypothesis with a candidate key-frame of its own (K = number of cases: what a key-frame holds fixes the counts of its case):
  a      clean inliers of the solver (match + inlier flag)
  g1     gross inliers of the solver: P1's outliers; nulled at :3309, their points stay in sFound and the key-frame holds them
  x      matched features that are no inliers (seeded NULL; their points are not in the key-frame)
  b      (b0, b5, b10) clean points planted for S1 in the rotation bins 0, 5 and 10 (key-frame angle = frame angle + 30 bin)
  g2     gross points planted for S1 (bin 0): found there, outliers of P2, not nulled, blocking their features in S2, optimised again in P3
  twin   clean points behind the g2 points in the key-frame that project onto the g2 points' features and carry their descriptors, but which the
         solver matched (as inliers) to features far away: outliers of P1, nulled, in sFound and so not searched in S1; searched in S2, where
         their feature is blocked by P2's outlier and nothing else in the fine window is near enough
  c      clean points in rotation bin 15: the fourth bin, dropped by ComputeThreeMaxima in S1 (c <= every b), alone and kept in S2
  bad    planted like b but isBad()
  fill   (tools/reloc_probe.py) points that project onto a feature with the complement of its descriptor: searched in both searches, hardly ever matched
Key-frame order: a, g1, b0, b5, b10, g2, twin, c, bad.  `expected(case)` derives ran / ngood / nadditional / ngood_final from these counts alone.
"""
import functools

import numpy as np

import oracle_lib as O
from rumi_slam_amd.capi import KP_DTYPE
from rumi_slam_amd.synth import synth_frame
from scene import K_TUM3

W, H = 640, 480
NFEATURES, NLEVELS, SEED = 1500, 8, 7
LOG_SF = float(np.log(np.float32(1.2)))
DEFAULTS = dict(min_good=10, enough=50, retry_above=30, th_coarse=10.0, dist_coarse=100, th_fine=3.0, dist_fine=64, check_orientation=1)
GROSS_PX = 12.0


def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


T_TRUE = np.concatenate([_unit([0.02, -0.03, 0.01, 1.0]), [0.10, -0.05, 0.20]]).astype(np.float32)
T_NEAR = np.concatenate([_unit([0.021, -0.0295, 0.0108, 1.0]), [0.104, -0.053, 0.197]]).astype(np.float32)     # a hypothesis a pixel or two off


def quat_matrix(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def project(T7, X):
    """Pixel coordinates of world points under Tcw, in double (the margin condition's arithmetic)."""
    T7 = np.asarray(T7, np.float64)
    Xc = np.asarray(X, np.float64) @ quat_matrix(T7[:4] / np.linalg.norm(T7[:4])).T + T7[4:]
    fx, fy, cx, cy = K_TUM3.astype(np.float64)
    return np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)


def backproject(T7, uv, z):
    T7 = np.asarray(T7, np.float64)
    fx, fy, cx, cy = K_TUM3.astype(np.float64)
    Xc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    return ((Xc - T7[4:]) @ quat_matrix(T7[:4] / np.linalg.norm(T7[:4]))).astype(np.float32)


def camera_centre(T7):
    """Sophus::SE3f::inverse().translation() in float, operation by operation as the facade's ORBmatcher::camera_centre and the device form it."""
    f = np.float32
    T = [f(v) for v in np.asarray(T7, np.float32)]
    qx, qy, qz, qw = -T[0], -T[1], -T[2], T[3]
    p = [T[4] * f(-1), T[5] * f(-1), T[6] * f(-1)]
    u0, u1, u2 = qy * p[2] - qz * p[1], qz * p[0] - qx * p[2], qx * p[1] - qy * p[0]
    u0, u1, u2 = u0 + u0, u1 + u1, u2 + u2
    c0, c1, c2 = qy * u2 - qz * u1, qz * u0 - qx * u2, qx * u1 - qy * u0
    return np.array([(p[0] + qw * u0) + c0, (p[1] + qw * u1) + c1, (p[2] + qw * u2) + c2], np.float32)


@functools.lru_cache(maxsize=None)
def frame(blank=False):
    """The shared frame: image, key-points, descriptors (the CPU extractor's, bit-equal to the device's), scale tables."""
    img = np.full((H, W), 110, np.uint8) if blank else synth_frame(SEED, W, H)
    ext = O.OracleExtractor(NFEATURES, 1.2, NLEVELS, 20, 7)
    _, keys, desc = ext.extract(img, (0, 1000))
    tab = ext.tables()
    return dict(img=img, keys=keys, desc=desc, sf=tab["scale"].copy(), inv_sigma2=tab["inv_sigma2"].copy())


def _hamming_rows(d, row):
    return np.unpackbits(d ^ row, axis=1).sum(1)


@functools.lru_cache(maxsize=None)
def _pools():
    """Features a planted point can use: away from the border, with a descriptor no other feature of the frame carries -- a planted point's own
    feature is then at distance 0 and every other one farther, so it takes its own while that is free.  -> (all, those of octave 2-4 for the
    gross points; first among them the ones whose fine window -- 3 * 1.2^octave px, the levels around it -- holds no other feature within the
    fine Hamming bound: a point that finds such a feature blocked finds nothing)."""
    F = frame()
    k, d, sf = F["keys"], F["desc"], F["sf"]
    _, first, counts = np.unique(d, axis=0, return_index=True, return_counts=True)
    unique = np.zeros(len(k), bool)
    unique[first[counts == 1]] = True
    ok = np.nonzero(unique & (k["x"] >= 70) & (k["x"] <= W - 70) & (k["y"] >= 70) & (k["y"] <= H - 70))[0]
    gross = ok[(k["octave"][ok] >= 2) & (k["octave"][ok] <= 4)]
    alone = []
    for f in gross:
        r = DEFAULTS["th_fine"] * float(sf[k["octave"][f]]) + 0.5
        near = (np.abs(k["x"] - k["x"][f]) < r) & (np.abs(k["y"] - k["y"][f]) < r) & (np.abs(k["octave"] - k["octave"][f]) <= 1)
        near[f] = False
        alone.append(not near.any() or _hamming_rows(d[near], d[f]).min() > DEFAULTS["dist_coarse"])
    alone = np.array(alone)
    return ok, np.concatenate([gross[alone], gross[~alone]]), int(alone.sum())


class _Table:
    """The point table all cases share."""

    def __init__(self):
        self.pos, self.mn, self.mx, self.desc, self.bad = [], [], [], [], []

    def add(self, f, shift=(0.0, 0.0), bad=False, invert=False):
        F = frame()
        k = F["keys"][f]
        z = 2.0 + ((f * 0.6180339887) % 1.0) * 4.0
        X = backproject(T_TRUE, np.array([[k["x"] + shift[0], k["y"] + shift[1]]], np.float64), np.array([z]))[0]
        dist = float(np.linalg.norm(X.astype(np.float64) - camera_centre(T_TRUE).astype(np.float64)))
        self.pos.append(X)
        self.mx.append(dist * 1.2 ** (int(k["octave"]) - 0.5))      # PredictScale = ceil(octave - 0.5) = the feature's octave
        self.mn.append(0.05 * dist)
        self.desc.append(~F["desc"][f] if invert else F["desc"][f].copy()); self.bad.append(1 if bad else 0)
        return len(self.pos) - 1

    def arrays(self):
        return dict(pos=np.array(self.pos, np.float32).reshape(-1, 3), min_dist=np.array(self.mn, np.float32), max_dist=np.array(self.mx, np.float32),
                    desc=np.array(self.desc, np.uint8).reshape(-1, 32), bad=np.array(self.bad, np.uint8))


_SHIFTS = [(GROSS_PX, 0.0), (-GROSS_PX, 0.0), (0.0, GROSS_PX), (0.0, -GROSS_PX)]      # balanced: the gross points pull no way in particular


def _kf_key(f, bin_):
    F = frame()
    k = F["keys"][f].copy()
    a = np.float32(k["angle"]) + np.float32(30 * bin_)
    if a >= np.float32(360):
        a = a - np.float32(360)
    k["angle"] = a
    return k


def _make_case(tab, name, a=0, g1=0, x=3, b=(0, 0, 0), g2=0, twin=0, c=0, bad=0, T0=T_TRUE, nkf0=False, all_features=False, params=None, constructed=True,
               fill=0):
    F = frame()
    n = len(F["keys"])
    anyp, grossp, n_alone = _pools()
    assert twin <= min(g2, n_alone)
    matches = np.full(n, -1, np.int32); inl = np.zeros(n, np.uint8)
    kf_keys, kf_mp = [], []
    spec = dict(a=a, g1=g1, x=x, b=tuple(b), g2=g2, twin=twin, c=c, bad=bad)
    # (the g2 points come first in the pool: the twins need its head)
    gset = set(grossp[:g1 + g2].tolist())
    gi = iter(grossp[g2:g2 + g1].tolist() + grossp[:g2].tolist())
    ai = iter(range(n)) if all_features else iter([f for f in anyp if f not in gset])
    feats = {}

    def hold(f, p, bin_=0):
        kf_keys.append(_kf_key(f, bin_)); kf_mp.append(p)

    feats["a"] = [next(ai) for _ in range(a)]
    for f in feats["a"]:
        p = tab.add(f); matches[f] = p; inl[f] = 1; hold(f, p)
    feats["g1"] = [next(gi) for _ in range(g1)]
    for j, f in enumerate(feats["g1"]):
        p = tab.add(f, _SHIFTS[j % 4]); matches[f] = p; inl[f] = 1; hold(f, p)
    feats["x"] = [next(ai) for _ in range(x)]
    for f in feats["x"]:
        matches[f] = tab.add(f)
    for name_b, cnt, bin_ in (("b0", b[0], 0), ("b5", b[1], 5), ("b10", b[2], 10)):
        feats[name_b] = [next(ai) for _ in range(cnt)]
        for f in feats[name_b]:
            hold(f, tab.add(f), bin_)
    feats["g2"] = [next(gi) for _ in range(g2)]
    for j, f in enumerate(feats["g2"]):
        hold(f, tab.add(f, _SHIFTS[j % 4]))
    feats["twin"] = [next(ai) for _ in range(twin)]                  # the far features the solver matched the twins to
    for ft, f in zip(feats["twin"], feats["g2"]):
        assert abs(float(F["keys"]["x"][ft] - F["keys"]["x"][f])) + abs(float(F["keys"]["y"][ft] - F["keys"]["y"][f])) > 40
        p = tab.add(f); matches[ft] = p; inl[ft] = 1; hold(f, p)
    feats["c"] = [next(ai) for _ in range(c)]
    for f in feats["c"]:
        hold(f, tab.add(f), 15)
    feats["bad"] = [next(ai) for _ in range(bad)]
    for f in feats["bad"]:
        hold(f, tab.add(f, bad=True))
    for j in range(fill):                                   # points that are searched and match nothing: the complement of a feature's descriptor
        f = int(anyp[j % len(anyp)])
        hold(f, tab.add(f, invert=True))
    if nkf0:
        kf_keys, kf_mp = [], []
    return dict(name=name, spec=spec, feats=feats, matches=matches, inliers=inl, Tcw7=np.asarray(T0, np.float32).copy(), nkf0=nkf0,
                kf_keys=np.array(kf_keys, KP_DTYPE) if kf_keys else np.zeros(0, KP_DTYPE), kf_mp=np.array(kf_mp, np.int32).reshape(-1),
                params=dict(DEFAULTS, **(params or {})), constructed=constructed)


def _make_dense(tab, name):
    """Every point of a 1500-feature key-frame projects onto ONE spot, the densest of the frame at octave 1, and the Hamming bound is off
    (dist_coarse 255: at 256 the member itself would accept "no candidate") with a wide window (th_coarse 30; enough = 100000 keeps the chain at S1): every query's list holds every feature of three levels inside 72 x 72 px, far more
    in all than four a pair.  The queries take those features one after another, nearest first."""
    F = frame()
    k = F["keys"]
    n = len(k)
    r = 30.0 * float(F["sf"][1])
    o1 = np.nonzero((k["octave"] == 1) & (k["x"] > 100) & (k["x"] < W - 100) & (k["y"] > 100) & (k["y"] < H - 100))[0]
    dens = [int(((np.abs(k["x"] - k["x"][f]) < r) & (np.abs(k["y"] - k["y"][f]) < r) & (k["octave"] <= 2)).sum()) for f in o1]
    f0 = int(o1[int(np.argmax(dens))])
    case = _make_case(tab, name, a=12, x=0, params=dict(th_coarse=30.0, dist_coarse=255, enough=100000), constructed=False)
    keys, mp = list(case["kf_keys"]), list(case["kf_mp"])
    for _ in range(n):
        keys.append(_kf_key(f0, 0)); mp.append(tab.add(f0))
    case["kf_keys"] = np.array(keys, KP_DTYPE); case["kf_mp"] = np.array(mp, np.int32)
    case["dense_window"] = max(dens)
    return case


@functools.lru_cache(maxsize=None)
def scene():
    """-> (cases by name (dict, insertion-ordered), the shared point table)."""
    tab = _Table()
    B3 = (10, 10, 10)
    cs = [
        _make_case(tab, "p1_two", a=2, T0=T_NEAR),                                   # n < 3: returns 0, pose untouched
        _make_case(tab, "p1_9", a=9, g1=1, T0=T_NEAR),                               # :3306 continue
        _make_case(tab, "p1_10", a=10, g1=1, T0=T_NEAR),                             # passes :3306; S1 finds nothing
        _make_case(tab, "p1_49", a=49, g1=2, T0=T_NEAR),                             # :3314 taken
        _make_case(tab, "p1_50", a=50, g1=2, T0=T_NEAR),                             # :3314 not taken: wins after P1
        _make_case(tab, "s1_49", a=30, b=(7, 6, 6)),                                 # :3317 49
        _make_case(tab, "s1_50", a=30, b=(7, 7, 6), T0=T_NEAR),                      # :3317 50; P2 = 50 wins
        _make_case(tab, "p2_30", a=10, b=(7, 7, 6), g2=20),                          # :3322 30: no S2
        _make_case(tab, "p2_31", a=11, b=(7, 7, 6), g2=19),                          # :3322 31: S2 runs, finds nothing
        _make_case(tab, "p2_49", a=29, b=(7, 7, 6), g2=2),                           # :3322 49: S2 runs
        _make_case(tab, "p2_50", a=30, b=(7, 7, 6), g2=2),                           # :3322 50: no S2, nothing nulled, wins with its outliers in the frame
        _make_case(tab, "s2_49", a=10, b=B3, g2=10, c=9),                            # :3330 40 + 9
        _make_case(tab, "s2_50", a=10, b=B3, g2=10, c=10, twin=3, T0=T_NEAR),        # :3330 40 + 10: P3; twins blocked by P2's outliers, which P3 optimises again
        _make_case(tab, "sfound", a=20, g1=3),                                       # P1's outliers stay in sFound: S1 does not search them
        _make_case(tab, "bad_point", a=20, b=(5, 5, 5), bad=4),
        _make_case(tab, "nkf_zero", a=20, nkf0=True),
        _make_case(tab, "big_1152", a=1152, x=0, all_features=True),                 # the LDS instantiation of k_pose_opt
        _make_case(tab, "big_1153", a=1153, x=0, all_features=True),                 # the global-memory one
        _make_dense(tab, "dense"),
    ]
    return {c["name"]: c for c in cs}, tab.arrays()


def standard_names():
    """The cases that run under the default parameters: hypotheses of one call."""
    return [n for n, c in scene()[0].items() if c["params"] == DEFAULTS]


def expected(case):
    """ran, ngood, nadditional, ngood_final from the constructed counts alone."""
    s, P = case["spec"], case["params"]
    nb = 0 if case["nkf0"] else sum(s["b"])
    g2 = 0 if case["nkf0"] else s["g2"]
    cc = 0 if case["nkf0"] else s["c"]
    e = dict(ran=1, ngood=[0, 0, 0], nadditional=[0, 0], ngood_final=-1)
    ng = s["a"] if s["a"] + s["g1"] + s["twin"] >= 3 else 0
    e["ngood"][0] = ng
    if ng < P["min_good"]:
        return e
    e["ran"] |= 2; e["ngood_final"] = ng
    if ng >= P["enough"]:
        return e
    e["ran"] |= 4; e["nadditional"][0] = nb + g2
    if ng + nb + g2 < P["enough"]:
        return e
    e["ran"] |= 8
    ng = s["a"] + nb
    e["ngood"][1] = ng; e["ngood_final"] = ng
    if not (P["retry_above"] < ng < P["enough"]):
        return e
    e["ran"] |= 16; e["nadditional"][1] = cc
    if ng + cc < P["enough"]:
        return e
    e["ran"] |= 32
    e["ngood"][2] = ng + cc; e["ngood_final"] = ng + cc
    return e


def run_chain(case, pts, pose_opt, search, keys=None, inv_sigma2=None):
    """Tracking.cc:3287-3345 for one hypothesis over two callables:
      pose_opt(Xw, obs, w, K4, T7) -> (nGood, T7, outlier)        Optimizer::PoseOptimization on the gathered correspondences
      search(T7, Ow3, skip, cur_mp, th, dist) -> (n, cur_mp)      ORBmatcher::SearchByProjection(F, pKF, sFound, th, ORBdist)
    -> dict ran, ngood, nadditional, ngood_final, Tcw, frame_mp, outlier_last, and `solves`: (pose, features, point ids) of every optimisation."""
    F = frame()
    keys = F["keys"] if keys is None else keys
    inv_sigma2 = F["inv_sigma2"] if inv_sigma2 is None else inv_sigma2
    P = case["params"]
    n, nmp = len(keys), len(pts["bad"])
    inl = case["inliers"][:n] != 0
    cur = np.where(inl, case["matches"][:n], -1).astype(np.int32)
    found = np.zeros(nmp, bool)
    found[cur[cur >= 0]] = True                                                   # :3299, before the first optimisation
    out_last = np.full(n, 255, np.uint8)
    r = dict(ran=1, ngood=[0, 0, 0], nadditional=[0, 0], ngood_final=-1, solves=[])
    T = case["Tcw7"].copy()

    def optimise(slot):
        nonlocal T
        idx = np.nonzero(cur >= 0)[0]
        ng, T, out = pose_opt(pts["pos"][cur[idx]], np.stack([keys["x"][idx], keys["y"][idx]], 1).astype(np.float32).reshape(-1, 2),
                              inv_sigma2[keys["octave"][idx]], K_TUM3, T)
        T = np.asarray(T, np.float32)
        out_last[idx] = out
        r["ngood"][slot] = int(ng)
        r["solves"].append((T.copy(), idx, cur[idx].copy()))
        return int(ng), idx, out

    def look(slot, th, dist):
        nonlocal cur
        skip = ((pts["bad"] != 0) | found).astype(np.uint8)
        nadd, cur = search(T, camera_centre(T), skip, cur, th, dist)
        r["nadditional"][slot] = int(nadd)
        return int(nadd)

    ng, idx, out = optimise(0)
    if ng >= P["min_good"]:
        r["ran"] |= 2
        cur[idx[out != 0]] = -1                                                   # :3309
        if ng < P["enough"]:
            r["ran"] |= 4
            nadd = look(0, P["th_coarse"], P["dist_coarse"])
            if nadd + ng >= P["enough"]:
                r["ran"] |= 8
                ng, idx, out = optimise(1)
                if P["retry_above"] < ng < P["enough"]:
                    r["ran"] |= 16
                    found[:] = False
                    found[cur[cur >= 0]] = True                                   # :3323-3326
                    nadd = look(1, P["th_fine"], P["dist_fine"])
                    if ng + nadd >= P["enough"]:
                        r["ran"] |= 32
                        ng, idx, out = optimise(2)
                        cur[idx[out != 0]] = -1                                   # :3333
        r["ngood_final"] = ng
    r.update(Tcw=T, frame_mp=cur, outlier_last=out_last)
    return r


def chain_oracle(case, pts=None):
    """run_chain over the CPU oracle."""
    F = frame()
    pts = scene()[1] if pts is None else pts
    P = case["params"]

    def search(T, Ow, skip, cur, th, dist):
        return O.search_by_projection_reloc(F["keys"], F["desc"], W, H, F["sf"], LOG_SF, T, Ow, K_TUM3, case["kf_keys"], case["kf_mp"], dict(pts, skip=skip), cur,
                                            th, dist, bool(P["check_orientation"]))
    return run_chain(case, pts, O.pose_optimization, search)


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    """chain_oracle of a case of scene(), computed once and shared (treat as read-only)."""
    return chain_oracle(scene()[0][name])
