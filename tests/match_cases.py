"""Constructed cases for the Hamming matchers: inputs small enough that the right answer is written down from the reference's rule
(cited as ORBmatcher.cc:NNN, never quoted) instead of being computed by the oracle or a kernel.

Nothing here needs a GPU or the oracle library to BUILD a case; ``call_oracle`` / ``call_gpu`` take the module to call as an argument.
Geometry is exact in float32: K = (512, 512, 320, 240), identity pose, every point at depth 4 with dyadic x, y, so u = 128 x + 320.

Families: A tie, B best == second, C distance threshold, D ratio boundary, E orientation histogram, F window / frame borders,
G sequential state, H sizes.  ``COVERAGE`` / ``NOT_APPLICABLE`` name, for every member x family cell, the cases or the reason."""
import math

import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
K4 = np.array([512, 512, 320, 240], np.float32)
Z = 4.0
SF = np.float32(1.2) ** np.arange(8, dtype=np.float32)
LOG_SF = float(np.log(np.float32(1.2)))
IDENT7 = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
TH_LOW, TH_HIGH = 50, 100

PROJ_MEMBERS = ["MP", "LAST", "RELOC", "SIM3P", "FUSE", "SIM3", "INIT"]
BOW_MEMBERS = ["BOW_F", "BOW_KF", "TRI"]
MEMBERS = PROJ_MEMBERS + BOW_MEMBERS
FAMILIES = "ABCDEFGH"
MEMBER_NAMES = {
    "MP": "SearchByProjection(F, MapPoints) :39", "LAST": "SearchByProjection(Cur, Last) :1498", "RELOC": "SearchByProjection(F, KF, found, th, ORBdist) :1685",
    "SIM3P": "SearchByProjection(KF, Scw, points, ...) :372 / :473", "FUSE": "Fuse :1015 / :1182 (search half)", "SIM3": "SearchBySim3 :1293",
    "INIT": "SearchForInitialization :581", "BOW_F": "SearchByBoW(KF, F) :198", "BOW_KF": "SearchByBoW(KF, KF) :682", "TRI": "SearchForTriangulation :806"}
# octave window of a member around the query's level L (None: INIT only looks at octave 0)
LEVELS = {"MP": (-1, 0), "LAST": (-1, 1), "RELOC": (-1, 1), "SIM3P": (-1, 0), "FUSE": (-1, 0), "SIM3": (-1, 0), "INIT": None}
# largest accepted best distance with the parameters the cases use
ACCEPT = {"MP": TH_HIGH, "LAST": TH_HIGH, "RELOC": 64, "SIM3P": 75, "FUSE": TH_LOW, "SIM3": TH_HIGH, "INIT": TH_LOW, "BOW_F": TH_LOW, "BOW_KF": TH_LOW - 1,
          "TRI": TH_LOW}
RATIO_MEMBERS = ["MP", "INIT", "BOW_F", "BOW_KF"]
ORI_MEMBERS = ["LAST", "RELOC", "INIT", "BOW_F", "BOW_KF", "TRI"]


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def desc_at(base, k, rng):
    """A copy of ``base`` with exactly ``k`` bits flipped: Hamming distance k to ``base``."""
    bits = np.unpackbits(np.asarray(base, np.uint8))
    bits[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def c_round(v):
    """C round(): half away from zero."""
    v = float(v)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def cell_of(x, y, w, h):
    """Grid cell (column, row) of a key-point in a w x h frame, or None when it falls outside the 64 x 48 grid (Frame.cc:752)."""
    cx = c_round(np.float32(x) * (np.float32(64) / np.float32(w)))
    cy = c_round(np.float32(y) * (np.float32(48) / np.float32(h)))
    return (cx, cy) if 0 <= cx < 64 and 0 <= cy < 48 else None


def visit_order(xy, w, h):
    """Indices in the order GetFeaturesInArea visits them: cell column outer, cell row inner, insertion order inside a cell."""
    c = [(cell_of(x, y, w, h), i) for i, (x, y) in enumerate(xy)]
    return [i for cc, i in sorted((cc, i) for cc, i in c if cc is not None)]


def rot_bin(a1, a2):
    """Histogram bin of a match, in explicit float32 (ORBmatcher.cc:303-308)."""
    rot = np.float32(a1) - np.float32(a2)
    if rot < 0:
        rot = np.float32(rot + np.float32(360.0))
    p = np.float32(rot * (np.float32(1.0) / np.float32(30)))
    b = c_round(p)
    return 0 if b == 30 else b


def csr(mapping):
    nodes = sorted(mapping)
    off, idx = [0], []
    for nd in nodes:
        idx.extend(mapping[nd]); off.append(len(idx))
    return np.array(nodes, np.uint32), np.array(off, np.int32), np.array(idx, np.uint32)


def _keys(rows):
    k = np.zeros(len(rows), KP_DTYPE)
    for i, (x, y, o, a) in enumerate(rows):
        k[i] = (x, y, 31, a, 1, o, -1)
    return k


class Case:
    def __init__(self, name, member, family, cite, inp, count, arr, nnratio=0.8, ori=False, pm=None):
        self.name, self.member, self.family, self.cite, self.inp = name, member, family, cite, inp
        self.count, self.arr, self.pm, self.nnratio, self.ori = count, np.asarray(arr, np.int32 if member != "TRI" else np.int64), pm, float(nnratio), bool(ori)

    @property
    def id(self):
        return f"{self.member}-{self.family}-{self.name}"


# ---------------------------------------------------------------------------------------------------------------------------------
# projection members: one frame of key-points, queries that project to chosen pixels
# ---------------------------------------------------------------------------------------------------------------------------------
class Proj:
    """A frame and queries at chosen pixels.  R = window radius in pixels at level 0 (a multiple of 4: MP's th is R / 4 because its
    radius is 4.0 * th * scale, ORBmatcher.cc:59-65; the others use th = R)."""

    def __init__(self, seed, w=640, h=480, R=8, level=0):
        self.rng = np.random.default_rng(seed)
        self.w, self.h, self.R, self.level = w, h, R, level
        self.f, self.q, self.occ = [], [], {}
        self.par = dict(orb_dist=64, ratio_hamming=1.5, variant=0, reproj=0)

    def base(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def feat(self, x, y, desc, octave=None, angle=0.0):
        self.f.append((np.float32(x), np.float32(y), self.level if octave is None else octave, angle, np.asarray(desc, np.uint8)))
        return len(self.f) - 1

    def query(self, u, v, desc, angle=0.0, level=None, kind="ok", octave1=None, pos=None, normal=None, min_dist=None, max_dist=None):
        """pos / normal / min_dist / max_dist: the point's attributes as given (float32 values) instead of the ones derived from (u, v, level);
        (u, v) then only places the query's own key-point."""
        self.q.append(dict(u=u, v=v, desc=np.asarray(desc, np.uint8), angle=angle, level=self.level if level is None else level, kind=kind,
                           octave1=octave1, pos=pos, normal=normal, min_dist=min_dist, max_dist=max_dist))
        return len(self.q) - 1

    def arrays(self):
        nq = len(self.q)
        keys = _keys([(x, y, o, a) for x, y, o, a, _ in self.f])
        desc = np.array([d for *_, d in self.f], np.uint8).reshape(-1, 32)
        pos, mx, mn, nrm, lev = np.zeros((nq, 3), np.float32), np.zeros(nq, np.float32), np.zeros(nq, np.float32), np.zeros((nq, 3), np.float32), np.zeros(nq, np.int32)
        for i, q in enumerate(self.q):
            p = np.array([(q["u"] - 320.0) / 128.0, (q["v"] - 240.0) / 128.0, Z])
            if q["kind"] == "behind":
                p[2] = -Z
            if q["kind"] == "z0":
                p = np.array([1.0, 1.0, 0.0])
            if q["pos"] is not None:
                p = np.asarray(q["pos"], np.float64)
            pos[i] = p
            assert pos[i].astype(np.float64).tobytes() == p.tobytes(), "camera-frame coordinates must be exact in float32"
            if q["pos"] is not None:                            # a constructed point states all four attributes itself
                mx[i], mn[i], nrm[i], lev[i] = q["max_dist"], q["min_dist"], q["normal"], q["level"]
                assert float(mx[i]) == q["max_dist"] and float(mn[i]) == q["min_dist"] and np.array_equal(nrm[i].astype(np.float64), np.asarray(q["normal"], np.float64))
                continue
            dist = float(np.linalg.norm(p))
            mx[i] = dist * 1.2 ** (q["level"] - 0.5)           # PredictScale = ceil(level - 0.5) = level, half a level clear of both neighbours
            mn[i] = 0.1
            if q["kind"] == "far":
                mx[i] = dist / 2                                # dist > 1.2 * mfMaxDistance
            if q["kind"] == "near":
                mn[i] = dist * 2                                # dist < 0.8 * mfMinDistance
            d = p / dist
            e = np.cross(d, [0.0, 1.0, 0.0]); e /= np.linalg.norm(e)
            nrm[i] = math.cos(math.radians(25)) * d + math.sin(math.radians(25)) * e     # viewing cosine 0.906: clear of 0.998 and of 0.5
            lev[i] = q["level"]
        qdesc = np.array([q["desc"] for q in self.q], np.uint8).reshape(-1, 32)
        qkeys = _keys([(q["u"], q["v"], q["level"] if q["octave1"] is None else q["octave1"], q["angle"]) for q in self.q])
        return dict(keys=keys, desc=desc, pos=pos, max_dist=mx, min_dist=mn, normal=nrm, level=lev, qdesc=qdesc, qkeys=qkeys, nq=nq,
                    u=np.array([q["u"] for q in self.q], np.float32), v=np.array([q["v"] for q in self.q], np.float32),
                    visible=np.array([q["kind"] == "ok" for q in self.q], np.uint8), occ=dict(self.occ), w=self.w, h=self.h, R=self.R, **self.par)

    def case(self, name, member, family, cite, win, count=None, nnratio=0.8, ori=False, prev=None, **par):
        """win[q] = the feature query q ends up matched to (-1 none), written down by the case; count = the reference's return value
        when it differs from the number of wins."""
        self.par.update(par)
        inp = self.arrays()
        n, nq = len(self.f), len(self.q)
        wins = sum(1 for f in win if f >= 0)
        pm = None
        if member in ("MP", "LAST", "RELOC", "SIM3P"):
            arr = np.full(n, -1, np.int32)
            for k, fi in enumerate(sorted(self.occ)):
                arr[fi] = -2 if member == "SIM3P" else nq + k
            for qi, fi in enumerate(win):
                if fi >= 0:
                    arr[fi] = qi
        else:
            arr = np.array(win, np.int32).reshape(-1)
        if member == "INIT":
            pm0 = np.stack([inp["u"], inp["v"]], 1) if prev is None else np.asarray(prev, np.float32)
            pm = pm0.copy()
            for qi, fi in enumerate(win):
                if fi >= 0:
                    pm[qi] = (self.f[fi][0], self.f[fi][1])
            inp["prev"] = pm0
        return Case(name, member, family, cite, inp, wins if count is None else count, arr, nnratio, ori, pm)


def _mp_fields(inp):
    """What Frame::isInFrustum leaves on the points, stated by construction (projection exact, level by design)."""
    nq, extra = inp["nq"], len(inp["occ"])
    tot = nq + extra
    z = lambda a, t: np.concatenate([np.asarray(a, t), np.zeros((extra,) + np.shape(a)[1:], t)])
    obs = np.concatenate([np.ones(nq, np.int32), np.array([inp["occ"][k] for k in sorted(inp["occ"])], np.int32)])
    return dict(track_in_view=z(inp["visible"], np.uint8), proj_x=z(inp["u"], np.float32), proj_y=z(inp["v"], np.float32), scale_level=z(inp["level"], np.int32),
                view_cos=z(np.full(nq, 0.906, np.float32), np.float32), track_depth=z(np.linalg.norm(inp["pos"], axis=1), np.float32),
                is_bad=np.zeros(tot, np.uint8), desc=z(inp["qdesc"], np.uint8), obs=obs), tot


def _state(inp, n, taken=None):
    a = np.full(n, -1, np.int32)
    for k, fi in enumerate(sorted(inp["occ"])):
        a[fi] = inp["nq"] + k if taken is None else taken
    return a


def _pts(inp, tot):
    pad = lambda a: np.concatenate([a, np.ones((tot - len(a),) + a.shape[1:], a.dtype)])
    return dict(skip=np.concatenate([np.zeros(inp["nq"], np.uint8), np.ones(tot - inp["nq"], np.uint8)]), pos=pad(inp["pos"]), normal=pad(inp["normal"]),
                min_dist=pad(inp["min_dist"]), max_dist=pad(inp["max_dist"]), desc=pad(inp["qdesc"]))


def _sim3_sides(inp):
    """Side 1: the queries (points of KF1's features, seen from camera 2 = the frame).  Side 2: every frame feature's own point, sitting at
    its pixel at depth 4, seen from camera 1 whose features are the queries' key-points; level of the nearest query."""
    side1 = dict(skip=np.zeros(inp["nq"], np.uint8), pc=inp["pos"], min_dist=inp["min_dist"], max_dist=inp["max_dist"], desc=inp["qdesc"])
    k = inp["keys"]
    pc = np.stack([(k["x"].astype(np.float64) - 320) / 128, (k["y"].astype(np.float64) - 240) / 128, np.full(len(k), Z)], 1)
    near = [int(np.argmin((inp["u"] - x) ** 2 + (inp["v"] - y) ** 2)) for x, y in zip(k["x"], k["y"])]
    dist = np.linalg.norm(pc, axis=1)
    side2 = dict(skip=np.asarray(inp.get("skip2", np.zeros(len(k))), np.uint8), pc=pc.astype(np.float32), min_dist=np.full(len(k), 0.1, np.float32),
                 max_dist=(dist * 1.2 ** (inp["level"][near] - 0.5)).astype(np.float32), desc=inp["desc"])
    return side1, side2


def call_oracle(O, c):
    """(count, result array[, prev_matched]) of ``oracle_lib`` for a case."""
    i, m = c.inp, c.member
    if m in BOW_MEMBERS:
        return _call_bow(O, None, None, c)
    n = len(i["keys"])
    if m == "MP":
        mp, _ = _mp_fields(i)
        return O.search_by_projection_mappoints(i["keys"], i["desc"], i["w"], i["h"], SF, mp, _state(i, n), i["R"] / 4.0, False, 0.0, c.nnratio)
    tot = i["nq"] + len(i["occ"])
    obs = _mp_fields(i)[0]["obs"]
    if m == "LAST":
        pts = _pts(i, tot)
        return O.search_by_projection_frame(i["keys"], i["desc"], i["w"], i["h"], SF, i.get("Tcw7", IDENT7), K4, i["qkeys"], np.arange(i["nq"], dtype=np.int32),
                                            np.zeros(i["nq"], np.uint8), pts["pos"], pts["desc"], obs, _state(i, n), float(i["R"]), c.ori)
    if m == "RELOC":
        pts = dict(_pts(i, tot), skip=np.zeros(tot, np.uint8))
        return O.search_by_projection_reloc(i["keys"], i["desc"], i["w"], i["h"], SF, LOG_SF, i.get("Tcw7", IDENT7), i.get("Ow", np.zeros(3, np.float32)), K4, i["qkeys"],
                                            np.arange(i["nq"], dtype=np.int32), pts, _state(i, n), float(i["R"]), i["orb_dist"], c.ori)
    if m == "SIM3P":
        return O.search_by_projection_sim3(i["keys"], i["desc"], i["w"], i["h"], SF, LOG_SF, i.get("Tcw7", IDENT7), i.get("Ow", np.zeros(3, np.float32)), K4, _pts(i, i["nq"]),
                                           _state(i, n, -2), i["R"], i["ratio_hamming"], i["variant"])
    if m == "FUSE":
        r = O.fuse_candidates(i["keys"], i["desc"], i["w"], i["h"], SF, LOG_SF, i.get("Tcw7", IDENT7), i.get("Ow", np.zeros(3, np.float32)), K4, _pts(i, i["nq"]), float(i["R"]), i["reproj"])
        return int(np.count_nonzero(r >= 0)), r
    if m == "SIM3":
        s1, s2 = _sim3_sides(i)
        return O.search_by_sim3(i["qkeys"], i["qdesc"], i["keys"], i["desc"], i["w"], i["h"], SF, LOG_SF, K4, s1, s2, float(i["R"]))
    if m == "INIT":
        return O.search_for_initialization(i["qkeys"], i["qdesc"], i["keys"], i["desc"], i["w"], i["h"], i["prev"], i["R"], c.nnratio, c.ori)
    raise KeyError(m)


def call_gpu(M, h, c):
    """The same through ``rumi_slam_amd.matcher`` (M) with the ORBmatcher handle h."""
    i, m = c.inp, c.member
    h.mfNNratio, h.mbCheckOrientation = c.nnratio, c.ori
    if m in BOW_MEMBERS:
        return _call_bow(None, M, h, c)
    n = len(i["keys"])
    F = M.FrameView(i["keys"], i["desc"], i["w"], i["h"], SF)
    tot = i["nq"] + len(i["occ"])
    obs = _mp_fields(i)[0]["obs"]
    Ow, T7 = i.get("Ow", np.zeros(3, np.float32)), i.get("Tcw7", IDENT7)
    if m == "MP":
        mp, _ = _mp_fields(i)
        return h.SearchByProjection_MapPoints(F, mp, _state(i, n), i["R"] / 4.0)
    if m == "LAST":
        pts = _pts(i, tot)
        return h.SearchByProjection_Frame(F, T7, K4, i["qkeys"], np.arange(i["nq"], dtype=np.int32), np.zeros(i["nq"], np.uint8), pts["pos"], pts["desc"],
                                          obs, _state(i, n), float(i["R"]))
    if m == "RELOC":
        pts = dict(_pts(i, tot), skip=np.zeros(tot, np.uint8))
        return M.SearchByProjection_Reloc(h, F, LOG_SF, T7, Ow, K4, i["qkeys"], np.arange(i["nq"], dtype=np.int32), pts, _state(i, n), float(i["R"]), i["orb_dist"])
    if m == "SIM3P":
        return M.SearchByProjection_Sim3(h, F, LOG_SF, T7, Ow, K4, _pts(i, i["nq"]), _state(i, n, -2), i["R"], i["ratio_hamming"], bool(i["variant"]))
    if m == "FUSE":
        r = M.FuseCandidates(h, F, LOG_SF, T7, Ow, K4, _pts(i, i["nq"]), float(i["R"]), bool(i["reproj"]))
        return int(np.count_nonzero(r >= 0)), r
    if m == "SIM3":
        s1, s2 = _sim3_sides(i)
        return M.SearchBySim3(h, M.FrameView(i["qkeys"], i["qdesc"], i["w"], i["h"], SF), F, K4, LOG_SF, s1, s2, float(i["R"]))
    if m == "INIT":
        return h.SearchForInitialization(M.FrameView(i["qkeys"], i["qdesc"], i["w"], i["h"], SF), F, i["prev"], i["R"])
    raise KeyError(m)


def call_gpu_fused(M, h, c):
    """MP cases through the fused frustum + search entry: the points go in as 3-D points, the tracking fields never leave the device."""
    i = c.inp
    h.mfNNratio = c.nnratio
    F = M.FrameView(i["keys"], i["desc"], i["w"], i["h"], SF)
    mp, tot = _mp_fields(i)
    pts = dict(_pts(i, tot), obs=mp["obs"])
    nto, nm, fm, _ = h.SearchLocalPoints(F, i.get("Rcw", np.eye(3, dtype=np.float32)).ravel(), i.get("tcw", np.zeros(3, np.float32)),
                                         i.get("Ow", np.zeros(3, np.float32)), K4, LOG_SF, 8, pts, _state(i, len(i["keys"])), i["R"] / 4.0,
                                         i.get("far", False), i.get("th_far", 50.0))
    return nm, fm


# ---------------------------------------------------------------------------------------------------------------------------------
# BoW members: two feature sets and the FeatureVector nodes that pair them
# ---------------------------------------------------------------------------------------------------------------------------------
class Bow:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.f1, self.f2, self.nodes = [], [], {}

    def base(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def feat1(self, desc, angle=0.0):
        self.f1.append((angle, np.asarray(desc, np.uint8))); return len(self.f1) - 1

    def feat2(self, desc, angle=0.0):
        self.f2.append((angle, np.asarray(desc, np.uint8))); return len(self.f2) - 1

    def node(self, nid, list1, list2):
        self.nodes[nid] = (list(list1), list(list2))

    def case(self, name, member, family, cite, win, nnratio=0.75, ori=False):
        """win[i1] = the second-set feature that first-set feature i1 ends up matched to (-1 none)."""
        n1, n2 = len(self.f1), len(self.f2)
        place = lambda n, feats: _keys([(10 + 10 * (j % 60), 10 + 10 * (j // 60), 0, feats[j][0]) for j in range(n)])
        inp = dict(k1=place(n1, self.f1), d1=np.array([d for _, d in self.f1], np.uint8).reshape(-1, 32), k2=place(n2, self.f2),
                   d2=np.array([d for _, d in self.f2], np.uint8).reshape(-1, 32), fv1=csr({k: v[0] for k, v in self.nodes.items()}),
                   fv2=csr({k: v[1] for k, v in self.nodes.items()}))
        wins = sum(1 for f in win if f >= 0)
        if member == "BOW_F":
            arr = np.full(n2, -1, np.int32)
            for k, f in enumerate(win):
                if f >= 0:
                    arr[f] = k                                   # map point id of first-set feature k is k
        elif member == "BOW_KF":
            arr = np.array(win, np.int32).reshape(-1)
        else:
            arr = np.array([(k, f) for k, f in enumerate(win) if f >= 0], np.int64).reshape(-1, 2)
        return Case(name, member, family, cite, inp, wins, arr, nnratio, ori)


def _call_bow(O, M, h, c):
    i, m = c.inp, c.member
    n1, n2 = len(i["k1"]), len(i["k2"])
    ids1 = np.arange(n1, dtype=np.int32)
    none1, none2 = np.full(n1, -1, np.int32), np.full(n2, -1, np.int32)
    F12, ep = np.zeros(9, np.float32), np.array([-1000, -1000], np.float32)       # bCoarse: no epipolar line; epipole far from every key-point
    if O is not None:
        if m == "BOW_F":
            return O.search_by_bow(i["k1"], i["d1"], ids1, np.zeros(n1, np.uint8), i["fv1"], i["k2"], i["d2"], i["fv2"], c.nnratio, c.ori)
        if m == "BOW_KF":
            return O.search_by_bow_kf(i["k1"], i["d1"], ids1, i["fv1"], i["k2"], i["d2"], n1 + np.arange(n2, dtype=np.int32), i["fv2"], np.zeros(n1 + n2, np.uint8),
                                      c.nnratio, c.ori)
        return O.search_for_triangulation(i["k1"], i["d1"], none1, i["fv1"], i["k2"], i["d2"], none2, i["fv2"], SF, F12, ep, False, True, c.ori)
    A, B = M.FrameView(i["k1"], i["d1"], 640, 480, SF), M.FrameView(i["k2"], i["d2"], 640, 480, SF)
    a, b = M.FeatureVector.from_csr(*i["fv1"]), M.FeatureVector.from_csr(*i["fv2"])
    if m == "BOW_F":
        return h.SearchByBoW(A, a, ids1, np.zeros(n1, np.uint8), B, b)
    if m == "BOW_KF":
        return M.SearchByBoW_KF(h, A, a, ids1, B, b, n1 + np.arange(n2, dtype=np.int32), np.zeros(n1 + n2, np.uint8))
    return M.SearchForTriangulation(h, A, a, none1, B, b, none2, F12, ep, False, True)


def call_gpu_bow_batch(M, h, c, K=3):
    """A BOW_F case as K identical candidate key-frames of one SearchByBoW_batch call."""
    i = c.inp
    h.mfNNratio, h.mbCheckOrientation = c.nnratio, c.ori
    n1 = len(i["k1"])
    A, B = M.FrameView(i["k1"], i["d1"], 640, 480, SF), M.FrameView(i["k2"], i["d2"], 640, 480, SF)
    a, b = M.FeatureVector.from_csr(*i["fv1"]), M.FeatureVector.from_csr(*i["fv2"])
    return M.SearchByBoW_batch(h, [A] * K, [a] * K, [np.arange(n1, dtype=np.int32)] * K, [np.zeros(n1, np.uint8)] * K, B, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------
U0, V0 = 325.0, 245.0                   # default query pixel; R = 8 window at level 0 spans x in (317, 333)
CITE_BEST = {"MP": "ORBmatcher.cc:94", "LAST": "ORBmatcher.cc:1578", "RELOC": "ORBmatcher.cc:1750", "SIM3P": "ORBmatcher.cc:458", "FUSE": "ORBmatcher.cc:1154",
             "SIM3": "ORBmatcher.cc:1393", "INIT": "ORBmatcher.cc:620", "BOW_F": "ORBmatcher.cc:255", "BOW_KF": "ORBmatcher.cc:748", "TRI": "ORBmatcher.cc:906"}
CITE_TH = {"MP": "ORBmatcher.cc:107", "LAST": "ORBmatcher.cc:1584", "RELOC": "ORBmatcher.cc:1756", "SIM3P": "ORBmatcher.cc:464", "FUSE": "ORBmatcher.cc:1161",
           "SIM3": "ORBmatcher.cc:1399", "INIT": "ORBmatcher.cc:629", "BOW_F": "ORBmatcher.cc:290", "BOW_KF": "ORBmatcher.cc:757", "TRI": "ORBmatcher.cc:906"}
CITE_RATIO = {"MP": "ORBmatcher.cc:108", "INIT": "ORBmatcher.cc:630", "BOW_F": "ORBmatcher.cc:291", "BOW_KF": "ORBmatcher.cc:758"}
# a ratio that lets an exact tie through: MP rejects only on >, the strict members need r > 1
TIE_RATIO = {"MP": 1.0, "INIT": 2.0, "BOW_F": 2.0, "BOW_KF": 2.0}


def _contest(member, seed, cands, win_pos, name, family, cite, nnratio=0.8, level=0, order=None, **par):
    """One query, candidates (dx, dy, dist[, octave]) around it; feature index = position in ``cands``; ``order`` = the visit order the
    case claims (checked against the grid rule); win_pos = the candidate the reference picks (-1 none)."""
    s = Proj(seed, level=level)
    b = s.base()
    for cd in cands:
        s.feat(U0 + cd[0], V0 + cd[1], desc_at(b, cd[2], s.rng), cd[3] if len(cd) > 3 else None)
    s.query(U0, V0, b)
    if order is not None:
        assert visit_order([(U0 + c[0], V0 + c[1]) for c in cands], 640, 480) == order, name
    return s.case(name, member, family, cite, [win_pos], nnratio=nnratio, **par)


def _bow_contest(member, seed, dists, win_pos, name, family, cite, nnratio=0.75):
    """One first-set feature, candidates at the given distances in the node's list order; their feature indices run AGAINST list order."""
    s = Bow(seed)
    b = s.base()
    k = s.feat1(b)
    n = len(dists)
    for j in range(n):                                             # feature index j sits at list position n - 1 - j
        s.feat2(desc_at(b, dists[n - 1 - j], s.rng))
    s.node(7, [k], [n - 1 - p for p in range(n)])
    return s.case(name, member, family, cite, [-1 if win_pos < 0 else n - 1 - win_pos], nnratio=nnratio)


def family_A():
    out = []
    for m in PROJ_MEMBERS:
        r = TIE_RATIO.get(m, 0.8)
        # feature 0 at x = 331 (cell column 33), feature 1 at x = 319 (column 32): the higher index is visited first and wins
        out.append(_contest(m, 10, [(6, 0, 20), (-6, 0, 20)], 1, "two", "A", CITE_BEST[m], r, order=[1, 0]))
        # three: columns 33, 32 (row 25), 32 (row 24): visit order 2, 1, 0
        out.append(_contest(m, 11, [(6, 0, 20), (-6, 4, 20), (-6, -4, 20)], 2, "three", "A", CITE_BEST[m], r, order=[2, 1, 0]))
    for m in BOW_MEMBERS:
        last = m == "TRI"                                           # :906 skips only on dist > bestDist, so an equal distance replaces the best
        out.append(_bow_contest(m, 12, [20, 20], 1 if last else 0, "two", "A", CITE_BEST[m], TIE_RATIO.get(m, 0.75)))
        out.append(_bow_contest(m, 13, [20, 20, 20], 2 if last else 0, "three", "A", CITE_BEST[m], TIE_RATIO.get(m, 0.75)))
    return out


def family_B():
    out = []
    # MP: the ratio test applies only when best and second share an octave (:108); r < 1 then rejects an exact tie
    out.append(_contest("MP", 20, [(6, 0, 20, 0), (-6, 0, 20, 0)], -1, "same_octave", "B", "ORBmatcher.cc:108", 0.9, level=0))
    out.append(_contest("MP", 21, [(6, 0, 20, 0), (-6, 0, 20, 1)], 1, "other_octave", "B", "ORBmatcher.cc:111", 0.9, level=1))
    out.append(_contest("INIT", 22, [(6, 0, 20), (-6, 0, 20)], -1, "r1", "B", CITE_RATIO["INIT"], 1.0))
    for m in ("BOW_F", "BOW_KF"):
        out.append(_bow_contest(m, 23, [20, 20], -1, "r1", "B", CITE_RATIO[m], 1.0))
    return out


def _single(member, seed, dist, win, name, family, cite, nnratio=0.8, **par):
    if member in BOW_MEMBERS:
        return _bow_contest(member, seed, [dist], 0 if win else -1, name, family, cite, nnratio)
    return _contest(member, seed, [(2, 1, dist)], 0 if win else -1, name, family, cite, nnratio, **par)


def family_C():
    out = []
    for m in MEMBERS:
        th = ACCEPT[m]
        out.append(_single(m, 30, th, True, f"at_{th}", "C", CITE_TH[m], 0.9))
        out.append(_single(m, 31, th + 1, False, f"at_{th + 1}", "C", CITE_TH[m], 0.9))
    # the reference's callers pass ratioHamming 1.5 and 1.0 (LoopClosing.cc:716, :738, :911); both overloads
    for variant in (0, 1):
        cite = "ORBmatcher.cc:464" if variant == 0 else "ORBmatcher.cc:571"
        out.append(_single("SIM3P", 32, 50, True, f"rh1_at_50_v{variant}", "C", cite, ratio_hamming=1.0, variant=variant))
        out.append(_single("SIM3P", 33, 51, False, f"rh1_at_51_v{variant}", "C", cite, ratio_hamming=1.0, variant=variant))
        out.append(_single("SIM3P", 34, 75, True, f"rh15_at_75_v{variant}", "C", cite, ratio_hamming=1.5, variant=variant))
        out.append(_single("SIM3P", 35, 76, False, f"rh15_at_76_v{variant}", "C", cite, ratio_hamming=1.5, variant=variant))
    out.append(_single("RELOC", 36, 100, True, "orbdist100_at_100", "C", "ORBmatcher.cc:1756", orb_dist=100))
    out.append(_single("RELOC", 37, 101, False, "orbdist100_at_101", "C", "ORBmatcher.cc:1756", orb_dist=100))
    return out


def family_D():
    out = []
    for r, lo, hi in [(0.5, 40, 80), (0.75, 30, 40)]:
        for m in RATIO_MEMBERS:
            strict = m != "MP"
            for best, ok in [(lo - 1, True), (lo, not strict), (lo + 1, False)]:
                name = f"r{r}_{best}_{hi}"
                if m in BOW_MEMBERS:
                    out.append(_bow_contest(m, 40 + best, [hi, best], 1 if ok else -1, name, "D", CITE_RATIO[m], r))
                else:                                                # same octave, so MP's test applies
                    out.append(_contest(m, 40 + best, [(6, 0, hi), (-6, 0, best)], 1 if ok else -1, name, "D", CITE_RATIO[m], r))
    return out


# E: (angle of the query side, angle of the frame side, intended bin).  rot = a1 - a2.
def _hist(groups):
    pairs = []
    for a1, a2, b, cnt in groups:
        assert rot_bin(a1, a2) == b, (a1, a2, b)
        rot = float(np.float32(a1) - np.float32(a2)) % 360.0
        assert cnt == 0 or (a1, a2) in ON_EDGE or min(abs(rot / 30.0 - (k + 0.5)) for k in range(13)) * 30.0 > 1e-3, "rot sits on a bin edge"
        pairs += [(a1, a2, b)] * cnt
    return pairs


# rot = 15 degrees: float32(15) * float32(1/30) = 0.5 exactly (the product 0.50000002607 rounds down), and round(0.5) = 1
ON_EDGE = {(15.0, 0.0)}
assert np.float32(15.0) * (np.float32(1.0) / np.float32(30)) == np.float32(0.5)
# a negative rot of -1e-6 becomes float32(360 - 1e-6) = 360.0f, whose product with float32(1/30) rounds to bin 12
assert np.float32(np.float32(0.0) - np.float32(1e-6)) + np.float32(360.0) == np.float32(360.0)
HISTOGRAMS = {
    # bins 3:5, 0:4 (rot == 0), 6:2, 12:2 (tiny negative rot), 1:1 (on the edge).  The scan's strict > keeps bin 6 as third (seen
    # before bin 12 with the same count): bins 3, 0, 6 survive, 12 and 1 go (:1802-1817)
    "equal_third": (_hist([(90.0, 0.0, 3, 5), (33.0, 33.0, 0, 4), (200.0, 20.0, 6, 2), (0.0, 1e-6, 12, 2), (15.0, 0.0, 1, 1)]), {3, 0, 6}, "ORBmatcher.cc:1814"),
    # max1 = 10, max2 = 1: 1 < 0.1f * 10 is false (the float product is 1.0), second and third are kept; the fourth single bin goes
    "cut_kept": (_hist([(60.0, 0.0, 2, 10), (155.0, 5.0, 5, 1), (250.0, 10.0, 8, 1), (300.0, 0.0, 10, 1)]), {2, 5, 8}, "ORBmatcher.cc:1820"),
    # max1 = 11, max2 = 1: 1 < 1.1 drops second and third
    # four bins of four: every comparison of the scan is strict, so the first three bins met keep their ranks and bin 9 goes (:1802)
    "four_equal": (_hist([(30.0, 0.0, 1, 4), (125.0, 5.0, 4, 4), (211.0, 1.0, 7, 4), (270.0, 0.0, 9, 4)]), {1, 4, 7}, "ORBmatcher.cc:1802"),
    "cut_dropped": (_hist([(60.0, 0.0, 2, 11), (155.0, 5.0, 5, 1), (250.0, 10.0, 8, 1)]), {2}, "ORBmatcher.cc:1820"),
}


def family_E():
    out = []
    for hname, (pairs, keep, cite) in HISTOGRAMS.items():
        assert len(pairs) >= 13
        for ori in (True, False):
            for m in ORI_MEMBERS:
                name = f"{hname}_{'on' if ori else 'off'}"
                win = [k if (not ori or b in keep) else -1 for k, (_, _, b) in enumerate(pairs)]
                if m in BOW_MEMBERS:
                    s = Bow(50)
                    for k, (a1, a2, _) in enumerate(pairs):          # one node per pair, descriptors 3 bits apart
                        b = s.base()
                        s.node(3 + 2 * k, [s.feat1(b, a1)], [s.feat2(desc_at(b, 3, s.rng), a2)])
                    out.append(s.case(name, m, "E", cite, win, 0.9, ori))
                else:
                    s = Proj(51)
                    for k, (a1, a2, _) in enumerate(pairs):          # one window per pair, 48 px apart
                        b = s.base()
                        u, v = 40.0 + 48 * (k % 12), 60.0 + 64 * (k // 12)
                        s.feat(u + 2, v + 1, desc_at(b, 3, s.rng), angle=a2)
                        s.query(u, v, b, angle=a1)
                    out.append(s.case(name, m, "E", cite, win, nnratio=0.9, ori=ori))
    return out


def family_F():
    out = []
    ulp_in = float(np.nextafter(np.float32(U0 + 8), np.float32(0)))          # 333 - 2^-15: |dx| = 8 - 2^-15 < r
    for m in PROJ_MEMBERS:
        lv = LEVELS[m]
        # |dx| == r is outside (strict <, Frame.cc:743 / KeyFrame.cc:918); one ulp less is inside.  The far candidate has the better descriptor.
        s = Proj(60); b = s.base()
        s.feat(U0 + 8, V0, desc_at(b, 2, s.rng)); s.feat(U0 - 3, V0 - 8, desc_at(b, 2, s.rng)); s.feat(U0 + 1, V0 + 1, desc_at(b, 30, s.rng)); s.query(U0, V0, b)
        out.append(s.case("on_radius", m, "F", "Frame.cc:743", [2]))
        s = Proj(61); b = s.base()
        s.feat(ulp_in, V0, desc_at(b, 2, s.rng)); s.feat(U0 + 1, V0 + 1, desc_at(b, 30, s.rng)); s.query(U0, V0, b)
        out.append(s.case("ulp_inside", m, "F", "Frame.cc:743", [0]))
        # x = 636 rounds to cell column 64: the key-point is in no cell and never a candidate (Frame.cc:757); x = 630 is in column 63
        s = Proj(62); b = s.base()
        assert cell_of(636, 245, 640, 480) is None and cell_of(630, 245, 640, 480) == (63, 25)
        s.feat(636, V0, desc_at(b, 2, s.rng)); s.feat(630, V0, desc_at(b, 30, s.rng)); s.query(632, V0, b)
        out.append(s.case("outside_grid", m, "F", "Frame.cc:757", [1]))
        # queries that are skipped before any window is formed; each has a perfect feature waiting where it would land
        if m != "INIT":
            s = Proj(63); b = [s.base() for _ in range(6)]
            f_ok = s.feat(100, 100, b[0]); s.query(100, 100, b[0])
            f_far = s.feat(200, 100, b[1]); s.query(200, 100, b[1], kind="far")
            f_near = s.feat(300, 100, b[2]); s.query(300, 100, b[2], kind="near")
            s.feat(400, 300, b[3]); f_mirror = s.feat(640 - 400, 480 - 300, b[3]); s.query(400, 300, b[3], kind="behind")
            s.query(500, 300, b[4], kind="z0")
            s.feat(630, 400, b[5]); s.query(704, 400, b[5])                 # u = 704 is right of the image
            win = [f_ok, -1, -1, -1, -1, -1]
            cite = "ORBmatcher.cc:1528"
            if m == "RELOC":                                               # :1706-1713 has no depth test: a point behind the camera lands mirrored
                win[3] = f_mirror
                cite = "ORBmatcher.cc:1708"
            if m == "LAST":                                                # :1516-1553 has no distance gate
                win[1], win[2] = f_far, f_near
            if m == "MP":                                                  # the gates live in Frame::isInFrustum; the search sees mbTrackInView
                s.q[4]["kind"] = "behind"; s.q[5]["kind"] = "far"
            out.append(s.case("gates", m, "F", cite, win))
            # u == 640: Frame members test u > mnMaxX (:1533, :1710), key-frame members IsInImage u < mnMaxX (KeyFrame.cc:928)
            s = Proj(64); b = s.base()
            s.feat(634, V0, desc_at(b, 3, s.rng)); s.query(640, V0, b)
            out.append(s.case("on_right_edge", m, "F", "KeyFrame.cc:928", [0 if m in ("MP", "LAST", "RELOC") else -1]))
        # frames whose grid cells are not 10 px: two tied candidates share a cell there (index order) but not on a 10 px grid
        for (w, h), xa, xb in [((752, 480), 99.0, 94.0), ((1241, 376), 97.0, 94.0)]:
            assert cell_of(xa, 100, w, h) == cell_of(xb, 100, w, h) and c_round(xa / 10) != c_round(xb / 10)
            s = Proj(65, w, h); b = s.base()
            s.feat(xa, 100, desc_at(b, 20, s.rng)); s.feat(xb, 100, desc_at(b, 20, s.rng)); s.query(96, 100, b)
            out.append(s.case(f"frame_{w}x{h}", m, "F", "Frame.cc:322", [0], nnratio=TIE_RATIO.get(m, 0.8)))
            s = Proj(66, w, h); b = s.base()                                # a window on the frame's far corner cells
            s.feat(w - 14, h - 9, desc_at(b, 9, s.rng)); s.query(w - 12, h - 12, b)
            out.append(s.case(f"corner_{w}x{h}", m, "F", "Frame.cc:707", [0]))
        # octave window at level 0 and level 7: candidates two below .. two above, the best descriptors OUTSIDE the member's window
        for L in (0, 7):
            dist_of = {-2: 10, -1: 20, 0: 30, 1: 15, 2: 5}
            s = Proj(67, level=L); b = s.base()
            offs = [o for o in (-2, -1, 0, 1, 2) if 0 <= L + o <= 7]
            for k, o in enumerate(offs):
                s.feat(U0 - 4 + 2 * k, V0 + 1, desc_at(b, dist_of[o], s.rng), octave=L + o)
            if m == "INIT":                                                 # :596-599: only octave-0 key-points query, only octave 0 answers
                s.query(U0, V0, b, octave1=0 if L == 0 else 1)
                win = offs.index(0) if L == 0 else -1
                cite = "ORBmatcher.cc:599"
            else:
                s.query(U0, V0, b)
                allowed = [o for o in offs if lv[0] <= o <= lv[1]]
                win = offs.index(min(allowed, key=lambda o: dist_of[o]))
                cite = {"MP": "ORBmatcher.cc:65", "LAST": "ORBmatcher.cc:1550", "RELOC": "ORBmatcher.cc:1731", "SIM3P": "ORBmatcher.cc:451", "FUSE": "ORBmatcher.cc:1122",
                        "SIM3": "ORBmatcher.cc:1386"}[m]
            out.append(s.case(f"octaves_L{L}", m, "F", cite, [win]))
    # Fuse's first overload gates every candidate by its reprojection error (:1144): e2 = 9 > 5.99 at octave 0 rejects the better descriptor
    for reproj, win in ((1, 1), (0, 0)):
        s = Proj(68); b = s.base()
        s.feat(U0 + 3, V0, desc_at(b, 2, s.rng)); s.feat(U0 + 2, V0, desc_at(b, 30, s.rng)); s.query(U0, V0, b)
        out.append(s.case(f"reproj_{reproj}", "FUSE", "F", "ORBmatcher.cc:1144", [win], reproj=reproj))
    return out


def family_G():
    out = []
    for m in ("MP", "LAST", "RELOC", "SIM3P"):
        # feature 0 (perfect descriptor) already holds a point: skipped when that point has observations; RELOC and SIM3P skip any holder
        for obs in (1, 0):
            s = Proj(70); b = s.base()
            s.feat(U0 + 2, V0, b); s.feat(U0 - 2, V0, desc_at(b, 20, s.rng)); s.query(U0, V0, b)
            s.occ[0] = obs
            over = obs == 0 and m in ("MP", "LAST")
            cite = {"MP": "ORBmatcher.cc:80", "LAST": "ORBmatcher.cc:1563", "RELOC": "ORBmatcher.cc:1743", "SIM3P": "ORBmatcher.cc:446"}[m]
            out.append(s.case(f"holder_obs{obs}", m, "G", cite, [0 if over else 1]))
        # two points want feature 0; the first takes it, the second sees it taken (its holder has one observation) and takes feature 1
        s = Proj(71); b = s.base()
        s.feat(U0 + 2, V0, desc_at(b, 5, s.rng)); s.feat(U0 - 2, V0, desc_at(b, 20, s.rng)); s.query(U0, V0, b); s.query(U0, V0, b)
        out.append(s.case("same_feature", m, "G", CITE_BEST[m], [0, 1]))
    # INIT: a later, better query steals the feature and the count drops by one (:631-634); an equal one does not (:617)
    for d1, name, win in ((10, "steal", [-1, 0]), (20, "equal_keeps", [0, -1])):
        s = Proj(72); b = s.base()
        f = desc_at(b, 20, s.rng)
        s.feat(U0 + 2, V0 + 1, f)
        s.query(U0, V0, b)                                                  # 20 bits from the feature
        s.query(U0 + 1, V0, desc_at(f, d1, s.rng))                          # d1 bits from it
        c = s.case(name, "INIT", "G", "ORBmatcher.cc:617", win)
        out.append(c)
        out.append(s.case(name + "_second_call", "INIT", "G", "ORBmatcher.cc:675", win, prev=c.pm))
    # SIM3: query 0 picks feature 0, whose own point prefers key-point 1 of the first key-frame: no agreement, nothing found (:1488)
    s = Proj(73); b = s.base()
    f0 = desc_at(b, 20, s.rng)
    s.feat(U0 + 2, V0, f0); s.query(U0, V0, b); s.query(U0 + 1, V0 + 1, desc_at(f0, 5, s.rng), kind="far")
    out.append(s.case("one_way", "SIM3", "G", "ORBmatcher.cc:1488", [-1, -1]))
    s = Proj(74); b = s.base()                                              # the same without the rival: agreement
    s.feat(U0 + 2, V0, desc_at(b, 20, s.rng)); s.query(U0, V0, b)
    out.append(s.case("two_way", "SIM3", "G", "ORBmatcher.cc:1488", [0]))
    # BoW: second-set feature 0 is taken by the first query; BOW_F (:248) and BOW_KF (:738) give the second query feature 1, TRI never
    # marks a feature matched (vbMatched2 is only read, :893) so both pair with feature 0
    for m in BOW_MEMBERS:
        s = Bow(75); b = s.base()
        k0, k1 = s.feat1(b), s.feat1(b)
        a, c2 = s.feat2(desc_at(b, 5, s.rng)), s.feat2(desc_at(b, 30, s.rng))
        s.node(9, [k0, k1], [a, c2])
        out.append(s.case("same_feature", m, "G", {"BOW_F": "ORBmatcher.cc:248", "BOW_KF": "ORBmatcher.cc:738", "TRI": "ORBmatcher.cc:893"}[m],
                          [a, a] if m == "TRI" else [a, c2]))
    return out


def family_H():
    out = []
    for m in MEMBERS:
        out.append(_single(m, 80, 7, True, "one_and_one", "H", CITE_BEST[m]))
    lattice = [((i % 17 - 8) * 0.75, (i // 17 - 8) * 0.75) for i in range(289)]       # 17 x 17 points inside the R = 8 window
    for n in (63, 64, 65, 257):
        pts = lattice[:n][::-1]                                             # feature 0 is the last lattice point, so index order is not visit order
        xy = [(U0 + dx, V0 + dy) for dx, dy in pts]
        order = visit_order(xy, 640, 480)
        assert len(order) == n and order != sorted(order)
        for m in PROJ_MEMBERS:
            # all at 30 bits but the last visited at 10; then all tied at 30: the first visited wins, which is not feature 0
            s = Proj(81); b = s.base()
            for i, (x, y) in enumerate(xy):
                s.feat(x, y, desc_at(b, 10 if i == order[-1] else 30, s.rng))
            s.query(U0, V0, b)
            out.append(s.case(f"n{n}_winner_last", m, "H", CITE_BEST[m], [order[-1]], nnratio=0.8))
            s = Proj(82); b = s.base()
            for x, y in xy:
                s.feat(x, y, desc_at(b, 30, s.rng))
            s.query(U0, V0, b)
            assert order[0] != 0
            out.append(s.case(f"n{n}_all_tied", m, "H", CITE_BEST[m], [order[0]], nnratio=TIE_RATIO.get(m, 0.8)))
        for m in BOW_MEMBERS:
            out.append(_bow_contest(m, 83, [30] * (n - 1) + [10], n - 1, f"n{n}_winner_last", "H", CITE_BEST[m], 0.75))
            out.append(_bow_contest(m, 84, [30] * n, n - 1 if m == "TRI" else 0, f"n{n}_all_tied", "H", CITE_BEST[m], TIE_RATIO.get(m, 0.75)))
    return out


NOT_APPLICABLE = {
    ("LAST", "B"): "no second-best is kept (:1557-1582)", ("RELOC", "B"): "no second-best is kept (:1738-1754)", ("SIM3P", "B"): "no second-best is kept (:442-462)",
    ("FUSE", "B"): "no second-best is kept (:1114-1158)", ("SIM3", "B"): "no second-best is kept (:1379-1397)", ("TRI", "B"): "no second-best is kept (:884-957)",
    ("LAST", "D"): "no ratio test", ("RELOC", "D"): "no ratio test", ("SIM3P", "D"): "no ratio test (ratioHamming scales the threshold, family C)",
    ("FUSE", "D"): "no ratio test", ("SIM3", "D"): "no ratio test", ("TRI", "D"): "no ratio test",
    ("MP", "E"): "no rotation histogram in this member", ("SIM3P", "E"): "no rotation histogram in this member", ("FUSE", "E"): "no rotation histogram in this member",
    ("SIM3", "E"): "no rotation histogram in this member",
    ("BOW_F", "F"): "candidates come from a FeatureVector node, no window or projection", ("BOW_KF", "F"): "candidates come from a FeatureVector node, no window or projection",
    ("TRI", "F"): "candidates come from a FeatureVector node, no window or projection",
    ("FUSE", "G"): "the search half keeps no state: points do not compete for features (:1116-1158)",
}

_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = family_A() + family_B() + family_C() + family_D() + family_E() + family_F() + family_G() + family_H()
        ids = [c.id for c in _ALL]
        assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
    return _ALL


def coverage():
    cov = {}
    for c in all_cases():
        cov.setdefault((c.member, c.family), []).append(c.name)
    return cov
