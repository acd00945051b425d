"""Constructed scenes for relocalisation by slot: rumi_track_compute_bow / rumi_track_reloc_bow / rumi_track_reloc_begin_resident.

The frame is reloc_cases.frame() (the oracle extractor's features, bit-equal to the device's).  Six candidate key-frames of a few dozen
features each are built FROM the frame: a key-frame feature is a copy of a frame feature's key-point and descriptor with chosen bits
flipped, and it is filed under that frame feature's FeatureVector node (a key-frame's mFeatVec is data: nothing asks its descriptor to
descend there).  Its Hamming distances to the features of the node are then known, and every condition below holds by construction;
`build()` still asserts each of them in numpy (`simulate` restates the walk of ORBmatcher.cc:198-370 for that purpose).

Two vocabulary settings over one synthetic tree (k = 10, L = 3):
  small   levelsup = 1: nodes of one to a few dozen features
  root    levelsup = L: the whole frame in ONE node of about 1500 features -- more than the 512 a node of rumi_search_by_bow_batch may hold

candidate   what it carries (all under nnratio = 0.75, check_orientation = true unless said)
  0 edges     best distance exactly TH_LOW (accepted), TH_LOW + 1 (refused); bestDist1 == nnratio * bestDist2 exactly in float, 30 against 40
              (refused); a NULL row entry and a bad point (skipped); a key-frame node the frame does not have; plain matches
  1 order     two frame features of one node at equal distance (refused at 0.75 whatever the order; at nnratio = 1.25 the earlier position
              wins), once anywhere in a node and once 16 or 32 positions apart, where one lane of a 16-lane walk meets both; two key-frame features contending for one frame feature: the first takes it, the second takes its runner-up, or nothing;
              in the root setting with the contended feature in each 512-position stretch of the node; its matches in four rotation bins,
              30 / 3 / 3 / 3 (the cut_kept histogram of match_cases.py three times over): 3 < 0.1f * 30 is false in float, so the second and
              the third bin stay and the fourth goes for being the fourth
  2 rotation  matches in four rotation bins, 12 / 8 / 6 / 3: ComputeThreeMaxima drops the fourth
  3 bad       a key-frame whose bad bit is set: not searched, count -1
  4 shared    29 against 39, one bit nearer than 30 against 40 (accepted); the points of candidate 0's plain matches again: one table row each
  5 sizes     plain matches in nodes of every size class the setting has
Point ids are the rows of one reloc_cases._Table (clean back-projections of their frame features under T_TRUE), so a refine chain can run on
the matches.
"""
import functools

import numpy as np

import oracle_lib as O
import reloc_cases as R
import voc_scene
from rumi_slam_amd.capi import KP_DTYPE

TH_LOW = 50
NNRATIO, NNRATIO_TIES = 0.75, 1.25
VOC_K, VOC_L, VOC_SEED = 10, 3, 3
SETTINGS = {"small": 1, "root": VOC_L}
ABSENT_NODE = 0x7FFFFFF0                # a node id no vocabulary of this size has
K = 6
SLOTS = [3, 7, 1, 9, 4, 6]              # the store slot of candidate k: not its index
EDGES, ORDER, ROTATION, BAD, SHARED, SIZES = range(K)
ROT_BINS = ((0, 12), (3, 8), (6, 6), (9, 3))
CUT_BINS = ((0, 30), (3, 3), (6, 3), (9, 3))      # candidate ORDER's histogram
N_PLAIN = 20


@functools.lru_cache(maxsize=None)
def voc_table():
    return voc_scene.synthetic_vocabulary(VOC_SEED, VOC_K, VOC_L)


@functools.lru_cache(maxsize=None)
def frame_fv(setting):
    """The frame's FeatureVector under a setting, from the CPU vocabulary: (node ids u32, offsets i32, indices u32)."""
    v = O.OracleVocabulary(*voc_table())
    return v.transform(R.frame()["desc"], SETTINGS[setting])[1]


def ham(row, rows):
    return np.unpackbits(np.asarray(rows, np.uint8).reshape(-1, 32) ^ np.asarray(row, np.uint8).reshape(1, 32), axis=1).sum(1).astype(np.int64)


def flipped(row, bits):
    d = np.array(row, np.uint8).copy()
    for b in bits:
        d[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return d


def bits_of(a, b, differ):
    """Bit numbers at which descriptors a and b differ (or agree)."""
    x = np.unpackbits((np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8)).reshape(32, 1), axis=1, bitorder="little").reshape(-1)
    return np.nonzero(x == (1 if differ else 0))[0]


def rot_bin(a, b):
    """ORBmatcher.cc:1592-1599 in float."""
    rot = np.float32(a) - np.float32(b)
    if rot < 0:
        rot = np.float32(rot + np.float32(360.0))
    bin_ = int(np.round(np.float32(rot * np.float32(1.0 / 30))))
    return 0 if bin_ == 30 else bin_


def simulate(kf, fv, f_keys, f_desc, point_bad, nnratio, check_ori):
    """SearchByBoW(KF, F) restated in numpy for the scene's own assertions -> (count, row, trace); trace[i] = (best, second, frame feature or
    -1, accepted) of key-frame feature i as the walk met it."""
    fn, fo, fi = fv
    row = np.full(len(f_keys), -1, np.int32)
    bins = np.full(len(f_keys), -1, np.int32)
    trace = {}
    node_at = {int(nd): a for a, nd in enumerate(fn)}
    for a, nd in enumerate(kf["fv"][0]):
        if int(nd) not in node_at:
            continue
        members = fi[fo[node_at[int(nd)]]:fo[node_at[int(nd)] + 1]].astype(np.int64)
        for i in kf["fv"][2][kf["fv"][1][a]:kf["fv"][1][a + 1]]:
            i = int(i)
            p = int(kf["mp"][i])
            if p < 0 or point_bad[p]:
                continue
            free = members[row[members] < 0]
            d = ham(kf["desc"][i], f_desc[free]) if len(free) else np.zeros(0, np.int64)
            order = np.argsort(d, kind="stable")
            best = int(d[order[0]]) if len(d) else 256
            second = int(d[order[1]]) if len(d) > 1 else 256
            ok = best <= TH_LOW and np.float32(best) < np.float32(nnratio) * np.float32(second)
            f = int(free[order[0]]) if len(d) else -1
            trace[i] = (best, second, f, bool(ok))
            if ok:
                row[f] = p
                bins[f] = rot_bin(kf["keys"]["angle"][i], f_keys["angle"][f])
    hist = np.bincount(bins[bins >= 0], minlength=30)
    if check_ori:
        m = [0, 0, 0]; ind = [-1, -1, -1]
        for i in range(30):
            s = int(hist[i])
            if s > m[0]:
                m = [s, m[0], m[1]]; ind = [i, ind[0], ind[1]]
            elif s > m[1]:
                m = [m[0], s, m[1]]; ind = [ind[0], i, ind[1]]
            elif s > m[2]:
                m[2] = s; ind[2] = i
        if m[1] < np.float32(0.1) * np.float32(m[0]):
            ind[1] = ind[2] = -1
        elif m[2] < np.float32(0.1) * np.float32(m[0]):
            ind[2] = -1
        drop = (bins >= 0) & ~np.isin(bins, [b for b in ind if b >= 0])
        row[drop] = -1
    return int((row >= 0).sum()), row, trace, hist


class _KeyFrame:
    def __init__(self):
        self.keys, self.desc, self.node, self.mp, self.tag = [], [], [], [], []

    def add(self, key, desc, node, mp, tag):
        self.keys.append(key); self.desc.append(desc); self.node.append(int(node)); self.mp.append(int(mp)); self.tag.append(tag)
        return len(self.mp) - 1

    def arrays(self):
        node = np.array(self.node, np.int64)
        ids = np.unique(node)
        idx = [np.nonzero(node == nd)[0] for nd in ids]
        off = np.zeros(len(ids) + 1, np.int32)
        off[1:] = np.cumsum([len(x) for x in idx])
        return dict(keys=np.array(self.keys, KP_DTYPE), desc=np.array(self.desc, np.uint8).reshape(-1, 32), mp=np.array(self.mp, np.int32), tag=list(self.tag),
                    fv=(ids.astype(np.uint32), off, (np.concatenate(idx) if idx else np.zeros(0)).astype(np.uint32)))


class _Builder:
    def __init__(self, setting):
        F = R.frame()
        self.setting = setting
        self.keys, self.desc = F["keys"], F["desc"]
        self.n = len(self.keys)
        self.fv = frame_fv(setting)
        fn, fo, fi = self.fv
        self.node_of = np.full(self.n, -1, np.int64); self.pos_of = np.full(self.n, -1, np.int64); self.size_of = np.zeros(self.n, np.int64)
        for a in range(len(fn)):
            m = fi[fo[a]:fo[a + 1]].astype(np.int64)
            self.node_of[m] = int(fn[a]); self.pos_of[m] = np.arange(len(m)); self.size_of[m] = len(m)
        _, first, counts = np.unique(self.desc, axis=0, return_index=True, return_counts=True)
        unique = np.zeros(self.n, bool)
        unique[first[counts == 1]] = True
        k = self.keys
        self.pool = [int(f) for f in np.nonzero(unique & (self.node_of >= 0) & (k["x"] >= 70) & (k["x"] <= R.W - 70) & (k["y"] >= 70) & (k["y"] <= R.H - 70))[0]]
        self.tab = R._Table()
        self.kfs = [_KeyFrame() for _ in range(K)]
        self.claimed = [set() for _ in range(K)]          # the frame features a candidate's gadgets rely on
        self.expect = [dict() for _ in range(K)]          # frame feature -> point id or -1, nnratio 0.75 with the orientation check
        self.expect_ties = [dict() for _ in range(K)]     # the same at nnratio 1.25, for the features of the tie gadgets only
        self.expect_ties_lane = [dict() for _ in range(K)]   # ... and of the tie that lies in one lane
        self.gadgets = []                                 # (name, candidate, key-frame features, frame features)
        self.rng = np.random.default_rng(11)

    def members(self, f):
        fn, fo, fi = self.fv
        a = int(np.nonzero(fn == self.node_of[f])[0][0])
        return fi[fo[a]:fo[a + 1]].astype(np.int64)

    def others(self, q, f, *more):
        """Distances from descriptor q to every feature of f's node except f and `more`."""
        m = self.members(f)
        m = m[~np.isin(m, [f, *more])]
        return ham(q, self.desc[m]) if len(m) else np.zeros(0, np.int64)

    def key(self, f, bin_=0):
        return R._kf_key(f, bin_)

    def free(self, k, want=lambda f: True):
        return [f for f in self.pool if f not in self.claimed[k] and want(f)]

    def pairs(self, k, want):
        """(f, g, D): unclaimed pool features of one node, f before g in the node, with want(D)."""
        for f in self.free(k):
            m = self.members(f)
            m = m[(m > f) & np.isin(m, self.pool) & ~np.isin(m, list(self.claimed[k]))]
            if not len(m):
                continue
            d = ham(self.desc[f], self.desc[m])
            for g, D in zip(m.tolist(), d.tolist()):
                if want(D):
                    yield f, int(g), int(D)

    # ---- gadgets -----------------------------------------------------------------------------------------------------------------------
    def plain(self, k, f, bin_=0, point=None, tag="plain"):
        """An exact copy of frame feature f: distance 0, every other feature of the node at 1 or more (f's descriptor is unique)."""
        assert f not in self.claimed[k]
        p = self.tab.add(f) if point is None else point
        i = self.kfs[k].add(self.key(f, bin_), self.desc[f].copy(), self.node_of[f], p, tag)
        self.claimed[k].add(f)
        self.expect[k][f] = p
        return i, p

    def threshold(self, k, flips, accepted):
        """Best distance exactly `flips`; every other feature of the node so far that the ratio test passes (accepted) or above TH_LOW."""
        far = int(np.floor(flips / NNRATIO)) + 2 if accepted else TH_LOW + 1
        for f in self.free(k):
            for _ in range(8):
                q = flipped(self.desc[f], self.rng.choice(256, flips, replace=False))
                o = self.others(q, f)
                if not len(o) or o.min() >= far:
                    p = self.tab.add(f)
                    i = self.kfs[k].add(self.key(f), q, self.node_of[f], p, f"th{flips}")
                    self.claimed[k].add(f)
                    self.expect[k][f] = p if accepted else -1
                    self.gadgets.append((f"th{flips}", k, [i], [f]))
                    return
        raise AssertionError(f"no frame feature for a best distance of {flips}")

    def ratio(self, k, best, second, accepted):
        """bestDist1 = best at f, bestDist2 = second at g, every other feature of the node farther than `second`."""
        gap = second - best
        for f, g, D in self.pairs(k, lambda D: (D - gap) % 2 == 0 and gap <= D <= 2 * best + gap):
            a = (D - gap) // 2
            b = best - a
            if b < 0:
                continue
            q = flipped(self.desc[f], list(self.rng.choice(bits_of(self.desc[f], self.desc[g], True), a, replace=False)) +
                        list(self.rng.choice(bits_of(self.desc[f], self.desc[g], False), b, replace=False)))
            assert ham(q, self.desc[[f, g]]).tolist() == [best, second]
            o = self.others(q, f, g)
            if len(o) and o.min() <= second:
                continue
            p = self.tab.add(f)
            i = self.kfs[k].add(self.key(f), q, self.node_of[f], p, f"ratio{best}_{second}")
            self.claimed[k].update((f, g))
            self.expect[k][f] = p if accepted else -1
            self.expect[k][g] = -1
            self.gadgets.append((f"ratio{best}_{second}", k, [i], [f, g]))
            return
        raise AssertionError(f"no pair of frame features for {best} against {second}")

    def tie(self, k, same_lane=False):
        """f before g in one node, both at distance D / 2 of the key-frame feature, everything else farther.  same_lane: g a multiple of 16 positions
        behind f (up to TH_LOW away: such pairs are few), drawn from a generator of its own so that the other gadgets stay what they were."""
        rng = np.random.default_rng(12) if same_lane else self.rng
        for f, g, D in self.pairs(k, lambda D: D % 2 == 0 and 2 <= D <= (2 * TH_LOW if same_lane else 60)):
            if same_lane and (self.pos_of[g] - self.pos_of[f]) % 16:
                continue
            q = flipped(self.desc[f], rng.choice(bits_of(self.desc[f], self.desc[g], True), D // 2, replace=False))
            assert ham(q, self.desc[[f, g]]).tolist() == [D // 2, D // 2]
            o = self.others(q, f, g)
            if len(o) and o.min() <= D // 2:
                continue
            p = self.tab.add(f)
            i = self.kfs[k].add(self.key(f), q, self.node_of[f], p, "tie")
            self.claimed[k].update((f, g))
            self.expect[k][f] = self.expect[k][g] = -1                 # d < 0.75 d never holds
            ties = self.expect_ties_lane if same_lane else self.expect_ties
            ties[k][f] = p; ties[k][g] = -1                            # d < 1.25 d: the earlier position
            self.gadgets.append(("tie_same_lane" if same_lane else "tie", k, [i], [f, g]))
            return
        raise AssertionError("no pair of frame features for a tie")

    def contend(self, k, runner_up, want=lambda f: True):
        """Two key-frame features nearest to frame feature f: an exact copy, then a copy one bit off.  runner_up: the second takes g, the
        nearest feature left, which passes both tests; else everything left is above TH_LOW and it takes nothing."""
        if runner_up:
            for f, g, D in self.pairs(k, lambda D: D <= 24):
                for f1, g1 in ((f, g), (g, f)):
                    if not want(f1):
                        continue
                    q2 = flipped(self.desc[f1], self.rng.choice(bits_of(self.desc[f1], self.desc[g1], False), 1))
                    o = self.others(q2, f1, g1)
                    if len(o) and not np.float32(D + 1) < np.float32(NNRATIO) * np.float32(o.min()):
                        continue
                    p1, p2 = self.tab.add(f1), self.tab.add(g1)
                    i1 = self.kfs[k].add(self.key(f1), self.desc[f1].copy(), self.node_of[f1], p1, "contend_first")
                    i2 = self.kfs[k].add(self.key(g1), q2, self.node_of[f1], p2, "contend_runner_up")      # (g1's angle: rotation bin 0 where it lands)
                    self.claimed[k].update((f1, g1))
                    self.expect[k][f1] = p1; self.expect[k][g1] = p2
                    self.gadgets.append(("contend_runner_up", k, [i1, i2], [f1, g1]))
                    return
            raise AssertionError("no pair of frame features for a runner-up")
        for f in self.free(k, want):
            q2 = flipped(self.desc[f], self.rng.choice(256, 1))
            o = self.others(q2, f)
            if len(o) and o.min() <= TH_LOW:
                continue
            p1, p2 = self.tab.add(f), self.tab.add(f)
            i1 = self.kfs[k].add(self.key(f), self.desc[f].copy(), self.node_of[f], p1, "contend_first")
            i2 = self.kfs[k].add(self.key(f), q2, self.node_of[f], p2, "contend_nothing")
            self.claimed[k].add(f)
            self.expect[k][f] = p1
            self.gadgets.append(("contend_nothing", k, [i1, i2], [f]))
            return
        raise AssertionError("no frame feature whose neighbours are all above TH_LOW")

    def skipped(self, k, bad):
        """A copy of f whose row entry is NULL, or whose point is bad: not searched."""
        f = self.free(k)[0]
        p = self.tab.add(f, bad=True) if bad else -1
        i = self.kfs[k].add(self.key(f), self.desc[f].copy(), self.node_of[f], p, "bad_point" if bad else "null")
        self.claimed[k].add(f)
        self.expect[k][f] = -1
        self.gadgets.append(("bad_point" if bad else "null", k, [i], [f]))

    def absent(self, k, count):
        for f in self.free(k)[:count]:
            i = self.kfs[k].add(self.key(f), self.desc[f].copy(), ABSENT_NODE, self.tab.add(f), "absent_node")
            self.claimed[k].add(f)
            self.expect[k][f] = -1
            self.gadgets.append(("absent_node", k, [i], [f]))


@functools.lru_cache(maxsize=None)
def build(setting):
    """-> dict: setting, levelsup, fv (the frame's), kfs [K] (keys, desc, mp, fv, tag), bad_slot [K], points (the table's arrays), expect [K]
    (full rows, nnratio 0.75, orientation check on), counts [K], expect_ties [K] (partial, nnratio 1.25), gadgets, sizes (node sizes met)."""
    B = _Builder(setting)
    # 0 edges
    B.threshold(EDGES, TH_LOW, True)
    B.threshold(EDGES, TH_LOW + 1, False)
    B.ratio(EDGES, 30, 40, False)
    B.skipped(EDGES, bad=False)
    B.skipped(EDGES, bad=True)
    B.absent(EDGES, 3)
    shared = [(f, B.plain(EDGES, f)[1]) for f in B.free(EDGES)[:N_PLAIN]]
    # 1 order
    B.tie(ORDER)
    stretches = [lambda f: True] if setting != "root" else [lambda f, s=s: B.pos_of[f] // 512 == s for s in range(int(B.size_of.max() - 1) // 512 + 1)]
    for want in stretches:
        B.contend(ORDER, False, want)
        B.contend(ORDER, True, want)
    if setting != "root":                                            # and once beyond a lane's first position, where the node is large enough
        deep = [f for f in B.free(ORDER) if B.pos_of[f] >= 16]
        if deep:
            B.contend(ORDER, False, lambda f: B.pos_of[f] >= 16)
    for f in B.free(ORDER)[:N_PLAIN]:
        B.plain(ORDER, f)
    B.tie(ORDER, same_lane=True)
    have = sum(p >= 0 for p in B.expect[ORDER].values())              # every match so far votes for bin 0
    for k, bins in ((ORDER, ((0, CUT_BINS[0][1] - have),) + CUT_BINS[1:]), (ROTATION, ROT_BINS)):       # 2 rotation
        for bin_, cnt in bins:
            for f in B.free(k)[:cnt]:
                B.plain(k, f, bin_, tag=f"bin{bin_}")
                if bin_ == bins[-1][0]:
                    B.expect[k][f] = -1
    # 3 bad slot
    for f in B.free(BAD)[:N_PLAIN]:
        B.plain(BAD, f)
    # 4 shared
    B.ratio(SHARED, 29, 39, True)
    for f, p in shared:
        if f not in B.claimed[SHARED]:
            B.plain(SHARED, f, point=p, tag="shared")
    # 5 sizes: one plain match per distinct node size, smallest and largest first
    sizes = sorted({int(B.size_of[f]) for f in B.free(SIZES)})
    pick = sizes[:12] + sizes[-12:]
    for s in dict.fromkeys(pick):
        B.plain(SIZES, [f for f in B.free(SIZES) if B.size_of[f] == s][-1], tag=f"size{s}")
    for f in B.free(SIZES)[:N_PLAIN]:
        B.plain(SIZES, f)

    kfs = [kf.arrays() for kf in B.kfs]
    assert all(len(kf["mp"]) <= 400 for kf in kfs)
    pts = B.tab.arrays()
    expect = np.full((K, B.n), -1, np.int32)
    for k in range(K):
        for f, p in B.expect[k].items():
            expect[k, f] = p
    counts = [(int((expect[k] >= 0).sum()) if k != BAD else -1) for k in range(K)]
    expect[BAD] = -1
    S = dict(setting=setting, levelsup=SETTINGS[setting], fv=B.fv, kfs=kfs, bad_slot=[k == BAD for k in range(K)], points=pts, expect=expect, counts=counts,
             expect_ties=B.expect_ties, expect_ties_lane=B.expect_ties_lane, gadgets=B.gadgets, sizes=sorted({int(B.size_of[f]) for k in range(K) for f in B.claimed[k]}),
             n=B.n, pos_of=B.pos_of, size_of=B.size_of)
    _assert_conditions(S)
    return S


def trace_of(S, k, nnratio=NNRATIO, check_ori=True):
    F = R.frame()
    return simulate(S["kfs"][k], S["fv"], F["keys"], F["desc"], S["points"]["bad"], nnratio, check_ori)


def _assert_conditions(S):
    """Every condition of the module docstring, from the distances alone."""
    seen = set()
    traces = {k: trace_of(S, k) for k in range(K)}
    for name, k, kf_feats, f_feats in S["gadgets"]:
        seen.add(name)
        tr = traces[k][2]
        if name == f"th{TH_LOW}":
            best, second, f, ok = tr[kf_feats[0]]
            assert best == TH_LOW and ok and f == f_feats[0]
        elif name == f"th{TH_LOW + 1}":
            best, second, f, ok = tr[kf_feats[0]]
            assert best == TH_LOW + 1 and not ok and f == f_feats[0]
        elif name == "ratio30_40":
            best, second, f, ok = tr[kf_feats[0]]
            assert (best, second) == (30, 40) and np.float32(30) == np.float32(NNRATIO) * np.float32(40) and not ok
        elif name == "ratio29_39":
            best, second, f, ok = tr[kf_feats[0]]
            assert (best, second) == (29, 39) and ok and f == f_feats[0]
        elif name in ("tie", "tie_same_lane"):
            best, second, f, ok = tr[kf_feats[0]]
            assert best == second and best > 0 and not ok and f == f_feats[0] and f_feats[0] < f_feats[1]
            if name == "tie_same_lane":
                assert S["pos_of"][f_feats[1]] > S["pos_of"][f_feats[0]] and (S["pos_of"][f_feats[1]] - S["pos_of"][f_feats[0]]) % 16 == 0
            best, second, f, ok = trace_of(S, k, NNRATIO_TIES)[2][kf_feats[0]]
            assert best == second and ok and f == f_feats[0]
        elif name == "contend_runner_up":
            (b1, _, f1, ok1), (b2, _, f2, ok2) = tr[kf_feats[0]], tr[kf_feats[1]]
            assert b1 == 0 and ok1 and f1 == f_feats[0] and ok2 and f2 == f_feats[1] and b2 > 1
            assert ham(S["kfs"][k]["desc"][kf_feats[1]], R.frame()["desc"][[f_feats[0]]])[0] == 1, "the taken feature was the nearer one"
        elif name == "contend_nothing":
            (b1, _, f1, ok1), (b2, _, f2, ok2) = tr[kf_feats[0]], tr[kf_feats[1]]
            assert b1 == 0 and ok1 and f1 == f_feats[0] and not ok2 and b2 > TH_LOW
        elif name in ("null", "bad_point", "absent_node"):
            assert kf_feats[0] not in tr
    assert seen >= {f"th{TH_LOW}", f"th{TH_LOW + 1}", "ratio30_40", "ratio29_39", "tie", "tie_same_lane", "contend_runner_up", "contend_nothing", "null", "bad_point", "absent_node"}
    hist = traces[ROTATION][3]
    assert sorted(hist[hist > 0].tolist(), reverse=True) == [c for _, c in ROT_BINS] and all(hist[b] == c for b, c in ROT_BINS)
    assert ROT_BINS[-1][1] >= 0.1 * ROT_BINS[0][1], "the fourth bin is dropped for being the fourth, not for being small"
    hist = traces[ORDER][3]
    assert all(hist[b] == c for b, c in CUT_BINS) and hist.sum() == sum(c for _, c in CUT_BINS)
    assert not np.float32(CUT_BINS[1][1]) < np.float32(0.1) * np.float32(CUT_BINS[0][1]) and S["counts"][ORDER] == hist.sum() - CUT_BINS[-1][1]
    rows0 = set(S["kfs"][EDGES]["mp"][S["kfs"][EDGES]["mp"] >= 0].tolist()) & set(S["kfs"][SHARED]["mp"].tolist())
    assert len(rows0) >= 10, "candidates 0 and 4 share points"
    if S["setting"] == "root":
        assert S["sizes"] == [int(S["size_of"].max())] and S["sizes"][0] > 512
        where = {int(S["pos_of"][f_feats[0]]) // 512 for name, k, _, f_feats in S["gadgets"] if name.startswith("contend")}
        assert where == set(range((S["sizes"][0] - 1) // 512 + 1)), "a contended feature in every 512-position stretch of the node"
    else:
        assert min(S["sizes"]) < 16 < max(S["sizes"]), S["sizes"]
    for k in range(K):                                       # the hand-stated rows are what the restated walk gives
        if k != BAD:
            cnt, row, _, _ = traces[k]
            assert np.array_equal(row, S["expect"][k]) and cnt == S["counts"][k], (S["setting"], k)


def fill_store(cov, S, K4):
    """The scene's key-frames and points into a rumi_slam_amd.covis.Covisibility; -> the objects that must stay alive."""
    from rumi_slam_amd import matcher as M
    F = R.frame()
    pts = S["points"]
    npt = len(pts["bad"])
    cov.set_keyframes(SLOTS, [5000 + 7 * k for k in range(K)], [0] * K, [int(b) for b in S["bad_slot"]], [kf["mp"] for kf in S["kfs"]], [[]] * K, [-1] * K, [[]] * K)
    cov.set_points(list(range(npt)), pts["bad"], [[]] * npt)
    cov.set_point_attributes(list(range(npt)), pts["pos"], np.zeros((npt, 3), np.float32), pts["min_dist"], pts["max_dist"], pts["desc"])
    keep = []
    for k, kf in enumerate(S["kfs"]):
        fr = M.FrameView(kf["keys"], kf["desc"], R.W, R.H, F["sf"])
        fv = M.FeatureVector.from_csr(*kf["fv"])
        cov.set_keyframe_features(SLOTS[k], fr, fv, K4)
        keep += [fr, fv]
    return keep
