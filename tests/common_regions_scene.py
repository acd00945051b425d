"""Scenes and checkers for rumi_common_regions_bow, the BoW stage of LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:576-651).

The checker of a (current key-frame, member) pair is the existing oracle, ``oracle_lib.search_by_bow_kf``.  The checker of a group's union is
``union``: LoopClosing.cc:635-651 restated in plain Python, j ascending, then k ascending, through a set of map points.  Nothing here needs a GPU.

A scene: one current key-frame, a table of distinct member key-frames whose features hold map points of ONE shared numbering, and groups (one per
candidate) of indices into the table, in vpCovKFi order."""
import numpy as np

from match_cases import KP_DTYPE, SF, csr, desc_at

CUR_POINT = "a map point that is not bad and that no member holds"


class KF:
    """keys (angle is read), desc [n, 32], fv = (node_ids, offsets, indices), mp [n] (-1 NULL; None for the current key-frame)."""

    def __init__(self, angles, desc, nodes, mp=None):
        n = len(angles)
        self.keys = np.zeros(n, KP_DTYPE)
        self.keys["x"], self.keys["y"] = 10 + 10 * (np.arange(n) % 60), 10 + 10 * (np.arange(n) // 60)
        self.keys["size"], self.keys["response"], self.keys["class_id"], self.keys["angle"] = 31, 1, -1, np.asarray(angles, np.float32)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(n, 32)
        self.fv = nodes if isinstance(nodes, tuple) else csr(nodes)
        self.mp = None if mp is None else np.asarray(mp, np.int32)

    @property
    def n(self):
        return len(self.keys)


class Scene:
    def __init__(self, name, cur, cur_good, kfs, mp_bad, groups, nnratio=0.9, ori=True):
        self.name, self.cur, self.kfs, self.groups, self.nnratio, self.ori = name, cur, list(kfs), [list(g) for g in groups], float(nnratio), bool(ori)
        self.cur_good, self.mp_bad = np.asarray(cur_good, np.uint8), np.asarray(mp_bad, np.uint8)
        assert len(self.cur_good) == cur.n and all(k.mp is not None and len(k.mp) == k.n for k in self.kfs)
        assert all(int(k.mp.max(initial=-1)) < len(self.mp_bad) for k in self.kfs)

    @property
    def members(self):
        return [k for g in self.groups for k in g]

    def sub(self, groups):
        """The same table with other groups."""
        return Scene(self.name, self.cur, self.cur_good, self.kfs, self.mp_bad, groups, self.nnratio, self.ori)


# ---- the union, restated ----------------------------------------------------------------------------------------------------------------
def union(n, member_points):
    """member_points[j][k]: the map point member j's search left at slot k of the current key-frame (-1 NULL), i.e. vvpMatchedMPs[j][k].
    Returns (vpMatchedPoints [n], vpKeyFrameMatchedMP [n] as j, numBoWMatches)."""
    point, member, seen, count = [-1] * n, [-1] * n, set(), 0
    for j, pts in enumerate(member_points):
        for k in range(len(pts)):
            p = int(pts[k])
            if p < 0:
                continue
            if p not in seen:
                seen.add(p)
                count += 1
                point[k] = p
                member[k] = j
    return np.array(point, np.int32), np.array(member, np.int32), count


def most_matches(nums):
    """(nIndexMostBoWMatchesKF, nMostBoWNumMatches): strictly greater, starting from (0, 0) (LoopClosing.cc:615-632)."""
    at, most = 0, 0
    for j, num in enumerate(nums):
        if num > most:
            most, at = int(num), j
    return at, most


def fold(scene, matches12, nmatches):
    """The four per-group results from the per-member ones."""
    n, G = scene.cur.n, len(scene.groups)
    point, member = np.full((G, n), -1, np.int32), np.full((G, n), -1, np.int32)
    num, most = np.zeros(G, np.int32), np.zeros((G, 2), np.int32)
    m = 0
    for g, grp in enumerate(scene.groups):
        pts = []
        for k in grp:
            f = matches12[m + len(pts)]
            pts.append(np.where(f >= 0, scene.kfs[k].mp[np.maximum(f, 0)] if scene.kfs[k].n else -1, -1))
        point[g], member[g], num[g] = union(n, pts)
        most[g] = most_matches(nmatches[m:m + len(grp)])
        m += len(grp)
    return point, member, num, most


# ---- the pair checker -------------------------------------------------------------------------------------------------------------------
def cur_ids(scene):
    """The current key-frame's map points as the single-pair entries want them: CUR_POINT (id nmp) where cur_good, else NULL; and mp_bad with that id."""
    nmp = len(scene.mp_bad)
    return np.where(scene.cur_good != 0, nmp, -1).astype(np.int32), np.concatenate([scene.mp_bad, [0]]).astype(np.uint8)


def oracle_pair(O, scene, k):
    c, K = scene.cur, scene.kfs[k]
    mp1, bad = cur_ids(scene)
    return O.search_by_bow_kf(c.keys, c.desc, mp1, c.fv, K.keys, K.desc, K.mp, K.fv, bad, scene.nnratio, scene.ori)


def expected(O, scene):
    """The six arrays as the literal loop gives them: every member through the oracle, every group through ``union``."""
    n, mem = scene.cur.n, scene.members
    matches12, nm = np.full((len(mem), n), -1, np.int32), np.zeros(len(mem), np.int32)
    cache = {}
    for i, k in enumerate(mem):
        if k not in cache:
            cache[k] = oracle_pair(O, scene, k)
        nm[i], matches12[i] = cache[k]
    return (matches12, nm) + fold(scene, matches12, nm)


# ---- through the library ----------------------------------------------------------------------------------------------------------------
def views(M, scene):
    cur = M.FrameView(scene.cur.keys, scene.cur.desc, 640, 480, SF)
    kfs = [(M.FrameView(K.keys, K.desc, 640, 480, SF), M.FeatureVector.from_csr(*K.fv), K.mp) for K in scene.kfs]
    return cur, M.FeatureVector.from_csr(*scene.cur.fv), kfs


def run_gpu(M, h, scene):
    cur, fv, kfs = views(M, scene)
    return M.CommonRegionsBoW(h, cur, fv, scene.cur_good, kfs, scene.mp_bad, scene.groups, scene.nnratio, scene.ori)


def gpu_pair(M, h, scene, k, v=None):
    """rumi_search_by_bow_kf on (current key-frame, table entry k); v: views(M, scene), when the caller keeps them."""
    cur, fv, kfs = v or views(M, scene)
    mp1, bad = cur_ids(scene)
    h.mfNNratio, h.mbCheckOrientation = scene.nnratio, scene.ori
    return M.SearchByBoW_KF(h, cur, fv, mp1, kfs[k][0], kfs[k][1], scene.kfs[k].mp, bad)


def same(got, want):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, want)) and len(got) == len(want)


def describe(got, want):
    names = ["matches12", "nmatches", "matched_point", "matched_member", "num_bow_matches", "most_matches"]
    return "; ".join(f"{nm}: {np.count_nonzero(np.asarray(a) != np.asarray(b))} differ" for nm, a, b in zip(names, got, want) if not np.array_equal(a, b))


# ---- constructed scenes -----------------------------------------------------------------------------------------------------------------
def from_case(c):
    """A BOW_KF case of match_cases as one group of one member; member feature i holds map point i."""
    i = c.inp
    cur, K = KF(i["k1"]["angle"], i["d1"], i["fv1"]), KF(i["k2"]["angle"], i["d2"], i["fv2"], np.arange(len(i["k2"]), dtype=np.int32))
    return Scene(c.id, cur, np.ones(cur.n, np.uint8), [K], np.zeros(K.n, np.uint8), [[0]], c.nnratio, c.ori)


class Build:
    """Features added one by one: cur(desc, node, angle, good) and, per member key-frame, feat(kf, desc, node, mp, angle)."""

    def __init__(self, seed, n_kfs=1):
        self.rng = np.random.default_rng(seed)
        self.c, self.k = [], [[] for _ in range(n_kfs)]

    def base(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def cur(self, desc, node, angle=0.0, good=1):
        self.c.append((desc, node, angle, good)); return len(self.c) - 1

    def feat(self, kf, desc, node, mp, angle=0.0):
        self.k[kf].append((desc, node, angle, mp)); return len(self.k[kf]) - 1

    @staticmethod
    def _kf(rows, mp):
        nodes = {}
        for i, r in enumerate(rows):
            if r[1] is not None:
                nodes.setdefault(r[1], []).append(i)
        desc = np.array([r[0] for r in rows], np.uint8).reshape(-1, 32)
        return KF([r[2] for r in rows], desc, nodes, [r[3] for r in rows] if mp else None)

    def scene(self, name, groups, nmp, bad=(), nnratio=0.9, ori=False, extra_nodes=None):
        cur = self._kf(self.c, False)
        kfs = [self._kf(r, True) for r in self.k]
        for kf, nodes in (extra_nodes or {}).items():              # nodes with an empty list (kf = -1: the current key-frame)
            t = cur if kf < 0 else kfs[kf]
            m = {int(nd): list(t.fv[2][t.fv[1][a]:t.fv[1][a + 1]]) for a, nd in enumerate(t.fv[0])}
            m.update({nd: [] for nd in nodes})
            t.fv = csr(m)
        mp_bad = np.zeros(nmp, np.uint8)
        mp_bad[list(bad)] = 1
        return Scene(name, cur, [r[3] for r in self.c], kfs, mp_bad, groups, nnratio, ori)


def case_gates():
    """A member feature without a map point (2 bits away) and one with a bad point (3 bits) would have been best and second best; the good ones
    are 20 and 40 bits away: 20 < 0.75 * 40 matches feature 2 (ORBmatcher.cc:738-742).  Counting the gated ones as second best (3) would reject."""
    s = Build(1)
    b = s.base()
    s.cur(b, 5)
    s.feat(0, desc_at(b, 2, s.rng), 5, -1); s.feat(0, desc_at(b, 3, s.rng), 5, 0); s.feat(0, desc_at(b, 20, s.rng), 5, 1); s.feat(0, desc_at(b, 40, s.rng), 5, 2)
    return s.scene("gates", [[0]], 3, bad=[0], nnratio=0.75), dict(matches12=[[2]], nmatches=[1], matched_point=[[1]], matched_member=[[0]], num=[1], most=[[0, 1]])


def case_cur_good():
    """Current feature 0 (cur_good = 0) sits on a perfect member feature and is skipped without taking it (:717-721); current feature 1, later in
    the node's list, gets that feature."""
    s = Build(2)
    b = s.base()
    s.cur(b, 5, good=0); s.cur(desc_at(b, 4, s.rng), 5)
    s.feat(0, b, 5, 7); s.feat(0, desc_at(b, 45, s.rng), 5, 3)
    return s.scene("cur_good", [[0]], 8), dict(matches12=[[-1, 0]], nmatches=[1], matched_point=[[-1, 7]], matched_member=[[-1, 0]], num=[1], most=[[0, 1]])


def case_one_sided_nodes():
    """Nodes 1 and 5 exist only in the current key-frame, 4 and 6 only in the member; only node 3 pairs up.  A perfect twin waits in node 4 / 5."""
    s = Build(3)
    a, b, c = s.base(), s.base(), s.base()
    s.cur(a, 1); s.cur(b, 3); s.cur(c, 5)
    s.feat(0, b, 3, 0); s.feat(0, a, 4, 1); s.feat(0, c, 6, 2)
    return s.scene("one_sided_nodes", [[0]], 3), dict(matches12=[[-1, 0, -1]], nmatches=[1], matched_point=[[-1, 0, -1]], matched_member=[[-1, 0, -1]], num=[1],
                                                      most=[[0, 1]])


def case_bin30():
    """rot = 900 - 0 gives round(900 * (1 / 30)) = 30, which is bin 0 (ORBmatcher.cc:767).  Bins: 3 x 5, 5 x 3, 7 x 3 and bin 0 = 2 (rot 0) + 2 (rot 900):
    the maxima are bins 3, 0, 5 (bin 5 is met before bin 7), so the three of bin 7 go.  Were rot 900 not folded into bin 0, bin 0 would go instead."""
    s = Build(4)
    rows = [(90.0, 0.0)] * 5 + [(150.0, 0.0)] * 3 + [(210.0, 0.0)] * 3 + [(33.0, 33.0)] * 2 + [(900.0, 0.0)] * 2
    for k, (a1, a2) in enumerate(rows):
        b = s.base()
        s.cur(b, 3 + 2 * k, angle=a1); s.feat(0, desc_at(b, 3, s.rng), 3 + 2 * k, k, angle=a2)
    keep = [k if not (8 <= k < 11) else -1 for k in range(15)]
    return s.scene("bin30", [[0]], 15, ori=True), dict(matches12=[keep], nmatches=[12], matched_point=[keep], matched_member=[[0 if k >= 0 else -1 for k in keep]],
                                                      num=[12], most=[[0, 12]])


def case_histogram_then_union():
    """Member 0: eleven matches in bin 2, one in bin 5 (slot 11) and one in bin 8 (slot 12): 1 < 0.1f * 11 drops both (:1820).  The point slot 11
    matched, P = 11, is also held by member 1, which matches it at slot 13.  The union must not see the removed match: P is first seen at
    (j = 1, k = 13).  Member 1 also matches slot 0 to point 0 again: already seen, nothing written."""
    s = Build(5, 2)
    rows = [(60.0, 0.0)] * 11 + [(155.0, 5.0), (250.0, 10.0)]
    bases = []
    for k, (a1, a2) in enumerate(rows):
        b = s.base(); bases.append(b)
        s.cur(b, 3 + 2 * k, angle=a1); s.feat(0, desc_at(b, 3, s.rng), 3 + 2 * k, k, angle=a2)
    b13 = s.base()
    s.cur(b13, 41)
    s.feat(1, desc_at(b13, 2, s.rng), 41, 11); s.feat(1, desc_at(bases[0], 5, s.rng), 3, 0, angle=60.0)
    m0 = list(range(11)) + [-1, -1, -1]
    m1 = [1] + [-1] * 12 + [0]
    pt = list(range(11)) + [-1, -1, 11]
    mem = [0] * 11 + [-1, -1, 1]
    return s.scene("histogram_then_union", [[0, 1]], 13, ori=True), dict(matches12=[m0, m1], nmatches=[11, 2], matched_point=[pt], matched_member=[mem], num=[12],
                                                                        most=[[0, 11]])


def hand_cases():
    return [case_gates(), case_cur_good(), case_one_sided_nodes(), case_bin30(), case_histogram_then_union()]


def expect_tuple(e):
    return (np.array(e["matches12"], np.int32), np.array(e["nmatches"], np.int32), np.array(e["matched_point"], np.int32), np.array(e["matched_member"], np.int32),
            np.array(e["num"], np.int32), np.array(e["most"], np.int32).reshape(-1, 2))


NODE_SIZES = [0, 1, 15, 16, 17, 33, 512, 513, 1024, 1025, 1100]      # above 512 a lane's `taken` flags lie in LDS words: 1024 is the last size of two, 1025 the first of three
CONTENDED_NODE = 1100


def contended_scene():
    """The 1100-feature node with two current features contending for one member feature in every 512-position stretch of the node (the helper
    of the by-slot suite, whose module imports this one: hence the import here).  Nine empty nodes lead the current key-frame's FeatureVector:
    the node pair is searched by the tenth sixteen-lane group of its workgroup, whose third LDS word lies 2624 bytes into the block -- past what a
    launch with one word too few would get (2048 bytes, which the hardware rounds up to 2560)."""
    from common_regions_resident_scene import contended_node_scene
    return contended_node_scene(CONTENDED_NODE, lead_nodes=9)


def node_size_scene(size):
    """One shared node; the member holds ``size`` features in it.  Three current features: the twin of the LAST list entry, the twin of the first, and
    one that ties between two entries.  One member feature in ten (list positions 7, 17, ...) has no map point, the third is bad; feature indices run against list order."""
    s = Build(100 + size)
    b = [s.base() for _ in range(3)]
    for d in b:
        s.cur(d, 9)
    s.cur(s.base(), 11)
    rows = []
    for p in range(size):                                            # list position p
        d = s.base()
        if p == size - 1: d = desc_at(b[0], 6, s.rng)
        elif p == 0: d = desc_at(b[1], 9, s.rng)
        elif p in (5, 12): d = desc_at(b[2], 12, s.rng)
        elif p == 7: d = desc_at(b[2], 1, s.rng)                    # the best for b[2], but NULL (p % 10 == 7)
        rows.append((d, -1 if p % 10 == 7 else p))
    for p in reversed(range(size)):                                  # feature index size - 1 - p sits at list position p
        s.feat(0, rows[p][0], None, rows[p][1])
    sc = s.scene(f"node_{size}", [[0]], max(size, 1), bad=[2] if size > 2 else [], nnratio=2.0)
    K = sc.kfs[0]
    K.fv = csr({9: [size - 1 - p for p in range(size)], 13: []})
    return sc


def cur_size_scene(n):
    """A current key-frame of n features over four nodes against two members of 40 features."""
    rng = np.random.default_rng(200 + n)
    base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    cur = KF(np.zeros(n), base, {3 + 2 * (i % 4): [j for j in range(n) if j % 4 == i % 4] for i in range(min(n, 4))})
    kfs = []
    for k in range(2):
        pick = rng.permutation(n)[:min(n, 40)]
        desc = np.array([desc_at(base[i], int(rng.integers(0, 10)), rng) for i in pick], np.uint8).reshape(-1, 32)
        nodes = {}
        for j, i in enumerate(pick):
            nodes.setdefault(3 + 2 * (int(i) % 4), []).append(j)
        kfs.append(KF(np.zeros(len(pick)), desc, nodes, pick.astype(np.int32)))
    return Scene(f"cur_{n}", cur, np.ones(n, np.uint8), kfs, np.zeros(n, np.uint8), [[0, 1]], 0.9, False)


def empty_member_scene():
    """A member with n = 0 (no features, no nodes) between two ordinary ones."""
    sc = cur_size_scene(65)
    sc.kfs.insert(1, KF(np.zeros(0), np.zeros((0, 32), np.uint8), {}, np.zeros(0, np.int32)))
    return sc.sub([[0, 1, 2]])


# ---- seeded scenes ----------------------------------------------------------------------------------------------------------------------
SEEDS = [11, 12]


def seeded_scene(seed, n=300, n_groups=3, members=11, n_nodes=40):
    """n_groups candidates with ``members`` members each of n features, drawn from a pool of map points.  The current key-frame sees points 0..n-1; the
    members of group 0 share about half of their points with it, those of group 1 a seventh, those of the last group next to none (fewer than 20
    BoW matches).  Three points in ten have a look-alike in the pool, so that members fill one slot with different points.  Two covisibles of the second candidate are covisibles of the first as well."""
    rng = np.random.default_rng(seed)
    P = 6 * n
    base = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    node_of = rng.integers(0, n_nodes, P) * 3 + 1
    angle_of = rng.uniform(0, 360, P).astype(np.float32)
    for q in np.nonzero(rng.random(n) < 0.3)[0]:                     # point n + q looks like point q: a member that holds it fills slot q with ANOTHER point
        base[n + q], node_of[n + q], angle_of[n + q] = desc_at(base[q], 10, rng), node_of[q], angle_of[q]

    def observe(points, turn):
        desc = np.array([desc_at(base[p], int(rng.integers(0, 14)), rng) for p in points], np.uint8).reshape(-1, 32)
        ang = np.mod(angle_of[points] + turn + rng.normal(0, 6, len(points)), 360).astype(np.float32)
        ang[rng.random(len(points)) < 0.08] = rng.uniform(0, 360)
        nd = np.where(rng.random(len(points)) < 0.1, rng.integers(0, n_nodes, len(points)) * 3 + 1, node_of[points])
        nodes = {}
        for i in rng.permutation(len(points)):                       # list order is not index order
            nodes.setdefault(int(nd[i]), []).append(int(i))
        return ang, desc, nodes

    cur = KF(*observe(np.arange(n), 0.0))
    shared = [n // 2, n // 7, 1] + [n // 10] * max(0, n_groups - 3)
    kfs, groups = [], []
    for g in range(n_groups):
        grp = []
        for j in range(members):
            if g == 1 and j in (3, 7):                               # a covisible of the first candidate as well
                grp.append(groups[g - 1][j + 1]); continue
            lo = 2 * n if g == 2 else n                              # the last group draws no look-alikes either
            pts = np.concatenate([rng.choice(n, shared[g], replace=False), lo + rng.choice(P - lo, n - shared[g], replace=False)])
            rng.shuffle(pts)
            ang, desc, nodes = observe(pts, 40.0 * (g + 1))
            mp = np.where(rng.random(n) < 0.1, -1, pts).astype(np.int32)
            kfs.append(KF(ang, desc, nodes, mp)); grp.append(len(kfs) - 1)
        groups.append(grp)
    mp_bad = (rng.random(P) < 0.05).astype(np.uint8)
    return Scene(f"seed{seed}", cur, (rng.random(n) < 0.85).astype(np.uint8), kfs, mp_bad, groups, 0.9, True)


def mixed_groups(scene):
    """Groups of 1, 2 and 11 members over a seeded scene's table, table entry 0 a member of two groups."""
    return scene.sub([[0], [5, 0], list(range(11, 22))])
