"""Scenes for rumi_common_regions_bow_resident (include/rumi_mapping.h): a ``common_regions_scene.Scene`` put into a covisibility store, the
groups as slots, and what the entry must answer.  The checkers stay those of common_regions_scene: the oracle's SearchByBoW(KF, KF) per pair and
the restatement of LoopClosing.cc:635-651 per group; the store's point ids are the scene's numbering, so matched_point compares as it is.

Slots: the current key-frame in slot 0, table entry k of the scene in slot k + 1.  Points: the scene's ids 0 .. nmp - 1 with its mp_bad; the
current key-frame's feature i owns id nmp + i, which no member holds."""
import numpy as np

from common_regions_scene import Build, fold, oracle_pair, seeded_scene
from match_cases import SF, csr, desc_at

CUR_SLOT = 0
K4 = [500.0, 500.0, 320.0, 240.0]


def slot_of(k):
    return int(k) + 1


def slot_groups(scene, groups=None):
    """The groups as slots; a table entry named in scene.alias (self_member_scene) is the current key-frame's own slot."""
    alias = getattr(scene, "alias", {})
    return [[alias.get(k, slot_of(k)) for k in g] for g in (scene.groups if groups is None else groups)]


def cur_row(scene):
    """The current key-frame's row and the bad bits of its points from cur_good: a good feature gets the fresh point nmp + i; a not-good
    feature alternates between NULL and a point whose bad bit is set.  Returns (row [n], ids of the row's points, their bad bits).
    (scene.cur_base, where a scene sets it, is the first of these ids instead of nmp: self_member_scene numbers them inside mp_bad.)"""
    nmp, n = getattr(scene, "cur_base", len(scene.mp_bad)), scene.cur.n
    row, ids, bad, odd = np.full(n, -1, np.int32), [], [], False
    for i in range(n):
        if scene.cur_good[i]:
            row[i] = nmp + i; ids.append(nmp + i); bad.append(0)
        else:
            if odd:
                row[i] = nmp + i; ids.append(nmp + i); bad.append(1)
            odd = not odd
    return row, np.array(ids, np.int32), np.array(bad, np.uint8)


def store_size(scene, spare_kf=0, spare_points=0):
    """(max_kf, max_points) a store needs for the scene."""
    return len(scene.kfs) + 1 + spare_kf, len(scene.mp_bad) + scene.cur.n + 1 + spare_points


def fill_store(cov, scene, kf_bad=()):
    """Puts the scene into ``cov``: the members' rows, the bad bits, the features and the FeatureVectors, and the current key-frame in CUR_SLOT.
    kf_bad: table entries whose key-frame bad bit is set.  Returns what went in, as host arrays: dict(rows = {slot: row}, pt_bad [all points],
    kf_bad = {slot: bit}, keep = the views the store's staged features point into)."""
    from rumi_slam_amd import matcher as M
    nmp = len(scene.mp_bad)
    row0, ids0, bad0 = cur_row(scene)
    slots = [CUR_SLOT] + [slot_of(k) for k in range(len(scene.kfs))]
    rows = [row0] + [K.mp for K in scene.kfs]
    bits = [0] + [1 if k in set(kf_bad) else 0 for k in range(len(scene.kfs))]
    n = len(slots)
    cov.set_keyframes(slots, [9000 + 3 * s for s in slots], [0] * n, bits, rows, [[]] * n, [-1] * n, [[]] * n)
    pt_bad = np.zeros(nmp + scene.cur.n, np.uint8)
    pt_bad[:nmp] = scene.mp_bad
    pt_bad[ids0] = bad0
    ids = np.unique(np.concatenate([np.arange(nmp, dtype=np.int32), ids0])).astype(np.int32)
    if len(ids):
        cov.set_points(ids, pt_bad[ids], [[]] * len(ids))
    keep = []
    for s, K in zip(slots, [scene.cur] + list(scene.kfs)):
        fr, fv = M.FrameView(K.keys, K.desc, 640, 480, SF), M.FeatureVector.from_csr(*K.fv)
        cov.set_keyframe_features(s, fr, fv, K4)
        keep.append((fr, fv))
    return dict(rows=dict(zip(slots, rows)), pt_bad=pt_bad, kf_bad=dict(zip(slots, bits)), keep=keep)


def new_store(scene, kf_bad=(), spare_kf=0, spare_points=0):
    from rumi_slam_amd.covis import Covisibility
    cov = Covisibility(*store_size(scene, spare_kf, spare_points))
    return cov, fill_store(cov, scene, kf_bad)


def run_resident(MP, h, cov, scene, groups=None, want_matches12=True):
    return MP.CommonRegionsBoWResident(h, cov, CUR_SLOT, slot_groups(scene, groups), scene.nnratio, scene.ori, want_matches12)


def expected_resident(O, scene, kf_bad=()):
    """The six arrays of the literal loop with the members of kf_bad left out as the entry leaves them out: row -1, count -1, no part in the
    union or in most_matches, the later members keep their j."""
    n, mem, bad = scene.cur.n, scene.members, set(kf_bad)
    matches12, nm = np.full((len(mem), n), -1, np.int32), np.zeros(len(mem), np.int32)
    cache = {}
    for i, k in enumerate(mem):
        if k in bad:
            nm[i] = -1
            continue
        if k not in cache:
            cache[k] = oracle_pair(O, scene, k)
        nm[i], matches12[i] = cache[k]
    return (matches12, nm) + fold(scene, matches12, nm)


# ---- constructed scenes -----------------------------------------------------------------------------------------------------------------
RES_NODE_SIZES = [0, 1, 15, 16, 17, 512, 513]
WHOLE_MEMBER = 1100


def contended_node_scene(size, name=None, lead_nodes=0):
    """One shared node; the member holds ``size`` features in it, list order against feature order.  In every 512-position stretch of the list
    two current features want the member feature at the stretch's LAST position (3 and 4 bits away): the first takes it, the second must find it
    taken and settles for the feature at the stretch's FIRST position (20 bits away) or, in a stretch of one, for nothing.  A lane that lost its
    `taken` bit past position 511 would hand the same feature out twice.  One member feature in ten holds no point, point 2 is bad.
    lead_nodes (at most 9): empty nodes with lower ids ahead of the shared one in the current key-frame's FeatureVector, so that the node pair falls
    to sixteen-lane group ``lead_nodes`` of its workgroup of sixteen."""
    s = Build(300 + size)
    rows = [[s.base(), (-1 if p % 10 == 7 else p)] for p in range(size)]
    for s0 in range(0, size, 512):
        last = min(s0 + 511, size - 1)
        b = s.base()
        rows[last] = [desc_at(b, 3, s.rng), last]
        if last != s0:
            rows[s0] = [desc_at(b, 20, s.rng), s0]
        s.cur(b, 9); s.cur(desc_at(b, 1, s.rng), 9)
    s.cur(s.base(), 11)                                              # a node the member lacks
    for p in reversed(range(size)):                                  # feature index size - 1 - p sits at list position p
        s.feat(0, rows[p][0], None, rows[p][1])
    sc = s.scene(name or f"contended_{size}", [[0]], max(size, 1), bad=[2] if size > 2 else [], nnratio=0.9, extra_nodes={-1: range(lead_nodes)})
    sc.kfs[0].fv = csr({9: [size - 1 - p for p in range(size)], 13: []})
    return sc


def union_scene():
    """Four current features in nodes of their own; three members whose nodes hold one feature each, so every pair matches (bestDist2 = 256).
         KF0: k0 -> P0, k1 -> P1                 KF1: k0 -> P0, k1 -> P2, k2 -> P1              KF2: k3 -> P0, k0 -> P3
       group 0 = [KF0, KF1]: P0 by both members at the same k (seen); P1 again at another k (seen); P2 first seen at k1, where P1 stands:
                             the later stands, the count keeps both -> points [0, 2, -1, -1], members [0, 1, -1, -1], 3; most = (1, 3).
       group 1 = [KF2, KF0]: KF0 serves two groups, P0 is in both -> points [3, 1, -1, 0], members [0, 1, -1, 0], 3; a tie 2 : 2 -> (0, 2)."""
    s = Build(77, 3)
    b = [s.base() for _ in range(4)]
    for k in range(4):
        s.cur(b[k], 3 + 2 * k)
    s.feat(0, desc_at(b[0], 3, s.rng), 3, 0); s.feat(0, desc_at(b[1], 3, s.rng), 5, 1)
    s.feat(1, desc_at(b[0], 4, s.rng), 3, 0); s.feat(1, desc_at(b[2], 4, s.rng), 7, 1); s.feat(1, desc_at(b[1], 4, s.rng), 5, 2)
    s.feat(2, desc_at(b[3], 5, s.rng), 9, 0); s.feat(2, desc_at(b[0], 5, s.rng), 3, 3)
    want = dict(matches12=[[0, 1, -1, -1], [0, 2, 1, -1], [1, -1, -1, 0], [0, 1, -1, -1]], nmatches=[2, 3, 2, 2],
                matched_point=[[0, 2, -1, -1], [3, 1, -1, 0]], matched_member=[[0, 1, -1, -1], [0, 1, -1, 0]], num=[3, 3], most=[[1, 3], [0, 2]])
    return s.scene("union", [[0, 1], [2, 0]], 4), want


def small_seeded(seed):
    """A seeded scene within the size limit: 3 groups x 4 members of 200 features; a key-frame serves groups 0 and 1."""
    s = seeded_scene(seed, n=200, n_groups=3, members=5, n_nodes=30)
    g = s.groups
    return s.sub([g[0][1:5], g[1][0:4], g[2][0:4]])


def self_member_scene(size=None):
    """The current key-frame as a member of its own groups: table entry `me` is the current key-frame once more (its row = cur_row, numbered
    inside mp_bad through cur_base) for the host-pointer entry and the oracle, and scene.alias sends it to CUR_SLOT for the by-slot entry.
    size None: the union scene's current key-frame, alone in one group and behind KF0 in another.  size given: a current key-frame of ``size``
    features in ONE node next to a 4-feature member, so that the `taken` words must be sized by the current key-frame, the largest member.
    Every not-good feature (no point, or a bad one) is an exact copy of its good neighbour: the neighbour matches itself at distance 0 only
    while the copy stays gated (else best = second = 0 and the ratio test refuses).  Most copies lie past list position 511, where a lane
    that owns one `taken` word has no bit for them."""
    from common_regions_scene import KF, Scene
    if size is None:
        base, _ = union_scene()
        cur, good, kfs, nmp, groups, small_bad = base.cur, base.cur_good, list(base.kfs), len(base.mp_bad), [[3], [0, 3]], base.mp_bad
    else:
        desc = contended_node_scene(size).kfs[0].desc.copy()
        good = np.ones(size, np.uint8)
        good[5::97] = 0
        desc[5::97] = desc[6::97][:len(desc[5::97])]                    # every not-good feature is an exact copy of its good neighbour
        cur = KF(np.zeros(size), desc, csr({9: list(range(size))[::-1]}))      # list order against feature order: feature f at position size - 1 - f
        nmp, small_bad = 8, np.zeros(8, np.uint8)
        kfs = [KF(np.zeros(4), desc[[0, 300, 700, size - 1]], csr({9: [0, 1, 2, 3]}), np.array([0, 1, 2, 3], np.int32))]
        groups = [[0, 1], [1]]
    probe = Scene("tmp", cur, good, [], small_bad, [], 0.9, False)
    row, ids, bits = cur_row(probe)                                  # ids nmp + i
    bad = np.concatenate([small_bad, np.zeros(cur.n, np.uint8)])
    bad[ids] = bits
    sc = Scene("self_alone" if size is None else f"self_{size}", cur, good, kfs + [KF(cur.keys["angle"], cur.desc, cur.fv, row)], bad, groups,
               0.9, False if size is not None else True)
    sc.cur_base, sc.alias = nmp, {len(kfs): CUR_SLOT}
    return sc
