"""Small constructed maps for rumi_search_in_neighbors_resident (include/rumi_mapping.h) and a host model of LocalMapping::SearchInNeighbors
(R/lib_src/LocalMapping.cc:649-743) on them.  TEST INFRASTRUCTURE, on top of the covisibility store as tests/resident_scene.py fills it.

A map is a list of key-frames (features, pose, map-point row) and a table of points (attributes, bad flag); observations follow from the rows.
``FuseModel`` replays ORBmatcher::Fuse's mutations (MapPoint::AddObservation, KeyFrame::AddMapPoint, MapPoint::Replace with the
ComputeDistinctiveDescriptors it ends with, MapPoint.cc:272-326) on plain Python containers, with the search of every (key-frame, point) pair
answered by the CPU oracle (oracle_lib.fuse_candidates).  Two drivers:

  reference(map)       the member as written: one oracle call per target on the map as it stands when the target's turn comes, then the reverse
                       pass.  The expectation.
  resident(map, ...)   what a caller of the one-call entry does: every pair answered from the map at the call, then the same replay; a point
                       whose descriptor a Replace changed is searched again (by the oracle here, by the single-target entry in the facade).

Slot numbers are not list positions and the key-frames enter the store in another order than the call lists them."""
import copy

import numpy as np

import oracle_lib as O
from rumi_slam_amd.capi import KP_DTYPE

W, H = 640, 480
K4 = np.float32([500.0, 500.0, 320.0, 240.0])
NLEVELS = 8
SF = (np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)).astype(np.float32)
LOG_SF = float(np.log(np.float32(1.2)))
BOUNDS = np.float32([0.0, 0.0, W, H])
TH = 3.0
TH_LOW = 50


def slot_of(k):
    """Slot of key-frame k of a map (0 = the current key-frame)."""
    return 7 + 5 * k


def keypoints(xy, octave, angle=None):
    k = np.zeros(len(xy), KP_DTYPE)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k["x"], k["y"], k["octave"] = xy[:, 0], xy[:, 1], np.asarray(octave, np.int32)
    k["size"], k["angle"], k["class_id"] = 31.0, (0.0 if angle is None else angle), -1
    return k


def pose_t(t):
    """Identity rotation, translation t: (Tcw7, Ow)."""
    t = np.asarray(t, np.float32)
    return np.float32([0, 0, 0, 1, t[0], t[1], t[2]]), (-t).astype(np.float32)


def pose_ry(angle, t):
    """Rotation about y by `angle`, translation t: (Tcw7, Ow = -R^T t)."""
    t = np.asarray(t, np.float32)
    q = np.float32([0.0, np.sin(angle / 2), 0.0, np.cos(angle / 2)])
    c, s = np.cos(angle), np.sin(angle)
    R = np.float64([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.concatenate([q, t]).astype(np.float32), (-(R.T @ t.astype(np.float64))).astype(np.float32)


def flip_bits(desc, bits, rng=None):
    """A copy of the 32-byte row with the `bits` lowest-numbered (or rng-chosen) bits inverted: Hamming distance exactly `bits`."""
    d = np.unpackbits(np.asarray(desc, np.uint8))
    idx = np.arange(bits) if rng is None else rng.choice(256, bits, replace=False)
    d[idx] ^= 1
    return np.packbits(d)


class KeyFrame:
    def __init__(self, keys, desc, Tcw7, Ow, row):
        self.keys = np.ascontiguousarray(keys, KP_DTYPE)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.Tcw7, self.Ow = np.float32(Tcw7), np.float32(Ow)
        self.row = [int(p) for p in row]
        assert len(self.keys) == len(self.desc) == len(self.row)

    @property
    def n(self):
        return len(self.keys)


class SinMap:
    """kfs[0] is the current key-frame, kfs[1 .. n_targets] the targets in call order, the rest observe points but take no part in the call.
    pos / normal [P, 3], min_dist / max_dist [P], desc [P, 32], bad [P]; has_attr [P] (False: the store never gets the point's attributes)."""

    def __init__(self, kfs, n_targets, pos, normal, min_dist, max_dist, desc, bad=None, has_attr=None):
        self.kfs, self.n_targets = list(kfs), int(n_targets)
        self.pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        P = len(self.pos)
        self.normal = np.ascontiguousarray(normal, np.float32).reshape(P, 3)
        self.min_dist = np.ascontiguousarray(min_dist, np.float32).reshape(P)
        self.max_dist = np.ascontiguousarray(max_dist, np.float32).reshape(P)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(P, 32)
        self.bad = np.zeros(P, bool) if bad is None else np.asarray(bad, bool).copy()
        self.has_attr = np.ones(P, bool) if has_attr is None else np.asarray(has_attr, bool).copy()

    @property
    def n_points(self):
        return len(self.pos)

    def observations(self):
        """obs[p] = {key-frame index: feature} from the rows (a bad point keeps none)."""
        obs = [dict() for _ in range(self.n_points)]
        for k, kf in enumerate(self.kfs):
            for f, p in enumerate(kf.row):
                if p >= 0 and not self.bad[p]:
                    assert k not in obs[p], "a point twice in one row"
                    obs[p][k] = f
        return obs


# ---- the oracle's answer for a list of points against one key-frame ----
def search(m, k, ids, skip, desc=None):
    """best feature of key-frame k per entry of ids (-1: none, skipped, or id < 0).  desc: the live descriptors [P, 32] (default: m.desc)."""
    ids = np.asarray(ids, np.int64)
    skip = np.asarray(skip, bool) | (ids < 0)
    if len(ids) == 0:
        return np.zeros(0, np.int32)
    safe = np.where(ids < 0, 0, ids)
    kf = m.kfs[k]
    pts = dict(skip=skip.astype(np.uint8), pos=m.pos[safe], normal=m.normal[safe], min_dist=m.min_dist[safe], max_dist=m.max_dist[safe],
               desc=(m.desc if desc is None else desc)[safe])
    out = O.fuse_candidates(kf.keys, kf.desc, W, H, SF, LOG_SF, kf.Tcw7, kf.Ow, K4, pts, TH, True)
    out[skip] = -1
    return out


def expected_call(m):
    """What the one-call entry must return for the map as it stands: (fwd_best [n_targets, n_cur], rev_point, rev_best)."""
    obs = m.observations()
    cur = m.kfs[0]
    ids = np.asarray(cur.row, np.int64)
    fwd = np.full((m.n_targets, cur.n), -1, np.int32)
    for t in range(m.n_targets):
        skip = np.array([p < 0 or m.bad[p] or (1 + t) in obs[p] for p in cur.row], bool)
        fwd[t] = search(m, 1 + t, ids, skip)
    rev, seen = [], set()
    for t in range(m.n_targets):
        for p in m.kfs[1 + t].row:
            if p >= 0 and not m.bad[p] and 0 not in obs[p] and p not in seen:
                seen.add(p)
                rev.append(p)
    rev = np.asarray(rev, np.int32)
    return fwd, rev, search(m, 0, rev, np.zeros(len(rev), bool))


# ---- the replay ----
class FuseModel:
    """The live map of one run: rows, observations, bad flags, mpReplaced, descriptors, and counters of the branches taken."""

    def __init__(self, m):
        self.m = m
        self.rows = [list(kf.row) for kf in m.kfs]
        self.obs = m.observations()
        self.obs0 = m.observations()   # as at the call
        self.bad = m.bad.copy()
        self.replaced = {}
        self.desc = m.desc.copy()
        self.n = dict(add=0, replace_pmp=0, replace_inkf=0, skip_bad=0, skip_inkf=0, rev_skip_incur=0, skip_inkf_new=0, rev_skip_entered=0, rev_dup=0, dirty=0, inkf_bad=0)
        self.dirty = set()             # points whose descriptor a Replace changed

    def add_observation(self, p, k, f):
        if k not in self.obs[p]:
            self.obs[p][k] = f

    def distinctive(self, p):          # MapPoint::ComputeDistinctiveDescriptors, MapPoint.cc:353-427 (no key-frame is bad here)
        o = sorted(self.obs[p].items())
        if not o:
            return
        D = np.stack([self.m.kfs[k].desc[f] for k, f in o])
        bits = np.unpackbits(D, axis=1).astype(np.int32)
        dist = (bits[:, None, :] != bits[None, :, :]).sum(2)
        med = np.sort(dist, axis=1)[:, int(0.5 * (len(o) - 1))]
        new = D[int(np.argmin(med))]
        if not np.array_equal(new, self.desc[p]):
            self.desc[p] = new
            self.dirty.add(p)
            self.n["dirty"] += 1

    def replace(self, p, q):           # p->Replace(q), MapPoint.cc:272-326
        if p == q:
            return
        o, self.obs[p] = self.obs[p], {}
        self.bad[p] = True
        self.replaced[p] = q
        for k, f in sorted(o.items()):
            if k not in self.obs[q]:
                self.rows[k][f] = q
                self.add_observation(q, k, f)
            else:
                self.rows[k][f] = -1
        self.distinctive(q)

    def fuse(self, k, ids, best, forward):
        """The loop of ORBmatcher::Fuse (ORBmatcher.cc:1037-1174) over ids with the search's answers in best."""
        nfused = 0
        for p, b in zip(ids, best):
            if p < 0:
                continue
            if self.bad[p]:
                self.n["skip_bad"] += forward
                continue
            if k in self.obs[p]:
                self.n["skip_inkf" if forward else "rev_skip_incur"] += 1
                if forward and k not in self.obs0[p]:                       # an earlier Replace moved the point into this target
                    self.n["skip_inkf_new"] += 1
                if not forward and not any(1 <= t <= self.m.n_targets for t in self.obs0[p]):      # it entered a target row in the forward pass
                    self.n["rev_skip_entered"] += 1
                continue
            if b < 0:
                continue
            q = self.rows[k][b]
            if q >= 0:
                if not self.bad[q]:
                    if len(self.obs[q]) > len(self.obs[p]):
                        self.replace(p, q)
                        self.n["replace_pmp"] += 1
                    else:
                        self.replace(q, p)
                        self.n["replace_inkf"] += 1
                else:
                    self.n["inkf_bad"] += 1
            else:
                self.add_observation(p, k, b)
                self.rows[k][b] = p
                self.n["add"] += 1
            nfused += 1
        return nfused

    def gate(self, k, ids):
        return np.array([p < 0 or bool(self.bad[p]) or k in self.obs[p] for p in ids], bool)

    def reverse_candidates(self):      # LocalMapping.cc:706-727 on the map as the forward pass left it
        out, seen = [], set()
        for t in range(self.m.n_targets):
            for p in self.rows[1 + t]:
                if p < 0 or self.bad[p]:
                    continue
                if p in seen:
                    self.n["rev_dup"] += 1
                    continue
                seen.add(p)
                out.append(p)
        return out

    def state(self):
        return (self.rows, [sorted(o.items()) for o in self.obs], self.bad.tolist(), sorted(self.replaced.items()), self.desc.tobytes())


def reference(m):
    """SearchInNeighbors as written.  Returns (model, nFused forward, nFused reverse, searched): searched = the reverse candidates whose search ran."""
    s = FuseModel(m)
    ids = list(m.kfs[0].row)           # vpMapPointMatches, copied once (:695)
    nf = 0
    for t in range(m.n_targets):
        best = search(m, 1 + t, ids, s.gate(1 + t, ids), s.desc)
        nf += s.fuse(1 + t, ids, best, 1)
    cand = s.reverse_candidates()
    g = s.gate(0, cand)
    best = search(m, 0, cand, g, s.desc)
    searched = [p for p, skip in zip(cand, g) if not skip]
    return s, nf, s.fuse(0, cand, best, 0), searched


def resident(m, fwd, rev_point, rev_best, research=True):
    """The caller of the one-call entry: the replay fed from (fwd, rev_point, rev_best).  A pair whose point's descriptor changed since the call
    is searched again on the live descriptor.  Returns (model, nFused forward, nFused reverse, missing): missing = reverse candidates that
    would be searched and are not in rev_point.  research=False: the replay without that second search (what the call-time answers alone give)."""
    s = FuseModel(m)
    ids = list(m.kfs[0].row)
    nf = 0
    for t in range(m.n_targets):
        best = np.array(fwd[t], np.int32)
        again = [i for i, p in enumerate(ids) if p in s.dirty and research]
        if again:
            sub = [ids[i] for i in again]
            best[again] = search(m, 1 + t, sub, s.gate(1 + t, sub), s.desc)
        nf += s.fuse(1 + t, ids, best, 1)
    table = {int(p): int(b) for p, b in zip(rev_point, rev_best)}
    cand = s.reverse_candidates()
    g = s.gate(0, cand)
    missing = [p for p, skip in zip(cand, g) if not skip and p not in table]
    best = np.array([table.get(p, -1) for p in cand], np.int32)
    again = [i for i, p in enumerate(cand) if p in s.dirty and not g[i]]
    if again:
        sub = [cand[i] for i in again]
        best[again] = search(m, 0, sub, np.zeros(len(sub), bool), s.desc)
    return s, nf, s.fuse(0, cand, best, 0), missing


# ---- a seeded map ----
def seeded_map(seed, n_targets=4, n_extra=2, n_world=150, n_feat=160):
    """World points in front of a row of cameras; every key-frame sees most of them with a pixel of noise and a few descriptor bits flipped, plus
    clutter.  A key-frame's feature either holds the world point's shared map point, a duplicate map point of its own (what Fuse merges), or
    nothing (what Fuse fills), so that the member's branches all occur."""
    rng = np.random.default_rng(seed)
    nk = 1 + n_targets + n_extra
    world = np.stack([rng.uniform(-2.5, 2.5, n_world), rng.uniform(-1.8, 1.8, n_world), rng.uniform(5.0, 9.0, n_world)], 1).astype(np.float32)
    wdesc = rng.integers(0, 256, (n_world, 32), dtype=np.uint8)
    level = rng.integers(1, 5, n_world)
    poses = [pose_t([0, 0, 0])] + [pose_ry(rng.uniform(-0.03, 0.03), rng.uniform(-0.25, 0.25, 3) * [1, 0.3, 0.3]) for _ in range(nk - 1)]
    pos, normal, mn, mx, desc = [], [], [], [], []

    def new_point(w):
        d = float(np.linalg.norm(world[w]))
        pos.append(world[w]); normal.append(world[w] / d)       # the mean viewing direction: from the cameras to the point
        mx.append(d * float(SF[level[w]])); mn.append(mx[-1] / float(SF[NLEVELS - 1]))
        desc.append(flip_bits(wdesc[w], int(rng.integers(0, 8)), rng))
        return len(pos) - 1

    shared = [-1] * n_world            # the map point several key-frames agree on
    kfs = []
    for k in range(nk):
        T7, Ow = poses[k]
        xy, octs, ds, row = [], [], [], []
        held, held0 = set(), (set(kfs[0].row) if kfs else set())       # the points of this row, and of the current key-frame's
        for w in rng.permutation(n_world):
            if len(xy) >= n_feat - 24 or rng.random() < 0.2:
                continue
            pc = project(T7, world[w])
            if pc is None:
                continue
            xy.append(pc + rng.uniform(-0.8, 0.8, 2)); octs.append(int(level[w]) - int(rng.integers(0, 2)))
            ds.append(flip_bits(wdesc[w], int(rng.integers(0, 24)), rng))
            r = rng.random()
            if k == 0:                 # the current key-frame: mostly its own fresh points, some shared with the extras
                if r < 0.75:
                    if shared[w] < 0 and rng.random() < 0.5:
                        shared[w] = new_point(w)
                        row.append(shared[w])
                    else:
                        row.append(new_point(w))
                else:
                    row.append(-1)
            else:
                if r < 0.3:
                    row.append(-1)
                elif r < 0.65 and shared[w] >= 0 and shared[w] not in held:
                    row.append(shared[w])
                elif r < 0.8 and k > 0:
                    if shared[w] < 0 or shared[w] in held0:
                        row.append(new_point(w))
                    else:
                        row.append(shared[w] if shared[w] not in held else -1)
                else:
                    p = new_point(w)
                    if shared[w] < 0:
                        shared[w] = p
                    row.append(p)
            held.add(row[-1])
        while len(xy) < n_feat:        # clutter
            xy.append(rng.uniform([4, 4], [W - 4, H - 4])); octs.append(int(rng.integers(0, NLEVELS)))
            ds.append(rng.integers(0, 256, 32, dtype=np.uint8)); row.append(-1)
        kfs.append(KeyFrame(keypoints(np.float32(xy), octs), np.stack(ds), T7, Ow, row))
    return SinMap(kfs, n_targets, np.float32(pos), np.float32(normal), mn, mx, np.stack(desc))


def project(T7, X):
    """Pixel of world point X in the camera T7 (double; for scene construction only), None when outside a margin of the image."""
    q, t = np.float64(T7[:4]), np.float64(T7[4:])
    x, y, z, w = q
    R = np.float64([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    pc = R @ np.float64(X) + t
    if pc[2] <= 0.1:
        return None
    u, v = K4[0] * pc[0] / pc[2] + K4[2], K4[1] * pc[1] / pc[2] + K4[3]
    return np.float64([u, v]) if 6 < u < W - 6 and 6 < v < H - 6 else None


CONSTRUCTED = [(23, 3), (21, 5), (20, 6)]          # (seed, targets) of the scenes whose branch counts the CPU test asserts


# ---- hand-made maps: one camera at the origin, points placed by the pixel they project to ----
IDENT = pose_t([0, 0, 0])


def point_at(u, v, level, desc, z=1.0):
    """Attributes of a point that the identity pose projects to (u, v) and predicts `level` for: the ratio max_dist / dist sits 0.28 levels below
    1.2^level, so the ceiling in PredictScale is not on an edge."""
    x = np.float32([(u - K4[2]) / K4[0] * z, (v - K4[3]) / K4[1] * z, z])
    d = float(np.linalg.norm(x.astype(np.float64)))
    mx = d * float(SF[level]) * 0.95
    return dict(pos=x, normal=(x / d).astype(np.float32), min_dist=mx / 10.0, max_dist=mx, desc=np.asarray(desc, np.uint8))


def pixel_of(pos):
    """The float arithmetic of the projection for the identity pose (se3f_mul adds zeros): what u, v the device and the oracle see."""
    p = np.float32(pos)
    return np.float32(K4[0] * p[0] / p[2] + K4[2]), np.float32(K4[1] * p[1] / p[2] + K4[3])


def tiny_map(points, targets, n_cur=None, extra_rows=None):
    """points: list of point_at() dicts; entry i of the current key-frame's row holds point i.  targets: list of (xy, octaves, descs) feature
    sets, all with the identity pose and empty rows (extra_rows[t]: another row).  The current key-frame's own features lie in a corner nobody
    projects to, n_cur of them (default: one per point, padded to 70: more than a wave, no multiple of 64)."""
    P = len(points)
    n_cur = max(70, P) if n_cur is None else n_cur
    rng = np.random.default_rng(5)
    cxy = np.stack([600 + (np.arange(n_cur) % 8) * 4.0, 440 + (np.arange(n_cur) // 8) * 3.0], 1)
    cur = KeyFrame(keypoints(cxy, np.zeros(n_cur, np.int32)), rng.integers(0, 256, (n_cur, 32), dtype=np.uint8), *IDENT,
                   list(range(P)) + [-1] * (n_cur - P))
    kfs = [cur]
    for t, (xy, octs, ds) in enumerate(targets):
        row = [-1] * len(xy) if not extra_rows or extra_rows[t] is None else extra_rows[t]
        kfs.append(KeyFrame(keypoints(np.float32(xy).reshape(-1, 2), octs), np.asarray(ds, np.uint8).reshape(-1, 32), *IDENT, row))
    return SinMap(kfs, len(targets), np.stack([p["pos"] for p in points]), np.stack([p["normal"] for p in points]),
                  [p["min_dist"] for p in points], [p["max_dist"] for p in points], np.stack([p["desc"] for p in points]))


# ---- the store ----
class StoreScene:
    """A covisibility store holding a SinMap: rows, observers with feature indices, attributes, features."""

    def __init__(self, m, max_points=None, arena_entries=0, reserve_features=None):
        """arena_entries, reserve_features: first sizes of the row arena and the feature arena (the store's defaults when not given)."""
        from rumi_slam_amd.covis import Covisibility
        from rumi_slam_amd.matcher import FeatureVector, FrameView
        self.m = m
        nk = len(m.kfs)
        self.store = Covisibility(slot_of(nk) + 4, (m.n_points + 64) if max_points is None else max_points, arena_entries=arena_entries)
        if reserve_features is not None:
            self.store.reserve_features(reserve_features)
        self.frames = [FrameView(kf.keys, kf.desc, W, H, SF) for kf in m.kfs]
        self.fv = FeatureVector({})
        order = list(range(nk))[::-1]
        self.store.set_keyframes([slot_of(k) for k in order], [9000 + 13 * slot_of(k) for k in order], [0] * nk, [0] * nk,
                                 [np.asarray(m.kfs[k].row, np.int32) for k in order], [[]] * nk, [-1] * nk, [[]] * nk)
        for k in order:
            self.store.set_keyframe_features(slot_of(k), self.frames[k], self.fv, K4)
        self.set_points(range(m.n_points))

    def set_points(self, ids):
        """(Re)stage observers, bad flags and attributes of the points `ids` from the map."""
        m, ids = self.m, [int(p) for p in ids]
        if not ids:
            return
        obs = m.observations()
        self.store.set_point_observations(ids, m.bad[ids].astype(np.uint8), [[(slot_of(k), f) for k, f in sorted(obs[p].items())] for p in ids])
        have = [p for p in ids if m.has_attr[p]]
        if have:
            self.store.set_point_attributes(have, m.pos[have], m.normal[have], m.min_dist[have], m.max_dist[have], m.desc[have])

    def set_row(self, k):
        s = slot_of(k)
        self.store.set_keyframes([s], [9000 + 13 * s], [0], [0], [np.asarray(self.m.kfs[k].row, np.int32)], [[]], [-1], [[]])

    def fuse_kf(self, k):
        from rumi_slam_amd.mapping import fuse_kf
        kf = self.m.kfs[k]
        return fuse_kf(kf.Tcw7, kf.Ow, BOUNDS, LOG_SF)

    def call(self, matcher, targets=None, th=TH, **kw):
        """targets: key-frame indices in call order (default 1 .. n_targets)."""
        from rumi_slam_amd.mapping import SearchInNeighborsResident
        targets = list(range(1, 1 + self.m.n_targets)) if targets is None else list(targets)
        return SearchInNeighborsResident(matcher, self.store, slot_of(0), self.fuse_kf(0), [slot_of(k) for k in targets],
                                         [self.fuse_kf(k) for k in targets], th, **kw)

    def raw_call(self, matcher, fwd, rev_point, rev_best, rev_cap, targets=None, th=TH):
        """The C entry on the caller's arrays: (status, *n_rev)."""
        import ctypes as C
        from rumi_slam_amd import capi, mapping
        targets = list(range(1, 1 + self.m.n_targets)) if targets is None else list(targets)
        slots = np.asarray([slot_of(k) for k in targets], np.int32)
        arr = (mapping.RumiFuseKF * max(len(targets), 1))(*[self.fuse_kf(k) for k in targets])
        cur, n_rev = self.fuse_kf(0), C.c_int32(-77)
        rc = mapping._lib().rumi_search_in_neighbors_resident(matcher._h, self.store._h, slot_of(0), C.byref(cur), capi.ptr(slots), C.byref(arr), len(targets),
                                                              float(th), capi.ptr(fwd), capi.ptr(rev_point), capi.ptr(rev_best), int(rev_cap), C.byref(n_rev))
        return rc, n_rev.value

    def single_target(self, matcher, k, ids, skip, th=TH):
        """rumi_fuse_candidates (the merged single-target entry) for key-frame k and the points ids."""
        from rumi_slam_amd.matcher import FuseCandidates
        m, kf = self.m, self.m.kfs[k]
        ids = np.asarray(ids, np.int64)
        safe = np.where(ids < 0, 0, ids)
        pts = dict(skip=(np.asarray(skip, bool) | (ids < 0)).astype(np.uint8), pos=m.pos[safe], normal=m.normal[safe], min_dist=m.min_dist[safe],
                   max_dist=m.max_dist[safe], desc=m.desc[safe])
        return FuseCandidates(matcher, self.frames[k], LOG_SF, kf.Tcw7, kf.Ow, K4, pts, th, True)


def clone(m):
    return copy.deepcopy(m)
