"""Small constructed maps for rumi_search_and_fuse_resident (include/rumi_mapping.h) and a host model of LoopClosing::SearchAndFuse
(R/lib_src/LoopClosing.cc:1996-2065) on them.  TEST INFRASTRUCTURE, on top of tests/search_in_neighbors_scene.py (key-frames, points, the
store, MapPoint::Replace with the ComputeDistinctiveDescriptors it ends with).

A map has loop-side key-frames that own the loop points, corrected key-frames that are searched under a pose derived from a Sim3 with scale
!= 1 (ORBmatcher.cc:1190-1191), and the list of loop point ids.  ``FuseSim3Model`` replays ORBmatcher::Fuse(pKF, Scw, vpPoints, th,
vpReplacePoint) (ORBmatcher.cc:1182-1291) and the Replace loop that follows each key-frame (LoopClosing.cc:2017-2023).  Two drivers:

  reference(map)        the member as written: one oracle call per key-frame on the map as it stands at its turn.  The expectation.
  resident(map, hits)   what a caller of the one-call entry does: every pair answered from the map at the call, then the same replay; a loop
                        point whose descriptor a Replace changed is searched again for the key-frames that follow."""
import numpy as np

import oracle_lib as O
import search_in_neighbors_scene as S

TH = 4.0
HIT_DTYPE = np.dtype([("kf", "<i4"), ("point", "<i4"), ("feature", "<i4"), ("occupant", "<i4")])


class SafMap(S.SinMap):
    """kfs: every key-frame of the map.  corrected: indices into kfs, in call order.  poses[k] = (Tcw7, Ow) a corrected key-frame is searched
    under.  ids: the loop point list (-1 and duplicates allowed).  sim3[k] = (q xyzw, t, s) the pose was derived from (None: hand-made)."""

    def __init__(self, kfs, corrected, poses, ids, pos, normal, min_dist, max_dist, desc, bad=None, has_attr=None, sim3=None):
        super().__init__(kfs, 0, pos, normal, min_dist, max_dist, desc, bad, has_attr)
        self.corrected, self.poses, self.ids, self.sim3 = list(corrected), dict(poses), [int(p) for p in ids], sim3


def search(m, k, ids, skip, desc=None):
    """best feature of key-frame k, under its corrected pose, per entry of ids (-1: none, skipped, or id < 0); no reprojection gate."""
    ids = np.asarray(ids, np.int64)
    skip = np.asarray(skip, bool) | (ids < 0)
    if len(ids) == 0:
        return np.zeros(0, np.int32)
    safe = np.where(ids < 0, 0, ids)
    kf = m.kfs[k]
    T7, Ow = m.poses[k]
    pts = dict(skip=skip.astype(np.uint8), pos=m.pos[safe], normal=m.normal[safe], min_dist=m.min_dist[safe], max_dist=m.max_dist[safe],
               desc=(m.desc if desc is None else desc)[safe])
    out = O.fuse_candidates(kf.keys, kf.desc, S.W, S.H, S.SF, S.LOG_SF, T7, Ow, S.K4, pts, TH, False)
    out[skip] = -1
    return out


def call_skip(m, k):
    """The gates the entry evaluates on the store: id < 0, bad, listed by key-frame k."""
    obs = m.observations()
    return np.array([p < 0 or bool(m.bad[p]) or k in obs[p] for p in m.ids], bool)


def dense_call(m):
    """[n_corrected, n_ids] best feature per pair on the map as it stands."""
    return np.stack([search(m, k, m.ids, call_skip(m, k)) for k in m.corrected]) if m.corrected else np.zeros((0, len(m.ids)), np.int32)


def expected_call(m):
    """What the one-call entry must return: (hits in (kf, point) order, hits per key-frame)."""
    best = dense_call(m)
    hits = [(kk, i, int(b), m.kfs[k].row[int(b)]) for kk, k in enumerate(m.corrected) for i, b in enumerate(best[kk]) if b >= 0]
    return np.array(hits, HIT_DTYPE).reshape(-1), (best >= 0).sum(1).astype(np.int32)


class FuseSim3Model(S.FuseModel):
    def __init__(self, m):
        super().__init__(m)
        self.bad0 = m.bad.copy()
        self.n.update(replace=0, occupant_added=0, loop_bad=0, self_replace=0)

    def add_observation(self, p, k, f):    # MapPoint::AddObservation overwrites the left index (MapPoint.cc:165-190)
        self.obs[p][k] = f

    def distinctive(self, p):              # `if (mbBad) return;`, MapPoint.cc:362
        if not self.bad[p]:
            super().distinctive(p)

    def fuse_kf(self, k, ids, best):
        """Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) with the search's answers in best, then the Replace loop."""
        found = {p for p in self.rows[k] if p >= 0 and not self.bad[p]}       # spAlreadyFound = pKF->GetMapPoints(), a snapshot
        rep, added, nfused = [-1] * len(ids), set(), 0
        for i, (p, b) in enumerate(zip(ids, best)):
            if p < 0:
                continue
            if self.bad[p]:
                self.n["skip_bad"] += 1
                self.n["loop_bad"] += not self.bad0[p]
                continue
            if p in found:
                self.n["skip_inkf"] += 1
                self.n["skip_inkf_new"] += k not in self.obs0[p]               # an earlier key-frame's Replace put it here
                continue
            if b < 0:
                continue
            q = self.rows[k][b]                                                # GetMapPoint(bestIdx), live
            if q >= 0:
                if not self.bad[q]:
                    rep[i] = q
                    self.n["occupant_added"] += q in added
                else:
                    self.n["inkf_bad"] += 1
            else:
                self.add_observation(p, k, b)
                self.rows[k][b] = p
                added.add(p)
                self.n["add"] += 1
            nfused += 1
        for i, q in enumerate(rep):                                            # LoopClosing.cc:2017-2023
            if q >= 0:
                self.n["replace"] += 1
                self.n["self_replace"] += q == ids[i]
                self.replace(q, ids[i])
        return nfused

    def gate(self, k, ids):
        return np.array([p < 0 or bool(self.bad[p]) or p in self.rows[k] for p in ids], bool)


def reference(m):
    """SearchAndFuse as written.  Returns (model, nFused)."""
    s = FuseSim3Model(m)
    nf = 0
    for k in m.corrected:
        nf += s.fuse_kf(k, m.ids, search(m, k, m.ids, s.gate(k, m.ids), s.desc))
    return s, nf


def resident(m, hits, research=True):
    """The caller of the one-call entry: the replay fed from the hits.  Returns (model, nFused, pairs searched again)."""
    s = FuseSim3Model(m)
    best = np.full((len(m.corrected), len(m.ids)), -1, np.int32)
    best[hits["kf"], hits["point"]] = hits["feature"]
    nf = again_n = 0
    for kk, k in enumerate(m.corrected):
        g = s.gate(k, m.ids)
        again = [i for i, p in enumerate(m.ids) if research and p in s.dirty and not g[i]]
        if again:
            sub = [m.ids[i] for i in again]
            best[kk, again] = search(m, k, sub, np.zeros(len(sub), bool), s.desc)
            again_n += len(again)
        nf += s.fuse_kf(k, m.ids, best[kk])
    return s, nf, again_n


def corrected_pose(q, tt, s):
    """A Sim3 (q, t = s * tt, s) and what ORBmatcher.cc:1190-1191 derives from it: Tcw = (R, t / s), Ow = -R^T (t / s)."""
    q = np.float32(q)
    t = (np.float32(tt) * np.float32(s)).astype(np.float32)
    td = (t / np.float32(s)).astype(np.float32)
    x, y, z, w = np.float64(q)
    R = np.float64([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return (np.concatenate([q, td]).astype(np.float32), (-(R.T @ np.float64(td))).astype(np.float32)), (q, t, np.float32(s))


def seeded_map(seed, n_corr=5, n_loop=2, n_world=110, n_feat=160):
    """World points in front of a row of cameras.  The loop-side key-frames hold the loop points (one per world point, for some a twin: a second
    loop point at the same place with nearly the same descriptor, held by another loop-side key-frame).  A corrected key-frame's feature holds
    a drifted duplicate that several corrected key-frames share (what Replace merges), a point of its own, or nothing (what Fuse fills)."""
    rng = np.random.default_rng(seed)
    world = np.stack([rng.uniform(-2.5, 2.5, n_world), rng.uniform(-1.8, 1.8, n_world), rng.uniform(5.0, 9.0, n_world)], 1).astype(np.float32)
    wdesc = rng.integers(0, 256, (n_world, 32), dtype=np.uint8)
    level = rng.integers(1, 5, n_world)
    # a quarter of the world points look different from the corrected side: their second appearance is 56 bits from the first, so a loop point
    # matches such a feature only once a Replace has given it a descriptor of that side
    wdesc2 = np.stack([S.flip_bits(d, 56, rng) if rng.random() < 0.25 else d for d in wdesc])
    pos, normal, mn, mx, desc = [], [], [], [], []

    def new_point(w, bits=8):
        d = float(np.linalg.norm(world[w]))
        pos.append(world[w]); normal.append(world[w] / d)
        mx.append(d * float(S.SF[level[w]])); mn.append(mx[-1] / float(S.SF[S.NLEVELS - 1]))
        desc.append(S.flip_bits(wdesc[w], int(rng.integers(0, bits)), rng))
        return len(pos) - 1

    loop = [[new_point(w)] + ([new_point(w, 3)] if rng.random() < 0.2 else []) for w in range(n_world)]
    dup = [-1] * n_world
    kfs, poses, sim3 = [], {}, {}
    for k in range(n_loop + n_corr):
        q7, _ = S.pose_ry(rng.uniform(-0.03, 0.03), rng.uniform(-0.25, 0.25, 3) * [1, 0.3, 0.3])
        if k >= n_loop:
            (T7, Ow), sim3[k] = corrected_pose(q7[:4], q7[4:], rng.uniform(0.8, 1.25))
            poses[k] = (T7, Ow)
        else:
            T7 = q7
        xy, octs, ds, row = [], [], [], []
        for w in rng.permutation(n_world):
            if len(xy) >= n_feat - 24 or rng.random() < 0.2:
                continue
            pc = S.project(T7, world[w])
            if pc is None:
                continue
            xy.append(pc + rng.uniform(-0.8, 0.8, 2)); octs.append(int(level[w]) - int(rng.integers(0, 2)))
            ds.append(S.flip_bits((wdesc2 if k >= n_loop and rng.random() < 0.6 else wdesc)[w], int(rng.integers(0, 24)), rng))
            r = rng.random()
            if k < n_loop:
                row.append(loop[w][k % len(loop[w])] if len(loop[w]) > 1 or r < 0.8 else -1)
            elif r < 0.4:
                row.append(-1)
            elif r < 0.8:
                if dup[w] < 0:
                    dup[w] = new_point(w)
                row.append(dup[w])
            else:
                row.append(new_point(w))
        while len(xy) < n_feat:        # clutter
            xy.append(rng.uniform([4, 4], [S.W - 4, S.H - 4])); octs.append(int(rng.integers(0, S.NLEVELS)))
            ds.append(rng.integers(0, 256, 32, dtype=np.uint8)); row.append(-1)
        Tst, Ost = S.pose_t([0, 0, 0]) if k >= n_loop else (T7, None)          # a corrected key-frame's own (drifted) pose is never read
        kfs.append(S.KeyFrame(S.keypoints(np.float32(xy), octs), np.stack(ds), Tst, np.zeros(3, np.float32) if Ost is None else Ost, row))
    held = sorted({p for kf in kfs[:n_loop] for p in kf.row if p >= 0})
    ids = [int(p) for p in rng.permutation(held)]
    bad = np.zeros(len(pos), bool)
    bad[ids[5]] = True                                       # a loop point that is bad at the call
    ids.insert(11, -1)
    ids.insert(40, ids[3])                                   # an id twice
    return SafMap(kfs, list(range(n_loop, n_loop + n_corr)), poses, ids, np.float32(pos), np.float32(normal), mn, mx, np.stack(desc), bad=bad, sim3=sim3)


CONSTRUCTED = [101, 102, 107]         # the seeds whose branch counts the CPU test asserts (chosen on the CPU, see test_search_and_fuse_cpu.py)


# ---- hand-made maps: every key-frame at the identity pose, points placed by the pixel they project to ----
def tiny_map(points, targets, rows=None, ids=None, pad_to=70):
    """points: list of S.point_at() dicts.  targets: list of (xy, octaves, descs) feature sets, each a corrected key-frame with the identity pose
    and an empty row (rows[t]: another row), padded with clutter in a corner nobody projects to up to pad_to features (more than a wave, no
    multiple of 64).  ids: the list (default: every point once)."""
    rng = np.random.default_rng(5)
    kfs = []
    for t, (xy, octs, ds) in enumerate(targets):
        xy, octs, ds = np.float32(xy).reshape(-1, 2), list(octs), np.asarray(ds, np.uint8).reshape(-1, 32)
        row = [-1] * len(xy) if not rows or rows[t] is None else list(rows[t])
        extra = max(0, pad_to - len(xy))
        cxy = np.stack([600 + (np.arange(extra) % 8) * 4.0, 440 + (np.arange(extra) // 8) * 3.0], 1).reshape(-1, 2)
        kfs.append(S.KeyFrame(S.keypoints(np.concatenate([xy, np.float32(cxy)]), octs + [7] * extra),
                              np.concatenate([ds, rng.integers(0, 256, (extra, 32), dtype=np.uint8)]), *S.IDENT, row + [-1] * extra))
    P = len(points)
    return SafMap(kfs, list(range(len(kfs))), {k: S.IDENT for k in range(len(kfs))}, list(range(P)) if ids is None else ids,
                  np.stack([p["pos"] for p in points]), np.stack([p["normal"] for p in points]), [p["min_dist"] for p in points],
                  [p["max_dist"] for p in points], np.stack([p["desc"] for p in points]))


class StoreScene(S.StoreScene):
    """A covisibility store holding a SafMap."""

    def fuse_kf(self, k):
        from rumi_slam_amd.mapping import fuse_kf
        T7, Ow = self.m.poses[k]
        return fuse_kf(T7, Ow, S.BOUNDS, S.LOG_SF)

    def call(self, matcher, corrected=None, ids=None, th=TH, **kw):
        from rumi_slam_amd.mapping import SearchAndFuseResident
        ks = self.m.corrected if corrected is None else list(corrected)
        return SearchAndFuseResident(matcher, self.store, [S.slot_of(k) for k in ks], [self.fuse_kf(k) for k in ks],
                                     self.m.ids if ids is None else ids, th, **kw)

    def raw_call(self, matcher, hits, hit_cap, per_kf, corrected=None, ids=None, th=TH, slots=None, kfs=None, n_kfs=None, n_points=None,
                 n_hits=True, store=True):
        """The C entry on the caller's arrays: (status, *n_hits, message).  matcher: an ORBmatcher, or None."""
        import ctypes as C
        from rumi_slam_amd import capi, mapping
        ks = self.m.corrected if corrected is None else list(corrected)
        slots = np.asarray([S.slot_of(k) for k in ks] if slots is None else slots, np.int32)
        arr = (mapping.RumiFuseKF * max(len(ks), 1))(*[self.fuse_kf(k) for k in ks]) if kfs is None else kfs
        ids = np.ascontiguousarray(self.m.ids if ids is None else ids, np.int32)
        n = C.c_int32(-77)
        rc = mapping._lib().rumi_search_and_fuse_resident(matcher._h if matcher is not None else None, self.store._h if store else None, capi.ptr(slots),
                                                          C.byref(arr), len(slots) if n_kfs is None else n_kfs, capi.ptr(ids),
                                                          len(ids) if n_points is None else n_points, float(th), capi.ptr(hits), int(hit_cap),
                                                          C.byref(n) if n_hits else None, capi.ptr(per_kf))
        return rc, n.value, capi.lib().rumi_last_error().decode()

    def single(self, matcher, k, ids, skip, th=TH, reproj=False):
        """rumi_fuse_candidates for key-frame k under its corrected pose: what the facade's per-key-frame Fuse calls."""
        from rumi_slam_amd.matcher import FuseCandidates
        m = self.m
        ids = np.asarray(ids, np.int64)
        safe = np.where(ids < 0, 0, ids)
        pts = dict(skip=(np.asarray(skip, bool) | (ids < 0)).astype(np.uint8), pos=m.pos[safe], normal=m.normal[safe], min_dist=m.min_dist[safe],
                   max_dist=m.max_dist[safe], desc=m.desc[safe])
        T7, Ow = m.poses[k]
        return FuseCandidates(matcher, self.frames[k], S.LOG_SF, T7, Ow, S.K4, pts, th, reproj)
