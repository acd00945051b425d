"""Maps for the tests of rumi_refresh_map_points_resident (include/rumi_mapping.h): one map, marshalled both as the RefreshBatch of the
block entry and the oracle (tests/refresh_scene.py) and as the edits that put it into a covisibility store.  TEST INFRASTRUCTURE.

``ResidentMap`` holds key-frames as RefreshBatch takes them plus the octave of every feature (the store derives ref_level from the reference
slot's resident key-points), and points as (position, reference key-frame, [(key-frame, feature), ...] in list order).  ref_feature and
ref_level of the batch follow from those the way the resident entry defines them: the feature the list holds for the reference key-frame, 0
where it does not list it, and that feature's octave."""
import numpy as np

from rumi_slam_amd import capi
from rumi_slam_amd.mapping import RefreshBatch

SF = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
K4 = [500.0, 500.0, 320.0, 240.0]


class ResidentMap:
    def __init__(self, keyframes, octaves, points):
        """keyframes: (desc [n, 32], scale factors, Ow, isBad) each; octaves[k]: [n] int; points: (pos, ref_kf or -1, [(k, f), ...]) each."""
        self.kfs = [(np.ascontiguousarray(d, np.uint8).reshape(-1, 32), np.asarray(sf, np.float32), np.asarray(Ow, np.float32), bool(bad))
                    for d, sf, Ow, bad in keyframes]
        self.octaves = [np.asarray(o, np.int32) for o in octaves]
        self.points = [(np.asarray(pos, np.float32), int(ref), [(int(k), int(f)) for k, f in obs]) for pos, ref, obs in points]
        self.n_kf, self.n_pts = len(self.kfs), len(self.points)

    @classmethod
    def from_scene(cls, sc):
        """A refresh_scene.RefreshScene: its ref_feature / ref_level already follow the rule above."""
        m = cls(sc.keyframes(), list(sc.octave), [(p[0], p[1], p[4]) for p in sc.points])
        for mine, theirs in zip(m.batch_points(), sc.points):
            assert mine[1:4] == (theirs[1], theirs[2], theirs[3]) or not theirs[4]
        return m

    def batch_points(self, order=None):
        pts = []
        for i in (range(self.n_pts) if order is None else order):
            pos, ref, obs = self.points[i]
            rf = dict(obs).get(ref, 0)
            pts.append((pos, max(ref, 0), rf, int(self.octaves[ref][rf]) if obs else 0, obs))
        return pts

    def batch(self, order=None):
        return RefreshBatch(self.kfs, self.batch_points(order))

    # ---- into a store: slot k = key-frame k, id p = point p
    def features(self, k):
        from rumi_slam_amd.matcher import FeatureVector, FrameView
        desc, sf, _, _ = self.kfs[k]
        keys = np.zeros(len(desc), capi.KP_DTYPE)
        keys["octave"] = self.octaves[k]
        return FrameView(keys, desc, 640, 480, sf), FeatureVector({})

    def initial_attributes(self, ids):
        """What the store holds before a refresh: the position, and a recognisable pattern everywhere else."""
        ids = list(ids)
        n = len(ids)
        pos = np.stack([self.points[p][0] for p in ids]) if n else np.zeros((0, 3), np.float32)
        normal = np.tile(np.array([0.25, -0.5, 0.75], np.float32), (n, 1)) + np.arange(n, dtype=np.float32)[:, None]
        return dict(pos=pos, normal=normal, min_dist=np.full(n, 0.5, np.float32), max_dist=np.full(n, 40.0, np.float32),
                    desc=np.full((n, 32), 0xA5, np.uint8))

    def set_keyframes(self, store, kfs, order_key=None):
        kfs = list(kfs)
        store.set_keyframes(kfs, [(k + 1 if order_key is None else int(order_key[k])) for k in kfs], [0] * len(kfs), [self.kfs[k][3] for k in kfs],
                            [np.full(len(self.kfs[k][0]), -1, np.int32) for k in kfs], [[] for _ in kfs], [-1] * len(kfs), [[] for _ in kfs])

    def set_features(self, store, kfs):
        for k in kfs:
            fr, fv = self.features(k)
            store.set_keyframe_features(k, fr, fv, K4)

    def set_centres(self, store, kfs):
        kfs = list(kfs)
        if kfs:
            store.set_keyframe_centres(kfs, np.stack([self.kfs[k][2] for k in kfs]))

    def set_points(self, store, pts, attributes=True, references=True):
        pts = list(pts)
        store.set_point_observations(pts, [0] * len(pts), [self.points[p][2] for p in pts])
        if attributes:
            a = self.initial_attributes(pts)
            store.set_point_attributes(pts, a["pos"], a["normal"], a["min_dist"], a["max_dist"], a["desc"])
        if references:
            store.set_point_reference(pts, [self.points[p][1] for p in pts])

    def load(self, store):
        self.set_keyframes(store, range(self.n_kf))
        self.set_features(store, range(self.n_kf))
        self.set_centres(store, range(self.n_kf))
        self.set_points(store, range(self.n_pts))

    def store(self, **kw):
        from rumi_slam_amd.covis import Covisibility
        s = Covisibility(max(self.n_kf, 1), max(self.n_pts, 1), **kw)
        self.load(s)
        return s

    def winning_rows(self, best_obs):
        """desc [n, 32] as the resident entry returns it for these best_obs (rows of a point without a winner: None)."""
        return [self.kfs[self.points[p][2][b][0]][0][self.points[p][2][b][1]] if b >= 0 else None for p, b in enumerate(best_obs)]

    def expected_records(self, ids, res, what_desc=True, what_normal=True, before=None):
        """The 64-byte attribute records [n, 64] after a write-back of the results ``res`` (entries in the order of ``ids``)."""
        ids = list(ids)
        a = self.initial_attributes(ids) if before is None else before
        rec = np.zeros((len(ids), 64), np.uint8)
        for i, p in enumerate(ids):
            f = np.concatenate([a["pos"][i], a["normal"][i], [a["min_dist"][i]], [a["max_dist"][i]]]).astype(np.float32)
            d = a["desc"][i].copy()
            if what_desc and res["best_obs"][i] >= 0:
                k, ft = self.points[p][2][int(res["best_obs"][i])]
                d = self.kfs[k][0][ft]
            if what_normal and res["updated"][i]:
                f[3:6] = res["normal"][i]
                f[6], f[7] = res["min_distance"][i], res["max_distance"][i]
            rec[i, :32] = f.view(np.uint8)
            rec[i, 32:] = d
        return rec


def constructed_map(seed=0, n_kf=320, nfeat=12):
    """The constructed set of tests/test_refresh_resident_gpu.py: every case a point of its own, named in ``cases`` (name -> point id)."""
    rng = np.random.default_rng(4100 + seed)
    bad = np.zeros(n_kf, bool)
    bad[300:320] = True                                                   # the last twenty key-frames are bad
    good = np.arange(300)
    desc = rng.integers(0, 256, (n_kf, nfeat, 32), dtype=np.uint8)
    octave = rng.integers(0, 7, (n_kf, nfeat)).astype(np.int32)
    octave[7, :] = 7                                                      # key-frame 7: every feature at the top octave
    Ow = rng.uniform(-9, 9, (n_kf, 3)).astype(np.float32)
    free = np.zeros(n_kf, np.int64)
    points, cases = [], {}

    def flip(row, nbits):
        row = row.copy()
        for b in rng.integers(0, 256, nbits):
            row[b >> 3] ^= np.uint8(1 << (b & 7))
        return row

    def add(name, kfs, ref=None, rows=None, ref_outside=False):
        """kfs in list order (not sorted: the stored order is what counts).  rows: descriptors to plant, else noisy copies of a landmark."""
        land = rng.integers(0, 256, 32, dtype=np.uint8)
        obs = []
        for j, k in enumerate(int(k) for k in kfs):
            f = int(free[k]); free[k] += 1
            assert f < nfeat, "constructed_map: a key-frame ran out of features"
            desc[k, f] = flip(land, int(rng.integers(1, 40))) if rows is None else rows[j]
            obs.append((k, f))
        if ref_outside:
            ref = next(k for k in range(n_kf) if k not in set(kfs) and not bad[k] and k != 7)
        elif ref is None:
            ref = obs[int(rng.integers(0, len(obs)))][0] if obs else -1
        cases[name] = len(points)
        points.append((np.array([rng.uniform(-5, 5), rng.uniform(-3.5, 3.5), rng.uniform(3, 14)], np.float32), int(ref), obs))

    pick = lambda n, pool=good: rng.permutation(pool)[:n]
    for n in (1, 2, 3, 16, 17, 32, 33, 64, 65, 66, 129, 300):
        add(f"len{n}", pick(n))
    add("empty", [])
    add("all_bad", np.arange(300, 305), ref=0)
    g = pick(6)
    add("bad_first", np.concatenate([[310], g]))
    add("bad_middle", np.concatenate([g[:3], [311], g[3:]]))
    add("bad_last", np.concatenate([g, [312]]))
    # the row length sits in the higher bin, the rows left in the lower one and at its edge
    add("len17_left16", np.concatenate([pick(10), [313], pick(6, good[200:])]))
    add("len18_left17", np.concatenate([pick(9), [314], pick(8, good[200:])]))
    add("len65_left64", np.concatenate([pick(40, good[:150]), [315], pick(24, good[150:])]))
    add("len66_left65", np.concatenate([pick(40, good[:150]), [316], pick(25, good[150:])]))
    add("len70_left60", np.concatenate([pick(30, good[:150]), np.arange(300, 310), pick(30, good[150:])]))
    # equal smallest medians: rows A A B B C ... -> positions 1 and 2 hold copies of one row X, position 0 a far row
    X, far = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)
    add("two_equal_medians", pick(5), rows=[far, X, X, flip(X, 3), flip(X, 5)])
    add("three_equal_medians", pick(7), rows=[far, flip(far, 90), X, X, X, flip(X, 2), flip(X, 4)])
    g = pick(4)
    add("winner_after_bad", [g[0], 318, g[1], g[2], g[3]], rows=[far, far, flip(far, 90), X, X])   # the winner: position 3, the third row left
    add("identical", pick(9), rows=[X] * 9)
    add("identical_wide", pick(80), rows=[X] * 80)
    add("ref_outside", pick(5), ref_outside=True)
    k = pick(6)
    add("ref_bad", np.concatenate([k, [317]]), ref=317)
    add("ref_top_octave", np.concatenate([pick(4, good[8:]), [7]]), ref=7)
    shared = pick(20)
    add("shared_a", shared)
    add("shared_b", shared)
    kfs = [(desc[k], SF, Ow[k], bad[k]) for k in range(n_kf)]
    m = ResidentMap(kfs, list(octave), points)
    m.cases = cases
    return m


def capacity_map(n_obs, seed=0):
    """One point observed by n_obs key-frames of 4 features each, and a small point behind it (refresh_scene.capacity_batch as a map)."""
    rng = np.random.default_rng(77 + seed)
    land = rng.integers(0, 256, 32, dtype=np.uint8)
    kfs, octs, obs = [], [], []
    for k in range(n_obs):
        d = rng.integers(0, 256, (4, 32), dtype=np.uint8)
        f = int(rng.integers(0, 4))
        d[f] = land ^ rng.integers(0, 2, 32, dtype=np.uint8)
        kfs.append((d, SF, rng.uniform(-8, 8, 3).astype(np.float32), False))
        octs.append(rng.integers(0, 8, 4).astype(np.int32))
        obs.append((k, f))
    return ResidentMap(kfs, octs, [(np.array([0.5, -0.2, 7.0], np.float32), 3, obs), (np.array([1.5, 0.2, 5.0], np.float32), 1, obs[:3])])


def outputs_equal(res, want, what_desc, what_normal):
    """Names of the resident outputs (trimmed dicts) that differ from the block entry's / the oracle's."""
    keys = (["best_obs", "best_median"] if what_desc else []) + (["normal", "min_distance", "max_distance", "updated"] if what_normal else [])
    return [k for k in keys if res[k].tobytes() != want[k].tobytes()]
