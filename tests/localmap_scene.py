"""Scenes for rumi_track_local_map (include/rumi_track.h): the point table of test_track_frame_gpu._scene joined with a covisibility store.
TEST INFRASTRUCTURE, not a test.

A table row gets its point id through a random permutation into a max_points about three times the table, so that a row taken for an id (or
the other way round) lands somewhere else.  Key-frames are windows over the table rows that overlap their neighbours; a point's observers are
the key-frames whose mp row holds it.  A few points have no observer (Observations() = 0: they can only enter the table as the frame's extras),
a few are bad.  host_table() states the table rules of the header in numpy: the local points in their order, then the frame's other points
that are not bad, each once in order of first feature, then the discarded ids that have no row yet."""
import numpy as np

from covis_scene import World

W, H = 640, 480


def cpu_source(seed=4242, n_keep=1.0):
    """test_track_frame_gpu._scene with the CPU oracle's extractor (bit-identical to the device's): (img0, sf, inv_sigma2, pts, last)."""
    import oracle_lib as O
    from rumi_slam_amd.synth import synth_frame
    from scene import K_TUM3
    from test_tracking_loop_gpu import PLANE_D
    orc = O.OracleExtractor(1000, 1.2, 8, 20, 7)
    tb = orc.tables()
    sf, inv_sigma2 = tb["scale"], tb["inv_sigma2"]
    img0 = synth_frame(seed)
    fx, fy, cx, cy = K_TUM3.astype(np.float64)
    _, keys0, desc0 = orc.extract(img0)
    n0 = len(keys0)
    pos = np.stack([(keys0["x"] - cx) / fx * PLANE_D, (keys0["y"] - cy) / fy * PLANE_D, np.full(n0, PLANE_D)], 1).astype(np.float32)
    dist0 = np.linalg.norm(pos, axis=1).astype(np.float32)
    lvl = keys0["octave"]
    pts = dict(pos=pos, normal=(pos / dist0[:, None]).astype(np.float32), max_dist=(dist0 * sf[lvl]).astype(np.float32),
               min_dist=(dist0 * sf[lvl] / sf[7]).astype(np.float32), desc=desc0.copy(), obs=np.ones(n0, np.int32), bad=np.zeros(n0, np.uint8),
               local=np.ones(n0, np.uint8))
    rng = np.random.default_rng(3)
    last = dict(keys=keys0, mp=np.where(rng.random(n0) < n_keep, np.arange(n0), -1).astype(np.int32), outlier=np.zeros(n0, np.uint8))
    return img0, sf, inv_sigma2, pts, last


class LocalMapScene:
    """pts: the table of _scene (its obs and bad are replaced by the store's).  rows_of_kf: the table rows of every key-frame's mp row (None: eight
    overlapping windows); no_observer / bad: table rows (None: drawn)."""

    def __init__(self, pts, seed=5, rows_of_kf=None, no_observer=None, bad=None):
        rng = np.random.default_rng(seed)
        n0 = len(pts["obs"])
        self.n0, self.max_points = n0, 3 * n0 + 7
        self.id_of_row = rng.permutation(self.max_points)[:n0].astype(np.int32)
        self.row_of_id = np.full(self.max_points, -1, np.int32)
        self.row_of_id[self.id_of_row] = np.arange(n0, dtype=np.int32)
        no_observer = rng.choice(n0, 30, replace=False) if no_observer is None else np.asarray(no_observer, int)
        bad = rng.choice(n0, 14, replace=False) if bad is None else np.asarray(bad, int)
        if rows_of_kf is None:
            n_kf, width = 8, n0 // 4
            rows_of_kf = []
            for k in range(n_kf):
                a = k * (n0 - width) // (n_kf - 1)
                r = [int(x) for x in range(a, a + width) if rng.random() < 0.9]
                rows_of_kf.append([r[j] for j in rng.permutation(len(r))])
        orphan = set(int(r) for r in no_observer)
        self.rows_of_kf = [[r for r in rows if r not in orphan] for rows in rows_of_kf]
        n_kf = len(self.rows_of_kf)
        self.world = w = World(max(n_kf, 1), self.max_points)
        keys = rng.permutation(10 * max(n_kf, 1))[:n_kf] + 1                      # pointer order is unrelated to slot order
        observers = [[] for _ in range(n0)]
        for k, rows in enumerate(self.rows_of_kf):
            mp = []
            for r in rows:
                mp.append(int(self.id_of_row[r])); observers[r].append(k)
                if rng.random() < 0.1:
                    mp.append(-1)
            w.add_kf(k, int(keys[k]), mp=mp, best=[j for j in (k - 1, k + 1) if 0 <= j < n_kf], parent=k - 1 if k > 0 else -1,
                     children=[k + 1] if k + 1 < n_kf else [])
        isbad = np.zeros(n0, np.uint8)
        isbad[bad] = 1
        for r in range(n0):
            w.add_pt(int(self.id_of_row[r]), observers[r], bool(isbad[r]))
        self.pts = dict(pts, obs=np.array([len(o) for o in observers], np.int32), bad=isbad, local=np.ones(n0, np.uint8))

    # ---- into a store ----
    def set_attributes(self, cov, rows=None, pts=None):
        pts = self.pts if pts is None else pts
        rows = np.arange(self.n0) if rows is None else np.asarray(rows, int)
        return cov.set_point_attributes(self.id_of_row[rows], pts["pos"][rows], pts["normal"][rows], pts["min_dist"][rows], pts["max_dist"][rows], pts["desc"][rows])

    def store(self, without_attributes=()):
        from rumi_slam_amd.covis import Covisibility
        cov = self.world.load(Covisibility(self.world.max_kf, self.max_points))
        skip = set(int(r) for r in without_attributes)
        self.set_attributes(cov, [r for r in range(self.n0) if r not in skip])
        return cov

    # ---- ids and rows ----
    def ids(self, rows):
        rows = np.asarray(rows, np.int32)
        return np.where(rows >= 0, self.id_of_row[np.maximum(rows, 0)], -1).astype(np.int32)

    def host_table(self, local_points, frame_points, discarded_ids=(), pts=None, stale=None):
        """The table the header describes, built on the host: (table_ids, frame_mp_in as rows, seen_in, points of rumi_track_local).
        stale: (in_view [len(discarded_ids)], proj5 [len(discarded_ids), 5]) -> the dense stale_in_view / stale_proj of the table."""
        pts = self.pts if pts is None else pts
        table = [int(p) for p in local_points]
        have = set(table)
        n_local = len(table)
        isbad = lambda p: bool(pts["bad"][self.row_of_id[p]])
        for p in frame_points:
            p = int(p)
            if p >= 0 and not isbad(p) and p not in have:
                table.append(p); have.add(p)
        for p in discarded_ids:
            if int(p) not in have:
                table.append(int(p)); have.add(int(p))
        table = np.array(table, np.int32).reshape(-1)
        row = {int(p): r for r, p in enumerate(table)}
        frame_mp_in = np.array([row[int(p)] if p >= 0 and not isbad(int(p)) else -1 for p in frame_points], np.int32)
        seen_in = np.zeros(len(table), np.uint8)
        for p in discarded_ids:
            seen_in[row[int(p)]] = 1
        src = self.row_of_id[table]                                               # the row of _scene's table each table row comes from
        out = {k: np.ascontiguousarray(pts[k][src]) for k in ("pos", "normal", "min_dist", "max_dist", "desc", "obs", "bad")}
        out["local"] = (np.arange(len(table)) < n_local).astype(np.uint8)
        if stale is not None:
            sin, sproj = np.zeros(len(table), np.uint8), np.zeros((len(table), 5), np.float32)
            for k, p in enumerate(discarded_ids):
                sin[row[int(p)]] = stale[0][k]; sproj[row[int(p)]] = stale[1][k]
            out["stale_in_view"], out["stale_proj"] = sin, sproj
        return table, frame_mp_in, seen_in, out


def seam_scene(pts, frame_rows, n_local, seed=5):
    """A store whose local list has exactly n_local points: ONE key-frame whose row holds n_local points, the first of which the frame holds
    (it votes for the key-frame); every other point has no observer, so whatever else the frame holds becomes an extra."""
    held = [int(r) for r in dict.fromkeys(int(r) for r in frame_rows if r >= 0)]
    rest = [r for r in range(len(pts["obs"])) if r not in set(held)]
    order = held[:1] + rest + held[1:]                                            # most of the row is not held by the frame
    return LocalMapScene(pts, seed, rows_of_kf=[order[:n_local]] if n_local > 0 else [], no_observer=[], bad=[])
