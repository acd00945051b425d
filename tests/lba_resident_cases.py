"""Constructed windows for rumi_local_ba_resident (include/rumi_opt.h): small maps as plain dictionaries, a plain-Python restatement of how
Optimizer::LocalBundleAdjustment builds its graph from the live objects (R/lib_src/Optimizer.cc:1003-1271, monocular branch), the
expected lists of every scene written out by hand, and the loader that puts a scene into a covisibility store.

TEST INFRASTRUCTURE (numpy only; the store is touched by ``to_store`` alone).

A scene:
  kfs[slot] = dict(key, map, bad, has_pose, pose7 float32[7], keys KP_DTYPE[n], sf float32[8], row [n] point ids or -1, q, t = the true pose)
  pts[id]   = dict(map (None: never given one), bad, pos float32[3], X = the true position, obs = [(slot, feature), ...] in the order the
              store is given them -- std::map order is ascending kfs[slot]["key"], whatever this order is)
"""
import numpy as np

from rumi_slam_amd import capi
from scene import K_TUM3, quat_from_rotvec, quat_rotate

NLEVELS = 8
SF = (np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)).astype(np.float32)


class Scene:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.kfs, self.pts = {}, {}
        self.K4 = K_TUM3.copy()
        self.moved = []                      # (slot, feature, id) of the observations placed 12 px off

    # key-frames on an arc of radius 3 m looking at a box of points (tests/ba_scene.py), the stored pose a little off the truth
    def add_kf(self, slot, key, n, map_id=0, bad=False, has_pose=True, pose_noise=(np.deg2rad(0.5), 0.01)):
        k = len(self.kfs)
        a = np.deg2rad(1.0) * (k % 40 - 20) + 0.001 * k
        q_wc = quat_from_rotvec(np.array([0.0, a, 0.0]))
        c = np.array([3.0 * np.sin(a), 0.02 * (k % 40) + 0.3 * (k // 40), 3.0 * (1 - np.cos(a))])
        q = q_wc * np.array([-1, -1, -1, 1.0])
        t = -quat_rotate(q, c[None])[0][0]
        dq = quat_from_rotvec(self.rng.normal(size=3) * pose_noise[0] / np.sqrt(3))
        x1, y1, z1, w1 = dq; x2, y2, z2, w2 = q
        qn = np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2,
                       w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])
        keys = np.zeros(n, capi.KP_DTYPE)
        keys["x"] = self.rng.uniform(20, 620, n); keys["y"] = self.rng.uniform(20, 460, n)
        keys["octave"] = self.rng.integers(0, NLEVELS, n)
        self.kfs[slot] = dict(key=int(key), map=map_id, bad=bool(bad), has_pose=has_pose, q=q, t=t,
                              pose7=np.concatenate([qn, t + self.rng.normal(size=3) * pose_noise[1] / np.sqrt(3)]).astype(np.float32),
                              keys=keys, sf=SF.copy(), row=[-1] * n)

    def add_point(self, pid, map_id=0, bad=False, noise=0.02):
        X = np.array([self.rng.uniform(-2, 2), self.rng.uniform(-1.5, 1.5), self.rng.uniform(3, 7)])
        self.pts[pid] = dict(map=map_id, bad=bool(bad), X=X, pos=(X + self.rng.normal(size=3) * noise / np.sqrt(3)).astype(np.float32), obs=[])

    def observe(self, slot, feature, pid, in_row=True, shift=0.0, octave=None):
        """Point pid is seen by feature `feature` of key-frame `slot`: the key-point goes where the true point projects under the true pose,
        plus pixel noise of its octave, plus `shift` pixels in x."""
        kf, P = self.kfs[slot], self.pts[pid]
        K = self.K4.astype(np.float64)
        Xc = quat_rotate(kf["q"], P["X"][None])[0][0] + kf["t"]
        assert Xc[2] > 0.1
        if octave is not None:
            kf["keys"]["octave"][feature] = octave
        sig = 1.2 ** int(kf["keys"]["octave"][feature])
        kf["keys"]["x"][feature] = K[0] * Xc[0] / Xc[2] + K[2] + self.rng.normal() * 0.5 * sig + shift
        kf["keys"]["y"][feature] = K[1] * Xc[1] / Xc[2] + K[3] + self.rng.normal() * 0.5 * sig
        if in_row:
            assert kf["row"][feature] == -1
            kf["row"][feature] = pid
        assert all(s != slot for s, _ in P["obs"])
        P["obs"].append((slot, feature))
        if shift:
            self.moved.append((slot, feature, pid))

    def shuffle_observers(self):
        for P in self.pts.values():
            self.rng.shuffle(P["obs"])


# ---- the reference's construction, restated ---------------------------------------------------------------------------------------------
def window(scene, cur, neigh, init):
    """Optimizer.cc:1003-1271 over the scene's dictionaries.  Returns dict(aborted, kf_slots, num_OptKF, num_fixedKF, mp_ids, edges =
    [(slot, id, feature)] in edge order, args = the argument tuple of Optimizer.LocalBundleAdjustment or None when aborted)."""
    kfs, pts = scene.kfs, scene.pts
    cur_map = kfs[cur]["map"]
    local, ba_local = [cur], {cur}                                     # :1007-1008
    for s in neigh:                                                    # :1011-1017
        ba_local.add(s)
        if not kfs[s]["bad"] and kfs[s]["map"] == cur_map:
            local.append(s)
    num_fixed, mp_ids, seen = 0, [], set()
    for s in local:                                                    # :1023-1039
        if s == init:
            num_fixed = 1
        for p in kfs[s]["row"]:
            if p >= 0 and not pts[p]["bad"] and pts[p]["map"] == cur_map and p not in seen:
                mp_ids.append(p); seen.add(p)
    by_key = lambda p: sorted(pts[p]["obs"], key=lambda o: kfs[o[0]]["key"])       # std::map<KeyFrame *, ...> iterates by pointer = order_key
    ok = lambda s: not kfs[s]["bad"] and kfs[s]["map"] == cur_map
    fixed, ba_fixed = [], set()
    for p in mp_ids:                                                   # :1042-1055
        for s, _ in by_key(p):
            if s not in ba_local and s not in ba_fixed:
                ba_fixed.add(s)
                if ok(s):
                    fixed.append(s)
    num_fixed += len(fixed)
    res = dict(aborted=num_fixed == 0, kf_slots=local + fixed, num_OptKF=len(local), num_fixedKF=num_fixed, mp_ids=mp_ids, edges=[], args=None)
    if res["aborted"]:                                                 # :1057-1060
        return res
    index = {s: i for i, s in enumerate(res["kf_slots"])}
    kf_pose = np.stack([kfs[s]["pose7"] for s in res["kf_slots"]]).astype(np.float32)
    kf_fixed = np.array([1 if (i >= len(local) or s == init) else 0 for i, s in enumerate(res["kf_slots"])], np.uint8)
    mp_pos = np.stack([pts[p]["pos"] for p in mp_ids]).astype(np.float32) if mp_ids else np.zeros((0, 3), np.float32)
    e_mp, e_kf, e_obs, e_w = [], [], [], []
    for i, p in enumerate(mp_ids):                                     # :1155-1199
        for s, f in by_key(p):
            if not ok(s):
                continue
            kp = kfs[s]["keys"][f]
            sc = kfs[s]["sf"][int(kp["octave"])]
            e_mp.append(i); e_kf.append(index[s]); e_obs.append((kp["x"], kp["y"]))
            e_w.append(np.float32(1.0) / (sc * sc))                    # mvInvLevelSigma2 = 1.0f / (mvScaleFactors^2), float arithmetic
            res["edges"].append((s, p, f))
    res["args"] = (kf_pose, kf_fixed, mp_pos, np.array(e_mp, np.int32), np.array(e_kf, np.int32), np.array(e_obs, np.float32).reshape(-1, 2),
                   np.array(e_w, np.float32), scene.K4.copy())
    return res


def flatten(scene, cur, neigh, init):
    """The arguments of Optimizer.LocalBundleAdjustment for the window (None where the reference returns at :1057-1060)."""
    return window(scene, cur, neigh, init)["args"]


# ---- into a store -----------------------------------------------------------------------------------------------------------------------
def centre_of(pose7):
    q = pose7[:4].astype(np.float64)
    R = quat_rotate(q / np.linalg.norm(q), np.zeros((1, 3)))[1]
    return (-R.T @ pose7[4:].astype(np.float64)).astype(np.float32)


def set_keyframes(store, scene, slots):
    slots = list(slots)
    kfs = scene.kfs
    store.set_keyframes(slots, [kfs[s]["key"] for s in slots], [kfs[s]["map"] for s in slots], [kfs[s]["bad"] for s in slots],
                        [np.array(kfs[s]["row"], np.int32) for s in slots], [[] for _ in slots], [-1] * len(slots), [[] for _ in slots])


def set_points(store, scene, ids):
    ids = list(ids)
    if ids:
        store.set_point_observations(ids, [scene.pts[p]["bad"] for p in ids], [scene.pts[p]["obs"] for p in ids])


def to_store(scene, device=-1, poses=True):
    from rumi_slam_amd.covis import Covisibility
    from rumi_slam_amd.matcher import FeatureVector, FrameView
    kfs, pts = scene.kfs, scene.pts
    slots, ids = sorted(kfs), sorted(pts)
    store = Covisibility(max(slots) + 1, max(ids) + 1, device=device)
    set_keyframes(store, scene, slots)
    for s in slots:
        store.set_keyframe_features(s, FrameView(kfs[s]["keys"], np.zeros((len(kfs[s]["keys"]), 32), np.uint8), 640, 480, kfs[s]["sf"]), FeatureVector({}), scene.K4)
    set_points(store, scene, ids)
    n = len(ids)
    store.set_point_attributes(ids, np.stack([pts[p]["pos"] for p in ids]), np.tile(np.array([0, 0, 1], np.float32), (n, 1)), np.full(n, 0.5, np.float32),
                               np.full(n, 40.0, np.float32), np.zeros((n, 32), np.uint8))
    with_map = [p for p in ids if pts[p]["map"] is not None]
    store.set_point_maps(with_map, [pts[p]["map"] for p in with_map])
    store.set_point_reference([p for p in ids if pts[p]["obs"]], [pts[p]["obs"][0][0] for p in ids if pts[p]["obs"]])
    if poses:
        posed = [s for s in slots if kfs[s]["has_pose"]]
        store.set_keyframe_poses(posed, np.stack([kfs[s]["pose7"] for s in posed]))
        store.set_keyframe_centres(posed, np.stack([centre_of(kfs[s]["pose7"]) for s in posed]))
    return store


# ---- the scenes; every `expect` is written from the construction, not computed by window() ---------------------------------------------------
def _case(scene, cur, neigh, init, **expect):
    return dict(scene=scene, cur=cur, neigh=list(neigh), init=init, expect=expect)


def point_order(with_map=True, mismatch=False, fixed_pose=True):
    """Scene 1.  Locals: 2 (current), 0, 1 in this order; 3 and 4 see local points from outside.  24 features a key-frame, key = 10 (slot + 1).
    Point 20 lies at feature 20 of the first local row (slot 2) and at feature 0 of the third (slot 1): it is listed once, where the first row
    has it.  Points 8..11 lie in two local rows.  The first row holds no point at feature 3, a bad point (30) at 5, a point of map 7 (31) at 7."""
    S = Scene(1)
    for s in range(5):
        S.add_kf(s, 10 * (s + 1), 24, has_pose=fixed_pose or s != 3)
    for p in list(range(21)) + [30, 31]:
        S.add_point(p, map_id=7 if p == 31 else 0, bad=p == 30)
    if not with_map:
        S.pts[0]["map"] = None                                         # a live point of one local row only
    first = {0: 0, 1: 1, 2: 2, 4: 4, 5: 30, 6: 6, 7: 31, 8: 8, 9: 9, 10: 10, 11: 11, 20: 20}      # feature -> point of slot 2; 3 stays empty
    for f, p in first.items():
        S.observe(2, f, p)
    for f, p in enumerate([8, 9, 10, 11, 12, 13, 14, 15]):
        S.observe(0, f, p)
    for f, p in enumerate([20, 12, 13, 16, 17, 18, 19]):
        S.observe(1, f, p)
    listed = [0, 1, 2, 4, 6, 8, 9, 10, 11, 20, 12, 13, 14, 15, 16, 17, 18, 19]
    for f, p in enumerate(listed):
        S.observe(3, f, p)
    for f, p in enumerate(listed[::2]):
        S.observe(4, f, p)
    if mismatch:                                                       # point 3 claims feature 2 of slot 0, whose row holds point 10 there
        S.observe(2, 3, 3)
        S.pts[3]["obs"].append((0, 2))
    n_edges = 12 - 2 + 8 + 7 + 18 + 9                                  # every observation made above, less those of points 30 and 31
    return _case(S, 2, [0, 1], -1, kf_slots=[2, 0, 1, 3, 4], num_OptKF=3, num_fixedKF=2, mp_ids=listed, n_edges=n_edges,
                 first_edges=[(2, 0, 0), (3, 0, 0), (4, 0, 0), (2, 1, 1), (3, 1, 1)])


def key_order():
    """Scene 2.  Slots ascend while order_keys descend (key = 100 - 10 slot); the observer rows are given shuffled.  Locals: 0 (current), 1;
    neighbour 5 is bad: neither local nor fixed, though it sees point 1.  Point 0 is seen from outside by 3, by 6 (bad) and by 7 (map 9);
    point 1 by 4 and 2; every later point by 2, 3 and 4.  In key order the walk meets 3 at point 0, then 4 (key 60) before 2 (key 80) at
    point 1: lFixedCameras = 3, 4, 2, which is neither slot order nor key order."""
    S = Scene(2)
    for s in range(8):
        S.add_kf(s, 100 - 10 * s, 40, map_id=9 if s == 7 else 0, bad=s in (5, 6))
    for p in range(40):
        S.add_point(p)
        S.observe(0, p, p)
        S.observe(1, 39 - p, p)
    for s in (3, 6, 7):
        S.observe(s, 0, 0)
    for s in (4, 2, 5):
        S.observe(s, 1, 1)
    for p in range(2, 40):
        for s in (2, 3, 4):
            S.observe(s, p, p)
    S.shuffle_observers()
    # edges of point 1 in key order: 4 (60), 2 (80), 1 (90), 0 (100); of point 0: 3 (70), 1 (90), 0 (100)
    return _case(S, 0, [1, 5], -1, kf_slots=[0, 1, 3, 4, 2], num_OptKF=2, num_fixedKF=3, mp_ids=list(range(40)), n_edges=3 + 4 + 38 * 5,
                 first_edges=[(3, 0, 0), (1, 0, 39), (0, 0, 0), (4, 1, 1), (2, 1, 1), (1, 1, 38), (0, 1, 1), (4, 2, 2), (3, 2, 2), (2, 2, 2), (1, 2, 37), (0, 2, 2)])


def fixed_count(outside=True, init=1):
    """Scene 3.  Four locals (0 current; 1, 2, 3), 32 features each, 48 points seen by three of them each; with `outside` slot 4 sees the
    first 24 points too.  init = 1 is local: a fixed vertex, num_fixedKF = 1 + the fixed cameras.  Without slot 4 and with init = -1 the
    window has no fixed key-frame."""
    S = Scene(3)
    for s in range(5):
        S.add_kf(s, 7 + 3 * s, 36)
    for p in range(48):
        S.add_point(p)
    used = {s: 0 for s in range(5)}
    for p in range(48):
        for s in [(p + j) % 4 for j in range(3)]:
            S.observe(s, used[s], p); used[s] += 1
    if outside:
        for p in range(24):
            S.observe(4, p, p)
    # rows in feature order: slot 0 holds 0, 2, 3, 4, 6, 7, 8, ...; the list walks slot 0, then what slots 1, 2, 3 add
    row0 = [p for p in range(48) if 0 in [(p + j) % 4 for j in range(3)]]
    rest = [p for p in range(48) if p not in row0]
    return _case(S, 0, [1, 2, 3], init, kf_slots=[0, 1, 2, 3] + ([4] if outside else []), num_OptKF=4,
                 num_fixedKF=(1 if init >= 0 else 0) + (1 if outside else 0), mp_ids=row0 + rest, n_edges=48 * 3 + (24 if outside else 0),
                 aborted=not outside and init < 0)


def seams(n_edges):
    """Scene 4, with 257 or 513 edges.  Locals 0 (current) and 1; fixed cameras 2, 3 and the seventy eight-feature key-frames 10..79.
    Point 0 has one observer (slot 0).  Point 1 has 72: the locals and all seventy small key-frames, a row longer than a wave.  Sixty points
    (2..61) are seen by 0, 1 and 2, point 62 also by slot 10: 1 + 72 + 180 + 4 = 257 edges over 63 points.  The larger window adds 64
    points seen by 0, 1, 2 and 3: 513 edges over 127 points.  Three observations of slot 2 (points 2, 3, 4; octave 0) lie 12 px off."""
    assert n_edges in (257, 513)
    S = Scene(4)
    nf = 64 if n_edges == 257 else 128
    for s in range(4):
        S.add_kf(s, 1000 + s, nf)
    for s in range(10, 80):
        S.add_kf(s, 5000 - s, 8)                                       # keys descend with the slot
    n_pts = 63 if n_edges == 257 else 127
    for p in range(n_pts):
        S.add_point(p)
    S.observe(0, 0, 0)
    S.observe(0, 1, 1); S.observe(1, 1, 1)
    for s in range(10, 80):
        S.observe(s, 0, 1)
    for p in range(2, 63):
        S.observe(0, p, p); S.observe(1, p, p)
        S.observe(2, p, p, shift=12.0 if p in (2, 3, 4) else 0.0, octave=0 if p in (2, 3, 4) else None)
    S.observe(10, 1, 62)
    for p in range(63, n_pts):
        for s in range(4):
            S.observe(s, p, p)
    S.shuffle_observers()
    # first appearance: point 1 brings the small key-frames in key order (79 has the smallest key, 4921), then point 2 brings slot 2
    fixed = list(range(79, 9, -1)) + [2] + ([3] if n_edges == 513 else [])
    return _case(S, 0, [1], -1, kf_slots=[0, 1] + fixed, num_OptKF=2, num_fixedKF=len(fixed), mp_ids=list(range(n_pts)), n_edges=n_edges,
                 first_edges=[(0, 0, 0), (0, 1, 1), (1, 1, 1)] + [(s, 1, 0) for s in range(79, 9, -1)] + [(0, 2, 2), (1, 2, 2), (2, 2, 2)])


def other_path():
    """Scene 6.  Thirty local key-frames of eight features: 30 optimised, one more than the tile solver takes.  Sixty points, four local
    observers each; slot 30 (64 features) sees them all from outside."""
    S = Scene(6)
    for s in range(30):
        S.add_kf(s, 11 + s, 8)
    S.add_kf(30, 5, 64)
    for p in range(60):
        S.add_point(p)
    for s in range(30):
        for f in range(8):
            S.observe(s, f, (2 * s + f) % 60)
    for p in range(60):
        S.observe(30, p, p)
    mp_ids = list(range(8))
    for s in range(1, 30):
        mp_ids += [p for p in ((2 * s + f) % 60 for f in range(8)) if p not in mp_ids]
    return _case(S, 0, list(range(1, 30)), -1, kf_slots=list(range(31)), num_OptKF=30, num_fixedKF=1, mp_ids=mp_ids, n_edges=240 + 60,
                 first_edges=[(30, 0, 0), (0, 0, 0), (27, 0, 6), (28, 0, 4), (29, 0, 2)])


ALL = {"point_order": point_order, "key_order": key_order, "fixed_count": fixed_count, "fixed_count_init_only": lambda: fixed_count(outside=False),
       "seams_257": lambda: seams(257), "seams_513": lambda: seams(513), "other_path": other_path}
