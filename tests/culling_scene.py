"""Synthetic maps for the tests of rumi_keyframe_culling (include/rumi_mapping.h), and the binding of their C++ oracle
(tests/cpp/culling_oracle.cc).  TEST INFRASTRUCTURE.

Key-frames stand along a trajectory; a map point is observed by key-frames of a window around its place, one free feature slot each, so the
map is consistent (mp[i] = p exactly when p lists (key-frame, i)) and every point's n_obs_count equals the length of its list.  `Rich`
key-frames hold mostly points with five or more observers at coarse octaves, so the loop finds them redundant; they come in runs, so that an
early cull takes observers away from the points of a later one (culled -> kept), and a share of their points has exactly three observers,
two of them rich, so that an early cull turns points bad and shrinks a later key-frame's nMPs (kept -> culled).  The "pointer order" of a
point's observations is a random permutation of the key-frame indices, fixed per scene.  The knobs: init / bad / cloud / not_erase
candidates, points bad at the call, points of exactly 3 and 4 observations, observers one and two octaves above the candidate's, a key-frame
without points, more than 100 candidates, more than 20 with abort_ba, an empty candidate list."""
import ctypes as C
import os
import subprocess

import numpy as np

from rumi_slam_amd.mapping import CULL_ABORT_BA, CULL_CLOUD, CullBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (seed, candidates, abort_ba).  Chosen on the CPU (tests/test_culling_cpu.py::test_committed_seeds_cover_every_branch states what they
# must show between them).
SCENES = [(0, 30, False), (1, 45, True), (1, 118, False), (2, 60, False), (0, 26, True), (17, 0, False)]


class CullScene:
    def __init__(self, seed, n_cand=30, abort_ba=False, nfeat=(90, 150), n_extra=8, rich_frac=0.5, flags=True):
        rng = np.random.default_rng(7000 + seed)
        self.seed, self.abort_ba = seed, abort_ba
        n_kf = self.n_kf = n_cand + n_extra
        self.n = rng.integers(nfeat[0], nfeat[1] + 1, n_kf)
        self.rich = np.zeros(n_kf, bool)
        t = 0
        while t < n_kf:                                            # runs of rich key-frames
            run = int(rng.integers(2, 6))
            if rng.random() < rich_frac:
                self.rich[t:t + run] = True
            t += run
        self.bias = np.where(self.rich, rng.integers(3, 6, n_kf), rng.integers(0, 4, n_kf))
        self.octave = [np.clip(self.bias[k] + rng.integers(-1, 2, self.n[k]), 0, 7).astype(np.int32) for k in range(n_kf)]
        self.mp = [np.full(self.n[k], -1, np.int32) for k in range(n_kf)]
        self.kf_bad, self.kf_init = np.zeros(n_kf, bool), np.zeros(n_kf, bool)
        self.not_erase, self.cloud = np.zeros(n_kf, bool), np.zeros(n_kf, bool)
        self.ptr_rank = rng.permutation(n_kf)                      # the order std::map<KeyFrame*, ...> would iterate in
        self.empty_kf = int(rng.integers(0, n_kf)) if n_kf else -1  # a key-frame no point lands on
        free = [list(rng.permutation(int(self.n[k]))) for k in range(n_kf)]
        self.points = []                                           # [is_bad, n_obs_count, [(kf, feature), ...]]

        def add(kfs):
            obs = []
            for k in sorted({int(k) for k in kfs}, key=lambda k: self.ptr_rank[k]):
                if k == self.empty_kf or len(free[k]) <= 2:
                    continue
                f = int(free[k].pop())
                self.mp[k][f] = len(self.points)
                obs.append((k, f))
            self.points.append([False, len(obs), obs])

        def window(t0, m, w, avoid_rich):
            lo, hi = max(0, t0 - w), min(n_kf, t0 + w + 1)
            pool = [k for k in range(lo, hi) if not (avoid_rich and self.rich[k] and rng.random() < 0.8)]
            return rng.choice(pool, min(m, len(pool)), replace=False) if pool else []

        if n_kf:
            total = int(self.n.sum())
            for _ in range(total // 9):                            # strong points
                add(window(int(rng.integers(0, n_kf)), int(rng.integers(5, 11)), 7, False))
            for _ in range(total // 30):                           # weak points: 2, 3 or 4 observers, mostly on ordinary key-frames
                add(window(int(rng.integers(0, n_kf)), int(rng.choice([2, 3, 3, 4, 4])), 4, True))
            rich = np.nonzero(self.rich)[0]
            for a, b in zip(rich, rich[1:]):                       # three observers, two of them neighbouring rich key-frames
                if b - a <= 2 and rng.random() < 0.7:
                    others = [k for k in range(max(0, a - 5), min(n_kf, b + 6)) if k not in (a, b)]
                    for _ in range(int(rng.integers(4, 14))):
                        add([a, b, int(rng.choice(others))])
            for i in rng.choice(len(self.points), max(1, len(self.points) // 60), replace=False):
                self.points[int(i)][0] = True                      # bad at the call, the lists still there
        self.cand = [int(k) for k in rng.permutation(n_kf)[:n_cand]]
        if flags and n_cand >= 8:
            c = list(rng.permutation(self.cand))
            self.kf_init[c[0]] = True
            self.kf_bad[c[1:3]] = True
            self.cloud[c[3:5]] = True
            self.cloud[[k for k in c[5:] if self.rich[k]][:1]] = True            # a cloud key-frame the plain variant culls or keeps
            self.not_erase[[k for k in c[5:] if self.rich[k] and not self.cloud[k]][:2]] = True
            self.not_erase[c[7]] = True
            if n_cand > 101:                                       # skipped candidates around the break: the break test sits behind `continue`
                self.kf_bad[self.cand[100]] = True
                self.cloud[self.cand[101]] = True
            if abort_ba and n_cand > 22:
                self.kf_bad[self.cand[20]] = True

    def keyframes(self, mp=None):
        mp = self.mp if mp is None else mp
        return [(self.octave[k], mp[k], self.kf_bad[k], self.kf_init[k], self.not_erase[k], self.cloud[k]) for k in range(self.n_kf)]

    def batch(self, order=None, shuffle_obs=None):
        """order: a permutation of the points (new position i holds old point order[i]); shuffle_obs: a seed to permute every list."""
        if order is None and shuffle_obs is None:
            return CullBatch(self.keyframes(), self.cand, [tuple(p) for p in self.points])
        order = np.arange(len(self.points)) if order is None else np.asarray(order)
        new_of = np.empty(len(order) + 1, np.int32)
        new_of[order] = np.arange(len(order))
        new_of[-1] = -1                                            # mp = -1 stays
        mp = [new_of[m] for m in self.mp]
        rng = np.random.default_rng(shuffle_obs)
        pts = []
        for i in order:
            bad, n, obs = self.points[int(i)]
            pts.append((bad, n, [obs[j] for j in rng.permutation(len(obs))] if shuffle_obs is not None else obs))
        return CullBatch(self.keyframes(mp), self.cand, pts)

    def flags(self, cloud):
        return (CULL_CLOUD if cloud else 0) | (CULL_ABORT_BA if self.abort_ba else 0)


def probe_batch(n_cand, n_feat, obs_range, seed=0, n_extra=40, n_rich=6):
    """The workloads of tools/culling_probe.py: n_cand candidates of n_feat features, obs_range observers a point.  Up to four observers of a
    point see it at octave 0 and the others at 2..6, so an ordinary key-frame keeps a share of slots nobody else covers and stays; n_rich
    key-frames see everything at octave 7 and are what the loop culls."""
    rng = np.random.default_rng(seed)
    n_kf = n_cand + n_extra
    octave = [np.zeros(n_feat, np.int32) for _ in range(n_kf)]
    rich = set(int(k) for k in rng.choice(n_kf, min(n_rich, n_kf), replace=False))
    mp = [np.full(n_feat, -1, np.int32) for _ in range(n_kf)]
    used = np.zeros(n_kf, np.int64)
    points = []
    mean = (obs_range[0] + obs_range[1]) / 2
    for _ in range(int(1.3 * n_kf * n_feat / mean)):               # a fixed number of attempts: the last slots of a key-frame may stay free
        m = int(rng.integers(obs_range[0], obs_range[1] + 1))
        t0 = int(rng.integers(0, n_kf))
        pool = [k for k in range(max(0, t0 - m), min(n_kf, t0 + m + 1)) if used[k] < n_feat]
        if len(pool) < obs_range[0]:
            continue
        obs = []
        fine = min(4, max(1, round(0.3 * m)))
        for j, k in enumerate(rng.choice(pool, min(m, len(pool)), replace=False)):
            k = int(k)
            mp[k][used[k]] = len(points)
            octave[k][used[k]] = 7 if k in rich else 0 if j < fine else int(rng.integers(2, 7))
            obs.append((k, int(used[k])))
            used[k] += 1
        points.append((False, len(obs), obs))
    kfs = [(octave[k], mp[k], False, False, False, False) for k in range(n_kf)]
    cand = [int(k) for k in rng.permutation(n_kf)[:n_cand]]
    return CullBatch(kfs, cand, points)


def small_batch():
    """Four key-frames of three features, two points: the base of the malformed inputs."""
    octv = np.zeros(3, np.int32)
    mp = [np.array([0, 1, -1], np.int32), np.array([0, -1, 1], np.int32), np.array([-1, 0, 1], np.int32), np.array([0, -1, -1], np.int32)]
    pts = [(False, 4, [(0, 0), (1, 0), (2, 1), (3, 0)]), (False, 3, [(0, 1), (1, 2), (2, 2)])]
    return CullBatch([(octv, m, False, False, False, False) for m in mp], [2, 0, 1], pts)


def capacity_batch(n_obs):
    """One point observed by n_obs key-frames of one feature each."""
    one, zero = np.zeros(1, np.int32), np.zeros(1, np.int32)
    return CullBatch([(one, zero, False, False, False, False)] * n_obs, [0, 1], [(False, n_obs, [(k, 0) for k in range(n_obs)])])


# ---- the C++ oracle ----
def build_oracle(out_dir):
    so = os.path.join(str(out_dir), "libculling_oracle.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "culling_oracle.cc"), "-o", so])
    L = C.CDLL(so)
    vp, i32 = C.c_void_p, C.c_int32
    L.cuo_keyframe_culling.argtypes = [vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    return L


def run_oracle(L, batch, flags, fill=0, state=False):
    """The oracle's outputs over arrays that held ``fill`` in every byte; with ``state`` also the map it leaves: kf_bad, kf_to_be_erased,
    pt_bad, pt_nobs, obs_in_map, mp_after (one array per key-frame)."""
    from rumi_slam_amd import capi
    out = batch.outputs(fill)
    extra = [None] * 6
    if state:
        sizes = [batch.kf[k].n for k in range(batch.n_kf)]
        st = dict(kf_bad=np.zeros(max(batch.n_kf, 1), np.uint8), kf_to_be_erased=np.zeros(max(batch.n_kf, 1), np.uint8),
                  pt_bad=np.zeros(max(batch.n_pts, 1), np.uint8), pt_nobs=np.zeros(max(batch.n_pts, 1), np.int32),
                  obs_in_map=np.zeros(batch.n_obs + 1, np.uint8), mp_after=np.zeros(sum(sizes) + 1, np.int32))
        extra = [capi.ptr(v) for v in st.values()]
    assert L.cuo_keyframe_culling(*batch.args(flags, out), *extra) == 0
    if not state:
        return out
    st["mp_after"] = np.split(st["mp_after"][:-1], np.cumsum(sizes)[:-1]) if sizes else []
    return out, st


def same_bytes(a, b, keys=None):
    return [k for k in (keys or a.keys()) if a[k].tobytes() != b[k].tobytes()]
