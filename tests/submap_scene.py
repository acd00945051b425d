"""Key-frame pairs for the tests of rumi_submap_match (include/rumi_match.h), and the binding of their C++ oracle (tests/cpp/submap_oracle.cc).
TEST INFRASTRUCTURE.

A scene is a table of frames (mvKeys, mvKeysUn, has-map-point flags, grid origin and inverse cell sizes) and a list of pairs (key-frame 1,
key-frame 2).  Seeded scenes: key-frames 2 hold clustered key-points on a quarter-pixel lattice, so that a query sees several candidates and
equal distances occur; a key-frame 1 is made of shifted copies of its partner's key-points, strangers and planted ties; mvKeysUn is mvKeys plus
a smooth radial shift of up to about two pixels, so the gate and the distance read different points; one key-frame 2 serves several pairs.
The constructed cases hold one rule each; tests/test_submap_cpu.py asserts the conditions each depends on and that a wrong restatement of the
rule gives another answer."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 3.0
SEEDS = [0, 1, 2]


def grid_inv(min_x, min_y, max_x, max_y):
    return (np.float32(64) / np.float32(np.float32(max_x) - np.float32(min_x)), np.float32(48) / np.float32(np.float32(max_y) - np.float32(min_y)))


class Frame:
    def __init__(self, keys, mp, un=None, bounds=(0, 0, 640, 480)):
        self.keys = np.ascontiguousarray(keys, np.float32).reshape(-1, 2)
        self.un = self.keys.copy() if un is None else np.ascontiguousarray(un, np.float32).reshape(-1, 2)
        self.mp = np.ascontiguousarray(mp, np.uint8).reshape(-1)
        assert len(self.keys) == len(self.un) == len(self.mp)
        self.bounds = tuple(float(b) for b in bounds)
        self.min_x, self.min_y = np.float32(bounds[0]), np.float32(bounds[1])
        self.w_inv, self.h_inv = grid_inv(*bounds)

    @property
    def n(self):
        return len(self.keys)


class Scene:
    def __init__(self, frames, pairs, name=""):
        self.frames, self.pairs, self.name = frames, [(int(a), int(b)) for a, b in pairs], name

    def only(self, p):
        """The same table with pair p alone."""
        return Scene(self.frames, [self.pairs[p]], f"{self.name}/pair{p}")

    def q_start(self):
        return np.concatenate([[0], np.cumsum([self.frames[a].n for a, _ in self.pairs])]).astype(np.int64)


def _undistort(keys, bounds, k):
    """A smooth radial shift about the image centre, up to about two pixels in the corners."""
    c = np.array([(bounds[0] + bounds[2]) / 2, (bounds[1] + bounds[3]) / 2], np.float64)
    d = keys.astype(np.float64) - c
    r2 = (d ** 2).sum(1, keepdims=True) / (400.0 ** 2)
    return (c + d * (1 + k * r2)).astype(np.float32)


def _lattice(rng, n, lo, hi):
    return (rng.integers(int(lo * 4), int(hi * 4), n) / 4.0).astype(np.float32)


def seeded_frames(rng, n2, n1, bounds, k):
    """One key-frame 2 and a key-frame 1 that sees it again."""
    nc = max(n2 // 3, 1)
    cx, cy = _lattice(rng, nc, 4, 636), _lattice(rng, nc, 4, 476)
    which = rng.integers(0, nc, n2)
    k2 = np.stack([cx[which] + rng.integers(-8, 9, n2) / 4.0, cy[which] + rng.integers(-8, 9, n2) / 4.0], 1).astype(np.float32)
    f2 = Frame(k2, rng.random(n2) < 0.75, _undistort(k2, bounds, k), bounds)
    return f2, seeded_partner(rng, f2, n1, bounds, k)


def seeded_partner(rng, f2, n1, bounds, k):
    k1 = np.empty((n1, 2), np.float32)
    for i in range(n1):
        t = rng.random()
        if f2.n and t < 0.7:                                       # a key-point of the partner, shifted by up to 2.5 pixels
            k1[i] = f2.keys[rng.integers(0, f2.n)] + rng.integers(-10, 11, 2) / 4.0
        else:
            k1[i] = [_lattice(rng, 1, 0, 640)[0], _lattice(rng, 1, 0, 480)[0]]
    f1 = Frame(k1, rng.random(n1) < 0.75, _undistort(k1, bounds, k), bounds)
    return f1


def plant_tie(rng, f1, f2, at):
    """Two key-points of f2 with map points at the same distance from a query with a map point, far from everything else.  In place."""
    i1 = int(rng.integers(0, f1.n))
    i2 = rng.choice(f2.n, 2, replace=False)
    f1.keys[i1] = f1.un[i1] = at
    f2.keys[i2[0]] = f2.un[i2[0]] = (at[0] + 1.25, at[1] - 0.5)
    f2.keys[i2[1]] = f2.un[i2[1]] = (at[0] - 1.25, at[1] + 0.5)
    f1.mp[i1] = 1
    f2.mp[i2] = 1


def seeded_scene(seed, n_pairs=6, n_range=(150, 400)):
    rng = np.random.default_rng(9100 + seed)
    bounds = [(0, 0, 640, 480), (-9, -7, 651, 489), (-14, -11, 655, 492)][seed % 3]
    k = [0.0, 0.004, -0.005][seed % 3] if seed else 0.003
    frames, pairs = [], []
    for p in range(n_pairs):
        n2, n1 = (int(v) for v in rng.integers(n_range[0], n_range[1] + 1, 2))
        if p in (2, 4) and frames:                                 # key-frame 2 of the first pair again
            f2i = 0
            f1 = seeded_partner(rng, frames[0], n1, bounds, k)
        else:
            f2, f1 = seeded_frames(rng, n2, n1, bounds, k)
            frames.append(f2)
            f2i = len(frames) - 1
        frames.append(f1)
        pairs.append((len(frames) - 1, f2i))
    plant_tie(rng, frames[pairs[1][0]], frames[pairs[1][1]], (333.0 + seed, 222.0))
    return Scene(frames, pairs, f"seed{seed}")


# ---- constructed cases: bounds 0 0 640 480, cells of ten pixels; cell k of a row covers [10 k - 5, 10 k + 5) -------------------------------------
def _fill(extra=6, at=(600, 440)):
    """Key-points far from every case's query, all with map points."""
    return [(at[0] + 3.5 * j, at[1]) for j in range(extra)]


def case_tie_order():
    """Two candidates at distance 1.5.  Query 0 at x = 15: candidate 0 lies in column 2, candidate 1 in column 1, which is walked first, so the
    larger index wins.  Query 1 at x = 20: candidates 2 and 3 share a cell, the lower index wins."""
    k1 = [(15, 20), (20, 60)] + _fill()
    k2 = [(16.5, 20), (13.5, 20), (21.5, 60), (18.5, 60)] + _fill()
    return Scene([Frame(k1, np.ones(len(k1))), Frame(k2, np.ones(len(k2)))], [(0, 1)], "tie_order"), {0: 1, 1: 2}


BELOW3 = float(np.nextafter(np.float32(3), np.float32(0)))


def case_thresholds():
    """Query 0: the candidate's raw point is at distance exactly 3 while its undistorted point passes the gate: rejected.  Query 1 at x = 0: a
    candidate at the largest float below 3: accepted.  Query 2: candidate 2 in the corner of the gate (2.5, 2.5) is at 3.54: rejected, candidate 3
    behind it in the list at (1, 2) is kept."""
    k1 = [(100, 100), (0, 200), (200, 300)] + _fill()
    k2 = [(103, 100), (BELOW3, 200), (202.5, 302.5), (201, 302)] + _fill()
    un2 = [(102.5, 100), (BELOW3, 200), (202.5, 302.5), (201, 302)] + _fill()
    return Scene([Frame(k1, np.ones(len(k1))), Frame(k2, np.ones(len(k2)), un2)], [(0, 1)], "thresholds"), {0: -1, 1: 1, 2: 3}


def case_gate_vs_distance():
    """Query 0 at (300, 300).  Candidate 0: undistorted inside the gate, raw at distance 4: rejected.  Candidate 1: raw at 1.41, undistorted
    outside the gate: never seen.  Candidate 2: raw at 0.5, undistorted three columns away: its cell is not visited.  Candidate 3 at 2: kept."""
    k1 = [(300, 300)] + _fill()
    k2 = [(304, 300), (301, 301), (300.5, 300), (302, 300)] + _fill()
    un2 = [(301, 300), (304, 301), (330, 300), (302, 300)] + _fill()
    return Scene([Frame(k1, np.ones(len(k1))), Frame(k2, np.ones(len(k2)), un2)], [(0, 1)], "gate_vs_distance"), {0: 3}


def case_null_slots():
    """Query 0: the nearest candidate (0) holds no map point, the farther one (1) does and is kept.  Query 1 holds no map point itself."""
    k1 = [(400, 100), (420, 140)] + _fill()
    k2 = [(400.5, 100), (402, 100), (421, 140)] + _fill()
    mp1, mp2 = np.ones(len(k1)), np.ones(len(k2))
    mp1[1] = 0
    mp2[0] = 0
    return Scene([Frame(k1, mp1), Frame(k2, mp2)], [(0, 1)], "null_slots"), {0: 1, 1: -1}


def case_many_to_one():
    k1 = [(500, 300), (501, 300)] + _fill()
    k2 = [(500.5, 300)] + _fill()
    return Scene([Frame(k1, np.ones(len(k1))), Frame(k2, np.ones(len(k2)))], [(0, 1)], "many_to_one"), {0: 0, 1: 0}


EDGE_BOUNDS = [(-12, -9, 652, 489), (8, 6, 632, 474)]


def case_grid_edges(which):
    """A negative (0) and a positive (1) grid origin.  Queries 0-3 leave by the four early returns (right, left, below, above); 4-7 have their window
    clipped at the left, right, top and bottom side and keep candidates 0-3; 8 and 9 stand next to key-points that PosInGrid drops (4: beyond the
    last column, 5: before the first) and keep nothing."""
    x0, y0, x1, y1 = EDGE_BOUNDS[which]
    cw, ch = (x1 - x0) / 64.0, (y1 - y0) / 48.0
    xm, ym = (x0 + x1) / 2.0, (y0 + y1) / 2.0
    k1 = [(x1 + 12, ym), (x0 - 20, ym), (xm, y1 + 12), (xm, y0 - 20),
          (x0 + 1, ym), (x0 + 63.2 * cw, ym + 30), (xm + 30, y0 + 1), (xm + 60, y0 + 47.2 * ch),
          (x1 - 2, ym - 40), (x0 - 0.5 * cw - 1, ym - 60)]
    k2 = [(x0 + 2, ym), (x0 + 63.1 * cw, ym + 30), (xm + 30, y0 + 2), (xm + 60, y0 + 47.1 * ch),
          (x1 - 1, ym - 40), (x0 - 0.5 * cw - 2, ym - 60)]
    k1 += _fill(at=(xm, ym + 100))
    k2 += _fill(at=(xm, ym + 100))
    sc = Scene([Frame(k1, np.ones(len(k1)), bounds=EDGE_BOUNDS[which]), Frame(k2, np.ones(len(k2)), bounds=EDGE_BOUNDS[which])], [(0, 1)], f"grid_edges{which}")
    return sc, {0: -1, 1: -1, 2: -1, 3: -1, 4: 0, 5: 1, 6: 2, 7: 3, 8: -1, 9: -1}


# Found by search on the CPU.  The rule: draw dx, dy as multiples of 2^-17 in (-3, 3) (so that 64 - dx is a float and the float subtraction
# 64 - (64 - dx) returns dx); d64 = float32(sqrt(float64(dx)^2 + float64(dy)^2)) is the reference's expression, d32 = sqrt(dx * dx + dy * dy) all in
# float32.  Take two draws A, B with d64(A) == d64(B) and d32(A) > d32(B): with A in front of B in the candidate list, the reference keeps A (B is
# not strictly nearer) and a float-only distance keeps B.
DOUBLE_A = (0.32921600341796875, -0.9442825317382812)          # d64 = d32 = 1.0000263452529907
DOUBLE_B = (-0.98137664794921875, -0.192230224609375)          # d64 = 1.0000263452529907, d32 = 1.0000262260437012


def case_double_distance():
    k1 = [(64, 64)] + _fill()
    k2 = [(64 - DOUBLE_A[0], 64 - DOUBLE_A[1]), (64 - DOUBLE_B[0], 64 - DOUBLE_B[1])] + _fill()
    return Scene([Frame(k1, np.ones(len(k1))), Frame(k2, np.ones(len(k2)))], [(0, 1)], "double_distance"), {0: 0}


def constructed_cases():
    """(scene, {query of pair 0: the key-point it must keep})."""
    return [case_tie_order(), case_thresholds(), case_gate_vs_distance(), case_null_slots(), case_many_to_one(), case_grid_edges(0), case_grid_edges(1),
            case_double_distance()]


def sizes_scene():
    """Key-frames 1 of 0, 1, 63, 64, 65 and 2000 key-points in one call; key-frame 2 number 0 serves three pairs; one key-frame 2 is empty."""
    rng = np.random.default_rng(77)
    b = (0, 0, 640, 480)
    f2a, _ = seeded_frames(rng, 300, 1, b, 0.003)
    f2b, _ = seeded_frames(rng, 2000, 1, b, 0.003)
    empty = Frame(np.zeros((0, 2)), np.zeros(0), bounds=b)
    frames = [f2a, f2b, empty]
    pairs = []
    for n1, f2i in [(0, 0), (1, 0), (63, 0), (64, 1), (65, 1), (2000, 1), (70, 2)]:
        frames.append(seeded_partner(rng, frames[f2i], n1, b, 0.003) if n1 else Frame(np.zeros((0, 2)), np.zeros(0), bounds=b))
        pairs.append((len(frames) - 1, f2i))
    return Scene(frames, pairs, "sizes")


def batch40_scene():
    return seeded_scene(40, n_pairs=40, n_range=(60, 300))


def probe_scene(n_pairs=40, n=2000, seed=0):
    """The shape of tools/submap_match_probe.py: n_pairs pairs of n key-points, every pair its own two frames."""
    rng = np.random.default_rng(seed)
    frames, pairs = [], []
    for p in range(n_pairs):
        f2, f1 = seeded_frames(rng, n, n, (0, 0, 640, 480), 0.003)
        frames += [f1, f2]
        pairs.append((2 * p, 2 * p + 1))
    return Scene(frames, pairs, f"probe{n_pairs}x{n}")


# ---- the device side of a scene ----
def device_frames(scene, on_device=False):
    from rumi_slam_amd.submap import SubmapFrame
    out = []
    for f in scene.frames:
        gi = (float(f.w_inv), float(f.h_inv))
        if on_device:
            import torch
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            out.append(SubmapFrame(t(f.keys), t(f.mp), t(f.un), float(f.min_x), float(f.min_y), grid_inv=gi))
        else:
            out.append(SubmapFrame(f.keys, f.mp, f.un, float(f.min_x), float(f.min_y), grid_inv=gi))
    return out


# ---- the C++ oracle ----
def build_oracle(out_dir):
    so = os.path.join(str(out_dir), "libsubmap_oracle.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "submap_oracle.cc"), "-o", so])
    L = C.CDLL(so)
    vp, i32 = C.c_void_p, C.c_int32
    L.smo_submap_match.argtypes = [i32, vp, vp, vp, vp, vp, i32, vp, vp, C.c_float, vp, vp, vp]
    return L


def oracle_inputs(scene):
    fs = scene.frames
    start = np.concatenate([[0], np.cumsum([f.n for f in fs])]).astype(np.int32)
    cat = lambda xs, shape, dt: np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros(shape, dt), dt)
    keys = cat([f.keys for f in fs] + [np.zeros((1, 2), np.float32)], (1, 2), np.float32)
    un = cat([f.un for f in fs] + [np.zeros((1, 2), np.float32)], (1, 2), np.float32)
    mp = cat([f.mp for f in fs] + [np.zeros(1, np.uint8)], (1,), np.uint8)
    bounds = np.array([[f.min_x, f.min_y, f.w_inv, f.h_inv] for f in fs], np.float32).reshape(-1, 4)
    return start, keys, un, mp, bounds


def run_oracle(L, scene, tol=TOL):
    """(best2 [Q], pair_start [P + 1], matches [k, 2]) as rumi_submap_match returns them."""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    start, keys, un, mp, bounds = oracle_inputs(scene)
    f1 = np.array([a for a, _ in scene.pairs], np.int32)
    f2 = np.array([b for _, b in scene.pairs], np.int32)
    q = int(scene.q_start()[-1])
    best2 = np.full(q + 1, -7, np.int32)
    pair_start = np.full(len(scene.pairs) + 1, -7, np.int32)
    matches = np.full((q + 1, 2), -7, np.int32)
    total = L.smo_submap_match(len(scene.frames), p(start), p(keys), p(un), p(mp), p(bounds), len(scene.pairs), p(f1), p(f2), float(tol),
                               p(best2), p(pair_start), p(matches))
    assert total == pair_start[-1]
    return best2[:q], pair_start, matches[:total]
