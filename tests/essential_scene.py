"""Synthetic Sim3 pose graphs for rumi_essential_graph / rumi_sim3_correct_points and the scalar C++ oracle (tests/cpp/essential_oracle.cc).

A scene is the flattened graph the facade would hand over after a loop closure: key-frames along a closed trajectory whose estimates drift in
rotation, translation and scale, a spanning tree, covisibility edges, old loop edges, and a new loop connection whose far end and neighbours
carry corrected Sim3s.  Measurements are formed as upstream forms them: S_j * S_i^-1 from the non-corrected poses for ordinary edges, from
the corrected ones for the new loop connection (Optimizer.cc:1425-1547), with vertex 0 = i and vertex 1 = j."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- Sim3 as (qx qy qz qw tx ty tz s), numpy ----
def qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def qrot(q, v):
    u = q[:3]
    uv = 2.0 * np.cross(u, v)
    return v + q[3] * uv + np.cross(u, uv)


def smul(A, B):
    return np.concatenate([qmul(A[:4], B[:4]), A[7] * qrot(A[:4], B[4:7]) + A[4:7], [A[7] * B[7]]])


def sinv(A):
    c = np.array([-A[0], -A[1], -A[2], A[3]])
    return np.concatenate([c, qrot(c, -A[4:7] / A[7]), [1.0 / A[7]]])


def smap(A, p):
    return A[7] * qrot(A[:4], p) + A[4:7]


def sim3(rotvec, t, s=1.0):
    rotvec = np.asarray(rotvec, float)
    th = np.linalg.norm(rotvec)
    q = np.array([0, 0, 0, 1.0]) if th < 1e-12 else np.concatenate([rotvec / th * np.sin(th / 2), [np.cos(th / 2)]])
    return np.concatenate([q, np.asarray(t, float), [float(s)]])


class Scene:
    def __init__(self, S, fixed, fix_scale, v0, v1, meas, isolated):
        self.S = np.ascontiguousarray(S, np.float64); self.fixed = np.ascontiguousarray(fixed, np.uint8)
        self.fix_scale = np.ascontiguousarray(fix_scale, np.uint8); self.v0 = np.ascontiguousarray(v0, np.int32)
        self.v1 = np.ascontiguousarray(v1, np.int32); self.meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 8)
        self.isolated = isolated

    @property
    def n_v(self):
        return len(self.S)

    @property
    def n_e(self):
        return len(self.v0)

    def args(self):
        return self.S, self.fixed, self.fix_scale, self.v0, self.v1, self.meas


def make_scene(n_free, seed=0, n_fixed=1, fix_scale="none", isolated=True, dup_share=0.15, merge=False, free_gauge=False, meas_noise=1.0):
    """n_fixed leading fixed key-frames (the map's first one; the merge variant fixes a whole group, which yields fixed-fixed, fixed-free and
    free-free edges), then n_free free ones; with `isolated` one more free vertex without edges sits in the middle of the index range.
    fix_scale: "none", "all", or "some" (every third vertex).  meas_noise scales the measurement noise: with large residuals Gauss-Newton converges
    linearly, which is what lets a run end on the three-bad-iterations rule with every gain ratio still far from zero."""
    rng = np.random.default_rng(seed)
    n = n_fixed + n_free
    # ground truth on a circle, camera-from-world
    truth = []
    for i in range(n):
        a = 2 * np.pi * i / max(n, 8)
        Twc = sim3([0, a, 0.1 * np.sin(a)], [4 * np.cos(a), 0.2 * np.sin(2 * a), 4 * np.sin(a)])
        truth.append(sinv(Twc))
    # drifting odometry: every relative motion picks up a little rotation, translation and scale error
    est = [truth[0].copy()]
    scale = 1.0
    for i in range(1, n):
        rel = smul(truth[i], sinv(truth[i - 1]))
        scale *= np.exp(rng.normal(0, 0.004) + 0.002)
        rel[4:7] *= scale
        noise = sim3(rng.normal(0, 0.002, 3), rng.normal(0, 0.004, 3))
        est.append(smul(noise, smul(rel, est[i - 1])))
    for S in est:
        S[7] = 1.0                                            # key-frame poses are SE(3): g2o::Sim3(R, t, 1.0)
    non_corrected = [S.copy() for S in est]
    # the loop closure: the last key-frame and its two predecessors carry corrected Sim3s (near the truth, with the scale the drift implies)
    n_corr = min(3, n_free) if not merge else 0
    vertex = [S.copy() for S in est]
    for i in range(n - n_corr, n):
        s = 1.0 / scale
        vertex[i] = np.concatenate([truth[i][:4], truth[i][4:7] * s, [s]])
        vertex[i] = smul(sim3(rng.normal(0, 0.001, 3), rng.normal(0, 0.002, 3)), vertex[i])
    if merge:                                                 # merge overload: the fixed group was corrected already (it sits at the truth)
        for i in range(n_fixed):
            vertex[i] = truth[i].copy()
    edges = []                                                # (i, j, measurement)

    def meas_of(i, j, corrected):
        Si = vertex[i] if corrected else non_corrected[i]
        Sj = vertex[j] if corrected else non_corrected[j]
        return smul(sim3(rng.normal(0, 0.02 * meas_noise, 3), rng.normal(0, 0.02 * meas_noise, 3), np.exp(rng.normal(0, 0.01 * meas_noise))), smul(Sj, sinv(Si)))

    # new loop connection: corrected far end and neighbours to the loop key-frame and its neighbours
    for i in range(n - n_corr, n):
        for j in range(0, min(2, n - n_corr)):
            edges.append((i, j, meas_of(i, j, True)))
    for i in range(1, n):                                     # spanning tree: child -> parent
        edges.append((i, i - 1, meas_of(i, i - 1, False)))
    for i in range(n):                                        # covisibility, both orientations
        for d in (2, 3, 5):
            j = i + d
            if j < n and rng.random() < 0.6:
                edges.append((i, j, meas_of(i, j, False)) if rng.random() < 0.5 else (j, i, meas_of(j, i, False)))
    for _ in range(n // 12):                                  # old loop edges
        i, j = sorted(rng.choice(n, 2, replace=False))
        if j - i > 3:
            edges.append((int(j), int(i), meas_of(int(j), int(i), False)))
    for k in range(len(edges)):                               # a share of vertex pairs twice, some of them the other way round
        if rng.random() < dup_share:
            i, j, _ = edges[k]
            edges.append((i, j, meas_of(i, j, False)) if rng.random() < 0.5 else (j, i, meas_of(j, i, False)))
    fixed = np.zeros(n, np.uint8)
    if not free_gauge:
        fixed[:n_fixed] = 1
    idx = np.arange(n)
    iso = None
    if isolated:                                              # one vertex without edges in the middle of the index range
        iso = n // 2
        idx = np.where(idx >= iso, idx + 1, idx)
        vertex.insert(iso, sim3([0.1, 0.2, 0.3], [1, 2, 3], 1.25))
        fixed = np.insert(fixed, iso, 0)
    nv = len(vertex)
    fs = np.zeros(nv, np.uint8)
    if fix_scale == "all":
        fs[:] = 1
    elif fix_scale == "some":
        fs[::3] = 1
    return Scene(np.array(vertex), fixed, fs, [idx[e[0]] for e in edges], [idx[e[1]] for e in edges], np.array([e[2] for e in edges]), iso)


# The committed scenes.  Seeds are picked so that the ORACLE alone finds them non-marginal (tests/test_essential_cpu.py): no trial with
# |rho| < 1e-3, no iteration whose improvement ratio lies within a factor of two of the 1e-3 threshold.  With small residuals Gauss-Newton
# converges quadratically and ends on trials whose chi2 change is rounding (|rho| ~ 1e-10, sign arbitrary): such a run is non-marginal only
# up to an iteration count (n_it; the one small-residual scene left runs a single iteration).  With large measurement noise (meas_noise = 20
# or 30: 0.4 .. 0.6 rad and m, 20 .. 30 % scale) it converges linearly, and the run of 20 ends after five or six iterations on the
# three-bad-iterations rule with every gain ratio above 1e-2.
SCENES = {
    "one_free": dict(n_it=20, n_free=1, seed=29, isolated=False, meas_noise=30),                # two edges, a duplicated pair: a wave mostly empty
    "two_free": dict(n_it=20, n_free=2, seed=8, meas_noise=30),                                # more than one row, an edge count that is no multiple of four
    "free9": dict(n_it=20, n_free=9, seed=1, meas_noise=30),                                   # 7 n = 63
    "free10": dict(n_it=20, n_free=10, seed=3, meas_noise=20),                 # 7 n = 70: one past the panel
    "free64": dict(n_it=20, n_free=64, seed=8, meas_noise=20),                 # 7 n = 448: whole panels
    "free65": dict(n_it=20, n_free=65, seed=5, meas_noise=20),                 # one past
    "free200": dict(n_it=20, n_free=200, seed=2, meas_noise=20),
    "merge": dict(n_it=20, n_free=30, seed=8, n_fixed=12, merge=True, meas_noise=20),   # fixed-fixed, fixed-free and free-free edges; ends on the three-bad rule
    "merge_short": dict(n_it=20, n_free=30, seed=1, n_fixed=12, merge=True),   # ends on ten rejected trials
    "fix_scale_all": dict(n_it=20, n_free=30, seed=8, fix_scale="all", meas_noise=20),
    "fix_scale_some": dict(n_it=20, n_free=30, seed=8, fix_scale="some", meas_noise=20),
    "fix_scale_small_residual": dict(n_it=1, n_free=20, seed=1, fix_scale="all"),       # sigma == 0 exactly: the scipy comparison runs on this one
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return make_scene(**{k: v for k, v in SCENES[name].items() if k != "n_it"})


# ---- the C++ oracle ----
@functools.lru_cache(maxsize=None)
def oracle():
    out_dir = tempfile.mkdtemp(prefix="essential_oracle_")
    so = os.path.join(out_dir, "libessential_oracle.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "essential_oracle.cc"), "-o", so])
    L = C.CDLL(so)
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    L.ego_error.argtypes = [vp] * 4; L.ego_error.restype = None
    for f in (L.ego_exp, L.ego_log, L.ego_inverse):
        f.argtypes = [vp, vp]; f.restype = None
    L.ego_mul.argtypes = [vp] * 3; L.ego_mul.restype = None
    L.ego_linear_system.argtypes = [i32, vp, vp, vp, i32, vp, vp, vp, f64, vp, vp, vp, vp]
    L.ego_essential_graph.argtypes = [i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    L.ego_correct_points.argtypes = [i32, i32, vp, vp, vp, vp]; L.ego_correct_points.restype = None
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run_oracle(sc, n_iterations=20):
    """dict(S, stats, trace, min_abs_rho, ratios) of the oracle on a scene."""
    S = sc.S.copy(); stats = np.zeros(4, np.int32); trace = np.zeros(n_iterations + 1); ratios = np.zeros(max(n_iterations, 1)); mr = C.c_double()
    rc = oracle().ego_essential_graph(sc.n_v, _p(S), _p(sc.fixed), _p(sc.fix_scale), sc.n_e, _p(sc.v0), _p(sc.v1), _p(sc.meas), n_iterations, _p(stats),
                                      _p(trace), C.byref(mr), _p(ratios))
    assert rc == 0
    return dict(S=S, stats=stats, trace=trace, min_abs_rho=mr.value, ratios=ratios[:n_iterations])


@functools.lru_cache(maxsize=None)
def oracle_result(name, n_iterations=None):
    """The oracle on a committed scene (at its own n_it unless told otherwise): computed once, shared by the tests; treat as read-only."""
    return run_oracle(scene(name), SCENES[name]["n_it"] if n_iterations is None else n_iterations)


def oracle_linear_system(sc, lam):
    nR = int(np.count_nonzero([(not sc.fixed[v]) and (np.any(sc.v0 == v) or np.any(sc.v1 == v)) for v in range(sc.n_v)]))
    n = 7 * nR
    H = np.zeros((n, n)); b = np.zeros(n); x = np.zeros(n); col = np.zeros(sc.n_v, np.int32)
    rc = oracle().ego_linear_system(sc.n_v, _p(sc.S), _p(sc.fixed), _p(sc.fix_scale), sc.n_e, _p(sc.v0), _p(sc.v1), _p(sc.meas), float(lam), _p(H), _p(b), _p(col), _p(x))
    assert rc == n, (rc, n)
    return H, b, col, x


def oracle_correct_points(mode, X, ref, tab_a, tab_b):
    X = np.ascontiguousarray(X, np.float32).copy(); ref = np.ascontiguousarray(ref, np.int32)
    dt = np.float64 if mode == 0 else np.float32
    A = np.ascontiguousarray(tab_a, dt); B = np.ascontiguousarray(tab_b, dt)
    oracle().ego_correct_points(mode, len(X), _p(X), _p(ref), _p(A), _p(B))
    return X


def correction_case(seed=3, n_v=9, n=300):
    """Points with reference vertices (some -1) and the two transform tables of both modes."""
    rng = np.random.default_rng(seed)
    X = rng.normal(0, 3, (n, 3)).astype(np.float32)
    ref = rng.integers(-1, n_v, n).astype(np.int32)
    ref[:4] = [-1, 0, n_v - 1, -1]
    A8 = np.array([sim3(rng.normal(0, 0.5, 3), rng.normal(0, 2, 3), np.exp(rng.normal(0, 0.1))) for _ in range(n_v)])
    B8 = np.array([sinv(smul(sim3(rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3), np.exp(rng.normal(0, 0.02))), a)) for a in A8])
    A7 = np.array([sim3(rng.normal(0, 0.5, 3), rng.normal(0, 2, 3))[:7] for _ in range(n_v)], np.float32)
    B7 = np.array([smul(sim3(rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3)), np.concatenate([a.astype(np.float64), [1.0]]))[:7] for a in A7], np.float32)
    return X, ref, (A8, B8), (A7, B7)
