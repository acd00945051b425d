"""Constructed cases for the Sim3 code: Horn's closed form of Sim3Solver::ComputeSim3 (R/lib_src/Sim3Solver.cc:437-540), CheckInliers (:542-562),
the sequential rule of iterate (:159-404), ComputeInliersNum (:564-664) and Optimizer::OptimizeSim3 (R/lib_src/Optimizer.cc:1920-2167).
Pure numpy: every case is built from a ground-truth similarity and named after the rule it holds.  Three references live here:

* ``horn64``            Horn's closed form in float64 over numpy.linalg.eigh: independent of the oracle's and of the kernels' restatement.
* ``check_inliers_f32`` CheckInliers as plain IEEE float32 in the order of sim3_check_inlier (the library is built with -ffp-contract=off), fed with a
                        hypothesis record: it decides every correspondence exactly, so thresholds can be tested one ulp apart.
* ``inliers_num_f64``   ComputeInliersNum with the map in float64 and the cast to float32 where upstream casts.

test_sim3_cases_cpu.py checks the cases and the oracle against these, test_sim3_cases_gpu.py the kernels."""
import collections

import numpy as np

from rumi_slam_amd.sim3solver import GlibcRand

F32 = np.float32
K_TUM = np.array([535.4, 539.2, 320.1, 247.6], F32)
K_POW2 = np.array([512, 512, 0, 0], F32)          # every product and quotient with power-of-two depths is exact
N_HYP = 70                                        # hypotheses of a scene case, at most

# ---- conditioning and tolerances ------------------------------------------------------------------------------------------------------
# A minimal set is three points: N has a well separated dominant eigenvalue unless the triangle is skinny.  G0 is the relative gap
# (l1 - l2) / |l1| of horn64 below which a triple goes to the property-only "skinny" case; with G0 = 0.05 between 55 and 70 of the 70 drawn
# triples of every parity case survive (asserted in the builder: at least 50).
G0 = 0.05
# Oracle against horn64 over every kept triple of every parity case, as test_sim3_cases_cpu.py::test_oracle_against_horn64 measures them: the worst
# case of 1273 triples, rounded up in the second digit.  dR: max |R - R64| (measured 1.405e-6, rot_623_150); dt: max |t - t64| / max(1, max |t64|)
# (6.772e-6, rot_3e-6); ds: |s - s64| / s64 (5.643e-7, rot_skew180); self: the worst distance of a mapped point of the triple from its counterpart
# over max(1, max |X1|), free-scale cases (2.635e-7).  The CPU test asserts that a fresh measurement does not exceed them.
ORACLE_DR = 1.5e-6
ORACLE_DT = 7.0e-6
ORACLE_DS = 5.8e-7
ORACLE_SELF = 2.7e-7
# Bounds of the device (a second, independent float restatement: other Jacobi sweeps, device sinf / cosf / atan2) against horn64 and against the
# oracle: four times the oracle's own distance, never looser than the 1e-4 of test_sim3solver_gpu._close.
TOL_DR = min(4 * ORACLE_DR, 1e-4)
TOL_DT = min(4 * ORACLE_DT, 1e-4)
TOL_DS = min(4 * ORACLE_DS, 1e-4)
# Property bounds of the skinny / collinear / two-coincident sets, where the rotation about the line is free: float32 closed form on metres.
# R is built from a float32 unit quaternion (rounding 6e-8 per product, a dozen products): orthonormal to 1e-5; the three points map onto each other
# to 2e-4 of their size when the set is exactly consistent (skinny sets amplify the 6e-8 coordinate rounding by 1 / gap <= 1e3).
PROP_ORTHO = 1e-5
PROP_SELF = 2e-4
PROP_SCALE = 2e-4


# ---- small linear algebra ---------------------------------------------------------------------------------------------------------------
def rotvec(v):
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def quat_of(R):
    """(x, y, z, w) of a rotation matrix, float64 (the eigenvector of Bar-Itzhack's matrix: no branches)."""
    R = np.asarray(R, np.float64)
    Kq = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                   [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                   [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                   [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, V = np.linalg.eigh(Kq)
    q = V[:, -1]
    return q if q[3] >= 0 else -q


def quat_R(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def sim8(R, t, s):
    return np.concatenate([quat_of(R), np.asarray(t, np.float64), [float(s)]])


def sim_Rts(S8):
    S8 = np.asarray(S8, np.float64)
    return quat_R(S8[:4]), S8[4:7].copy(), float(S8[7])


def sim_mul(a, b):
    """(R, t, s) product: a after b."""
    return a[0] @ b[0], a[2] * (a[0] @ b[1]) + a[1], a[2] * b[2]


def sim_inv(a):
    return a[0].T, -(a[0].T @ a[1]) / a[2], 1.0 / a[2]


def project(K, P):
    K = np.asarray(K, np.float64); P = np.asarray(P, np.float64).reshape(-1, 3)
    return np.stack([K[0] * P[:, 0] / P[:, 2] + K[2], K[1] * P[:, 1] / P[:, 2] + K[3]], 1)


# ---- reference 1: Horn's closed form in float64 ----------------------------------------------------------------------------------------
Horn = collections.namedtuple("Horn", "R t s gap e0 angle")


def horn64(p1, p2, fix_scale):
    """Horn 1987 on three (or more) correspondences p1[i] <-> p2[i]: p1 = s R p2 + t.  Returns R, t, s, the relative gap between the two largest
    eigenvalues of N, e0 of eigh's eigenvector as it came (either sign) and the rotation angle in [0, pi]."""
    p1 = np.asarray(p1, np.float64); p2 = np.asarray(p2, np.float64)
    o1, o2 = p1.mean(0), p2.mean(0)
    a, b = (p1 - o1).T, (p2 - o2).T
    M = b @ a.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, V = np.linalg.eigh(N)
    q = V[:, -1]
    gap = (w[-1] - w[-2]) / max(abs(w[-1]), 1e-300)
    e0 = float(q[0])
    if e0 < 0:
        q = -q
    nv = np.linalg.norm(q[1:])
    ang = 2 * np.arctan2(nv, q[0])
    R = rotvec(q[1:] / nv * ang) if nv > 0 else np.eye(3)
    P3 = R @ b
    den = (P3 * P3).sum()
    s = 1.0 if fix_scale or den == 0 else float((a * P3).sum() / den)
    return Horn(R, o1 - s * (R @ o2), s, float(gap), e0, float(ang))


# ---- reference 2: CheckInliers in float32, in the order of sim3_check_inlier ----------------------------------------------------------
def thresholds(sigma2):
    """mvnMaxError1 / 2 are vector<size_t> upstream (Sim3Solver.h:77-78): 9.210 * sigma2 in double, truncated, compared as float."""
    return np.floor(9.210 * np.asarray(sigma2, F32).astype(np.float64)).astype(F32)


def rows_from_record(T12_record):
    """The end of sim3_minimal_solve: rows of [sR | t] of T12 and T21 from the 16-float record (R row-major, t, s, valid, 0, 0)."""
    rec = np.asarray(T12_record, F32)
    R, t, s = rec[:9].reshape(3, 3), rec[9:12], rec[12]
    sinv = F32(1.0 / np.float64(s))
    T12, T21 = np.zeros((3, 4), F32), np.zeros((3, 4), F32)
    for r in range(3):
        for c in range(3):
            T12[r, c] = s * R[r, c]
            T21[r, c] = sinv * R[c, r]
        T12[r, 3] = t[r]
    for r in range(3):
        T21[r, 3] = -((T21[r, 0] * t[0] + T21[r, 1] * t[1]) + T21[r, 2] * t[2])
    return T12, T21


def errors_f32(T12_record, X1, X2, K1, K2):
    """err1, err2 of every correspondence, float32 operation by operation."""
    a, b = np.asarray(X1, F32).reshape(-1, 3), np.asarray(X2, F32).reshape(-1, 3)
    K1, K2 = np.asarray(K1, F32), np.asarray(K2, F32)
    T12, T21 = rows_from_record(T12_record)
    with np.errstate(all="ignore"):
        u1 = K1[0] * a[:, 0] / a[:, 2] + K1[2]; v1 = K1[1] * a[:, 1] / a[:, 2] + K1[3]
        u2 = K2[0] * b[:, 0] / b[:, 2] + K2[2]; v2 = K2[1] * b[:, 1] / b[:, 2] + K2[3]
        p = [((T12[k, 0] * b[:, 0] + T12[k, 1] * b[:, 1]) + T12[k, 2] * b[:, 2]) + T12[k, 3] for k in range(3)]
        r = [((T21[k, 0] * a[:, 0] + T21[k, 1] * a[:, 1]) + T21[k, 2] * a[:, 2]) + T21[k, 3] for k in range(3)]
        d1x = u1 - (K1[0] * p[0] / p[2] + K1[2]); d1y = v1 - (K1[1] * p[1] / p[2] + K1[3])
        d2x = (K2[0] * r[0] / r[2] + K2[2]) - u2; d2y = (K2[1] * r[1] / r[2] + K2[3]) - v2
        err1 = d1x * d1x + d1y * d1y; err2 = d2x * d2x + d2y * d2y
    assert err1.dtype == F32 and err2.dtype == F32
    return err1, err2


def check_inliers_f32(T12_record, X1, X2, thr1, thr2, K1, K2):
    """The inlier mask of one hypothesis; thr1 / thr2 = thresholds(sigma2).  NaN and inf compare false: an outlier."""
    err1, err2 = errors_f32(T12_record, X1, X2, K1, K2)
    with np.errstate(all="ignore"):
        return (err1 < np.asarray(thr1, F32)) & (err2 < np.asarray(thr2, F32))


def record_of(R, t, s, valid=1.0):
    return np.concatenate([np.asarray(R, F32).ravel(), np.asarray(t, F32), [F32(s), F32(valid), 0, 0]]).astype(F32)


def records_of(res):
    """The [H,16] records of a result dict of Sim3Ransac / O.sim3_ransac."""
    H = len(res["s"])
    return np.concatenate([res["R"].reshape(H, 9), res["t"], res["s"][:, None], res["valid"][:, None].astype(F32), np.zeros((H, 2), F32)], 1).astype(F32)


def m_symmetric_f32(p1, p2):
    """Whether M = Pr2 Pr1^T of a triple comes out exactly symmetric in the float32 order of ComputeSim3: then N12 = N13 = N14 = 0 exactly, no Jacobi
    rotation touches row 0, the eigenvector is (1, 0, 0, 0) and the set counts as degenerate (:493-494)."""
    P1, P2 = np.asarray(p1, F32).T.copy(), np.asarray(p2, F32).T.copy()          # column i = correspondence i
    O1 = ((P1[:, 0] + P1[:, 1]) + P1[:, 2]) / F32(3); O2 = ((P2[:, 0] + P2[:, 1]) + P2[:, 2]) / F32(3)
    Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
    M = np.zeros((3, 3), F32)
    for r in range(3):
        for c in range(3):
            M[r, c] = (Pr2[r, 0] * Pr1[c, 0] + Pr2[r, 1] * Pr1[c, 1]) + Pr2[r, 2] * Pr1[c, 2]
    if not (M[1, 2] == M[2, 1] and M[2, 0] == M[0, 2] and M[0, 1] == M[1, 0]):
        return False
    # row 0 is decoupled; (1,0,0,0) is dominant when trace M is not below the lower block's largest eigenvalue (M = 0: first diagonal entry wins)
    Md = M.astype(np.float64)
    low = np.array([[Md[0, 0] - Md[1, 1] - Md[2, 2], Md[0, 1] + Md[1, 0], Md[2, 0] + Md[0, 2]],
                    [Md[0, 1] + Md[1, 0], -Md[0, 0] + Md[1, 1] - Md[2, 2], Md[1, 2] + Md[2, 1]],
                    [Md[2, 0] + Md[0, 2], Md[1, 2] + Md[2, 1], -Md[0, 0] - Md[1, 1] + Md[2, 2]]])
    return bool(np.trace(Md) >= np.linalg.eigvalsh(low)[-1])


# ---- reference 3: ComputeInliersNum --------------------------------------------------------------------------------------------------
def reproj2_f64(S, K, X, kp):
    """Squared reprojection error as :621-627: map and project in double, cast to float, difference and dot product in float.  S = (R, t, s)."""
    R, t, s = S
    X = np.asarray(X, F32).astype(np.float64).reshape(-1, 3)
    kp = np.asarray(kp, F32).reshape(-1, 2)
    K = np.asarray(K, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        P = s * (X @ R.T) + t
        u = (K[0] * P[:, 0] / P[:, 2] + K[2]).astype(F32); v = (K[1] * P[:, 1] / P[:, 2] + K[3]).astype(F32)
        dx, dy = kp[:, 0] - u, kp[:, 1] - v
        return dx * dx + dy * dy


def inliers_num_f64(pair_start, pair_denominator, S_c1w2, S_c2w1, K4_1, K4_2, X1, X2, kp1, kp2, sigma2_1, sigma2_2, edge1, edge2, margins=False):
    """ComputeInliersNum: (median ratio, ratio per pair, flags) and, with margins, per key-point the smaller relative distance of its two errors from their
    thresholds.  S_c1w2 / S_c2w1: per pair 8 doubles (x y z w, t, s) or (R, t, s).  The edge flags are crossed as upstream crosses them (:630): a
    failing err1 is rescued by the map-2 point's flag, a failing err2 by the map-1 point's; the thresholds 2 * 9.210 * sigma2 are doubles and strict."""
    ps = np.asarray(pair_start, np.int64); n_pairs, total = len(ps) - 1, int(ps[-1])
    flags, rel = np.zeros(total, np.uint8), np.full(total, np.inf)
    ratios = np.zeros(n_pairs, F32)
    s1, s2 = np.asarray(sigma2_1, F32).astype(np.float64), np.asarray(sigma2_2, F32).astype(np.float64)
    as_rts = lambda S: S if isinstance(S, tuple) else sim_Rts(S)
    for p in range(n_pairs):
        a, b = int(ps[p]), int(ps[p + 1])
        if b > a:
            e1 = reproj2_f64(as_rts(S_c1w2[p]), K4_1, X2[a:b], kp1[a:b]).astype(np.float64)       # map-2 point into key-frame 1
            e2 = reproj2_f64(as_rts(S_c2w1[p]), K4_2, X1[a:b], kp2[a:b]).astype(np.float64)       # map-1 point into key-frame 2
            t1, t2 = 2 * 9.210 * s1[a:b], 2 * 9.210 * s2[a:b]
            with np.errstate(all="ignore"):
                ok1 = (e1 < t1) | (np.asarray(edge2[a:b]) != 0)
                ok2 = (e2 < t2) | (np.asarray(edge1[a:b]) != 0)
                rel[a:b] = np.minimum(np.abs(e1 - t1) / t1, np.abs(e2 - t2) / t2)
            flags[a:b] = ok1 & ok2
        den = int(pair_denominator[p])
        ratios[p] = F32(int(flags[a:b].sum())) / F32(den) if den else F32(0)
    med = F32(np.sort(ratios)[n_pairs // 2]) if n_pairs else F32(0)
    return (med, ratios, flags, rel) if margins else (med, ratios, flags)


# ---- a scripted rand() ----------------------------------------------------------------------------------------------------------------------
class ScriptRand(GlibcRand):
    """rand() that replays a list of words: the minimal sets a solver draws are then the test's choice."""

    def __init__(self, words):
        self._w, self._i = [int(w) for w in words], 0

    def _next_word(self):
        v = self._w[self._i]
        self._i += 1
        return v << 1                                   # rand() returns the word >> 1

    def state(self):
        return [self._i]

    def set_state(self, st):
        self._i = int(st[0])


def script_words(N, triples):
    """rand() values under which a solver with N correspondences draws these minimal sets (:176-191)."""
    out = []
    for tri in triples:
        avail = list(range(N))
        for want in tri:
            r, d = avail.index(int(want)), len(avail)
            w = -(-r * (1 << 31) // d)                  # the smallest word with int(word / 2^31 * d) == r
            assert int((float(w) / 2147483648.0) * d) == r
            out.append(w)
            avail[r] = avail[-1]
            avail.pop()
    return out


def replay_upstream(valid, n_inliers, median, min_inliers, max_its, n_per_call, mode, best_ratio=0.0):
    """Upstream's loop (:176-216 / :243-289 / :315-403) over per-iteration results.  A degenerate set returns early from ComputeSim3 (:493-494) and the
    iteration goes on with the previous iteration's transform, so it repeats that iteration's count and ratio (nothing on a solver's first iteration).
    Returns (iteration it returns at or None, iterations run, calls made, best inliers, best ratio)."""
    it, best_n, last, calls = 0, 0, None, 0
    while it < max_its:
        calls += 1
        for _ in range(n_per_call):
            if it >= max_its:
                break
            r_i = float(median[it]) if median is not None else 0.0
            if valid[it]:
                last = (int(n_inliers[it]), r_i)
            elif last is None:
                last = (0, r_i)
            n_i, r_i = last
            it += 1
            ok = n_i >= best_n if mode != "rumination" else (r_i >= best_ratio and n_i >= best_n)
            if ok:
                best_n = n_i
                if mode == "rumination":
                    best_ratio = r_i
                if (n_i > min_inliers) if mode != "rumination" else (r_i > 0.10 and n_i > min_inliers):
                    return it - 1, it, calls, best_n, best_ratio
    return None, it, calls, best_n, best_ratio


# ---- scene cases ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """One solver's worth of correspondences with its minimal sets.  keep[h]: the triple is well conditioned and the hypothesis is compared with horn64
    and the oracle; props[h]: the hypothesis is checked by properties only; expect_valid / expect_n / expect_mask: stated outcomes (None: not stated)."""

    def __init__(self, id, rule, X1, X2, s1, s2, K1, K2, tri, fix_scale=False, truth=None, score=None, keep=None, props=None, expect_valid=None,
                 expect_n=None, expect_mask=None, extra=None):
        self.id, self.rule = id, rule
        self.X1, self.X2 = np.ascontiguousarray(X1, F32), np.ascontiguousarray(X2, F32)
        self.n = len(self.X1)
        self.s1 = np.ascontiguousarray(np.broadcast_to(np.asarray(s1, F32), (self.n,)))
        self.s2 = np.ascontiguousarray(np.broadcast_to(np.asarray(s2, F32), (self.n,)))
        self.K1, self.K2 = np.asarray(K1, F32), np.asarray(K2, F32)
        self.tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
        self.H = len(self.tri)
        assert self.H <= N_HYP and self.tri.min() >= 0 and self.tri.max() < self.n
        self.fix_scale, self.truth, self.score = bool(fix_scale), truth, score
        self.keep = np.zeros(self.H, bool) if keep is None else np.asarray(keep, bool)
        self.props = np.zeros(self.H, bool) if props is None else np.asarray(props, bool)
        self.expect_valid, self.expect_n, self.expect_mask = expect_valid, expect_n or {}, expect_mask or {}
        self.extra = extra or {}
        self.thr1, self.thr2 = thresholds(self.s1), thresholds(self.s2)
        self.horn = [horn64(self.X1[t], self.X2[t], self.fix_scale) for t in self.tri]

    def args(self):
        return self.X1, self.X2, self.s1, self.s2, self.K1, self.K2, self.tri

    def __repr__(self):
        return self.id


def _box(rng, n):
    """Points of the 3 x 2 x 5 m box in front of a camera."""
    return np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1, 1, n), rng.uniform(3, 8, n)], 1)


def _recentre(R, s):
    """The translation that puts the image of the box's centre 5.5 s in front of camera 1: every point keeps a positive depth under any rotation."""
    return np.array([0, 0, 5.5 * s]) - s * (R @ np.array([0, 0, 5.5]))


def _score_set(rng, R, s, t, per_pair=20):
    """ComputeInliersNum data of two key-frame pairs under the truth gSc1c2 = (R, t, s).  The solver's key-frames sit at the origins of their maps, so
    gSw1w2 = gSc1c2 (:344-347); pair 0 is the solver's own pair, pair 1 two other key-frames.  A fifth of the key-points are wrong matches; no error under
    the truth is closer than 1e-2 (relative) to its threshold."""
    ident = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
    truth = (R, t, s)
    A, B, W1, W2, ps = [], [], [], [], [0]
    for p in range(2):
        m = per_pair + p
        if p == 0:
            S1, S2 = ident, ident
        else:
            R2 = rotvec(rng.normal(size=3) * 0.08); t2 = rng.normal(size=3) * 0.2
            R1 = rotvec(rng.normal(size=3) * 0.08) @ R2 @ R.T
            S2 = sim8(R2, t2, 1.0)
            S1 = None
        Pc2 = _box(rng, m)
        R2m, t2m, _ = sim_Rts(S2)
        Pw2 = (Pc2 - t2m) @ R2m                                    # R2^T (Pc2 - t2)
        Pw1 = s * (Pw2 @ R.T) + t
        if S1 is None:
            t1 = np.array([0, 0, 5.5 * s]) - R1 @ Pw1.mean(0)
            S1 = sim8(R1, t1, 1.0)
        W1.append(Pw1.astype(F32)); W2.append(Pw2.astype(F32))
        A.append(S1); B.append(S2)
        ps.append(ps[-1] + m)
    X1, X2 = np.concatenate(W1), np.concatenate(W2)
    total = ps[-1]
    sg1 = (F32(1.2) ** (2 * rng.integers(0, 4, total))).astype(F32); sg2 = (F32(1.2) ** (2 * rng.integers(0, 4, total))).astype(F32)
    kp1, kp2 = np.zeros((total, 2), F32), np.zeros((total, 2), F32)
    comp1 = [sim_mul(sim_Rts(A[p]), truth) for p in range(2)]; comp2 = [sim_mul(sim_Rts(B[p]), sim_inv(truth)) for p in range(2)]
    for p in range(2):
        for i in range(ps[p], ps[p + 1]):
            wrong = rng.random() < 0.2
            for _ in range(100):
                o1 = project(K_TUM, comp1[p][2] * (comp1[p][0] @ X2[i].astype(np.float64)) + comp1[p][1])[0] + rng.normal(0, 0.7, 2)
                o2 = project(K_TUM, comp2[p][2] * (comp2[p][0] @ X1[i].astype(np.float64)) + comp2[p][1])[0] + rng.normal(0, 0.7, 2)
                if wrong:
                    o2 = o2 + rng.uniform(25, 80, 2) * rng.choice([-1, 1], 2)
                kp1[i], kp2[i] = o1, o2
                e1 = float(reproj2_f64(comp1[p], K_TUM, X2[i], kp1[i])[0]); e2 = float(reproj2_f64(comp2[p], K_TUM, X1[i], kp2[i])[0])
                th1, th2 = 2 * 9.210 * float(sg1[i]), 2 * 9.210 * float(sg2[i])
                if abs(e1 - th1) > 1e-2 * th1 and abs(e2 - th2) > 1e-2 * th2:
                    break
            else:
                raise AssertionError("no key-point clear of its threshold")
    edge1 = np.zeros(total, np.uint8); edge2 = np.zeros(total, np.uint8)
    edge1[[3, ps[1] + 2]] = 1; edge2[[5, ps[1] + 7]] = 1
    return dict(pair_start=np.array(ps, np.int32), pair_denominator=np.array([ps[1] + 3, ps[2] - ps[1]], np.int32), S_c1w1=np.stack(A), S_c2w2=np.stack(B),
                S_kf1w=ident.copy(), S_kf2w=ident.copy(), K4_1=K_TUM, K4_2=K_TUM, X1=X1, X2=X2, kp1=kp1, kp2=kp2, sigma2_1=sg1, sigma2_2=sg2,
                edge1=edge1, edge2=edge2)


def _scene(id, rule, seed, R, s, t=None, n=30, n_clean=14, fix_scale=False, score=False, parity=True):
    """X1 = s R X2 + t: the first n_clean correspondences are consistent to float32 rounding and supply the minimal sets, the others carry 4 mm of
    noise and every fourth of them is a wrong match, so that CheckInliers has both answers to give."""
    rng = np.random.default_rng(seed)
    R = np.asarray(R, np.float64)
    t = _recentre(R, s) if t is None else np.asarray(t, np.float64)
    X2 = _box(rng, n).astype(F32)
    X1 = s * (X2.astype(np.float64) @ R.T) + t
    X1[n_clean:] += rng.normal(0, 0.004 * s, (n - n_clean, 3))
    bad = np.arange(n_clean, n)[::4]
    X1[bad] = s * (_box(rng, len(bad)) @ R.T) + t
    sg = lambda: (F32(1.2) ** (2 * rng.integers(0, 8, n))).astype(F32)
    tri = GlibcRand(seed).draw_window(n_clean, N_HYP)
    c = Case(id, rule, X1, X2, sg(), sg(), K_TUM, K_TUM, tri, fix_scale=fix_scale, truth=(R, t, 1.0 if fix_scale else s),
             score=_score_set(rng, R, s, t) if score else None)
    gaps = np.array([h.gap for h in c.horn])
    if parity:
        c.keep = gaps >= G0
        assert c.keep.sum() >= 50, f"{id}: only {c.keep.sum()} of {c.H} triples have gap >= {G0}"
    return c


AXIS_SKEW = np.array([1, 2, -2]) / 3.0


def rotation_cases():
    spec = [("rot_z90", "90 deg about z", [0, 0, np.pi / 2]),
            ("rot_111_120", "120 deg about (1,1,1): a cyclic permutation of the axes", np.array([1, 1, 1]) / np.sqrt(3) * 2 * np.pi / 3),
            ("rot_x180", "180 deg about x: trace <= 0, R00 largest", [np.pi, 0, 0]),
            ("rot_y180", "180 deg about y: trace <= 0, R11 largest", [0, np.pi, 0]),
            ("rot_z180", "180 deg about z: trace <= 0, R22 largest", [0, 0, np.pi]),
            ("rot_skew180", "180 deg about (1,2,-2)/3: e0 of the quaternion is 0", AXIS_SKEW * np.pi),
            ("rot_skew179_99", "179.99 deg about (1,2,-2)/3", AXIS_SKEW * np.radians(179.99)),
            ("rot_623_150", "150 deg about (6,2,3)/7: trace <= 0 with R00 largest and every quaternion component far from 0", np.array([6, 2, 3]) / 7 * np.radians(150)),
            ("rot_263_150", "150 deg about (2,6,3)/7: trace <= 0 with R11 largest", np.array([2, 6, 3]) / 7 * np.radians(150)),
            ("rot_326_150", "150 deg about (3,2,6)/7: trace <= 0 with R22 largest", np.array([3, 2, 6]) / 7 * np.radians(150)),
            ("rot_1e-3", "1e-3 rad about x: the sin / cos branch of SO3::exp at a small angle", [1e-3, 0, 0]),
            ("rot_3e-6", "3e-6 rad about y: the Taylor branch of SO3::exp (theta < 1e-5)", [0, 3e-6, 0]),
            ("rot_1e-6", "1e-6 rad about (1,2,-2)/3: the Taylor branch of SO3::exp", AXIS_SKEW * 1e-6),
            ("rot_1e-5", "1e-5 rad about z: minimal sets on either side of the theta < 1e-5 switch of SO3::exp", [0, 0, 1e-5])]
    out = []
    for k, (id, rule, v) in enumerate(spec):
        c = _scene(id, rule, 100 + k, rotvec(v), 1.25, score=True)
        c.extra["rotvec"] = np.asarray(v, np.float64)
        if id in ("rot_3e-6", "rot_1e-6"):
            # the angle horn64 finds is the truth's plus the float32 rounding of metres over a metre of baseline (a few 1e-7)
            c.keep &= np.array([h.angle < 1e-5 for h in c.horn])
            assert c.keep.sum() >= 50, f"{id}: {c.keep.sum()} triples under the Taylor threshold"
        out.append(c)
    return out


def scale_cases():
    Rs = rotvec([0.05, -0.2, 0.08])
    out = [_scene("scale_0.05", "scale 0.05, free scale", 200, Rs, 0.05),
           _scene("scale_0.5_n257", "scale 0.5 over n = 257: one correspondence past the 256-stride loop of k_sim3_ransac", 201, Rs, 0.5, n=257),
           _scene("scale_8", "scale 8, free scale", 202, Rs, 8.0),
           _scene("scale_20", "scale 20, free scale: the largest |t|-relative error of the closed form", 203, Rs, 20.0),
           _scene("fix_scale_on_1.25", "fix_scale on data of scale 1.25: s == 1 exactly, the inlier count collapses", 204, Rs, 1.25, fix_scale=True),
           _scene("far_translation", "t = (50, -30, 100)", 205, Rs, 1.0, t=[50.0, -30.0, 100.0])]
    return out


def skinny_case():
    """Triples of a consistent scene whose N has a poorly separated dominant eigenvalue (gap < G0): the rotation about the triangle's long side is weakly
    determined, so the device may differ from the oracle; properties only."""
    rng = np.random.default_rng(300)
    R, s = rotvec([0.3, -0.5, 0.4]), 1.25
    t = _recentre(R, s)
    n = 30
    X2 = _box(rng, n).astype(F32)
    X1 = (s * (X2.astype(np.float64) @ R.T) + t).astype(F32)
    pool = GlibcRand(300).draw_window(n, 3000)
    gaps = np.array([horn64(X1[tr], X2[tr], False).gap for tr in pool])
    sel = pool[(gaps < G0) & (gaps > 1e-3)][:40]
    assert len(sel) >= 20
    sg = np.ones(n, F32)
    return Case("skinny", "gap < G0: properties only", X1, X2, sg, sg, K_TUM, K_TUM, sel, truth=(R, t, s), props=np.ones(len(sel), bool))


def degenerate_case():
    """Five minimal sets in one consistent scene (R = 90 deg about z, s = 1.5, t = (0.25, 0.5, 1)), coordinates on a grid of 1/8 so that the centroids
    of coincident points are exact.
    0: three coincident points in both maps   -> Pr1 = Pr2 = 0, M = 0, invalid.
    1: three coincident points in map 2 only  -> Pr2 = 0, M = 0, invalid.
    2: a collinear triple                     -> valid; the rotation about the line is free.
    3: two coincident points plus one         -> valid; likewise.
    4: an ordinary triple."""
    rng = np.random.default_rng(310)
    R, s, t = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]]), 1.5, np.array([0.25, 0.5, 1.0])
    n = 24
    X2 = (np.round(_box(rng, n) * 8) / 8)
    X2[0:3] = [0.5, -0.25, 4.0]
    X2[3:6] = [-0.75, 0.5, 5.0]
    X2[6:9] = [[0, 0, 4], [0.5, 0.25, 4.5], [1, 0.5, 5]]
    X2[9:12] = [[0.25, 0.75, 6], [0.25, 0.75, 6], [-1, 0.5, 4]]
    X1 = s * (X2 @ R.T) + t
    X1[3:6] = [[0.5, 1.0, 6.0], [2.0, -0.5, 7.0], [1.0, 0.25, 8.5]]            # distinct in map 1 while coincident in map 2
    tri = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14]], np.int32)
    sg = np.ones(n, F32)
    c = Case("degenerate", "coincident / collinear minimal sets", X1, X2, sg, sg, K_TUM, K_TUM, tri, truth=(R, t, s),
             props=[False, False, True, True, True], expect_valid=np.array([False, False, True, True, True]))
    assert np.array_equal(X1.astype(F32).astype(np.float64), X1), "the scene is exactly representable"
    return c


def _trap_points(seed, n=30):
    rng = np.random.default_rng(seed)
    X2 = _box(rng, n).astype(F32)
    X1 = X2.copy()
    X1[3:] += rng.normal(0, 0.002, (n - 3, 3)).astype(F32)
    return rng, X1, X2


def identity_trap_cases():
    out = []
    # a triple bit-identical in both maps inside a consistent scene: M is exactly symmetric, q = (1,0,0,0), the set is degenerate although the identity
    # it stands for explains every correspondence.  Upstream returns early (:493-494); a selector that forgot `valid` would converge on it.
    rng, X1, X2 = _trap_points(400)
    n = len(X1)
    sg = np.full(n, 1.44, F32)
    tri = np.concatenate([[[0, 1, 2], [2, 0, 1]], GlibcRand(400).draw_window(n - 3, 20) + 3]).astype(np.int32)
    ev = np.ones(len(tri), bool); ev[:2] = False
    out.append(Case("trap_identity_triple", "bit-identical triple in a consistent scene: valid = 0 and n_inliers = n", X1, X2, sg, sg, K_TUM, K_TUM, tri,
                    truth=(np.eye(3), np.zeros(3), 1.0), expect_valid=ev, expect_n={0: n, 1: n}, score=_score_set(rng, np.eye(3), 1.0, np.zeros(3))))
    # maps identical throughout: every hypothesis is degenerate
    tri = GlibcRand(401).draw_window(n, 24)
    out.append(Case("trap_identical_maps", "maps identical throughout: every hypothesis invalid", X2, X2, sg, sg, K_TUM, K_TUM, tri,
                    truth=(np.eye(3), np.zeros(3), 1.0), expect_valid=np.zeros(len(tri), bool), expect_n={h: n for h in range(len(tri))}))
    # X1 = 2 X2 + (1, 2, 4) on a grid of 1/8: exact in float32.  Where the three coordinates of a triple sum to multiples of 3 grid steps the centroids are
    # exact too, M = 2 Pr2 Pr2^T is exactly symmetric and the set is degenerate; elsewhere the centroid's rounding decides.
    rng = np.random.default_rng(402)
    G = np.round(_box(rng, n) * 8).astype(np.int64)
    for k in range(0, 9, 3):                                           # three triples with exact centroids
        G[k + 2] += (-G[k:k + 3].sum(0)) % 3
    X2g = (G / 8.0).astype(F32)
    X1g = (2 * X2g.astype(np.float64) + np.array([1, 2, 4.0])).astype(F32)
    assert np.array_equal(X1g.astype(np.float64), 2 * X2g.astype(np.float64) + np.array([1, 2, 4.0]))
    tri = np.concatenate([[[0, 1, 2], [3, 4, 5], [6, 7, 8]], GlibcRand(402).draw_window(n, 27)]).astype(np.int32)
    flagged = np.array([m_symmetric_f32(X1g[tr], X2g[tr]) for tr in tri])
    assert flagged[:3].all() and not flagged.all()
    c = Case("trap_pure_scale", "X1 = 2 X2 + (1,2,4), exactly representable: symmetric M wherever the centroids are exact", X1g, X2g, sg, sg, K_TUM, K_TUM, tri,
             truth=(np.eye(3), np.array([1, 2, 4.0]), 2.0), expect_valid=~flagged)
    c.props = ~flagged
    out.append(c)
    return out


def trap_sequence_scene():
    """The identity trap for the sequential rule: correspondences 0-2 bit-identical, 3-21 consistent with 2 mm of noise, 22-29 wrong matches.  Minimal sets
    by name: I = the identical triple (invalid, yet the identity it stands for has more than min_inliers inliers), B = a triple with two wrong matches
    (valid, few inliers), G = a clean triple (valid, converges).  min_inliers = 15."""
    rng, X1, X2 = _trap_points(410)
    n = len(X1)
    X1[22:] = _box(rng, n - 22).astype(F32)
    sg = np.full(n, 1.44, F32)
    names = dict(I=[0, 1, 2], I2=[2, 1, 0], B=[3, 22, 23], B2=[24, 5, 25], G=[4, 9, 14], G2=[6, 11, 17])
    score = _score_set(rng, np.eye(3), 1.0, np.zeros(3))
    return dict(X1=X1, X2=X2, s1=sg, s2=sg, K=K_TUM, names=names, min_inliers=15, score=score, n=n)


def ordinary_scene(seed, n):
    """A clean solver for either side of the trap: every minimal set converges."""
    c = _scene(f"ordinary_{seed}", "consistent scene", seed, rotvec([0.05, -0.2, 0.08]), 1.25, n=n, n_clean=n, parity=False)
    return dict(X1=c.X1, X2=c.X2, s1=c.s1, s2=c.s2, K=K_TUM, n=n, min_inliers=n // 2)


# ---- the threshold ladder -------------------------------------------------------------------------------------------------------------------
LADDER_SIGMA2 = [1.0, 0.1, 0.109, 1.44, 4.2998]          # thresholds 9, 0, 1, 13, 39
LADDER_DELTAS = [1e-1, -1e-1, 1e-2, -1e-2, 1e-3, -1e-3, 1e-5, -1e-5, 1e-6, -1e-6]
Rung = collections.namedtuple("Rung", "index term sigma2 delta")          # delta: relative distance of the error from the threshold; "ulp-" / "ulp+" pairs


def ladder_case():
    """n = 129 (one past two waves of k_s3b_check): 29 consistent correspondences that supply the minimal sets, and per error term and per sigma2 twelve
    correspondences whose error under the truth sits at (1 + delta) * threshold, the last two a float32 step of one coordinate apart on either side of
    the threshold (under the truth's float32 rows; a step of a coordinate moves the error by some 1e-5 relative, float32 coordinates allow no finer).
    The term under test has the sigma2 of the rung, the other term sigma2 = 100 (threshold 921).  sigma2 = 0.1 gives threshold 0: its four correspondences
    have zero error and still are no inliers."""
    rng = np.random.default_rng(500)
    R, s = rotvec([0.05, -0.2, 0.08]), 1.25
    t = _recentre(R, s)
    K = K_TUM.astype(np.float64)
    rec = record_of(R, t, s)
    X1, X2, s1, s2, rungs = [], [], [], [], []

    def place(term, target, du_sign=1.0):
        """A correspondence whose err<term> under the truth is `target` (float64 construction)."""
        b = _box(rng, 1)[0].astype(F32).astype(np.float64)
        a = s * (R @ b) + t
        phi = rng.uniform(-0.7, 0.7)
        d = np.sqrt(target) * np.array([np.cos(phi), np.sin(phi)]) * du_sign
        if term == 1:                                        # move a's projection in camera 1
            u, v = project(K, a)[0] + d
            a = np.array([(u - K[2]) / K[0] * a[2], (v - K[3]) / K[1] * a[2], a[2]])
        else:                                                # move b's projection in camera 2
            u, v = project(K, b)[0] + d
            b = np.array([(u - K[2]) / K[0] * b[2], (v - K[3]) / K[1] * b[2], b[2]])
        return a.astype(F32), b.astype(F32)

    def err_of(term, a, b):
        e1, e2 = errors_f32(rec, a[None], b[None], K_TUM, K_TUM)
        return (e1 if term == 1 else e2)[0]

    for term in (1, 2):
        for sig in LADDER_SIGMA2:
            thr = float(thresholds([sig])[0])
            if thr == 0:
                for _ in range(2):
                    b = _box(rng, 1)[0].astype(F32)
                    a = (s * (R @ b.astype(np.float64)) + t).astype(F32)
                    rungs.append(Rung(len(X1), term, sig, 0.0))
                    X1.append(a); X2.append(b); s1.append(sig if term == 1 else 100.0); s2.append(sig if term == 2 else 100.0)
                continue
            for dlt in LADDER_DELTAS:
                a, b = place(term, thr * (1 + dlt))
                rungs.append(Rung(len(X1), term, sig, dlt))
                X1.append(a); X2.append(b); s1.append(sig if term == 1 else 100.0); s2.append(sig if term == 2 else 100.0)
            # the one-step pair: walk one coordinate of the moved point until the float32 error crosses the threshold
            a, b = place(term, thr)
            moved = a if term == 1 else b                    # the offset points along +u, so a larger x is a larger error
            up = err_of(term, a, b) < F32(thr)
            for _ in range(4000):
                if (err_of(term, a, b) < F32(thr)) != up:
                    break
                moved[0] = np.nextafter(moved[0], F32(np.inf) if up else F32(-np.inf))
            else:
                raise AssertionError("the threshold was not crossed")
            # moved[0] is the first value on the far side; its predecessor (towards where the walk came from) is on the near side
            far = moved[0]
            near = np.nextafter(far, F32(-np.inf) if up else F32(np.inf))
            for x0, name in ((near, "near"), (far, "far")):
                pa, pb = a.copy(), b.copy()
                (pa if term == 1 else pb)[0] = x0
                is_in = err_of(term, pa, pb) < F32(thr)
                rungs.append(Rung(len(X1), term, sig, "ulp-" if is_in else "ulp+"))
                X1.append(pa); X2.append(pb); s1.append(sig if term == 1 else 100.0); s2.append(sig if term == 2 else 100.0)
            assert rungs[-1].delta != rungs[-2].delta, "the pair straddles the threshold under the truth"
    n_rungs = len(X1)
    pad = 129 - n_rungs
    assert pad >= 12
    b = _box(rng, pad).astype(F32)
    a = (s * (b.astype(np.float64) @ R.T) + t).astype(F32)
    X1 = np.concatenate([np.stack(X1), a]); X2 = np.concatenate([np.stack(X2), b])
    s1 = np.concatenate([np.array(s1, F32), np.ones(pad, F32)]); s2 = np.concatenate([np.array(s2, F32), np.ones(pad, F32)])
    tri = GlibcRand(500).draw_window(pad, N_HYP) + n_rungs
    c = Case("ladder_n129", "err1 / err2 at (1 + delta) * threshold, both terms, five sigma2; n = 129", X1, X2, s1, s2, K_TUM, K_TUM, tri, truth=(R, t, s),
             extra=dict(rungs=rungs))
    c.keep = np.array([h.gap for h in c.horn]) >= G0
    assert c.n == 129 and c.keep.sum() >= 50
    return c


def identity_path_case():
    """On the identity path (a degenerate triple: R = I, t = 0, s = 1, so p = b and r = a exactly) with K = (512, 512, 0, 0) and power-of-two depths every
    operation of CheckInliers is exact and the mask can be stated outright."""
    x9 = F32(3.0 / 128)                                      # 512 * x / 4 == 3: err == 9.0f == threshold(sigma2 = 1): not an inlier (strict <)
    xp = np.nextafter(x9, F32(0))                            # its predecessor: err < 9: an inlier
    xn = np.nextafter(x9, F32(1))
    rows = [  # a (point 1 in camera 1), b (point 2 in camera 2), sigma2_1, sigma2_2, inlier, why
        ([1, 0, 4], [1, 0, 4], 1, 1, 1, "triple"), ([0, 1, 4], [0, 1, 4], 1, 1, 1, "triple"), ([-1, -1, 4], [-1, -1, 4], 1, 1, 1, "triple"),
        ([0, 0, 4], [x9, 0, 4], 1, 100, 0, "err1 == 9.0f == thr1"), ([0, 0, 4], [xp, 0, 4], 1, 100, 1, "err1 one step under thr1"),
        ([0, 0, 4], [xn, 0, 4], 1, 100, 0, "err1 one step over thr1"),
        ([0, 0, 4], [x9, 0, 4], 100, 1, 0, "err2 == 9.0f == thr2"), ([0, 0, 4], [xp, 0, 4], 100, 1, 1, "err2 one step under thr2"),
        ([0, x9, 4], [0, 0, 4], 100, 1, 0, "err2 == thr2 along y"),
        ([0, 0, 4], [0, 0, 4], 0.1, 1, 0, "threshold 0: no inlier at zero error"), ([0, 0, 4], [0, 0, 4], 1, 0.1, 0, "threshold 0 on the other term"),
        ([0, 0, 4], [0, 0, 4], 0.109, 0.109, 1, "threshold 1, zero error"),
        ([0, 0, 1], [1.0 / 512, 0, 1], 0.109, 100, 0, "err1 == 1.0f == thr1"), ([0, 0, 1], [np.nextafter(F32(1.0 / 512), F32(0)), 0, 1], 0.109, 100, 1, "one step under 1"),
        ([0, 0, 0], [0, 0, 4], 1, 1, 0, "a = 0: 0 / 0 = NaN"), ([0.1, 0.1, 0], [0.1, 0.1, 4], 1, 1, 0, "a.z = 0: inf"),
        ([0.5, 0.25, 4], [0.5, 0.25, 0], 1, 1, 0, "b.z = 0: inf"),
        ([0.5, 0.25, 4], [-0.5, -0.25, -4], 1, 1, 1, "b = -a: behind camera 2, same projection, err == 0: upstream has no depth test"),
        ([-0.5, 0.25, -8], [-0.5, 0.25, -8], 1, 1, 1, "both behind their cameras, err == 0"),
        ([0, 0, 4], [0.5, 0, 4], 100, 100, 0, "64 px off: a plain outlier"),
        ([0.25, 0.5, 8], [0.25, 0.5, 8], 1, 1, 1, "plain inlier"), ([0.25, 0.5, 8], [0.25, 0.5, 8], 1, 1, 1, "plain inlier"),
        ([0.25, 0.5, 8], [0.25, 0.5, 8], 1, 1, 1, "plain inlier"), ([0.25, 0.5, 8], [0.25, 0.5, 8], 1, 1, 1, "plain inlier")]
    X1 = np.array([r[0] for r in rows], F32); X2 = np.array([r[1] for r in rows], F32)
    s1 = np.array([r[2] for r in rows], F32); s2 = np.array([r[3] for r in rows], F32)
    mask = np.array([r[4] for r in rows], bool)
    tri = np.array([[0, 1, 2], [2, 0, 1]], np.int32)
    c = Case("identity_path_n24", "exact rungs, threshold 0 and 1, NaN / inf / negative depths on the identity path", X1, X2, s1, s2, K_POW2, K_POW2, tri,
             truth=(np.eye(3), np.zeros(3), 1.0), expect_valid=np.zeros(2, bool), expect_n={0: int(mask.sum()), 1: int(mask.sum())},
             expect_mask={0: mask, 1: mask}, extra=dict(why=[r[5] for r in rows]))
    assert c.n == 24
    return c


def minimal_n3_case():
    """n = 3: the smallest solver; the six orders of its one minimal set, repeated."""
    rng = np.random.default_rng(600)
    R, s = rotvec([0.2, 0.1, -0.3]), 0.8
    t = _recentre(R, s)
    X2 = _box(rng, 3).astype(F32)
    X1 = (s * (X2.astype(np.float64) @ R.T) + t).astype(F32)
    perms = [[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]]
    tri = np.array((perms * 12)[:N_HYP], np.int32)
    sg = np.ones(3, F32)
    c = Case("minimal_n3", "three correspondences", X1, X2, sg, sg, K_TUM, K_POW2 + F32(8), tri, fix_scale=True, truth=(R, t, 1.0))
    c.props = np.zeros(c.H, bool)
    return c


_cache = {}


def all_cases():
    """Every scene case, built once."""
    if "all" not in _cache:
        _cache["all"] = (rotation_cases() + scale_cases() + [skinny_case(), degenerate_case()] + identity_trap_cases()
                         + [ladder_case(), identity_path_case(), minimal_n3_case()])
        ids = [c.id for c in _cache["all"]]
        assert len(set(ids)) == len(ids)
        assert sum(c.n == 257 for c in _cache["all"]) == 1 and sum(c.n == 129 for c in _cache["all"]) == 1
    return _cache["all"]


def case(id):
    return next(c for c in all_cases() if c.id == id)


def parity_error(c, res, ref=None):
    """Worst distance of a result dict from horn64 (ref None) or from another result dict over the kept triples: (dR, dt, ds, self-residual)."""
    dR = dt = ds = sr = 0.0
    for h in np.flatnonzero(c.keep):
        if ref is None:
            R0, t0, s0 = c.horn[h].R, c.horn[h].t, c.horn[h].s
        else:
            R0, t0, s0 = ref["R"][h].astype(np.float64), ref["t"][h].astype(np.float64), float(ref["s"][h])
        R, t, s = res["R"][h].astype(np.float64), res["t"][h].astype(np.float64), float(res["s"][h])
        dR = max(dR, np.abs(R - R0).max()); dt = max(dt, np.abs(t - t0).max() / max(1.0, np.abs(t0).max())); ds = max(ds, abs(s - s0) / s0)
        p1, p2 = c.X1[c.tri[h]].astype(np.float64), c.X2[c.tri[h]].astype(np.float64)
        if not c.fix_scale:
            sr = max(sr, np.abs(s * (p2 @ R.T) + t - p1).max() / max(1.0, np.abs(p1).max()))
    return dR, dt, ds, sr


def check_properties(c, res, h):
    """A valid hypothesis where the rotation is weakly determined: finite, a rotation, maps its own three points onto their counterparts, the truth's scale."""
    R, t, s = res["R"][h].astype(np.float64), res["t"][h].astype(np.float64), float(res["s"][h])
    assert np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s), f"{c.id}[{h}]: not finite"
    assert abs(np.linalg.det(R) - 1) < PROP_ORTHO and np.abs(R @ R.T - np.eye(3)).max() < PROP_ORTHO, f"{c.id}[{h}]: not a rotation"
    p1, p2 = c.X1[c.tri[h]].astype(np.float64), c.X2[c.tri[h]].astype(np.float64)
    res3 = np.abs(s * (p2 @ R.T) + t - p1).max() / max(1.0, np.abs(p1).max())
    assert res3 < PROP_SELF, f"{c.id}[{h}]: the minimal set maps {res3:.2e} off itself"
    if not c.fix_scale:
        assert abs(s - c.truth[2]) < PROP_SCALE * c.truth[2], f"{c.id}[{h}]: scale {s} against {c.truth[2]}"


# ---- ComputeInliersNum cases --------------------------------------------------------------------------------------------------------------
def _ulp_pair_kp(sigma2):
    """Key-point offsets (4, dy) whose float32 error 16 + dy * dy is the largest float32 below 2 * 9.210 * sigma2 (an inlier: the comparison is in double
    and strict) and the next float32 (not an inlier)."""
    thr = 2 * 9.210 * float(F32(sigma2))
    lo = F32(thr)
    if float(lo) >= thr:
        lo = np.nextafter(lo, F32(0))
    hi = np.nextafter(lo, F32(np.inf))
    assert float(lo) < thr <= float(hi)
    out = []
    for e in (lo, hi):
        dy0 = F32(np.sqrt(float(e) - 16.0))
        cand = dy0
        for k in range(200):
            for cand in (_step(dy0, k), _step(dy0, -k)):
                if F32(F32(4) * F32(4)) + cand * cand == e:
                    break
            else:
                continue
            break
        else:
            raise AssertionError("no dy gives the wanted float32 error")
        out.append(cand)
    return out, (lo, hi)


def _step(x, k):
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf))
    return x


def inliers_num_cases():
    """Dicts of the arguments of rumi_sim3_inliers / O.sim3_inliers plus `expect` (stated flags where the rule is the point) and `id`."""
    rng = np.random.default_rng(700)
    ident = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
    R, t, s = rotvec([0.3, -0.2, 0.5]), np.array([0.2, -0.1, 0.4]), 1.3
    S12, S21 = sim8(R, t, s), sim8(*sim_inv((R, t, s)))
    rows = []          # pair, X1, X2, kp1, kp2, sigma1, sigma2, edge1, edge2, expect, why

    def generic(off1, off2, e1, e2, expect, why):
        X2 = _box(rng, 1)[0].astype(F32)
        X1 = (s * (R @ X2.astype(np.float64)) + t).astype(F32)
        kp1 = project(K_TUM, s * (R @ X2.astype(np.float64)) + t)[0] + off1
        kp2 = project(K_TUM, X2.astype(np.float64))[0] + off2
        rows.append((0, X1, X2, kp1, kp2, 1.0, 1.44, e1, e2, expect, why))

    generic([0.5, -0.5], [0.3, 0.2], 0, 0, 1, "both errors small")
    generic([30, 0], [0, 0], 0, 1, 1, "err1 fails, rescued by edge2 (the map-2 point's flag)")
    generic([0, 0], [0, 30], 1, 0, 1, "err2 fails, rescued by edge1 (the map-1 point's flag)")
    generic([30, 0], [0, 0], 1, 0, 0, "err1 fails, only edge1 set: the wrong side, not rescued")
    generic([0, 0], [0, 30], 0, 1, 0, "err2 fails, only edge2 set: the wrong side, not rescued")
    generic([30, 0], [0, 30], 1, 1, 1, "both fail, both flags: rescued")
    generic([30, 0], [0, 30], 0, 0, 0, "both fail, no flag")
    generic([0.2, 0.1], [0.1, 0.1], 1, 1, 1, "inlier with both flags")
    # pair 1: identity maps, K = (512, 512, 0, 0), the point on the axis at depth 4: u = v = 0 exactly and the error is kp . kp in float32
    P = np.array([0, 0, 4], F32)
    for sig in (1.0, 1.44):
        (dlo, dhi), _ = _ulp_pair_kp(sig)
        rows.append((1, P, P, [4, dlo], [0, 0], sig, 1.0, 0, 0, 1, f"err1 one float32 under 2*9.210*{sig}"))
        rows.append((1, P, P, [4, dhi], [0, 0], sig, 1.0, 0, 0, 0, f"err1 one float32 over 2*9.210*{sig}"))
        rows.append((1, P, P, [0, 0], [4, dlo], 1.0, sig, 0, 0, 1, f"err2 one float32 under 2*9.210*{sig}"))
        rows.append((1, P, P, [0, 0], [4, dhi], 1.0, sig, 0, 0, 0, f"err2 one float32 over 2*9.210*{sig}"))
    rows.append((1, P, np.array([0.1, 0.1, 0], F32), [0, 0], [0, 0], 1.0, 1.0, 0, 0, 0, "pz == 0: inf, not an inlier"))
    rows.append((1, np.array([0, 0, 0], F32), P, [0, 0], [0, 0], 1.0, 1.0, 0, 0, 0, "0 / 0 = NaN, not an inlier"))
    rows.append((1, P, np.array([0.5, 0.25, -4], F32), [-64, -32], [0, 0], 1.0, 1.0, 0, 0, 1, "pz < 0 with zero error: an inlier, upstream has no depth test"))
    rows.append((1, P, np.array([0.1, 0.1, 0], F32), [0, 0], [0, 0], 1.0, 1.0, 0, 1, 1, "pz == 0 rescued by edge2"))
    # pair 2: no correspondences (ratio 0); pair 3: two inliers over denominator 0 (ratio 0)
    rows.append((3, P, P, [0, 0], [0, 0], 1.0, 1.0, 0, 0, 1, "inlier of the pair with denominator 0"))
    rows.append((3, P, P, [1, 1], [0, 0], 1.0, 1.0, 0, 0, 1, "inlier of the pair with denominator 0"))

    def build(id, pairs, dens):
        """pairs: which of the four pairs take part, in order; the median is element [n/2] of the sorted ratios."""
        sel = [[r for r in rows if r[0] == p] for p in pairs]
        flat = [r for group in sel for r in group]
        ps = np.cumsum([0] + [len(g) for g in sel]).astype(np.int32)
        simA = {0: S12, 1: ident, 2: ident, 3: ident}; simB = {0: S21, 1: ident, 2: ident, 3: ident}
        # one K per call: the generic pair is used with K_TUM, the exact pairs with K_POW2, never mixed
        K = K_TUM if pairs == [0] else K_POW2
        col = lambda j, dt, w: (np.array([r[j] for r in flat], dt).reshape(-1, w) if flat else np.zeros((0, w), dt))
        return dict(id=id, pair_start=ps, pair_denominator=np.array(dens, np.int32), S_c1w2=np.stack([simA[p] for p in pairs]), S_c2w1=np.stack([simB[p] for p in pairs]),
                    K4_1=K, K4_2=K, X1=col(1, F32, 3), X2=col(2, F32, 3), kp1=col(3, F32, 2), kp2=col(4, F32, 2), sigma2_1=col(5, F32, 1).ravel(),
                    sigma2_2=col(6, F32, 1).ravel(), edge1=col(7, np.uint8, 1).ravel(), edge2=col(8, np.uint8, 1).ravel(),
                    expect=np.array([r[9] for r in flat], np.uint8), why=[r[10] for r in flat])

    n1 = sum(r[0] == 1 for r in rows)
    return [build("edges_one_pair", [0], [10]),                                   # n_pairs = 1: the median is the only ratio
            build("ulp_two_pairs", [1, 3], [n1]  + [0]),                          # n_pairs = 2: [n/2] is the upper of the two; here the zero-denominator pair is the lower
            build("two_pairs_upper_middle", [3, 1], [4, 2 * n1]),                 # ratios 0.5 and below: the larger one is returned
            build("four_pairs", [1, 2, 3, 1], [n1, 5, 0, 3 * n1]),                # n_pairs = 4 with an empty pair and a zero denominator: element [2] of the sorted ratios
            build("empty_pair_only", [2], [7])]                                   # one pair of zero correspondences: total == 0


def inliers_args(c):
    return (c["pair_start"], c["pair_denominator"], c["S_c1w2"], c["S_c2w1"], c["K4_1"], c["K4_2"], c["X1"], c["X2"], c["kp1"], c["kp2"], c["sigma2_1"],
            c["sigma2_2"], c["edge1"], c["edge2"])


# ---- OptimizeSim3 cases ---------------------------------------------------------------------------------------------------------------------
def optimize_cases():
    """Dicts with the arguments of rumi_optimize_sim3 / O.optimize_sim3 (pair form) and the outcome the case is named after."""
    out = []
    # perfect data started at the truth: identity rotation, s = 2, t = (1, 2, 0), grid points at power-of-two depths under K = (512, 512, 0, 0): both maps and
    # both projections are exact in double, chi2 == 0, b == 0, the step is 0, rho == 0 and Levenberg-Marquardt stops at once
    rng = np.random.default_rng(800)
    n = 24
    P2 = np.stack([rng.integers(-8, 9, n) / 8.0, rng.integers(-8, 9, n) / 8.0, 2.0 ** rng.integers(1, 4, n)], 1)
    P1 = 2 * P2 + np.array([1, 2, 0.0])
    S = np.array([0, 0, 0, 1, 1, 2, 0, 2.0])
    o1, o2 = project(K_POW2, P1), project(K_POW2, P2)
    assert np.array_equal(o1.astype(F32).astype(np.float64), o1) and np.array_equal(o2.astype(F32).astype(np.float64), o2)
    out.append(dict(id="perfect_at_truth", S0=S, S_true=S, P1c=P1.astype(F32), P2c=P2.astype(F32), obs1=o1.astype(F32), obs2=o2.astype(F32), w1=np.ones(n, F32),
                    w2=np.ones(n, F32), K=K_POW2, skip12=None, skip21=None, expect=dict(res=(n, 0, 0), unchanged=True)))

    def noisy(id, seed, n, n_out, R, s, init_rot, noise=0.3, skips=None, expect=None):
        rng = np.random.default_rng(seed)
        t = _recentre(R, s)
        P2 = _box(rng, n); P1 = s * (P2 @ R.T) + t
        o1 = project(K_TUM, P1) + rng.normal(0, noise, (n, 2)); o2 = project(K_TUM, P2) + rng.normal(0, noise, (n, 2))
        o1[:n_out] += 50.0 * rng.choice([-1, 1], (n_out, 2))
        R0 = rotvec(np.array([0.6, -0.5, 0.62]) * init_rot) @ R
        S0 = sim8(R0, t + np.array([0.01, -0.01, 0.01]), s * 1.01)
        d = dict(id=id, S0=S0, S_true=sim8(R, t, s), P1c=P1.astype(F32), P2c=P2.astype(F32), obs1=o1.astype(F32), obs2=o2.astype(F32), w1=np.ones(n, F32),
                 w2=np.ones(n, F32), K=K_TUM, skip12=None, skip21=None, expect=expect or {})
        if skips:
            d["skip12"], d["skip21"] = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            d["skip12"][skips[0]] = 1; d["skip21"][skips[1]] = 1
        return d

    Rs = rotvec([0.04, -0.12, 0.07])
    # n - nBad < 10 on each side of the boundary: four matches 50 px off are removed after the first pass
    out.append(noisy("ten_survivors", 801, 14, 4, Rs, 1.3, 0.005, expect=dict(nBad=4, early=0)))
    out.append(noisy("nine_survivors", 802, 13, 4, Rs, 1.3, 0.005, expect=dict(nBad=4, early=1, nIn=0)))
    # a truth with a 180 deg rotation (quaternion w of about 0), started 0.01 rad away
    out.append(noisy("half_turn", 803, 40, 0, rotvec(AXIS_SKEW * np.pi), 1.1, 0.01, expect=dict(nBad=0, early=0, nIn=40)))
    # one correspondence with only its 2-1 edge (skip12) and one with only its 1-2 edge (skip21): status 3, not counted (:2450-2451)
    out.append(noisy("one_sided_edges", 804, 30, 0, Rs, 1.3, 0.005, skips=(5, 11), expect=dict(nBad=0, early=0, nIn=28, status3=[5, 11])))
    return out


def optimize_args(c):
    return (c["S0"], c["P1c"], c["P2c"], c["obs1"], c["obs2"], c["w1"], c["w2"], c["K"], c["K"], 10.0, False, True)


# ---- the identity trap under the sequential rule: drivers shared by the CPU test (over the oracle) and the GPU test (over the device) --------------------
SEQUENCES = {"first": ["I", "G"],                        # the degenerate set is the solver's first iteration
             "middle": ["B", "I", "B2", "I2", "G"]}      # and in the middle: it repeats the count of the iteration before, which did not return


def _filler(count, seed=5):
    g = GlibcRand(seed)
    return [g.rand() for _ in range(count)]


def trap_scene():
    """trap_sequence_scene, built once."""
    if "trap" not in _cache:
        _cache["trap"] = trap_sequence_scene()
    return _cache["trap"]


def trap_solver(opt, arrangement):
    """A mirror Sim3Solver over the trap scene whose generator draws the named minimal sets, then G2 for ever.  Returns (solver, the sets, the scene)."""
    from rumi_slam_amd.sim3solver import Sim3Solver
    sc = trap_scene()
    tri = np.array([sc["names"][k] for k in SEQUENCES[arrangement]] + [sc["names"]["G2"]] * 40, np.int32)
    s = Sim3Solver(opt, sc["X1"], sc["X2"], sc["s1"], sc["s2"], sc["K"], sc["K"], rng=ScriptRand(script_words(sc["n"], tri)), indices1=np.arange(sc["n"]) * 2,
                   mN1=2 * sc["n"])
    s.SetRansacParameters(0.99, sc["min_inliers"], 300)
    return s, tri, sc


def drive(s, mode, score, n_per_call=20):
    """while (!converged && !bNoMore) iterate(n_per_call), in the three forms of iterate."""
    conv = no_more = False
    ratio, calls, T, vb, n_in = 0.0, 0, None, None, 0
    while not conv and not no_more:
        calls += 1
        if mode == "plain":
            T, no_more, vb, n_in = s.iterate(n_per_call)
            conv = n_in > 0
        elif mode == "converge":
            T, no_more, vb, n_in, conv = s.iterate_converge(n_per_call)
        else:
            T, no_more, conv, ratio = s.iterate_rumination(n_per_call, score, ratio)
    return dict(conv=conv, calls=calls, T=T, vb=vb, n_in=n_in, ratio=ratio)


BATCH_FIRST, BATCH_LAST = [[0, 5, 10]], [[1, 7, 13]]     # the minimal sets of the two ordinary solvers (N = 16 and N = 20)


def trap_batch_solvers(opt, arrangement):
    """Three mirror solvers over one scripted generator: an ordinary one (N = 16, converges at once), the trap (N = 30) or, for "identical", a solver whose
    maps are identical throughout with six iterations left, and another ordinary one (N = 20).  Returns (solvers, generator, iterations the middle one uses)."""
    from rumi_slam_amd.sim3solver import Sim3Solver
    for key, (seed, n) in (("ordA", (420, 16)), ("ordC", (421, 20))):
        if key not in _cache:
            _cache[key] = ordinary_scene(seed, n)
    A, C, trap = _cache["ordA"], _cache["ordC"], trap_scene()
    if arrangement == "identical":
        mid = dict(trap, X1=trap["X2"])
        mid_words, used = _filler(18, 6), 6
    else:
        mid = trap
        seq = [trap["names"][k] for k in SEQUENCES[arrangement]]
        mid_words, used = script_words(trap["n"], seq), len(seq)
    rng = ScriptRand(script_words(A["n"], BATCH_FIRST) + mid_words + script_words(C["n"], BATCH_LAST) + _filler(900))
    solvers = []
    for sc in (A, mid, C):
        s = Sim3Solver(opt, sc["X1"], sc["X2"], sc["s1"], sc["s2"], sc["K"], sc["K"], rng=rng, indices1=np.arange(sc["n"]) * 2, mN1=2 * sc["n"])
        s.SetRansacParameters(0.99, sc["min_inliers"], 300)
        solvers.append(s)
    if arrangement == "identical":
        solvers[1].mRansacMaxIts = 6
    return solvers, rng, used
