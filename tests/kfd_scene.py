"""Frames for the tests of the PD frame selector (include/rumi_kfd.h), and the binding of their scalar oracle (tests/cpp/kfd_oracle.cc).
TEST INFRASTRUCTURE.

The texture is a sum of random sinusoids evaluated analytically, so a frame "shifted by (dx, dy)" is the same function sampled at (x - dx, y - dy):
sub-pixel ground truth without interpolation.  The constructed cases hold one rule of the tracker each; tests/test_kfd_cpu.py asserts on the
oracle's per-level diagnosis that each case takes the path it is named after, tests/test_kfd_gpu.py that the device gives the oracle's bits."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# how a level ended (the oracle's diag): code | iterations << 8
SKIP_BOUNDS, GATE_MIN_EIG, GATE_DET, LEFT_FRAME, EPS_BREAK, OSCILLATION, ALL_ITERATIONS = range(7)


class Texture:
    """128 + sum of a_k sin(2 pi (u_k x + v_k y) + phi_k): wavelengths from `lo` to `hi` pixels, so that every LK level sees structure."""

    def __init__(self, seed, terms=24, lo=9.0, hi=70.0, amp=100.0):
        rng = np.random.default_rng(seed)
        wl = np.exp(rng.uniform(np.log(lo), np.log(hi), terms))
        th = rng.uniform(0, 2 * np.pi, terms)
        self.u, self.v = np.cos(th) / wl, np.sin(th) / wl
        self.phi = rng.uniform(0, 2 * np.pi, terms)
        a = rng.uniform(0.5, 1.0, terms)
        self.a = a * amp / np.sqrt((a ** 2).sum() * 0.5) / 2.5          # about 2.5 sigma inside the 8-bit range

    def frame(self, w, h, shift=(0.0, 0.0)):
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        x, y = x - shift[0], y - shift[1]
        f = np.full((h, w), 128.0)
        for a, u, v, p in zip(self.a, self.u, self.v, self.phi):
            f += a * np.sin(2 * np.pi * (u * x + v * y) + p)
        return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def grid_points(w, h, margin=40, step=8.0, jitter_seed=5):
    """Points at least `margin` pixels inside a w x h frame, on a jittered lattice (fractional coordinates)."""
    rng = np.random.default_rng(jitter_seed)
    xs, ys = np.arange(margin, w - margin + 1e-6, step), np.arange(margin, h - margin + 1e-6, step)
    p = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2) + rng.uniform(0, 0.999, (len(xs) * len(ys), 2))
    p[:, 0] = np.clip(p[:, 0], margin, w - margin)
    p[:, 1] = np.clip(p[:, 1], margin, h - margin)
    return p.astype(np.float32)


def level_sizes(w, h):
    out = [(h, w)]
    for _ in range(2):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


# ---- the C++ oracle ---------------------------------------------------------------------------------------------------------------------------
class KfoStep(C.Structure):
    _fields_ = [("selected", C.c_int32), ("n_tracked", C.c_int32), ("n_good", C.c_int32), ("moptf", C.c_float), ("pd_out", C.c_float), ("th", C.c_float)]


def build_oracle(out_dir):
    so = os.path.join(str(out_dir), "libkfd_oracle.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "kfd_oracle.cc"), "-o", so])
    L = C.CDLL(so)
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    L.kfo_grey_bgr.argtypes = [vp, i32, i32, i32, vp]
    L.kfo_pyr_down.argtypes = [vp, i32, i32, vp]
    L.kfo_scharr.argtypes = [vp, i32, i32, vp]
    L.kfo_window.argtypes = [vp, vp, vp, i32, i32, f32, f32, f32, f32, vp, vp, vp, vp, vp, vp]
    L.kfo_track.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp]
    L.kfo_pd_update.argtypes = [vp, f32, C.c_double]
    L.kfo_pd_update.restype = f32
    L.kfo_create.argtypes = [f32, f32, f32]
    L.kfo_create.restype = vp
    L.kfo_destroy.argtypes = [vp]
    L.kfo_set_pd.argtypes = [vp, f32, f32, f32]
    L.kfo_reset.argtypes = [vp]
    L.kfo_old.argtypes = [vp, vp]
    L.kfo_prev_input.argtypes = [vp]
    L.kfo_prev_input.restype = f32
    L.kfo_step.argtypes = [vp, vp, i32, i32, i32, C.c_double, C.POINTER(KfoStep), vp, vp]
    L.kfo_set_keypoints.argtypes = [vp, vp, i32]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def oracle_grey(L, bgr):
    bgr = np.ascontiguousarray(bgr)
    h, w, _ = bgr.shape
    out = np.zeros((h, w), np.uint8)
    L.kfo_grey_bgr(_p(bgr), w, h, bgr.strides[0], _p(out))
    return out


def oracle_pyr_down(L, img):
    img = np.ascontiguousarray(img)
    h, w = img.shape
    out = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
    L.kfo_pyr_down(_p(img), w, h, _p(out))
    return out


def oracle_scharr(L, img):
    img = np.ascontiguousarray(img)
    h, w = img.shape
    out = np.zeros((h, w, 2), np.int16)
    L.kfo_scharr(_p(img), w, h, _p(out))
    return out


def oracle_window(L, img, der, nxt, p, q):
    """The window whose top-left corner is the float position p in `img`, and the mismatch sums against the window at q in `nxt`:
    (I, Ix, Iy [31, 31] i32, weights [8] i32 (prev then next), A [3] i64, b [2] i64)."""
    h, w = img.shape
    I, Ix, Iy = (np.zeros((31, 31), np.int32) for _ in range(3))
    wts, A, b = np.zeros(8, np.int32), np.zeros(3, np.int64), np.zeros(2, np.int64)
    L.kfo_window(_p(np.ascontiguousarray(img)), _p(np.ascontiguousarray(der)), _p(np.ascontiguousarray(nxt)), w, h, float(p[0]), float(p[1]), float(q[0]), float(q[1]),
                 _p(I), _p(Ix), _p(Iy), _p(wts), _p(A), _p(b))
    return I, Ix, Iy, wts, A, b


def oracle_track(L, prev, cur, pts, dumps=False):
    """(next [n, 2] f32, status [n] u8, diag [n, 3] i32 indexed by level) and, with dumps, the levels and derivatives of `prev` as KFDSampler.track
    returns them."""
    prev, cur = np.ascontiguousarray(prev), np.ascontiguousarray(cur)
    h, w = prev.shape
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    nxt, status, diag = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros((n, 3), np.int32)
    sizes = level_sizes(w, h)
    total = sum(a * b for a, b in sizes)
    pyr, der = np.zeros(total, np.uint8), np.zeros(2 * total, np.int16)
    L.kfo_track(_p(prev), _p(cur), w, h, _p(pts), n, _p(nxt), _p(status), _p(diag), _p(pyr) if dumps else None, _p(der) if dumps else None)
    if not dumps:
        return nxt, status, diag
    levels, derivs, o = [], [], 0
    for a, b in sizes:
        levels.append(pyr[o:o + a * b].reshape(a, b))
        derivs.append(der[2 * o:2 * (o + a * b)].reshape(a, b, 2))
        o += a * b
    return nxt, status, diag, levels, derivs


class OracleSampler:
    """KFDSample over the oracle.  `extract(grey) -> (mono, keypoints, descriptors)` stands for the ORB extractor of the selected frames."""

    def __init__(self, L, extract, Kp=0.8, Kd=0.005, th=10.0):
        self.L, self.extract = L, extract
        self.h = L.kfo_create(Kp, Kd, th)

    def __del__(self):
        self.L.kfo_destroy(self.h)

    def set_pd(self, Kp, Kd, th):
        self.L.kfo_set_pd(self.h, Kp, Kd, th)

    def reset(self):
        self.L.kfo_reset(self.h)

    def old(self):
        n = self.L.kfo_old(self.h, None)
        out = np.zeros((n, 2), np.float32)
        self.L.kfo_old(self.h, _p(out))
        return out

    def prev_input(self):
        return np.float32(self.L.kfo_prev_input(self.h))

    def step(self, grey, t):
        """(KfoStep, next, status, extraction or None)"""
        grey = np.ascontiguousarray(grey)
        h, w = grey.shape
        n = self.L.kfo_old(self.h, None)
        nxt, status = np.zeros((max(n, 1), 2), np.float32), np.zeros(max(n, 1), np.uint8)
        out = KfoStep()
        self.L.kfo_step(self.h, _p(grey), w, h, grey.strides[0], float(t), C.byref(out), _p(nxt), _p(status))
        ext = None
        if out.selected:
            ext = self.extract(grey)
            xy = np.ascontiguousarray(np.stack([ext[1]["x"], ext[1]["y"]], 1), np.float32)
            self.L.kfo_set_keypoints(self.h, _p(xy), len(xy))
        return out, nxt[:out.n_tracked], status[:out.n_tracked], ext


# ---- the 8-frame sequence of the step tests ---------------------------------------------------------------------------------------------------------
SEQ_SHIFTS = [(0, 0), (0.4, 0.2), (0.9, 0.1), (3.2, 1.1), (3.5, 1.4), (3.6, 1.4), (6.1, 2.9), (6.3, 3.0)]     # camera position per frame
SEQ_TIMES = [10.0, 10.033, 10.067, 10.1, 10.15, 10.183, 10.217, 10.25]
SEQ_PD = (0.8, 0.005, 1.5)                                                                                   # Kp, Kd, th: a flow above ~1.5 px selects


def sequence(w=160, h=128, seed=21):
    tex = Texture(seed)
    return [tex.frame(w, h, s) for s in SEQ_SHIFTS]


# ---- constructed cases: one rule of the tracker each ----------------------------------------------------------------------------------------------------
def checker(w, h, cell, shift=0):
    """Cells of `cell` pixels, 30 / 220, moved right by `shift` whole pixels."""
    cx = ((np.arange(w) - shift) // cell) % 2
    cy = (np.arange(h) // cell) % 2
    return np.where(cx[None, :] ^ cy[:, None], 220, 30).astype(np.uint8)


class Case:
    """prev, cur, pts and what the oracle must report: status [n] and {(point, level): code} (test_kfd_cpu.py asserts both)."""

    def __init__(self, name, prev, cur, pts, status, codes):
        self.name, self.prev, self.cur = name, prev, cur
        self.pts = np.asarray(pts, np.float32).reshape(-1, 2)
        self.status, self.codes = list(status), dict(codes)


def constructed_cases(w, h, seed=21):
    tex = Texture(seed)
    base = tex.frame(w, h)
    cases = []
    # The level-0 window starts at floor(pt - 15) and the bounds test lets it start 31 pixels before the frame or on its last pixel.  32 off: refused
    # by the test.  31 off: admitted, but the one column or row of derivatives under the window has dx = 0 (or dy = 0) by reflection, so the
    # normal matrix is singular and the minEig gate ends it.  30 off: tracked.
    off = []
    for p32, p31, p30 in [((-16.25, 64), (-15.25, 64), (-14.25, 64)), ((w + 15.0, 64), (w + 14.25, 64), (w + 13.25, 64)),
                          ((80, -17.0), (80, -15.25), (80, -14.25)), ((80, h + 15.0), (80, h + 14.25), (80, h + 13.25))]:
        off += [p32, p31, p30]
    cases.append(Case("borders", base, base, off, [0, 0, 1] * 4, {(i, 0): [SKIP_BOUNDS, GATE_MIN_EIG, EPS_BREAK][i % 3] for i in range(12)}))
    # moving out to the left: found on levels 2 and 1, then the window start passes -31 on level 0 (point 0 at once, point 1 after some iterations)
    cases.append(Case("leaves_frame", base, tex.frame(w, h, (-6, 0)), [(-10, 64.3), (-5, 64)], [0, 0], {(0, 0): LEFT_FRAME, (1, 0): LEFT_FRAME}))
    flat = base.copy()
    flat[30:90, 40:110] = 77
    cases.append(Case("flat_patch", flat, flat, [(75.3, 60.2)], [0], {(0, 0): GATE_MIN_EIG}))
    # One straight edge: Iy = 0, the matrix has rank 1.  minEig and D are both zero; the reference tests minEig first, and D < FLT_EPSILON can never
    # be the only one to fire (minEig >= 1e-4 means both eigenvalues are at least 0.19, so D >= 0.036).
    edge = np.full((h, w), 40, np.uint8)
    edge[:, 80:] = 200
    cases.append(Case("edge_only", edge, edge, [(80.3, 60.2)], [0], {(0, 0): GATE_MIN_EIG, (0, 1): GATE_MIN_EIG, (0, 2): GATE_MIN_EIG}))
    cases.append(Case("integer_point", base, tex.frame(w, h, (1, 0)), [(64, 64)], [1], {(0, 0): EPS_BREAK}))
    # checkers: two-pixel cells vanish under pyrDown (levels 2 and 1 are flat: the point is lost there and found again on level 0)
    c2 = checker(w, h, 2)
    cases.append(Case("lost_then_recovered", c2, checker(w, h, 2, 1), [(80, 64)], [1], {(0, 2): GATE_MIN_EIG, (0, 1): GATE_MIN_EIG, (0, 0): EPS_BREAK}))
    cases.append(Case("all_iterations", c2, checker(w, h, 2, 1), [(80.4, 64.3)], [1], {(0, 0): ALL_ITERATIONS}))
    cases.append(Case("oscillation", checker(w, h, 4), checker(w, h, 4, 1), [(80, 64)], [1], {(0, 1): OSCILLATION}))
    cases.append(Case("oscillation_half_period", c2, checker(w, h, 2, 2), [(80.4, 64.3)], [1], {(0, 0): OSCILLATION}))
    return cases
