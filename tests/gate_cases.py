"""Constructed cases for the projection gates: the chain of float comparisons that decides whether a map point is searched, where, and at which
pyramid level (depth sign, image rectangle, distance range, viewing cosine, PredictScale, window radius).  Every case stands ON an edge of one
gate and states, from the reference's rule (cited by file and line, never quoted), at which gate each member drops the point.

Nothing here needs a GPU or the oracle library to BUILD a case.  Geometry is exact in float32 up to the gate a case stands on:
K = (512, 512, 320, 240); the identity pose, or POSE_X (a half turn about x, q = (1, 0, 0, 0), with a dyadic translation, so Ow != 0); a default
point at camera coordinates (0, 0, 4): dist = 4, dot = 4 n_z, viewCos = n_z; dyadic x, y at z = 4 give u = 128 x + 320.  What follows a gate
(the norm of an off-axis point, the level of an accepted one) is evaluated operation by operation in numpy float32, and the builder asserts
that none of those values is itself near an edge.

Families: Z depth, I image rectangle, D distance range, C viewing cosine, L predicted level, R window radius, V division variant, S fields of
a rejected point.  ``COVERAGE`` / ``NOT_APPLICABLE`` name, for every member x family cell, the cases or the reason.

Verdict classes (what a case spells out per point: None = searched, or the letter of the gate that drops it):
  F     Frame::isInFrustum, and SearchByProjection(F, points) behind it   Frame.cc:558-617           z < 0 | closed rectangle | D | C in float
  LAST  SearchByProjection(Cur, Last)                                      ORBmatcher.cc:1516-1553   1/z < 0 through double | closed | - | -
  RELOC SearchByProjection(F, KF, found, th, ORBdist)                      ORBmatcher.cc:1700-1733   - | closed | D | -
  KF    SearchByProjection(KF, Scw, points) both overloads, Fuse           ORBmatcher.cc:389-436, 491-539, 1058-1112   z < 0 | [min, max) | D | C in double
  SIM3  SearchBySim3                                                       ORBmatcher.cc:1329-1371   z < 0 | [min, max) | D on |Pc| | -"""
import math

import numpy as np

import match_cases as MC
from match_cases import K4, LOG_SF, SF, Proj

f32 = np.float32
FAMILIES = "ZIDCLRVS"
SEARCH_MEMBERS = ["MP", "LAST", "RELOC", "SIM3P", "FUSE", "SIM3"]
MEMBERS = ["FRUSTUM"] + SEARCH_MEMBERS + ["SIN", "SAF"]
MEMBER_NAMES = {"FRUSTUM": "Frame::isInFrustum Frame.cc:558 (k_is_in_frustum, k_track_frustum)", "MP": MC.MEMBER_NAMES["MP"], "LAST": MC.MEMBER_NAMES["LAST"],
                "RELOC": MC.MEMBER_NAMES["RELOC"], "SIM3P": MC.MEMBER_NAMES["SIM3P"], "FUSE": MC.MEMBER_NAMES["FUSE"], "SIM3": MC.MEMBER_NAMES["SIM3"],
                "SIN": "Fuse as LocalMapping::SearchInNeighbors calls it", "SAF": "Fuse as LoopClosing::SearchAndFuse calls it"}
CLASS_OF = {"FRUSTUM": "F", "MP": "F", "LAST": "LAST", "RELOC": "RELOC", "SIM3P": "KF", "FUSE": "KF", "SIM3": "SIM3"}
W, H = 640, 480
BOUNDS = (0.0, 0.0, float(W), float(H))
# Frame::ComputeImageBounds of the 752 x 480 EuRoC camera (Frame.cc:799-826): negative, non-integral minima.  Stated here so that building a case
# needs no oracle; the CPU test holds them against oracle_lib.image_bounds, the GPU test against the tracker's.
EUROC_K = np.array([458.654, 457.296, 367.215, 248.375], f32)
EUROC_DIST = np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0], f32)
EUROC_BOUNDS = tuple(float.fromhex(h) for h in ("-0x1.0f975ep+7", "-0x1.738004p+6", "0x1.bfc0fp+9", "0x1.1ac6ccp+9"))
assert all(float(f32(b)) == b for b in EUROC_BOUNDS) and EUROC_BOUNDS[0] < -100 and EUROC_BOUNDS[0] != round(EUROC_BOUNDS[0])
FX, CX, CY = f32(512), f32(320), f32(240)
COS_DEFAULT = f32(0.75)
ONE_TWO, POINT_EIGHT = f32(1.2), f32(0.8)
MIN_DEFAULT, MAX_DEFAULT, LEVEL_DEFAULT = 1.0, 8.0, 4        # on-axis: ratio 8 / 4 = 2, log(2) / log(1.2) = 3.80 -> level 4, 0.2 clear of both neighbours


def up(x, n=1):
    x = f32(x)
    for _ in range(n):
        x = np.nextafter(x, f32(np.inf))
    return x


def down(x, n=1):
    x = f32(x)
    for _ in range(n):
        x = np.nextafter(x, f32(-np.inf))
    return x


# ---------------------------------------------------------------------------------------------------------------------------------
# poses
# ---------------------------------------------------------------------------------------------------------------------------------
class Pose:
    """Rcw is diagonal with entries +-1 (the identity, or a half turn about x), so R P + t, P - Ow and Ow = -R^T t are exact for dyadic entries."""

    def __init__(self, name, q, t):
        self.name = name
        self.q, self.t = np.array(q, f32), np.array(t, f32)
        d = {(0, 0, 0, 1): (1, 1, 1), (1, 0, 0, 0): (1, -1, -1)}[tuple(int(v) for v in q)]
        self.R = np.diag(np.array(d, f32))
        self.Ow = (-(self.R.T.astype(np.float64) @ self.t.astype(np.float64))).astype(f32) + f32(0)       # + 0: no negative zero
        self.T7 = np.concatenate([self.q, self.t]).astype(f32)

    def world(self, pc):
        """The world point that this pose takes to the camera-frame point pc."""
        pc64 = np.asarray(pc, np.float64)
        P = self.R.T.astype(np.float64) @ (pc64 - self.t.astype(np.float64))
        Pw = P.astype(f32)
        if self.name == "I":
            Pw = np.asarray(pc, f32).copy()                     # keeps a negative zero as it is
        else:
            assert np.array_equal(Pw.astype(np.float64), P), "world coordinates must be exact in float32"
            back = (self.R.astype(np.float64) @ Pw.astype(np.float64)) + self.t.astype(np.float64)
            assert np.array_equal(back, pc64), "R P + t must give the camera-frame point back exactly"
            assert np.array_equal(self.R.T.astype(np.float64) @ pc64, Pw.astype(np.float64) - self.Ow.astype(np.float64))
        return Pw

    def world_dir(self, n_cam):
        return (self.R.T @ np.asarray(n_cam, f32)).astype(f32) + f32(0)

    def par(self):
        return {} if self.name == "I" else dict(Tcw7=self.T7, Ow=self.Ow, Rcw=self.R, tcw=self.t)


POSE_I = Pose("I", (0, 0, 0, 1), (0, 0, 0))
POSE_X = Pose("X", (1, 0, 0, 0), (0.5, -0.25, 1.0))
assert POSE_X.Ow.tolist() == [-0.5, -0.25, 1.0] and POSE_X.R.tolist() == [[1, 0, 0], [0, -1, 0], [0, 0, -1]]


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 arithmetic of what follows a gate, operation by operation
# ---------------------------------------------------------------------------------------------------------------------------------
def proj_div(x, z, c):
    """fx * x / z + c (Pinhole::project)."""
    with np.errstate(all="ignore"):
        return f32(f32(f32(FX * f32(x)) / f32(z)) + c)


def proj_inv(x, z, c, through_double=False):
    """fx * (x * (1 / z)) + c (ORBmatcher.cc:510-515; :1346-1351 takes the reciprocal in double)."""
    with np.errstate(all="ignore"):
        invz = f32(1.0 / float(z)) if through_double else f32(f32(1) / f32(z))
        return f32(f32(FX * f32(f32(x) * invz)) + c)


def norm3(p):
    p = np.asarray(p, f32)
    return f32(np.sqrt(f32(f32(p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])))


def dot3(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return f32(f32(a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])


def level_of(max_dist, dist, margin=1e-3):
    """MapPoint::PredictScale (MapPoint.cc:538-570) for a ratio that is NOT near a step: asserts the margin."""
    ratio = f32(f32(max_dist) / f32(dist))
    s = math.log(float(ratio)) / LOG_SF
    assert abs(s - round(s)) > margin, ("ratio on a level step", float(ratio), s)
    return min(max(math.ceil(s), 0), 7)


class Spec:
    """One point under one pose, with everything the frustum test would write if every gate let it through."""

    def __init__(self, pc, pose=POSE_I, n_cam=None, min_dist=MIN_DEFAULT, max_dist=MAX_DEFAULT, level=None, u=None, v=None, centre=(CX, CY)):
        self.pose, self.pc = pose, np.asarray(pc, f32)
        self.K = np.array([FX, FX, centre[0], centre[1]], f32)
        self.pos = pose.world(self.pc)
        n_cam = (math.sqrt(1 - float(COS_DEFAULT) ** 2), 0.0, COS_DEFAULT) if n_cam is None else n_cam
        self.n_cam = np.asarray(n_cam, f32)
        self.normal = pose.world_dir(self.n_cam)
        self.min_dist, self.max_dist = float(f32(min_dist)), float(f32(max_dist))
        assert self.min_dist == min_dist and self.max_dist == max_dist
        self.u = proj_div(self.pc[0], self.pc[2], self.K[2]) if u is None else f32(u)
        self.v = proj_div(self.pc[1], self.pc[2], self.K[3]) if v is None else f32(v)
        self.dist = norm3(self.pc)                              # |P - Ow| = |R^T Pc|, the same three squares
        with np.errstate(all="ignore"):
            self.cos = f32(dot3(self.pc, self.n_cam) / self.dist)
        self.depth = self.dist
        self.level = level
        if level is None and self.dist > 0 and np.isfinite(self.dist):
            self.level = level_of(self.max_dist, self.dist)

    def on_axis(self):
        return self.pc[0] == 0 and self.pc[1] == 0


def on_axis(c=COS_DEFAULT, z=4.0, **kw):
    """(0, 0, z) with the normal (sqrt(1 - c^2), 0, c): dot = z c and viewCos = c exactly."""
    c = f32(c)
    s = Spec((0.0, 0.0, z), n_cam=(math.sqrt(max(0.0, 1 - float(c) ** 2)), 0.0, c), **kw)
    assert s.dist == abs(f32(z)) and (z == 0 or s.cos == (c if z > 0 else -c)) and (z == 0 or (s.u == 320 and s.v == 240))
    return s


def x_for_u(target, c=CX, z=4.0, form=proj_div):
    """A float x whose projection at depth z is exactly the float `target` (the final + c rounds, so neighbours of the algebraic solution are tried)."""
    target = f32(target)
    x0 = f32((float(target) - float(c)) * z / float(FX))
    for k in range(0, 64):
        for x in (up(x0, k), down(x0, k)):
            if form(x, z, c) == target:
                return x
    raise AssertionError(f"no float projects to {float(target)!r}")


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
FIELDS = [("track_in_view", np.uint8), ("proj_x", f32), ("proj_y", f32), ("scale_level", np.int32), ("view_cos", f32), ("track_depth", f32)]


def fields_of(spec, stage):
    """The six values Frame::isInFrustum leaves on the point (Frame.cc:560-562 clears the flag and the projection first; :584-585 writes the
    projection once the rectangle is passed; :608-616 the rest on acceptance; the arrays of a batch start from zero)."""
    if stage in ("Z", "I", "skip"):
        return (0, f32(-1), f32(-1), 0, f32(0), f32(0))
    if stage in ("D", "C"):
        return (0, spec.u, spec.v, 0, f32(0), f32(0))
    assert stage is None and spec.level is not None
    return (1, spec.u, spec.v, spec.level, spec.cos, spec.depth)


class FrustumCase:
    member = "FRUSTUM"

    def __init__(self, name, family, cite, specs, stages, bounds=BOUNDS, skip=None, log_sf=None):
        """log_sf: the constant the case's level step was found for (None: the level is clear of every step, any entry may run the case)."""
        self.name, self.family, self.cite, self.specs, self.stages, self.bounds = name, family, cite, list(specs), list(stages), tuple(float(b) for b in bounds)
        self.log_sf = log_sf
        self.pose, self.K = specs[0].pose, specs[0].K
        assert all(s.pose is self.pose and np.array_equal(s.K, self.K) for s in specs) and 1 <= len(specs) <= 8
        n = len(specs)
        self.skip = np.zeros(n, np.uint8) if skip is None else np.asarray(skip, np.uint8)
        self.pts = dict(pos=np.stack([s.pos for s in specs]).astype(f32), normal=np.stack([s.normal for s in specs]).astype(f32),
                        min_dist=np.array([s.min_dist for s in specs], f32), max_dist=np.array([s.max_dist for s in specs], f32))
        rows = [fields_of(s, "skip" if sk else st) for s, st, sk in zip(specs, stages, self.skip)]
        self.exp = {k: np.array([r[j] for r in rows], t) for j, (k, t) in enumerate(FIELDS)}

    @property
    def id(self):
        return f"FRUSTUM-{self.family}-{self.name}"


def same_bytes(got, exp, rows=None):
    """Field by field, bit for bit (NaN equals NaN, -0 differs from 0); returns the names that differ."""
    sel = slice(None) if rows is None else rows

    def raw(a, t):
        a = np.ascontiguousarray(np.asarray(a, t)[sel]).copy()
        if t is f32:                                            # every NaN is the same NaN: the sign and payload of 0 / 0 are the hardware's (x86 returns
            a.view(np.uint32)[np.isnan(a)] = 0x7FC00000         # the negative quiet NaN), not a rule of the reference
        return a.tobytes()
    return [k for k, t in FIELDS if raw(got[k], t) != raw(exp[k], t)]


def _witness_xy(spec):
    """Where a feature can wait for the point: its pixel, moved inside the 64 x 48 grid when the pixel is on or beyond an image edge."""
    if not (np.isfinite(spec.u) and np.isfinite(spec.v)) or abs(float(spec.u)) > 1e4 or abs(float(spec.v)) > 1e4:
        return 320.0, 240.0, False
    wx, wy = min(max(float(spec.u), 0.0), 634.5), min(max(float(spec.v), 0.0), 474.5)
    assert MC.cell_of(wx, wy, W, H) is not None and abs(wx - float(spec.u)) <= 6 and abs(wy - float(spec.v)) <= 6
    return wx, wy, (wx, wy) == (float(spec.u), float(spec.v))


def search_cases(member, name, family, cite, spec, stage, octaves=None, win=None, R=8, offset=(0.0, 0.0), level=None, bits=None, **par):
    """The point as the only query of a member's search, with a perfect-descriptor feature waiting where it lands (``octaves``: one feature per
    entry, all at that pixel + offset; default: one at the point's level).  win: index of the feature the reference picks; default: feature 0
    when no gate drops the point.  Returns one case per variant of the member (both overloads of SIM3P, both reproj values of FUSE)."""
    if member == "SIM3" and spec.pose is not POSE_I:
        return []                                               # SearchBySim3 takes the points in camera coordinates already
    L = LEVEL_DEFAULT if spec.level is None else spec.level
    L = L if level is None else level
    octaves = [L] if octaves is None else octaves
    wx, wy, exact = _witness_xy(spec)
    out = []
    variants = {"SIM3P": [dict(variant=0), dict(variant=1)], "FUSE": [dict(reproj=0), dict(reproj=1)] if exact and offset == (0.0, 0.0) else [dict(reproj=0)]}.get(member, [{}])
    for var in variants:
        if "variant" in par and "variant" in var and par["variant"] != var["variant"]:
            continue
        s = Proj(900, R=R)
        b = s.base()
        for k, o in enumerate(octaves):
            s.feat(wx + offset[0], wy + offset[1], b if bits is None else MC.desc_at(b, bits[k], s.rng), octave=o)
        s.query(wx, wy, b, level=L, pos=spec.pos, normal=spec.normal, min_dist=spec.min_dist, max_dist=spec.max_dist)
        w = (0 if stage is None else -1) if win is None else win
        tag = "".join(f"_{k[0]}{v}" for k, v in var.items())
        c = s.case(name + tag, member, family, cite, [w], **{**spec.pose.par(), **var, **par})
        c.spec, c.stage = spec, stage
        if member == "MP":
            c.fields = {k: np.array([r], t) for (k, t), r in zip(FIELDS, fields_of(spec, stage))}
        out.append(c)
    return out


def row(name, family, cite, spec, F, LAST, RELOC, KF, SIM3, members=None, bounds=BOUNDS, **kw):
    """One point through every member that has the gate: F / LAST / RELOC / KF / SIM3 = where that class drops it (None: it is searched)."""
    verdict = dict(F=F, LAST=LAST, RELOC=RELOC, KF=KF, SIM3=SIM3)
    if None in (F, RELOC, KF, SIM3):                            # a point said to be searched must not sit beyond a later gate by accident
        assert not (spec.dist < POINT_EIGHT * f32(spec.min_dist) or spec.dist > ONE_TWO * f32(spec.max_dist)), (name, "distance range")
    if None in (F, KF) and family != "C":
        assert spec.cos > 0.55, (name, "viewing cosine", float(spec.cos))
    out = []
    for m in (["FRUSTUM"] + SEARCH_MEMBERS if members is None else members):
        st = verdict[CLASS_OF[m]]
        if st == "n/a":
            continue
        if m == "FRUSTUM":
            out.append(FrustumCase(name, family, cite, [spec], [st], bounds))
        elif bounds == BOUNDS:
            out += search_cases(m, name, family, cite, spec, st, **kw)
    return out


TINY = 2.0 ** -10


def family_Z():
    out = []
    near = dict(min_dist=2.0 ** -12, max_dist=2.0 ** -9)      # dist = 2^-10: inside [0.8 min, 1.2 max], ratio 2 -> level 4
    # z = +2^-10 on the axis: every member searches it at the principal point
    out += row("plus_tiny", "Z", "Frame.cc:574", on_axis(z=TINY, **near), None, None, None, None, None)
    # z = -2^-10: dropped by the sign test everywhere (Frame.cc:574, ORBmatcher.cc:404, :506, :1062, :1343; :1528 through 1/z) -- except that
    # :1706-1713 has no depth test, so the relocalisation search takes it at the principal point (x = y = 0)
    out += row("minus_tiny", "Z", "ORBmatcher.cc:1708", on_axis(z=-TINY, **near), "Z", "Z", None, "Z", "Z")
    # z = -0.0 with x = 1: -0.0 < 0 is false, so the sign tests of Frame.cc:574, ORBmatcher.cc:404 / :506 / :1062 / :1343 let it through and the
    # rectangle drops the infinite u; :1526-1528 computes 1 / -0.0 = -inf < 0 and drops it at the depth test.  Either way nothing is searched,
    # and the frustum test leaves (-1, -1).
    z0 = Spec((1.0, 0.0, -0.0), n_cam=(0, 0, 1), level=0)
    assert np.signbit(z0.pos[2]) and np.isinf(z0.u)
    out += row("minus_zero", "Z", "ORBmatcher.cc:1528", z0, "I", "Z", "I", "I", "I")
    # P = Ow: 0 / 0 = NaN passes the NaN-tolerant rectangle test of Frame.cc:579-582 and ORBmatcher.cc:1710-1713, the point dies at the distance
    # gate (dist = 0 < 0.8 min) with NaN left in the projection; KeyFrame::IsInImage (KeyFrame.cc:928) is false for NaN.  Not a case for
    # SearchByProjection(Cur, Last): without a distance gate it goes on to GetFeaturesInArea with NaN, which converts NaN to int.
    for pose in (POSE_I, POSE_X):
        o = Spec((0.0, 0.0, 0.0), pose=pose, n_cam=(0, 0, 1), level=0)
        assert np.array_equal(o.pos, pose.Ow) and np.isnan(o.u) and np.isnan(o.v) and o.dist == 0
        out += row(f"at_Ow_pose{pose.name}", "Z", "Frame.cc:593", o, "D", "n/a", "D", "I", "I")
    return out


def _edge_points(bounds, centre, form=proj_div):
    """(name, pc, axis, position): u or v exactly on each of the four bounds, one float outside and one inside each; the other coordinate in
    the middle of the image."""
    mnx, mny, mxx, mxy = (f32(b) for b in bounds)
    xm, ym = f32(0.25), f32(0.125)                              # 32 and 16 pixels from the principal point
    out = []
    for nm, b, axis, outward in (("min_x", mnx, 0, down), ("max_x", mxx, 0, up), ("min_y", mny, 1, down), ("max_y", mxy, 1, up)):
        inward = up if outward is down else down
        c = f32(centre[axis])
        a_on = x_for_u(b, c, 4.0, form)
        for pos, step in (("on", None), ("out", outward), ("in", inward)):
            a = a_on
            while step is not None and form(a, 4.0, c) == b:    # the nearest coordinate whose projection leaves the bound (the + c rounds)
                a = step(a)
            pc = (a, ym, 4.0) if axis == 0 else (xm, a, 4.0)
            out.append((f"{nm}_{pos}", pc, nm, pos))
    return out


def family_I():
    out = []
    # The undistorted bounds of the EuRoC camera are odd multiples of 2^-16 (min x) and 2^-17 (min y); with the principal point at (320, 240)
    # every projection that far from it is a multiple of 2^-15, so no point lands ON them.  Those cases put the principal point at (0, 0): then
    # u = 128 x, every float bound is reached exactly and its float neighbours too.
    for bname, bounds, centre in (("img", BOUNDS, (CX, CY)), ("euroc", EUROC_BOUNDS, (f32(0), f32(0)))):
        for nm, pc, edge, pos in _edge_points(bounds, centre):
            towards = np.asarray(pc, np.float64) / np.linalg.norm(np.asarray(pc, np.float64))       # the EuRoC corners are 60 degrees off the axis
            sp = Spec(pc, n_cam=towards.astype(f32), centre=centre)
            got = sp.u if edge.endswith("x") else sp.v
            b = f32(bounds[["min_x", "min_y", "max_x", "max_y"].index(edge)])
            beyond = (got < b) if edge.startswith("min") else (got > b)
            assert (got == b) if pos == "on" else (got != b and beyond == (pos == "out") and abs(float(got) - float(b)) < 1e-3), (nm, got, b)
            # Frame members: closed on all four edges (Frame.cc:579-582, ORBmatcher.cc:1533-1536, :1710-1713); key-frame members: KeyFrame::IsInImage
            # is [min, max) (KeyFrame.cc:928)
            closed = None if pos in ("on", "in") else "I"
            half = None if pos == "in" or (pos == "on" and edge.startswith("min")) else "I"
            out += row(f"{bname}_{nm}", "I", "KeyFrame.cc:928" if half != closed else "Frame.cc:579", sp, closed, closed, closed, half, half, bounds=bounds)
    # the same edge under the turned and translated pose: u = 640 exactly, and one float beyond
    for pos, tgt in (("on", f32(640)), ("out", up(640))):
        sp = Spec((x_for_u(tgt), 0.125, 4.0), pose=POSE_X, n_cam=(0, 0, 1))
        assert sp.u == tgt and not np.array_equal(sp.pos, sp.pc)
        out += row(f"poseX_max_x_{pos}", "I", "KeyFrame.cc:928", sp, None if pos == "on" else "I", None if pos == "on" else "I", None if pos == "on" else "I", "I", "n/a")
    return out


# D: the float products 1.2f * max and 0.8f * min (MapPoint.cc:527-536) at dist = 4
MAX_IN = next(m for m in (down(f32(4.0 / 1.2), 4 - k) for k in range(9)) if f32(ONE_TWO * up(m)) > 4 >= f32(ONE_TWO * m))      # the largest float with fl(1.2f m) <= 4
assert f32(ONE_TWO * MAX_IN) == 4 and f32(ONE_TWO * down(MAX_IN)) < 4 and float(MAX_IN) == 3.3333332538604736
assert f32(POINT_EIGHT * f32(5)) == 4 and float(POINT_EIGHT) * 5.0 > 4 and f32(POINT_EIGHT * up(5)) > 4


def max_rounds_up():
    """(z, max): a depth just above 4 and a range for which the exact product 1.2f * max lies below z and rounds UP onto it.  The float product
    of MapPoint.cc:535 keeps the point (dist == 1.2f max); the product taken in double, or fused into the comparison, would drop it.  (At
    dist = 4 itself no float max does this: the products step by 1.2 ulps.)"""
    for k in range(1, 400):
        z = up(4, k)
        m0 = f32(float(z) / 1.2)
        for m in (down(m0, 2), down(m0), m0, up(m0), up(m0, 2)):
            if f32(ONE_TWO * m) == z and float(ONE_TWO) * float(m) < float(z):
                return z, m
    raise AssertionError("no range whose product rounds up onto the distance")


def family_D():
    out = []
    z, m = max_rounds_up()
    sp = Spec((0.0, 0.0, float(z)), n_cam=(0, 0, 1), max_dist=float(m), level=0)
    assert sp.dist == z and sp.cos == 1 and (sp.u, sp.v) == (320, 240)
    out += row("max_rounds_up", "D", "MapPoint.cc:535", sp, None, None, None, None, None)
    # LAST has no distance gate (:1516-1553): the class's verdict is None throughout
    # dist == fl(1.2f max): not beyond it, searched; ratio = 0.83 -> nScale clamps to level 0.  One float less: dist > 1.2f max.
    out += row("max_on", "D", "MapPoint.cc:535", on_axis(max_dist=float(MAX_IN), level=0), None, None, None, None, None)
    out += row("max_below", "D", "MapPoint.cc:535", on_axis(max_dist=float(down(MAX_IN)), level=0), "D", None, "D", "D", "D")
    # min = 5: fl(0.8f * 5) == 4 == dist, inside; the product taken in double is 4.00000006 > dist, which would drop it.  One float more: outside.
    out += row("min_on", "D", "MapPoint.cc:529", on_axis(min_dist=5.0), None, None, None, None, None)
    out += row("min_above", "D", "MapPoint.cc:529", on_axis(min_dist=float(up(5))), "D", None, "D", "D", "D")
    return out


def cos_disagreement_search():
    """The issue that asked for these cases expected a point for which fl(dot / dist) < 0.5f (Frame.cc:599-601) and (double)dot < 0.5 * (double)dist
    (ORBmatcher.cc:426) disagree.  There is none: dist / 2 is a float, so dot < dist / 2 means dot <= pred(dist / 2) and
    dot / dist <= 0.5 (1 - 2^-24) = pred(0.5f), which rounds to at most pred(0.5f) < 0.5f; and dot >= dist / 2 gives a quotient >= 0.5 exactly.
    This walks the float neighbours of dist / 2 for many dist (normal and power-of-two) and returns every disagreement it finds: none."""
    found = []
    rng = np.random.default_rng(5)
    dists = [f32(4), up(4), down(4), f32(2 ** -100), f32(3e38)] + [f32(v) for v in rng.uniform(0.5, 64.0, 4000)]
    for d in dists:
        h = f32(d / f32(2))
        for dot in (down(h, 3), down(h, 2), down(h), h, up(h), up(h, 2)):
            if bool(f32(dot / d) < f32(0.5)) != bool(float(dot) < 0.5 * float(d)):
                found.append((float(dot), float(d)))
    return found


def off_axis_rounding():
    """An off-axis point and a unit-ish normal for which the float dot product (two products, two rounded sums) is >= dist / 2 while the exact sum
    of the same float products is below it: a body that accumulated the dot product in double, or fused a multiply into an add, would drop the
    point that ORBmatcher.cc:426 and Frame.cc:599 keep."""
    pc = np.array([1.0, 0.0, 4.0], f32)
    d = norm3(pc)
    h = f32(d / f32(2))
    c0 = f32(0.45)
    for k in range(-2000, 2000):
        nz = up(c0, k) if k >= 0 else down(c0, -k)
        nx = f32(float(h) - 4.0 * float(nz))                   # so that nx + 4 nz is within a rounding of dist / 2
        for nxx in (down(nx), nx, up(nx)):
            fl = dot3(pc, (nxx, 0.0, nz))
            exact = float(nxx) + 4.0 * float(nz)              # 4 nz is exact in float, 1 * nx too: the only rounding is the last sum
            if fl >= h and exact < float(h) and 0 < float(nxx) < 1:
                return pc, np.array([nxx, 0.0, nz], f32), d, fl
    raise AssertionError("no rounding-up dot product found")


def family_C():
    out = []
    half, below = f32(0.5), down(0.5)
    # viewCos == 0.5 is not below the limit (Frame.cc:601; dot == 0.5 dist at ORBmatcher.cc:426 / :533 / :1093); one float less is.  No cosine gate in
    # :1516-1553, :1700-1733, :1329-1371: those members are listed in NOT_APPLICABLE.
    out += row("at_half", "C", "Frame.cc:601", on_axis(c=half), None, "n/a", "n/a", None, "n/a")
    out += row("below_half", "C", "Frame.cc:601", on_axis(c=below), "C", "n/a", "n/a", "C", "n/a")
    out += row("poseX_at_half", "C", "ORBmatcher.cc:426", Spec((0, 0, 4.0), pose=POSE_X, n_cam=(math.sqrt(0.75), 0.0, half)), None, "n/a", "n/a", None, "n/a")
    out += row("poseX_below_half", "C", "ORBmatcher.cc:426", Spec((0, 0, 4.0), pose=POSE_X, n_cam=(math.sqrt(0.75), 0.0, below)), "C", "n/a", "n/a", "C", "n/a")
    # float versus double: no input separates fl(dot / dist) < 0.5f from dot < 0.5 dist (cos_disagreement_search); what can be separated is the dot
    # product itself: its last float sum rounds UP onto dist / 2 here, so both forms keep the point and a wider accumulation would not
    pc, n, d, fl = off_axis_rounding()
    sp = Spec(pc, n_cam=n, max_dist=MAX_DEFAULT)
    assert sp.cos >= half and fl == f32(d / f32(2))
    out += row("dot_rounds_up", "C", "ORBmatcher.cc:426", sp, None, "n/a", "n/a", None, "n/a")
    return out


# mfLogScaleFactor as rumi_track_* derives it from the scale factor itself: log(1.2f) correctly rounded to float (Frame.cc:106 takes the float log
# of the float factor).  The tests' LOG_SF is numpy's float32 log, one float above it, so the two constants put some level steps between
# different pairs of ratios (1.2f itself predicts level 1 with LOG_SF and level 2 with this one); entries that take the constant get LOG_SF.
LOG_SF_TRACK = float(f32(math.log(float(f32(1.2)))))
assert LOG_SF_TRACK == 0.18232159316539764 and f32(LOG_SF) == up(LOG_SF_TRACK)


def level_steps(log_sf):
    """For k = 0..7 the float ratios (r, nextafter(r)) between which ceil(log(r) / logSF) steps from k to k + 1, with their distances from k."""
    try:
        import mpmath
        mpmath.mp.prec = 200
        lg = lambda r: float(mpmath.log(mpmath.mpf(float(r))) / mpmath.mpf(log_sf) - k)
    except ImportError:                                          # pragma: no cover
        lg = lambda r: math.log(float(r)) / log_sf - k
    out = []
    for k in range(8):
        r = f32(math.exp(k * log_sf))
        while lg(r) > 0:
            r = down(r)
        while lg(up(r)) <= 0:
            r = up(r)
        lo, hi = lg(r), lg(up(r))
        assert lo <= 0 < hi
        out.append((k, r, up(r), lo, hi))
    return out


LEVEL_STEPS, LEVEL_STEPS_TRACK = level_steps(LOG_SF), level_steps(LOG_SF_TRACK)
for _steps in (LEVEL_STEPS, LEVEL_STEPS_TRACK):
    assert _steps[0][1] == 1 and _steps[0][3] == 0                 # log(1) is 0 in every library
    assert all(hi >= 1e-9 and (k == 0 or -lo >= 1e-9) for k, _, _, lo, hi in _steps), "a step closer than 1e-9 to an integer depends on the last bit of log"
assert LEVEL_STEPS[1][1] == f32(1.2) and LEVEL_STEPS_TRACK[1][2] == f32(1.2)


def _level_row(name, cite, ratio, level, rising=True, members=None, log_sf=LOG_SF):
    """dist = 4, max = 4 ratio (exact): the frustum test reports `level`; a searching member shows it through its octave window: a perfect feature
    one octave below the lower level of the pair and one above the upper (two above for the relocalisation search, whose window reaches L + 1)."""
    mx = f32(f32(4) * f32(ratio))
    assert f32(mx / f32(4)) == f32(ratio) and float(mx) == 4.0 * float(ratio)
    sp = on_axis(max_dist=float(mx), min_dist=0.5, level=level)
    out = [FrustumCase(name, "L", cite, [sp], [None], log_sf=log_sf)]
    for m in SEARCH_MEMBERS if members is None else members:
        if m == "LAST":
            continue                                            # the level is the last frame's key-point octave (:1538), not PredictScale
        lo, hi = MC.LEVELS[m]
        window = [o for o in range(8) if level + lo <= o <= level + hi]
        # one feature per octave at the point's pixel; the descriptor distance grows with the octave (falls, for the pair at level 0 / 1, whose
        # windows both start at octave 0), so the winner is the lowest (highest) octave of the member's window around the level
        win = window[0] if rising else window[-1]
        out += search_cases(m, name, "L", cite, sp, None, octaves=list(range(8)), win=win, level=4, bits=[2 * o if rising else 2 * (7 - o) for o in range(8)])
    return out


def family_L():
    out = []
    for k, r, r_up, _, _ in LEVEL_STEPS:
        out += _level_row(f"step{k}_lo", "MapPoint.cc:546", r, k, rising=k > 0)
        out += _level_row(f"step{k}_hi", "MapPoint.cc:546", r_up, min(k + 1, 7), rising=k > 0)
    # the same steps for the constant the tracker derives itself: through the frustum entries only
    for k, r, r_up, _, _ in LEVEL_STEPS_TRACK:
        out += _level_row(f"track_step{k}_lo", "MapPoint.cc:563", r, k, members=[], log_sf=LOG_SF_TRACK)
        out += _level_row(f"track_step{k}_hi", "MapPoint.cc:563", r_up, min(k + 1, 7), members=[], log_sf=LOG_SF_TRACK)
    # ratio in [1 / 1.2, 1): inside the distance gate, nScale <= 0 -> level 0 (:547); ratio above 1.2^8: clamped to nLevels - 1 (:549)
    out += _level_row("ratio_0.875", "MapPoint.cc:547", 0.875, 0, rising=False)
    out += _level_row("ratio_5", "MapPoint.cc:549", 5.0, 7)
    return out


COS_998 = f32(0.998)
assert float(COS_998) > 0.998 > float(down(COS_998))


def family_R():
    """RadiusByViewingCos (ORBmatcher.cc:1776-1781, used at :59): the float view cosine against the double literal 0.998; r *= th only when
    th != 1.0 (:42, :61).  The feature sits between the two radii: at 2.5 th sf it is out of the window, at 4 th sf inside."""
    out = []
    s4 = float(SF[LEVEL_DEFAULT])
    for th, dx in ((1.0, 6.5), (3.0, 20.0)):
        assert 2.5 * th * s4 < dx < 4.0 * th * s4
        for nm, c, win in (("at_998", COS_998, -1), ("below_998", down(COS_998), 0)):
            out += search_cases("MP", f"th{th:g}_{nm}", "R", "ORBmatcher.cc:1777", on_axis(c=c), None, win=win, R=int(4 * th), offset=(dx, 0.0))
    # bFarPoints (:49): mTrackDepth > thFarPoints drops the point; equal keeps it
    out += search_cases("MP", "far_equal", "R", "ORBmatcher.cc:49", on_axis(), None, win=0, far=True, th_far=4.0)
    out += search_cases("MP", "far_above", "R", "ORBmatcher.cc:49", on_axis(z=float(up(4))), None, win=-1, far=True, th_far=4.0)
    return out


def division_pairs():
    """Points whose fx * x / z + cx and fx * (x * (1 / z)) + cx fall on different sides of an image bound: (x, z, u by division, u by
    reciprocal, bound).  z = 3 near x = -+1.875 (u = 0, u = 640) is tried first and has none with this camera: within 40 floats of either
    coordinate the two forms round to the same side.  z = 5 near x = 3.125 has one: the quotient stays one float below 640, the product with
    fl(1 / 5) reaches 640."""
    out = []
    for z in (3.0, 5.0):
        assert f32(1.0 / z) == f32(1) / f32(z)                  # :1346's reciprocal through double is :510's float reciprocal here
        for x0, bound in ((-320.0 * z / 512.0, 0.0), (320.0 * z / 512.0, 640.0)):
            for k in range(-40, 41):
                x = up(x0, k) if k >= 0 else down(x0, -k)
                ud, ui = proj_div(x, z, CX), proj_inv(x, z, CX)
                if (0 <= float(ud) < 640) != (0 <= float(ui) < 640):
                    out.append((x, z, ud, ui, bound))
                    break
    return out


DIVISION_PAIRS = division_pairs()
assert DIVISION_PAIRS, "no float near an image bound separates the two projection forms"


def family_V():
    out = []
    for x, z, ud, ui, bound in DIVISION_PAIRS:
        tag = ("min_x" if bound == 0 else "max_x") + f"_z{z:g}"
        in_d, in_i = 0 <= float(ud) < 640, 0 <= float(ui) < 640
        assert in_d != in_i and proj_inv(x, z, CX, through_double=True) == ui
        # :408 (first overload) and :1069 (Fuse) project through the camera model, fx * x / z + cx; :510-515 and :1346-1351 multiply by 1 / z
        sp_d = Spec((x, 0.0, z), n_cam=(0, 0, 1))
        sp_i = Spec((x, 0.0, z), n_cam=(0, 0, 1), u=ui)
        out += search_cases("SIM3P", f"{tag}_division", "V", "ORBmatcher.cc:408", sp_d, None if in_d else "I", variant=0)
        out += search_cases("SIM3P", f"{tag}_reciprocal", "V", "ORBmatcher.cc:510", sp_i, None if in_i else "I", variant=1)
        out += search_cases("FUSE", f"{tag}_division", "V", "ORBmatcher.cc:1069", sp_d, None if in_d else "I")
        out += search_cases("SIM3", f"{tag}_reciprocal", "V", "ORBmatcher.cc:1346", sp_i, None if in_i else "I")
    return out


def family_S():
    """What Frame::isInFrustum leaves on a point it rejects, per stage; off-axis, so that no field equals a cleared value by accident."""
    out = []
    pc = (1.0, 0.5, 4.0)                                        # u = 448, v = 304
    ok = Spec(pc, n_cam=(0, 0, 1))
    assert (ok.u, ok.v) == (448, 304)
    behind = Spec((1.0, 0.5, -4.0), n_cam=(0, 0, -1))
    outside = Spec((4.0, 0.5, 4.0), n_cam=(0, 0, 1))            # u = 832
    too_far = Spec(pc, n_cam=(0, 0, 1), max_dist=2.0, level=0)
    too_near = Spec(pc, n_cam=(0, 0, 1), min_dist=16.0)
    oblique = Spec(pc, n_cam=(1, 0, 0))                         # viewCos = 1 / dist < 0.5
    assert 0 < oblique.cos < 0.5
    out.append(FrustumCase("rejected_at_Z", "S", "Frame.cc:561", [behind], ["Z"]))
    out.append(FrustumCase("rejected_at_I", "S", "Frame.cc:561", [outside], ["I"]))
    out.append(FrustumCase("rejected_at_D_far", "S", "Frame.cc:585", [too_far], ["D"]))
    out.append(FrustumCase("rejected_at_D_near", "S", "Frame.cc:585", [too_near], ["D"]))
    out.append(FrustumCase("rejected_at_C", "S", "Frame.cc:585", [oblique], ["C"]))
    # a point SearchLocalPoints does not evaluate (Tracking.cc:3015-3022) keeps cleared fields, between two that are accepted
    out.append(FrustumCase("skipped", "S", "Frame.cc:560", [ok, Spec(pc, n_cam=(0, 0, 1)), ok], [None, None, None], skip=[0, 1, 0]))
    out.append(FrustumCase("all_stages", "S", "Frame.cc:560", [ok, behind, outside, too_far, too_near, oblique, ok], [None, "Z", "I", "D", "D", "C", None]))
    # mTrackDepth is |Pc| (Frame.cc:569, :612): (2, 0.5, 4) has norm 4.5 under the turned, translated pose; its distance along z is 4
    deep = Spec((2.0, 0.5, 4.0), pose=POSE_X, n_cam=(0, 0, 1), max_dist=9.0)
    assert deep.depth == 4.5 and deep.dist == 4.5 and (deep.u, deep.v) == (576, 304) and deep.level == 4 and deep.cos == f32(4) / f32(4.5)
    out.append(FrustumCase("depth_is_norm_poseX", "S", "Frame.cc:612", [deep], [None]))
    return out


_SAME = "runs sim3_query, the one body FuseCandidates stands on here: its arithmetic is that of ORBmatcher.cc:1058-1112 and the FUSE cases hold it"
NOT_APPLICABLE = {
    ("LAST", "C"): "no viewing-cosine gate (ORBmatcher.cc:1516-1553)", ("RELOC", "C"): "no viewing-cosine gate (ORBmatcher.cc:1706-1733)",
    ("SIM3", "C"): "no viewing-cosine gate (ORBmatcher.cc:1329-1371)",
    ("LAST", "L"): "the level is the last frame's key-point octave, not PredictScale (ORBmatcher.cc:1538)",
    ("FRUSTUM", "R"): "the window belongs to the search, not to the frustum test (ORBmatcher.cc:59-65)",
    ("LAST", "R"): "radius = th * scale factor, no cosine factor (ORBmatcher.cc:1541)", ("RELOC", "R"): "radius = th * scale factor, no cosine factor (ORBmatcher.cc:1729)",
    ("SIM3P", "R"): "radius = th * scale factor, no cosine factor (ORBmatcher.cc:432, :539)", ("FUSE", "R"): "radius = th * scale factor, no cosine factor (ORBmatcher.cc:1101)",
    ("SIM3", "R"): "radius = th * scale factor, no cosine factor (ORBmatcher.cc:1369)",
    ("FRUSTUM", "V"): "one projection form only, the camera model's fx * x / z + cx (Frame.cc:577)", ("MP", "V"): "projected by Frame::isInFrustum (Frame.cc:577)",
    ("LAST", "V"): "one projection form only, the camera model's (ORBmatcher.cc:1531)", ("RELOC", "V"): "one projection form only, the camera model's (ORBmatcher.cc:1708)",
    ("MP", "S"): "the search reads the fields, it writes none (ORBmatcher.cc:44-71)", ("LAST", "S"): "no per-point fields are written (ORBmatcher.cc:1516-1553)",
    ("RELOC", "S"): "no per-point fields are written (ORBmatcher.cc:1700-1733)", ("SIM3P", "S"): "no per-point fields are written (ORBmatcher.cc:389-436)",
    ("FUSE", "S"): "no per-point fields are written (ORBmatcher.cc:1058-1112)", ("SIM3", "S"): "no per-point fields are written (ORBmatcher.cc:1329-1371)",
    **{(m, f): _SAME for m in ("SIN", "SAF") for f in FAMILIES},
}

_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = family_Z() + family_I() + family_D() + family_C() + family_L() + family_R() + family_V() + family_S()
        ids = [c.id for c in _ALL]
        assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
    return _ALL


def frustum_cases():
    return [c for c in all_cases() if c.member == "FRUSTUM"]


def member_cases(m):
    return [c for c in all_cases() if c.member == m]


def sim3_query_cases():
    """The cases that run sim3_query: both overloads of SearchByProjection(KF, Scw, points) under the identity pose."""
    return [c for c in member_cases("SIM3P")]


def coverage():
    cov = {}
    for c in all_cases():
        cov.setdefault((c.member, c.family), []).append(c.name)
    return cov


# ---------------------------------------------------------------------------------------------------------------------------------
# entries that match_cases.py does not have
# ---------------------------------------------------------------------------------------------------------------------------------
def pts_of(c):
    """A frustum case's points in the form the fused and the tracker entries take."""
    n = len(c.specs)
    return dict(c.pts, desc=np.full((n, 32), 0x5A, np.uint8), obs=np.ones(n, np.int32), skip=c.skip.copy(), bad=np.zeros(n, np.uint8),
                local=(1 - c.skip).astype(np.uint8))


def oracle_frustum(O, c):
    return O.is_in_frustum(c.pose.R.ravel(), c.pose.t, c.pose.Ow, c.K, c.bounds, None, c.log_sf or LOG_SF, 8, 0.5, c.pts)


def tracker_cases():
    """The frustum cases the tracker can run: it derives mfLogScaleFactor itself, so a case found for the tests' constant is not its case."""
    return [c for c in frustum_cases() if c.log_sf in (None, LOG_SF_TRACK)]


def oracle_mp(O, c):
    """SearchLocalPoints on the CPU: the oracle's frustum test, then its SearchByProjection(F, points) on the fields it wrote."""
    i, sp = c.inp, c.spec
    pts = MC._pts(i, i["nq"])
    fr = O.is_in_frustum(sp.pose.R.ravel(), sp.pose.t, sp.pose.Ow, K4, W, H, LOG_SF, 8, 0.5, pts)
    mp = dict(fr, is_bad=np.zeros(i["nq"], np.uint8), desc=i["qdesc"], obs=np.ones(i["nq"], np.int32))
    n, fm = O.search_by_projection_mappoints(i["keys"], i["desc"], W, H, SF, mp, np.full(len(i["keys"]), -1, np.int32), i["R"] / 4.0, bool(i.get("far", False)),
                                             float(i.get("th_far", 50.0)), c.nnratio)
    return n, fm, fr


def call_oracle(O, c):
    return oracle_mp(O, c)[:2] if c.member == "MP" else MC.call_oracle(O, c)


def mp_from_fields(c):
    """The expected frustum fields of an MP case as the input of SearchByProjection(F, points) itself (k_queries_mappoints)."""
    i = c.inp
    return dict(c.fields, is_bad=np.zeros(i["nq"], np.uint8), desc=i["qdesc"], obs=np.ones(i["nq"], np.int32))
