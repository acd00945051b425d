"""Constructed cases for the pose optimiser and the bundle adjustments: the random scenes of ba_scene.py bent until they sit on one
property each -- a size on a kernel's boundary, a graph in an unusual order, a landmark of a chosen degree, a start far enough away
that Levenberg-Marquardt rejects trials.  TEST INFRASTRUCTURE (numpy only): nothing here needs a GPU or the oracle to BUILD a case.

Three conditions make a case fit for a parity test; ``check_margin``, ``check_decisive`` and ``check_stable`` state them on the oracle alone (the tests
assert them, so a bad seed fails loudly instead of making a flaky comparison):
  margin     no chi2 the call compares with a threshold lies within MARGIN (1e-3, ten times the 1e-4 parity bound of rumi_opt.h) of it;
  decisive   (bundle adjustments, whose iteration and trial counts are compared) every LM trial changes chi2 by at least GAIN (1e-10) of it and
             no iteration ends on rho == 0: an accept / reject decision closer to a tie than that is taken by the rounding of a sum, and two
             correct implementations that add in different orders may take it differently;
  stability  (rough starts, hopeless frames) one float ulp on every observation changes no flag, no iteration / trial / rejection count,
             and the pose by at most 1e-5.
The seeds below were chosen on the CPU oracle so that both hold."""
import numpy as np

from ba_scene import _project, ba_problem, pose_problem
from scene import K_TUM3, quat_rotate

MARGIN = 1e-3
# a chi2 summed over a thousand edges in another order moves by about 1e3 * 2^-53 = 1e-13 of itself: a thousand times that
GAIN = 1e-10
POSE_SIZES = [3, 4, 9, 10, 11, 255, 256, 257, 511, 512, 513, 1151, 1152, 1153, 2305]
# seed of pose_problem(seed, n, 0.1) per size (margin >= MARGIN; n >= 10: no LM iteration of the oracle ends on the exact ties qmax == 10 / rho == 0)
POSE_SEEDS = {3: 100, 4: 100, 9: 102, 10: 105, 11: 104, 255: 101, 256: 102, 257: 101, 511: 100, 512: 100, 513: 101, 600: 100, 1151: 101, 1152: 100,
              1153: 100, 1500: 103, 2305: 108}
BATCH_SIZES = [1153, 0, 2, 3, 1152, 9, 10, 600, 1500]
DEGREES = (0, 1, 2, 15, 16, 17, 32, 33)
COUNTS = (1, 15, 16, 17, 31, 33)
COUNT_SEEDS = {1: 10, 15: 0, 16: 1, 17: 1, 31: 2, 33: 1}          # window(seed, nMP); 16 and 17: with rejected trials
# rough_start_pose(n, seed, offset).  0.4 m: below 512 correspondences, register + LDS edges, global-memory edges.  3 m and 5 m: the third round
# (the last with the robust kernel) ends elsewhere than it would without the kernel, so the round that switches it off shows in the flags.
ROUGH_POSE = [(300, 226, 0.4), (700, 25, 0.4), (1300, 259, 0.4), (12, 1, 3.0), (100, 50, 5.0)]
HOPELESS = [(12, 9), (40, 1), (200, 8)]                            # hopeless_frame(n, seed)
EXACT = [(300, 1), (1300, 2)]                                      # exact_frame(n, seed)


def ba_args(b):
    return (b["kf_pose"], b["kf_fixed"], b["mp_pos"], b["e_mp"], b["e_kf"], b["e_obs"], b["e_w"], b["K"])


def pose_args(p):
    return (p["Xw"], p["obs"], p["inv_sigma2"], p["K"], p["T0"])


def ulp_up(a):
    """Every float one ulp upward."""
    a = np.asarray(a, np.float32)
    return np.nextafter(a, np.float32(np.inf))


# ---------------------------------------------------------------------------------------------------------------------------------
# pose problems
# ---------------------------------------------------------------------------------------------------------------------------------
def pose_case(n):
    """The frame of a boundary size: pose_problem with 10 % outliers and the seed chosen for that size."""
    return pose_problem(POSE_SEEDS[n], n, 0.1)


def exact_frame(n, seed):
    """Noise-free observations and the start at the truth: every correspondence an inlier, nothing to optimise."""
    p = pose_problem(seed, n, 0.0)
    T0 = p["truth"].astype(np.float32)
    T0[:4] /= np.linalg.norm(T0[:4])
    u, v, z = _project(T0[:4].astype(np.float64), T0[4:].astype(np.float64), p["Xw"].astype(np.float64), K_TUM3.astype(np.float64))
    assert (z > 0.5).all()
    p["obs"] = np.stack([u, v], 1).astype(np.float32)
    p["T0"] = T0
    return p


def rough_start_pose(n, seed, offset=0.4, outlier_frac=0.3):
    """The start translation `offset` metres from the truth, 30 % outliers: the first steps overshoot and LM rejects trials."""
    p = pose_problem(seed, n, outlier_frac)
    d = np.random.default_rng(1000 + seed).normal(size=3)
    p["T0"] = p["T0"].copy()
    p["T0"][4:] = (p["truth"][4:] + offset * d / np.linalg.norm(d)).astype(np.float32)
    return p


def hopeless_frame(n, seed):
    """Observations uniform over the image, unit weights: nothing fits, every correspondence ends as an outlier after the first round
    and the three later rounds have no active edge."""
    p = pose_problem(seed, n, 0.0)
    rng = np.random.default_rng(2000 + seed)
    m = len(p["inv_sigma2"])
    p["obs"] = np.stack([rng.uniform(0, 640, m), rng.uniform(0, 480, m)], 1).astype(np.float32)
    p["inv_sigma2"] = np.ones(m, np.float32)
    return p


def pose_batch(probs):
    """Concatenated arguments of PoseOptimizationBatch for a list of problems (None or 0 correspondences allowed)."""
    start = np.cumsum([0] + [len(p["inv_sigma2"]) for p in probs]).astype(np.int32)
    cat = lambda k, w: np.concatenate([np.asarray(p[k], np.float32).reshape(-1, w) for p in probs]).reshape((-1, w) if w > 1 else (-1,))
    return start, cat("Xw", 3), cat("obs", 2), cat("inv_sigma2", 1), probs[0]["K"], np.stack([p["T0"] for p in probs])


def truncated(p, n):
    """The first n correspondences of a frame."""
    q = dict(p)
    for k in ("Xw", "obs", "inv_sigma2"):
        q[k] = p[k][:n]
    return q


# ---------------------------------------------------------------------------------------------------------------------------------
# bundle-adjustment windows
# ---------------------------------------------------------------------------------------------------------------------------------
def permuted(b, rng, fixed="interleaved"):
    """The same graph with key-frames, landmarks and edges in another order.  fixed = "interleaved": a random key-frame order whose first
    key-frame is an optimised one; "last": every optimised key-frame before every fixed one.  Returns (window, inv) with inv["kf"],
    inv["mp"], inv["edge"] the new index of every old one: result_of_permuted[inv[...]] is in the order of `b`."""
    nkf, nmp, ne = len(b["kf_fixed"]), len(b["mp_pos"]), len(b["e_mp"])
    kf_order = rng.permutation(nkf)                                   # new -> old
    if fixed == "last":
        kf_order = np.concatenate([kf_order[b["kf_fixed"][kf_order] == 0], kf_order[b["kf_fixed"][kf_order] == 1]])
    else:
        free = np.flatnonzero(b["kf_fixed"][kf_order] == 0)
        if len(free) and free[0] != 0:
            kf_order[[0, free[0]]] = kf_order[[free[0], 0]]
    mp_order = rng.permutation(nmp)
    e_order = rng.permutation(ne)
    inv = dict(kf=np.argsort(kf_order), mp=np.argsort(mp_order), edge=np.argsort(e_order))
    w = dict(b)
    w["kf_pose"] = b["kf_pose"][kf_order]; w["kf_fixed"] = b["kf_fixed"][kf_order]; w["mp_pos"] = b["mp_pos"][mp_order]
    w["e_mp"] = inv["mp"][b["e_mp"]][e_order].astype(np.int32); w["e_kf"] = inv["kf"][b["e_kf"]][e_order].astype(np.int32)
    w["e_obs"] = b["e_obs"][e_order]; w["e_w"] = b["e_w"][e_order]
    return w, inv


def window(seed, n_mp, degrees=(), n_opt=5, n_fixed=30, fixed_only=(), deg_range=(3, 8), pose_noise=(np.deg2rad(1.0), 0.02), point_noise=0.03):
    """The key-frames of ba_problem(seed, n_opt, n_fixed) -- fixed ones first -- over n_mp landmarks in a box every key-frame has in front of
    it (|x|, |y| <= 1, 5 <= z <= 8), each observed by exactly the number of key-frames asked for: degrees[j] for landmark j, 3 to 8 for the
    others.  Landmarks listed in fixed_only are observed by fixed key-frames alone.  Gaussian pixel noise by octave, no outliers; edges
    grouped by landmark, ascending."""
    base = ba_problem(seed, n_opt, n_fixed, 1, 0.0, pose_noise=pose_noise)
    rng = np.random.default_rng(7000 + seed)
    K = K_TUM3.astype(np.float64)
    nkf = n_opt + n_fixed
    X = np.stack([rng.uniform(-1, 1, n_mp), rng.uniform(-1, 1, n_mp), rng.uniform(5, 8, n_mp)], 1)
    e_mp, e_kf, e_obs, e_w = [], [], [], []
    for p in range(n_mp):
        d = degrees[p] if p < len(degrees) else int(rng.integers(deg_range[0], deg_range[1] + 1))
        pool = np.flatnonzero(base["kf_fixed"]) if p in fixed_only else np.arange(nkf)
        assert d <= len(pool)
        for k in np.sort(rng.choice(pool, d, replace=False)):
            u, v, z = _project(base["truth_q"][k], base["truth_t"][k], X[p:p + 1], K)
            assert z[0] > 0.5
            octave = int(rng.integers(0, 8))
            du, dv = rng.normal(size=2) * 1.2 ** octave
            e_mp.append(p); e_kf.append(k); e_obs.append((u[0] + du, v[0] + dv)); e_w.append(1.0 / (np.float32(1.2) ** np.float32(2 * octave)))
    b = dict(base)
    b["mp_pos"] = (X + rng.normal(size=X.shape) * point_noise / np.sqrt(3)).astype(np.float32)
    b["e_mp"] = np.array(e_mp, np.int32); b["e_kf"] = np.array(e_kf, np.int32)
    b["e_obs"] = np.array(e_obs, np.float32).reshape(-1, 2); b["e_w"] = np.array(e_w, np.float32)
    b["truth_X"] = X
    return b


def with_degrees(seed, n_mp=40, degrees=DEGREES):
    """5 optimised and 30 fixed key-frames (still a window of the batched path: at most 29 optimised, at most 512 in all); landmark j < len(degrees)
    is observed by exactly degrees[j] key-frames.  k_baw_system gives a landmark 16 lanes: 15, 16, 17, 32 and 33 sit around one and two rounds."""
    return window(seed, n_mp, degrees)


def single_edge(seed):
    """One landmark, one edge, from an optimised key-frame."""
    b = window(seed, 1, (35,))
    k = int(np.flatnonzero((b["kf_fixed"] == 0)[b["e_kf"]])[0])
    for key in ("e_mp", "e_kf", "e_obs", "e_w"):
        b[key] = b[key][k:k + 1]
    return b


def without_observations_of(b, kf):
    """The window with every edge of key-frame kf removed."""
    keep = b["e_kf"] != kf
    w = dict(b)
    for key in ("e_mp", "e_kf", "e_obs", "e_w"):
        w[key] = b[key][keep]
    return w


def mirrored_landmark(b, kf=None, Xc=(0.3, -0.2, 4.0)):
    """One more landmark: the point reflection, through the optical centre of a fixed key-frame, of the point Xc in front of it, with a single
    edge from that key-frame that carries its exact projection (the reflected point projects to the same pixel).  Residual zero, depth
    negative: the erase rule can only fire by its depth clause."""
    kf = int(np.flatnonzero(b["kf_fixed"])[0]) if kf is None else kf
    q = b["kf_pose"][kf, :4].astype(np.float64); t = b["kf_pose"][kf, 4:].astype(np.float64)
    q /= np.linalg.norm(q)
    _, R = quat_rotate(q, np.zeros((1, 3)))
    Xw = (R.T @ (-np.asarray(Xc, np.float64) - t)).astype(np.float32)                 # world point whose camera coordinates are -Xc
    u, v, z = _project(q, t, Xw[None].astype(np.float64), K_TUM3.astype(np.float64))   # projected from the float32 point: the residual is rounding only
    assert z[0] < -1.0
    w = dict(b)
    w["mp_pos"] = np.concatenate([b["mp_pos"], Xw[None]])
    w["e_mp"] = np.concatenate([b["e_mp"], np.array([len(b["mp_pos"])], np.int32)])
    w["e_kf"] = np.concatenate([b["e_kf"], np.array([kf], np.int32)])
    w["e_obs"] = np.concatenate([b["e_obs"], np.array([[u[0], v[0]]], np.float32)])
    w["e_w"] = np.concatenate([b["e_w"], np.ones(1, np.float32)])
    return w


def rough_start(seed, n_opt=5, n_fixed=3, n_points=150, pose_noise=(np.deg2rad(4.0), 0.1), point_noise=0.1, outlier_frac=0.05):
    """ba_problem started far from the truth: LM rejects trials, and may stop before its iteration limit."""
    return ba_problem(seed, n_opt, n_fixed, n_points, outlier_frac, pose_noise=pose_noise, point_noise=point_noise)


def with_unit_quaternions(b):
    """The window with every key-frame quaternion re-normalised in float until that changes nothing: the conversions a bundle adjustment puts
    around its iterations (float -> unit double -> unit float) then return the input bit for bit."""
    w = dict(b)
    kp = b["kf_pose"].copy()
    for _ in range(4):
        q = kp[:, :4].astype(np.float64)
        q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])      # float32, summed left to right
        kp[:, :4] = q / n[:, None]
    w["kf_pose"] = kp
    return w


def invalid_graphs(b):
    """The three graphs the batched path's device-side validation refuses: a landmark index == nMP, a key-frame index == -1, an edge twice
    (of an optimised key-frame: the check counts a landmark's edges per optimised key-frame).  Returns {name: window}."""
    out = {}
    mid = len(b["e_mp"]) // 2
    w = dict(b); w["e_mp"] = b["e_mp"].copy(); w["e_mp"][mid] = len(b["mp_pos"]); out["e_mp == nMP"] = w
    w = dict(b); w["e_kf"] = b["e_kf"].copy(); w["e_kf"][mid] = -1; out["e_kf == -1"] = w
    e = int(np.flatnonzero((b["kf_fixed"] == 0)[b["e_kf"]])[len(b["e_kf"]) // 8])
    w = dict(b)
    for key in ("e_mp", "e_kf", "e_obs", "e_w"):
        w[key] = np.concatenate([b[key][:e + 1], b[key][e:]])
    out["duplicated edge"] = w
    return out


_CACHE = {}


def ba_case(name):
    """The named bundle-adjustment windows of the two test files (built once)."""
    if name not in _CACHE:
        _CACHE[name] = _BA_CASES[name]()
    return _CACHE[name]


_BA_CASES = {
    # the four solver routes of the permutation tests, about 150 landmarks each
    "batched": lambda: ba_problem(202, 5, 3, 150),                                    # 5 optimised key-frames: the window-batched path
    "tiles": lambda: ba_problem(208, 8, 3, 150),                                      # on a profiled handle: the host loop over k_ba_solve_tiles
    "panel": lambda: window(4, 150, (), 31, 3, deg_range=(10, 20)),                   # 31 optimised: the one-workgroup panel solver
    "large": lambda: window(2, 150, (), 44, 2, deg_range=(10, 20)),                   # 44 optimised: block-sparse Schur + blocked Cholesky
    "degrees": lambda: with_degrees(1),
    "single edge": lambda: single_edge(10),
    "fixed only": lambda: window(1, 40, (2, 1, 5), fixed_only=(0, 1)),                # landmarks 0 and 1 are seen by fixed key-frames alone
    "no observation": lambda: without_observations_of(with_degrees(1), 30),           # key-frame 30 is the first optimised one
    "mirrored": lambda: mirrored_landmark(with_degrees(1)),
    "rough early": lambda: rough_start(0),                                            # stops before the iteration limit
    "rough early, unit quaternions": lambda: with_unit_quaternions(rough_start(4)),       # (a seed whose quaternions do reach a fixed point)
    "rough rejecting": lambda: rough_start(10, n_fixed=1, pose_noise=(np.deg2rad(25.0), 1.0), point_noise=0.3, outlier_frac=0.1),   # three rejections in a row
    **{f"count {n}": (lambda n=n: window(COUNT_SEEDS[n], n)) for n in COUNTS},
}
BA_CASE_NAMES = list(_BA_CASES)
# Nine unknowns and more under two residuals: LM drives chi2 to the last bit within its iteration limit, whatever the seed (none of 60 is
# decisive), and then stops on a tie.  Poses, landmarks and flags are compared for these two, the iteration and trial counts are not.
TIED = ("single edge", "count 1")
GLOBAL_KW = dict(n_iterations=10, robust=True)
# which bundle adjustments run on which window: local, merge and global BA each take at least one solver route
BA_KINDS = {"batched": ("local", "merge"), "tiles": ("merge",), "panel": ("global", "local"), "large": ("local",), "rough early": ("local", "merge", "global"),
            "rough early, unit quaternions": ("global",),
            "rough rejecting": ("local", "merge", "global")}
BA_CASE_KINDS = [(n, k) for n in BA_CASE_NAMES for k in BA_KINDS.get(n, ("local", "merge"))]
ROUGH_BA = ["rough early", "rough rejecting"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the two conditions on the input (O = oracle_lib)
# ---------------------------------------------------------------------------------------------------------------------------------
def run_oracle(O, kind, a, **kw):
    """kind: "pose" | "local" | "merge" | "global".  Returns (result tuple, trace)."""
    fn = dict(pose=O.pose_optimization, local=O.local_ba, merge=O.merge_ba, **{"global": O.bundle_adjustment})[kind]
    if kind == "global" and not kw:
        kw = GLOBAL_KW
    r = fn(*a, **kw)
    return r, O.opt_last_trace()


def check_margin(O, kind, a, **kw):
    r, tr = run_oracle(O, kind, a, **kw)
    assert tr["margin"] >= MARGIN, f"{kind}: a chi2 lies {tr['margin']:.2e} (relative) from its threshold; choose another seed"
    return r, tr


def check_decisive(O, kind, a, **kw):
    r, tr = run_oracle(O, kind, a, **kw)
    assert tr["gain"] >= GAIN and tr["ended_rho0"] == 0, f"{kind}: an LM decision within {tr['gain']:.1e} of a tie ({tr['ended_rho0']} iterations ended on rho == 0)"
    return r, tr


def check_stable(O, kind, a, **kw):
    """One ulp on every observation: same flags and counts, the pose(s) within 1e-5."""
    r0, t0 = run_oracle(O, kind, a, **kw)
    a1 = list(a)
    i_obs = 1 if kind == "pose" else 5
    a1[i_obs] = ulp_up(a[i_obs])
    r1, t1 = run_oracle(O, kind, tuple(a1), **kw)
    for k in ("trials", "rejected", "ended_qmax", "ended_rho0"):
        assert t0[k] == t1[k], f"{kind}: {k} {t0[k]} -> {t1[k]} after one ulp on the observations"
    assert np.array_equal(np.asarray(r0[0]), np.asarray(r1[0])), f"{kind}: count {r0[0]} -> {r1[0]}"
    assert np.abs(np.asarray(r0[1], np.float64) - np.asarray(r1[1], np.float64)).max() <= 1e-5, f"{kind}: pose moved"
    if kind == "pose":
        assert np.array_equal(r0[2], r1[2]), "pose: outlier flags changed"
    elif kind != "global":
        assert np.array_equal(r0[3], r1[3]), f"{kind}: erase flags changed"
    return r0, t0
