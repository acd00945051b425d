"""The constructed optimiser cases (opt_cases.py) on the GPU against the CPU oracle: k_pose_opt on both sides of each of its size boundaries and
in a batch that needs both of its instantiations, the bundle adjustments on graphs in any order through every solver route, landmarks of
the degrees and windows of the landmark counts around k_baw_system's 16 x 16 tiling, the depth clause of the erase rule alone, starts rough
enough that Levenberg-Marquardt rejects trials, and the batched path's device-side validation.

Every comparison first asserts, on the oracle alone, that the input keeps its distance from every threshold (and, for the rough starts and
hopeless frames, that one ulp on the observations changes nothing): then poses and landmarks agree to 1e-4 and every flag and count
exactly.  The oracle's answers are computed once per input and shared."""
import numpy as np
import pytest

import opt_cases as C
import oracle_lib as O
from ba_scene import pose_problem
from test_optimizer_gpu import RTOL, _pose_close

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def opt():
    from rumi_slam_amd.optimizer import Optimizer
    o = Optimizer()
    try:
        yield o
    finally:
        o.close()


_REF = {}


def _ref(kind, key, a, stable=False, decisive=None, **kw):
    """The oracle's (result, trace) for an input, once; the conditions on the input are asserted on the way (decisive: every bundle adjustment
    whose iteration and trial counts are compared, that is all but opt_cases.TIED)."""
    if (kind, key) not in _REF:
        _REF[kind, key] = C.check_margin(O, kind, a, **kw)
        if (kind != "pose") if decisive is None else decisive:
            C.check_decisive(O, kind, a, **kw)
        if stable:
            C.check_stable(O, kind, a, **kw)
    return _REF[kind, key]


# ---------------------------------------------------------------------------------------------------------------------------------
# pose optimisation
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_pose(got, ref, tag):
    ng, T, out = got
    ng_ref, T_ref, out_ref = ref
    print(f"{tag}: n_good {ng} / {ng_ref}, {np.count_nonzero(out != out_ref)} flags differ, |dT| {np.abs(T - T_ref).max():.2e}")
    assert ng == ng_ref, f"{tag}: n_good {ng} vs {ng_ref}"
    assert np.array_equal(out, out_ref), f"{tag}: {np.count_nonzero(out != out_ref)} outlier flags differ"
    _pose_close(T, T_ref, tag)


@pytest.mark.parametrize("n", C.POSE_SIZES)
def test_pose_size_boundaries(opt, n):
    """n < 3 returns early (3 is the first that runs), n < 10 runs one round (9, 10, 11), a thread keeps 2 edges in registers and 256 threads
    make that 512 (511, 512, 513; 255, 256, 257: the second register edge comes into use), kPoseLdsEdges = 1152 switches to the global-memory
    instantiation (1151, 1152, 1153), 2305 gives a thread ten edges, eight of them from memory."""
    p = C.pose_case(n)
    ref, _ = _ref("pose", ("size", n), C.pose_args(p))
    _check_pose(opt.PoseOptimization(*C.pose_args(p)), ref, f"n = {n}")


def test_pose_batch_needs_both_instantiations(opt):
    """Frames on both sides of kPoseLdsEdges in one batch: both instantiations are launched with skipSmall, each leaves the other's frames alone.
    The same kernel at the same block size with fixed-order reductions: every frame is bit for bit its single call."""
    tiny = pose_problem(7, 300)
    probs = [C.pose_case(n) if n >= 3 else C.truncated(tiny, n) for n in C.BATCH_SIZES]
    start, Xw, obs, w, K, T0 = C.pose_batch(probs)
    assert list(np.diff(start)) == C.BATCH_SIZES
    ng, T, out = opt.PoseOptimizationBatch(start, Xw, obs, w, K, T0)
    for i, (n, p) in enumerate(zip(C.BATCH_SIZES, probs)):
        flags = out[start[i]:start[i + 1]]
        if n < 3:
            assert ng[i] == 0 and T[i].tobytes() == p["T0"].tobytes() and not flags.any(), f"frame {i} (n = {n}): returns 0, pose untouched"
            continue
        single = opt.PoseOptimization(*C.pose_args(p))
        assert ng[i] == single[0] and T[i].tobytes() == single[1].tobytes() and np.array_equal(flags, single[2]), f"frame {i} (n = {n}) differs from its single call"
        _check_pose((ng[i], T[i], flags), _ref("pose", ("size", n), C.pose_args(p))[0], f"batch frame {i} (n = {n})")


@pytest.mark.parametrize("n,seed,offset", C.ROUGH_POSE)
def test_pose_rough_start(opt, n, seed, offset):
    """0.4 m off with 30 % outliers: the oracle rejects at least five trials (lambda *= ni; ni *= 2), and ends where the kernel ends.  3 m and 5 m
    off: the start is outside the basin of the truth, and which round switches the robust kernel off decides the flags."""
    p = C.rough_start_pose(n, seed, offset)
    ref, tr = _ref("pose", ("rough", n, seed, offset), C.pose_args(p), stable=True)
    assert tr["rejected"] >= 5
    _check_pose(opt.PoseOptimization(*C.pose_args(p)), ref, f"rough start n = {n}")


@pytest.mark.parametrize("n,seed", C.EXACT)
def test_pose_start_at_the_truth(opt, n, seed):
    p = C.exact_frame(n, seed)
    ref, _ = _ref("pose", ("exact", n, seed), C.pose_args(p))
    ng, T, out = opt.PoseOptimization(*C.pose_args(p))
    assert ng == n and not out.any() and np.abs(T - p["T0"]).max() <= 2e-7, f"|T - T0| {np.abs(T - p['T0']).max():.2e}"
    _check_pose((ng, T, out), ref, f"exact n = {n}")


@pytest.mark.parametrize("n,seed", C.HOPELESS)
def test_pose_hopeless_frame(opt, n, seed):
    """Every correspondence an outlier after the first round: the three later rounds have no active edge and are skipped, the pose is the input."""
    p = C.hopeless_frame(n, seed)
    ref, tr = _ref("pose", ("hopeless", n, seed), C.pose_args(p), stable=True)
    assert ref[0] == 0 and ref[2].all()
    ng, T, out = opt.PoseOptimization(*C.pose_args(p))
    assert ng == 0 and out.all()
    assert np.abs(T - p["T0"]).max() <= 2 * EPS, f"|T - T0| {np.abs(T - p['T0']).max():.2e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# bundle adjustment
# ---------------------------------------------------------------------------------------------------------------------------------
def _run(o, kind, a):
    if kind == "local":
        return o.LocalBundleAdjustment(*a)
    if kind == "merge":
        return o.MergeBundleAdjustment(*a)
    return o.BundleAdjustment(*a, **C.GLOBAL_KW) + (None,)


def _check_ba(kind, b, got, ref, tr, tag="", counts=True):
    """Iterations and trials equal to the oracle's, poses and landmarks at RTOL, fixed key-frames untouched, erase flags equal."""
    stats, kp, mp, er = got
    its = ref[0]
    print(f"{tag} {kind}: stats {stats} oracle iterations {its} trials {tr['trials']} rejected {tr['rejected']}")
    if counts and kind == "merge":
        assert (stats[0], stats[3]) == (its[0], its[1]), f"{tag}: LM iterations of the two passes {stats} vs {its}"
    elif counts:
        assert stats[0] == its, f"{tag}: LM iterations {stats[0]} vs {its}"
    if counts:
        assert stats[1] == tr["trials"], f"{tag}: LM trials {stats[1]} vs {tr['trials']}"
    assert stats[2] == np.count_nonzero(b["kf_fixed"] == 0)
    for k in range(len(kp)):
        _pose_close(kp[k], ref[1][k], f"{tag} key-frame {k}")
    fixed = b["kf_fixed"] == 1
    assert np.array_equal(kp[fixed], b["kf_pose"][fixed]), "fixed key-frames must not move"
    scale = np.maximum(np.linalg.norm(ref[2], axis=1), 1e-2)
    assert (np.linalg.norm(mp - ref[2], axis=1) <= RTOL * scale).all(), f"{tag}: landmarks"
    if kind != "global":
        assert np.array_equal(er, ref[3]), f"{tag}: {np.count_nonzero(er != ref[3])} erase flags differ"


@pytest.mark.parametrize("name,kind", [("batched", "local"), ("batched", "merge"), ("tiles", "merge"), ("panel", "global"), ("panel", "local"), ("large", "local")])
def test_ba_graph_in_any_order(opt, name, kind):
    """rumi_opt.h takes key-frames and edges "in any order": fixed key-frames interleaved or last, landmarks and edges shuffled, through the
    window-batched path (which sorts the graph by landmark on the device), the host loop over k_ba_solve_tiles (a profiled handle), the
    one-workgroup panel solver (31 optimised key-frames) and the large path (44: co-observation pair lists)."""
    from rumi_slam_amd.optimizer import Optimizer
    b = C.ba_case(name)
    o = opt
    if name == "tiles":
        o = Optimizer()
    try:
        if name == "tiles":
            o.set_profiling(True)
        ref0, tr0 = _ref(kind, name, C.ba_args(b))
        g0 = _run(o, kind, C.ba_args(b))
        _check_ba(kind, b, g0, ref0, tr0, name)
        if name == "tiles":
            assert o.kernel_ms()["trials"] == g0[0][1] > 0                   # the profiled (host) loop ran every trial
        for seed, fixed in ((1, "interleaved"), (2, "last")):
            w, inv = C.permuted(b, np.random.default_rng(seed), fixed)
            ref, tr = _ref(kind, (name, fixed), C.ba_args(w))
            g = _run(o, kind, C.ba_args(w))
            _check_ba(kind, w, g, ref, tr, f"{name} {fixed}")
            # mapped back: the result of the window as it was
            assert np.array_equal(g[0], g0[0]), f"stats {g[0]} vs {g0[0]}"
            for k in range(len(g0[1])):
                _pose_close(g[1][inv["kf"]][k], g0[1][k], f"{name} {fixed} key-frame {k} against the unpermuted window")
            scale = np.maximum(np.linalg.norm(g0[2], axis=1), 1e-2)
            assert (np.linalg.norm(g[2][inv["mp"]] - g0[2], axis=1) <= RTOL * scale).all()
            if kind != "global":
                assert np.array_equal(g[3][inv["edge"]], g0[3])
    finally:
        if o is not opt:
            o.close()


@pytest.mark.parametrize("name", ["degrees", "single edge"] + [f"count {n}" for n in C.COUNTS])
@pytest.mark.parametrize("kind", ["local", "merge"])
def test_ba_degrees_and_counts(opt, name, kind):
    """k_baw_system gives a landmark 16 lanes and a chunk 16 landmarks: landmarks observed 0, 1, 2, 15, 16, 17, 32 and 33 times, windows of
    1, 15, 16, 17, 31 and 33 landmarks, a graph of one edge.

    The window of one landmark and the graph of one edge (opt_cases.TIED) have more unknowns than residuals: the oracle drives chi2 to its last
    bit and stops on a tie (test_optimizer_cases_cpu.py shows it), so their iteration and trial counts are not compared.  Measured on the
    MI355X: single edge, local BA, 7 iterations / 7 trials against the oracle's 5 / 5; one landmark, merge BA, second pass 2 iterations and
    11 trials in all against 3 and 17; poses, landmarks and erase flags agree."""
    b = C.ba_case(name)
    ref, tr = _ref(kind, name, C.ba_args(b), decisive=name not in C.TIED)
    _check_ba(kind, b, _run(opt, kind, C.ba_args(b)), ref, tr, name, counts=name not in C.TIED)


@pytest.mark.parametrize("kind", ["local", "merge"])
def test_ba_special_vertices(opt, kind):
    """An optimised key-frame nobody observes from keeps its pose (H_pp = lambda I, b_p = 0); a landmark only fixed key-frames see is refined."""
    b = C.ba_case("no observation")
    ref, tr = _ref(kind, "no observation", C.ba_args(b))
    got = _run(opt, kind, C.ba_args(b))
    _check_ba(kind, b, got, ref, tr, "no observation")
    assert np.abs(got[1][30] - b["kf_pose"][30]).max() <= 2 * EPS, f"the unobserved key-frame moved by {np.abs(got[1][30] - b['kf_pose'][30]).max():.2e}"
    f = C.ba_case("fixed only")
    ref, tr = _ref(kind, "fixed only", C.ba_args(f))
    got = _run(opt, kind, C.ba_args(f))
    _check_ba(kind, f, got, ref, tr, "fixed only")
    assert np.linalg.norm(ref[2][:2] - f["mp_pos"][:2], axis=1).min() > 1e-3, "the oracle refines the landmarks only fixed key-frames see"
    assert np.linalg.norm(got[2][:2] - f["mp_pos"][:2], axis=1).min() > 1e-3


@pytest.mark.parametrize("route", ["batched", "host loop"])
@pytest.mark.parametrize("kind", ["local", "merge"])
def test_ba_depth_clause_alone(opt, kind, route):
    """chi2 > 5.991 || depth <= 0: a landmark behind its only (fixed) key-frame whose residual is zero is erased, and stays where it is; on the
    window-batched path (k_baw_finalize, k_baw_mark) and, on a profiled handle, ba_run's host loop (k_ba_finalize, k_ba_mark)."""
    from rumi_slam_amd.optimizer import Optimizer
    b = C.ba_case("mirrored")
    ref, tr = _ref(kind, "mirrored", C.ba_args(b))
    o = opt if route == "batched" else Optimizer()
    try:
        if o is not opt:
            o.set_profiling(True)
        got = _run(o, kind, C.ba_args(b))
        if o is not opt:
            assert o.kernel_ms()["trials"] == got[0][1] > 0
    finally:
        if o is not opt:
            o.close()
    _check_ba(kind, b, got, ref, tr, "mirrored")
    assert ref[3][-1] == 1 and got[3][-1] == 1, "erased by the depth clause"
    assert np.abs(got[2][-1] - b["mp_pos"][-1]).max() <= 1e-6


@pytest.mark.parametrize("name", C.ROUGH_BA)
@pytest.mark.parametrize("kind", ["local", "merge", "global"])
def test_ba_rough_start(opt, name, kind):
    """Iterations AND trials equal to the oracle's: a call that stops on three small gains before its limit, and one that rejects trials two and
    three in a row (the second rejection multiplies lambda by the doubled ni)."""
    b = C.ba_case(name)
    ref, tr = _ref(kind, name, C.ba_args(b), stable=True)
    if name == "rough rejecting":
        assert tr["rejected_run"] >= 2
    elif kind == "local":
        assert ref[0] < 10
    _check_ba(kind, b, _run(opt, kind, C.ba_args(b)), ref, tr, name)


def test_global_ba_of_zero_and_one_iteration(opt):
    b = C.ba_case("rough early, unit quaternions")
    a = C.ba_args(b)
    _, kp, mp = O.bundle_adjustment(*a, 0, True)
    assert kp.tobytes() == b["kf_pose"].tobytes() and mp.tobytes() == b["mp_pos"].tobytes(), "the conversions around the iterations return this input bit for bit"
    stats, kp, mp = opt.BundleAdjustment(*a, n_iterations=0, robust=True)
    assert kp.tobytes() == b["kf_pose"].tobytes() and mp.tobytes() == b["mp_pos"].tobytes(), "no iteration: nothing moves"
    assert stats[0] == 0 and stats[1] == 0 and stats[3] == 0
    ref, tr = _ref("global", "one iteration", a, n_iterations=1, robust=True)
    got = opt.BundleAdjustment(*a, n_iterations=1, robust=True) + (None,)
    assert ref[0] == 1
    _check_ba("global", b, got, ref, tr, "one iteration")


def _raw_local_ba(o, b):
    """rumi_local_ba through the C entry, so that the outputs of a refused call can be looked at: (status, kf_pose, mp_pos, erase)."""
    from rumi_slam_amd import capi
    kp = np.ascontiguousarray(b["kf_pose"], np.float32).copy(); mp = np.ascontiguousarray(b["mp_pos"], np.float32).copy()
    kfix = np.ascontiguousarray(b["kf_fixed"], np.uint8); em = np.ascontiguousarray(b["e_mp"], np.int32); ek = np.ascontiguousarray(b["e_kf"], np.int32)
    eo = np.ascontiguousarray(b["e_obs"], np.float32); ew = np.ascontiguousarray(b["e_w"], np.float32); K4 = np.ascontiguousarray(b["K"], np.float32)
    erase = np.full(len(em), 0xA5, np.uint8); stats = np.zeros(4, np.int32)
    P = capi.ptr
    rc = o._lib.rumi_local_ba(o._h, len(kfix), P(kp), P(kfix), len(mp), P(mp), len(em), P(em), P(ek), P(eo), P(ew), P(K4), None, P(erase), P(stats))
    return rc, kp, mp, erase


def test_invalid_graphs_on_the_batched_path():
    """The window-batched path validates on the device: an edge index out of range (err bit 0), a landmark observed twice by a key-frame (bit 1).
    RUMI_E_INVALID, nothing written, and the handle goes on working."""
    from rumi_slam_amd import capi
    from rumi_slam_amd.optimizer import Optimizer
    b = C.ba_case("batched")
    ref, tr = _ref("local", "batched", C.ba_args(b))
    o = Optimizer()
    try:
        for name, w in C.invalid_graphs(b).items():
            rc, kp, mp, erase = _raw_local_ba(o, w)
            assert rc == capi.RUMI_E_INVALID, f"{name}: status {rc}"
            assert kp.tobytes() == w["kf_pose"].tobytes() and mp.tobytes() == w["mp_pos"].tobytes() and (erase == 0xA5).all(), f"{name}: outputs touched"
            with pytest.raises(capi.RumiError) as e:
                o.LocalBundleAdjustment(*C.ba_args(w))
            assert e.value.code == capi.RUMI_E_INVALID
            _check_ba("local", b, o.LocalBundleAdjustment(*C.ba_args(b)), ref, tr, f"after {name}")
    finally:
        o.close()


def test_invalid_window_inside_a_batch():
    """rumi_local_ba_batch returns the worst status; the invalid window reports RUMI_E_INVALID and keeps its arrays, its neighbours are bit for bit
    their single calls."""
    from rumi_slam_amd import capi
    from rumi_slam_amd.optimizer import Optimizer
    b, b2 = C.ba_case("batched"), C.ba_case("count 33")
    o = Optimizer()
    try:
        single = [o.LocalBundleAdjustment(*C.ba_args(b)), o.LocalBundleAdjustment(*C.ba_args(b2))]
        for name, w in C.invalid_graphs(b).items():
            res, rc, status = o.LocalBundleAdjustmentBatch([C.ba_args(b), C.ba_args(w), C.ba_args(b2)], 2, return_status=True)
            assert rc == capi.RUMI_E_INVALID and status == [capi.RUMI_OK, capi.RUMI_E_INVALID, capi.RUMI_OK], f"{name}: {rc} {status}"
            assert res[1][1].tobytes() == w["kf_pose"].tobytes() and res[1][2].tobytes() == w["mp_pos"].tobytes() and not res[1][3].any(), f"{name}: outputs touched"
            for s, g in zip(single, (res[0], res[2])):
                assert np.array_equal(s[0], g[0]) and s[1].tobytes() == g[1].tobytes() and s[2].tobytes() == g[2].tobytes() and np.array_equal(s[3], g[3]), \
                    f"{name}: a neighbour differs from its single call"
        with pytest.raises(capi.RumiError):                                   # the default still raises
            o.LocalBundleAdjustmentBatch([C.ba_args(b), C.ba_args(w)], 1)
    finally:
        o.close()
