"""GPU tests of the sub-map alignment session (include/rumi_opt.h: rumi_submap_sim3_begin / _score / _ransac / _end; rumi_slam_amd.submap.SubmapSim3).

* Per iteration the session returns the bytes rumi_sim3_ransac returns for the same solver and triple with the resident set as its score set (second handle),
  and the integers and ratios of the CPU oracle; the transforms are within test_sim3solver_gpu._close of the oracle's.
* The sequential rule equals upstream's loop: mirror Sim3Solver objects run one after the other in blocks of 20 over one generator and one shared ratio, and
  submap_sim3_cases.replay over the per-iteration tables.
* Nothing depends on the chunk length.
All references are computed once per scene and shared."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import sim3_cases as S3
import submap_sim3_cases as SC
from rumi_slam_amd import capi
from rumi_slam_amd.optimizer import SIM3_CONVERGED, SIM3_EXHAUSTED, SIM3_NOT_REACHED
from rumi_slam_amd.sim3solver import GlibcRand, Sim3Solver
from rumi_slam_amd.submap import SUBMAP_SOLVER_DTYPE, SubmapSim3, SubmapSolver, draw_stream
from sim3_scene import sim3_ransac_problem
from test_sim3solver_gpu import _close

pytestmark = pytest.mark.gpu

SOLVER_N, SOLVER_ITS = (3, 40, 90, 129), (1, 7, 20, 33)


@pytest.fixture(scope="module")
def opt():
    from rumi_slam_amd.optimizer import Optimizer
    return Optimizer()


@pytest.fixture(scope="module")
def ref_opt():
    from rumi_slam_amd.optimizer import Optimizer
    return Optimizer()


def _cut(score, sizes, denoms):
    """The score set with pair p cut to its first sizes[p] matches and denominator denoms[p]."""
    ps = score["pair_start"]
    keep = np.concatenate([np.arange(ps[p], ps[p] + sizes[p]) for p in range(len(sizes))]).astype(np.int64)
    out = dict(score)
    for k in ("X1", "X2", "kp1", "kp2", "sigma2_1", "sigma2_2", "edge1", "edge2"):
        out[k] = np.ascontiguousarray(score[k][keep])
    out["pair_start"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    out["pair_denominator"] = np.array(denoms, np.int32)
    out["S_c1w1"], out["S_c2w2"] = score["S_c1w1"][:len(sizes)], score["S_c2w2"][:len(sizes)]
    return out


_scenes = {}


def scene(kind):
    """score set + four solvers (n = 3, 40, 90, 129) that share sim3_ransac_problem's world similarity; built once per kind.
    five: 5 pairs of 300 (longer than a slab of 256, no multiple of 64), 3, 0, 100 under denominator 150, and 64 matches.
    one / two / sixtyfour: that many pairs."""
    if kind in _scenes:
        return _scenes[kind]
    if kind == "five":
        base = sim3_ransac_problem(40, n_pairs=5, per_pair=330)["score"]
        score = _cut(base, [300, 3, 0, 100, 64], [305, 3, 4, 150, 0])
    elif kind == "sixtyfour":
        score = sim3_ransac_problem(41, n_pairs=64, per_pair=30)["score"]
    else:
        n = dict(one=1, two=2)[kind]
        score = sim3_ransac_problem(42 + n, n_pairs=n, per_pair=70)["score"]
    solvers = []
    for j, (n, its) in enumerate(zip(SOLVER_N, SOLVER_ITS)):
        pr = sim3_ransac_problem(50 + j, n_pairs=1, per_pair=20, n_solver=n, outlier_frac=0.3 if n > 3 else 0.0)
        solvers.append(dict(X1=pr["X1"], X2=pr["X2"], s1=pr["sigma2_1"], s2=pr["sigma2_2"], K=pr["K"], S_kf1w=pr["score"]["S_kf1w"], S_kf2w=pr["score"]["S_kf2w"], n=n,
                            its=its, fix_scale=(j == 1)))
    _scenes[kind] = dict(score=score, solvers=solvers)
    return _scenes[kind]


def _submap_solvers(sc, min_inliers):
    return [SubmapSolver(s["X1"], s["X2"], s["s1"], s["s2"], s["K"], s["K"], s["S_kf1w"], s["S_kf2w"], m, s["its"], s["fix_scale"]) for s, m in zip(sc["solvers"], min_inliers)]


def _bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


NEVER = tuple(SOLVER_N)                 # nIn > n cannot hold: nothing converges
IN_SOLVER_2 = (3, 40, 45, 60)           # solver 2 has 90 correspondences of which about 63 are consistent


def _per_solver(sc, tri, handle):
    """The reference of every iteration: rumi_sim3_ransac per solver with the resident set under that solver's key-frames, and the oracle."""
    out, h = [], 0
    for s in sc["solvers"]:
        seg = tri[h:h + s["its"]]
        score = dict(sc["score"], S_kf1w=s["S_kf1w"], S_kf2w=s["S_kf2w"])
        args = (s["X1"], s["X2"], s["s1"], s["s2"], s["K"], s["K"], seg)
        g = handle.Sim3Ransac(*args, fix_scale=s["fix_scale"], score=score, want_inliers=False)
        o = O.sim3_ransac(*args, fix_scale=s["fix_scale"], score=score)
        out.append((g, o))
        h += s["its"]
    return out


_refs = {}


def reference(kind, ref_opt, seed=5):
    key = (kind, seed)
    if key not in _refs:
        sc = scene(kind)
        tri = draw_stream(_submap_solvers(sc, NEVER), GlibcRand(seed))
        _refs[key] = (tri, _per_solver(sc, tri, ref_opt))
    return _refs[key]


@pytest.mark.parametrize("kind", ["five", "one", "two", "sixtyfour"])
def test_per_iteration_bytes(opt, ref_opt, kind):
    sc = scene(kind)
    tri, refs = reference(kind, ref_opt)
    ses = SubmapSim3(opt)
    ses.set_chunk(0)
    ses.begin(sc["score"])
    rc, out = ses.ransac_status(_submap_solvers(sc, NEVER), tri, want_all=True)
    ses.end()
    capi.check(rc)
    assert out["its_consumed"] == sum(SOLVER_ITS) and (out["state"] == SIM3_EXHAUSTED).all() and np.array_equal(out["its"], SOLVER_ITS)
    h = 0
    for (g, o), s in zip(refs, sc["solvers"]):
        sl = slice(h, h + s["its"])
        assert _bytes_equal(out["T12_all"][sl], S3.records_of(g)), "T12 bytes against rumi_sim3_ransac"
        assert np.array_equal(out["n_inliers_all"][sl], g["n_inliers"]) and _bytes_equal(out["median_all"][sl], g["median"])
        assert np.array_equal(out["n_inliers_all"][sl], o["n_inliers"]) and np.array_equal(out["median_all"][sl], o["median"])
        T = out["T12_all"][sl]
        _close(dict(R=T[:, :9].reshape(-1, 3, 3), t=T[:, 9:12], s=T[:, 12], valid=T[:, 13] != 0), o)
        h += s["its"]
    # the scene exercises what it was built for
    if kind == "five":
        d = np.diff(sc["score"]["pair_start"])
        assert d[0] > 256 and d[0] % 64 and d[1] == 3 and d[2] == 0 and sc["score"]["pair_denominator"][3] > d[3] and sc["score"]["pair_denominator"][4] == 0
        assert out["median_all"].max() > 0


def _composed(score, Sw):
    """gSc1w2 = gSc1w1 * gSw1w2 and gSc2w1 = gSc2w2 * gSw1w2^-1 per pair as 8 doubles, formed on the host (numpy)."""
    A = np.stack([S3.sim8(*S3.sim_mul(S3.sim_Rts(a), Sw)) for a in score["S_c1w1"]])
    B = np.stack([S3.sim8(*S3.sim_mul(S3.sim_Rts(b), S3.sim_inv(Sw))) for b in score["S_c2w2"]])
    return A, B


def _inliers_ref(ref_opt, score, A, B):
    return ref_opt.ComputeInliersNum(score["pair_start"], score["pair_denominator"], A, B, score["K4_1"], score["K4_2"], score["X1"], score["X2"], score["kp1"],
                                     score["kp2"], score["sigma2_1"], score["sigma2_2"], score["edge1"], score["edge2"])


def test_score_equals_sim3_inliers(opt, ref_opt):
    sc = scene("five")["score"]
    truth = (S3.rotvec([0.05, -0.2, 0.08]), np.array([0.4, -0.2, 0.3]), 1.25)
    off = (S3.rotvec([0.05, -0.2, 0.085]), np.array([0.41, -0.2, 0.3]), 1.25)
    ident = (np.eye(3), np.zeros(3), 1.0)
    Ss = [_composed(sc, w) for w in (truth, off, ident)]
    ses = SubmapSim3(opt)
    ses.begin(sc)
    for sel in ([0], [0, 1, 2]):
        med, ratio, inl = ses.score([Ss[k] for k in sel])
        for row, k in enumerate(sel):
            m, r, i = _inliers_ref(ref_opt, sc, *Ss[k])
            assert np.float32(m) == med[row] and _bytes_equal(ratio[row], r) and np.array_equal(inl[row], i)
        # without the masks and ratios
        L = ses._lib
        med2 = np.zeros(len(sel), np.float32)
        A = np.ascontiguousarray([Ss[k][0] for k in sel]); B = np.ascontiguousarray([Ss[k][1] for k in sel])
        capi.check(L.rumi_submap_sim3_score(opt._h, len(sel), capi.ptr(A), capi.ptr(B), None, None, capi.ptr(med2)))
        assert _bytes_equal(med2, med)
    assert med[0] > med[2] and inl[0].any() and not inl[0].all(), "the truth scores above the identity, and both answers occur"
    ses.end()


@pytest.mark.parametrize("c", S3.inliers_num_cases(), ids=lambda c: c["id"])
def test_score_on_constructed_inlier_cases(opt, ref_opt, c):
    """The ComputeInliersNum cases of sim3_cases (edge flags crossed, one float32 either side of the threshold, NaN / inf, empty pair, zero denominator)."""
    ses = SubmapSim3(opt)
    ses.begin(dict(c, S_c1w1=c["S_c1w2"], S_c2w2=c["S_c2w1"]))
    med, ratio, inl = ses.score([(c["S_c1w2"], c["S_c2w1"])])
    ses.end()
    m, r, i = ref_opt.ComputeInliersNum(*S3.inliers_args(c))
    assert np.float32(m) == med[0] and _bytes_equal(ratio[0], r) and np.array_equal(inl[0], i)
    assert np.array_equal(inl[0], c["expect"])


def _upstream_loop(ref_opt, sc, min_inliers, rng, best_ratio=0.0):
    """CloudMerging.cc:663-741 with the mirror solver: per solver while (!bNoMore && !bConverge) iterate(20), the ratio shared, break at convergence."""
    rows, ratio, conv_at = [], best_ratio, None
    for j, (s, m) in enumerate(zip(sc["solvers"], min_inliers)):
        if conv_at is not None:
            rows.append(None)
            continue
        sol = Sim3Solver(ref_opt, s["X1"], s["X2"], s["s1"], s["s2"], s["K"], s["K"], fix_scale=s["fix_scale"], rng=rng)
        sol.SetRansacParameters(0.99, m, 300)
        sol.mRansacMaxIts = s["its"]
        score = dict(sc["score"], S_kf1w=s["S_kf1w"], S_kf2w=s["S_kf2w"])
        conv = no_more = False
        while not conv and not no_more:
            _, no_more, conv, ratio = sol.iterate_rumination(20, score, ratio)
        rows.append((conv, sol.mnIterations, sol.mnBestInliers, np.float32(ratio), sol.mBestRotation.copy(), sol.mBestTranslation.copy(), np.float32(sol.mBestScale)))
        if conv:
            conv_at = j
    return rows, conv_at, float(ratio)


def _check_against_upstream(out, rows, conv_at, ratio):
    assert out["converged"] == conv_at and np.float32(out["best_ratio"]) == np.float32(ratio)
    for j, row in enumerate(rows):
        if row is None:
            assert out["state"][j] == SIM3_NOT_REACHED and out["its"][j] == 0 and out["best_hyp"][j] == -1
            continue
        conv, its, best_n, r, R, t, s = row
        assert out["state"][j] == (SIM3_CONVERGED if conv else SIM3_EXHAUSTED)
        assert out["its"][j] == its and out["best_inliers"][j] == best_n and out["best_ratio_after"][j] == r
        if out["best_hyp"][j] >= 0:          # mBest* of the mirror solver: the same kernels' bytes
            T = out["T12"][j]
            assert _bytes_equal(T[:9].reshape(3, 3), R) and _bytes_equal(T[9:12], t) and T[12] == s
    assert out["its_consumed"] == sum(r[1] for r in rows if r is not None)


def _check_against_replay(out, sc_solvers):
    """submap_sim3_cases.replay over the per-iteration tables the call returned (the consumed part of the stream)."""
    tables, h, used = [], 0, out["its_consumed"]
    for (m, its) in sc_solvers:
        a, b = min(h, used), min(h + its, used)
        T = out["T12_all"][a:b]
        pad = its - (b - a)
        tables.append((np.concatenate([T[:, 13] != 0, np.zeros(pad, bool)]), np.concatenate([out["n_inliers_all"][a:b], np.zeros(pad, np.int32)]),
                       np.concatenate([out["median_all"][a:b], np.zeros(pad, np.float32)])))
        h += its
    res, consumed, ratio = SC.replay(sc_solvers, tables, out["best_ratio_in"])
    assert consumed == used and np.float32(ratio) == np.float32(out["best_ratio"])
    for j, r in enumerate(res):
        got = (out["state"][j], out["its"][j], out["best_hyp"][j], out["best_inliers"][j], out["best_ratio_after"][j])
        assert got == (r.state, r.its, r.best_hyp, r.best_inliers, np.float32(r.best_ratio_after)), (j, got, r)
    return res


def _run(ses, solvers, rng, chunk, best_ratio=0.0):
    ses.set_chunk(chunk)
    out = ses.ransac(solvers, rng, best_ratio, want_all=True)
    out["best_ratio_in"] = best_ratio
    return out


def _same_outputs(a, b):
    assert _bytes_equal(a["results"], b["results"]) and a["its_consumed"] == b["its_consumed"]
    for k in ("n_inliers_all", "median_all", "T12_all"):
        assert _bytes_equal(a[k], b[k]), k         # the entries past its_consumed hold the fill of both calls


@pytest.mark.parametrize("min_inliers,best_ratio", [(IN_SOLVER_2, 0.0), (NEVER, 0.0), (IN_SOLVER_2, 0.3)], ids=["converges_in_solver_2", "never_converges", "best_ratio_in"])
def test_rule_against_upstream_loop_and_chunks(opt, ref_opt, min_inliers, best_ratio):
    sc = scene("five")
    rows, conv_at, ratio = _upstream_loop(ref_opt, sc, min_inliers, GlibcRand(5), best_ratio)
    if min_inliers is IN_SOLVER_2 and best_ratio == 0.0:
        assert conv_at == 2, "the scene converges in solver 2"
    if min_inliers is NEVER:
        assert conv_at is None
    want_rng = GlibcRand(5)
    want_rng.advance(sum(r[1] for r in rows if r is not None))
    want_next = want_rng.rand()
    ses = SubmapSim3(opt)
    ses.begin(sc["score"])
    solvers = _submap_solvers(sc, min_inliers)
    outs = []
    for chunk in (1, 7, 64, None, 0):             # edges on every iteration (so on the converging one), on the solver boundary at 28, one chunk, the default
        rng = GlibcRand(5)
        out = _run(ses, solvers, rng, chunk, best_ratio)
        assert rng.rand() == want_next, "the generator stands after the draws of the last consumed iteration"
        _check_against_upstream(out, rows, conv_at, ratio)
        outs.append(out)
    ses.end()
    _check_against_replay(outs[0], [(m, s.its) for m, s in zip(min_inliers, solvers)])
    for o in outs[1:]:
        _same_outputs(outs[0], o)
    assert sum(SOLVER_ITS[:2]) + SOLVER_ITS[2] == 28 and 28 % 7 == 0          # the chunk of 7 ends on a solver boundary


def _trap_session(opt):
    t = S3.trap_scene()
    ses = SubmapSim3(opt)
    return t, ses


def _trap_solver(t, names, min_inliers, score):
    ident = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
    tri = np.array([t["names"][k] for k in names], np.int32)
    return SubmapSolver(t["X1"], t["X2"], t["s1"], t["s2"], t["K"], t["K"], ident, ident, min_inliers, len(names)), tri


def _oracle_tables(t, tri, score):
    o = O.sim3_ransac(t["X1"], t["X2"], t["s1"], t["s2"], t["K"], t["K"], tri, score=score)
    return o["valid"], o["n_inliers"], o["median"]


@pytest.mark.parametrize("names,min_inliers,expect", [
    (["B", "B"], 30, dict(state=SIM3_EXHAUSTED, best_hyp=1, its=2)),                       # two identical iterations: the later one is held
    (["I", "G"], 15, dict(state=SIM3_CONVERGED, best_hyp=1, its=2)),                       # a degenerate set first: no convergence on the identity it stands for
    (["B", "I", "B2", "I2", "G"], 15, dict(state=SIM3_CONVERGED, best_hyp=4, its=5)),      # and in the middle
    (["I", "I2", "I"], 15, dict(state=SIM3_EXHAUSTED, best_hyp=0, best_inliers=0)),        # nothing but degenerate sets: 0 inliers under the first one's ratio
], ids=["tie", "degenerate_first", "degenerate_middle", "degenerate_only"])
def test_constructed_scenes(opt, names, min_inliers, expect):
    t, ses = _trap_session(opt)
    sol, tri = _trap_solver(t, names, min_inliers, t["score"])
    tables = _oracle_tables(t, tri, t["score"])
    if "I" in names:
        assert not tables[0][names.index("I")] and tables[1][names.index("I")] > min_inliers, "the trap: an invalid set whose identity has the inliers to converge"
    want, used, ratio = SC.replay([(min_inliers, len(names))], [tables])
    ses.begin(t["score"])
    outs = []
    for chunk in (1, None):
        rng = S3.ScriptRand(S3.script_words(t["n"], tri) + [0] * 9)
        out = _run(ses, [sol], rng, chunk)
        assert np.array_equal(out["triples"], tri) and rng.state() == [3 * used]
        outs.append(out)
    ses.end()
    _same_outputs(*outs)
    out, w = outs[0], want[0]
    assert (out["state"][0], out["its"][0], out["best_hyp"][0], out["best_inliers"][0]) == (w.state, w.its, w.best_hyp, w.best_inliers)
    assert out["best_ratio_after"][0] == np.float32(w.best_ratio_after) and out["its_consumed"] == used
    for k, v in expect.items():
        assert out[k][0] == v, (k, out[k][0], v)
    _check_against_replay(out, [(min_inliers, len(names))])


@pytest.mark.parametrize("slack,state", [(1, SIM3_CONVERGED), (0, SIM3_EXHAUSTED)], ids=["nIn_is_min_plus_1", "nIn_is_min"])
def test_ratio_exactly_one_tenth(opt, slack, state):
    """Denominators of ten times the clean hypothesis' counts: both ratios, so the median, are exactly 0.1f, and (double)0.1f > 0.10."""
    t, ses = _trap_session(opt)
    tri = np.array([t["names"]["G"], t["names"]["B"]], np.int32)
    ones = dict(t["score"], pair_denominator=np.ones(2, np.int32))
    cnt = O.sim3_ransac(t["X1"], t["X2"], t["s1"], t["s2"], t["K"], t["K"], tri, score=ones)["ratio"][0]          # count / 1
    assert cnt.min() >= 1 and np.array_equal(cnt, np.round(cnt))
    score = dict(t["score"], pair_denominator=(10 * cnt).astype(np.int32))
    valid, n_in, med = _oracle_tables(t, tri, score)
    assert valid.all() and med[0] == np.float32(0.1) and float(med[0]) > 0.10
    m = int(n_in[0]) - slack
    sol = SubmapSolver(t["X1"], t["X2"], t["s1"], t["s2"], t["K"], t["K"], score["S_kf1w"], score["S_kf2w"], m, 2)
    want, used, _ = SC.replay([(m, 2)], [(valid, n_in, med)])
    assert want[0].state == state
    ses.begin(score)
    out = _run(ses, [sol], S3.ScriptRand(S3.script_words(t["n"], tri)), 0)
    ses.end()
    assert out["state"][0] == state and out["its"][0] == want[0].its and out["its_consumed"] == used and out["best_inliers"][0] == want[0].best_inliers
    assert out["median_all"][0] == np.float32(0.1)


def test_two_runs_and_a_replaced_set(opt, ref_opt):
    sc5, sc1 = scene("five"), scene("one")
    tri, _ = reference("five", ref_opt)
    ses = SubmapSim3(opt)
    ses.set_chunk(0)
    solvers = _submap_solvers(sc5, IN_SOLVER_2)
    ses.begin(sc5["score"])
    a = ses.ransac_status(solvers, tri, want_all=True)
    b = ses.ransac_status(solvers, tri, want_all=True)
    assert a[0] == b[0] == capi.RUMI_OK
    _same_outputs(a[1], b[1])
    # begin again: the set is replaced, the results are those of the new set
    ses.begin(sc1["score"])
    c = ses.ransac_status(_submap_solvers(sc1, NEVER), tri, want_all=True)
    _, refs1 = reference("one", ref_opt)
    assert c[0] == capi.RUMI_OK and _bytes_equal(c[1]["median_all"], np.concatenate([g["median"] for g, _ in refs1]))
    assert not _bytes_equal(c[1]["median_all"][:a[1]["its_consumed"]], a[1]["median_all"][:a[1]["its_consumed"]])
    ses.end()


def test_errors_leave_outputs_untouched(opt):
    sc = scene("five")
    solvers = _submap_solvers(sc, NEVER)
    tri = draw_stream(solvers, GlibcRand(1))
    ses = SubmapSim3(opt)
    L = ses._lib

    def untouched(out):
        for k in ("results", "raw_used", "n_inliers_all", "median_all", "T12_all"):
            assert (np.frombuffer(out[k].tobytes(), np.uint8) == 0x77).all(), k

    def refused(solv, t, msg=None):
        rc, out = ses.ransac_status(solv, t, want_all=True, fill=0x77)
        assert rc == capi.RUMI_E_INVALID
        untouched(out)
        if msg:
            assert msg in capi.lib().rumi_last_error().decode()

    # no set: every entry but begin refuses
    refused(solvers, tri, "no score set")
    med = np.full(1, 7.0, np.float32); A = np.zeros((1, 5, 8))
    assert L.rumi_submap_sim3_score(opt._h, 1, capi.ptr(A), capi.ptr(A), None, None, capi.ptr(med)) == capi.RUMI_E_INVALID and med[0] == 7.0
    assert L.rumi_submap_sim3_end(opt._h) == capi.RUMI_E_INVALID
    # begin validates as rumi_sim3_ransac does
    bad = dict(sc["score"], pair_start=sc["score"]["pair_start"][::-1].copy())
    with pytest.raises(capi.RumiError, match="ascending"):
        ses.begin(bad)
    refused(solvers, tri, "no score set")            # a refused begin leaves no set behind
    ses.begin(sc["score"])
    t2 = tri.copy(); t2[1 + 7 + 3, 1] = 90            # solver 2 has n = 90: index 90 is one past its range
    refused(solvers, t2, "out of range")
    t2 = tri.copy(); t2[0, 0] = -1
    refused(solvers, t2, "out of range")
    # ranges out of order, a solver below three correspondences, its < 1
    rec = np.zeros(len(solvers), SUBMAP_SOLVER_DTYPE)
    first = 0
    for r, s in zip(rec, solvers):
        r["first"], r["n"], r["min_inliers"], r["its"] = first, s.N, s.min_inliers, s.its
        r["K4_1"], r["K4_2"], r["S_kf1w"], r["S_kf2w"] = s.K1, s.K2, s.S_kf1w, s.S_kf2w
        first += s.N
    cat = lambda name: np.concatenate([getattr(s, name) for s in solvers])
    arrays = (cat("X1"), cat("X2"), cat("s1"), cat("s2"))
    for field, j, value in (("first", 2, 0), ("n", 0, 2), ("its", 1, 0), ("first", 3, int(rec["first"][3]) + 1)):
        r2 = rec.copy(); r2[field][j] = value
        refused((r2,) + arrays, tri)
    # the untouched call still works, and end drops the set
    rc, out = ses.ransac_status((rec,) + arrays, tri)
    assert rc == capi.RUMI_OK and out["its_consumed"] == len(tri)
    ses.end()
    refused(solvers, tri, "no score set")
    # no solvers: nothing consumed
    ses.begin(sc["score"])
    rc, out = ses.ransac_status([], np.zeros((0, 3), np.int32))
    assert rc == capi.RUMI_OK and out["its_consumed"] == 0
    ses.end()
