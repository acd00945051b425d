"""rumi_essential_graph / rumi_sim3_correct_points on the device against the scalar oracle (tests/cpp/essential_oracle.cc)."""
import ctypes as C

import numpy as np
import pytest

import essential_scene as es

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def opt():
    from rumi_slam_amd.optimizer import Optimizer
    o = Optimizer(max_pose_edges=64, max_pose_batch=1, max_kf=256, max_mp=1024, max_edges=4096)
    yield o
    o.close()


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def check_against_oracle(opt, name, n_it=None):
    sc, ref = es.scene(name), es.oracle_result(name, n_it)
    k = es.SCENES[name]["n_it"] if n_it is None else n_it
    S, stats, trace = opt.essential_graph(*sc.args(), n_iterations=k)
    it = int(ref["stats"][0])
    print(name, "stats", stats, ref["stats"], "poses", rel(S, ref["S"]), "trace", rel(trace[:it + 1], ref["trace"][:it + 1]))
    assert np.array_equal(stats, ref["stats"])
    assert rel(S, ref["S"]) < 1e-4                                   # the project's parity for optimisers
    assert rel(trace[:it + 1], ref["trace"][:it + 1]) < 1e-6
    assert np.all(np.isnan(trace[it + 1:])) and np.all(np.isnan(ref["trace"][it + 1:]))
    if sc.isolated is not None:                                      # the vertex without edges: bit-identical
        assert S[sc.isolated].tobytes() == sc.S[sc.isolated].tobytes()
    assert S[sc.fixed.astype(bool)].tobytes() == sc.S[sc.fixed.astype(bool)].tobytes()
    return S, stats, trace


@pytest.mark.parametrize("name", list(es.SCENES))
def test_matches_oracle(opt, name):
    check_against_oracle(opt, name)


@pytest.mark.parametrize("n_it", [1, 3, 20])
def test_iteration_counts(opt, n_it):
    check_against_oracle(opt, "free65", n_it)


def test_two_calls_same_bytes(opt):
    sc = es.scene("free65")
    a = opt.essential_graph(*sc.args(), n_iterations=20)
    b = opt.essential_graph(*sc.args(), n_iterations=20)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_free_gauge_is_accepted(opt):
    # no fixed vertex: the gauge is free and the result unpinned; only status, finiteness and a chi2 that does not grow are checked
    sc = es.make_scene(n_free=12, seed=2, free_gauge=True)
    assert not sc.fixed.any()
    S, stats, trace = opt.essential_graph(*sc.args(), n_iterations=5)
    assert np.all(np.isfinite(S)) and stats[0] >= 1
    assert trace[stats[0]] <= trace[0]


def test_only_fixed_fixed_edges_is_an_empty_graph(opt):
    sc = es.scene("two_free")
    S, stats, trace = opt.essential_graph(sc.S, np.ones(sc.n_v, np.uint8), sc.fix_scale, sc.v0, sc.v1, sc.meas, n_iterations=3)
    assert S.tobytes() == sc.S.tobytes() and not stats.any() and np.all(np.isnan(trace))


def test_stop_flag(opt):
    sc = es.scene("free9")
    S, stats, trace = opt.essential_graph(*sc.args(), n_iterations=5, stop_flag=np.ones(1, np.uint8))
    assert list(stats[[0, 1, 3]]) == [0, 0, 3] and S.tobytes() == sc.S.tobytes()
    assert abs(trace[0] - es.oracle_result("free9")["trace"][0]) <= 1e-6 * trace[0] and np.all(np.isnan(trace[1:]))


def test_zero_iterations_reports_the_first_chi2(opt):
    sc = es.scene("free9")
    S, stats, trace = opt.essential_graph(*sc.args(), n_iterations=0)
    assert list(stats[[0, 1, 3]]) == [0, 0, 0] and S.tobytes() == sc.S.tobytes() and len(trace) == 1
    assert abs(trace[0] - es.oracle_result("free9")["trace"][0]) <= 1e-6 * trace[0]


def _malformed():
    sc = es.scene("two_free")
    def mod(**kw):
        d = dict(S=sc.S.copy(), fixed=sc.fixed.copy(), fs=sc.fix_scale.copy(), v0=sc.v0.copy(), v1=sc.v1.copy(), meas=sc.meas.copy())
        for k, f in kw.items():
            f(d[k])
        return d
    def setv(i, j, v):
        def f(a):
            a[i, j] = v
        return f
    def set1(i, v):
        def f(a):
            a[i] = v
        return f
    return {
        "v0 negative": mod(v0=set1(0, -1)), "v0 too large": mod(v0=set1(1, sc.n_v)), "v1 negative": mod(v1=set1(0, -3)), "v1 too large": mod(v1=set1(2, sc.n_v + 5)),
        "self edge": mod(v0=set1(0, int(sc.v1[0]))), "nan pose": mod(S=setv(1, 5, np.nan)), "inf pose": mod(S=setv(0, 4, np.inf)),
        "pose quaternion": mod(S=setv(1, 3, 2.0)), "pose scale": mod(S=setv(1, 7, 0.0)), "nan measurement": mod(meas=setv(0, 6, np.nan)),
        "measurement quaternion": mod(meas=setv(1, 0, 1.5)), "measurement scale": mod(meas=setv(0, 7, -1.0)),
    }


@pytest.mark.parametrize("what", list(_malformed()))
def test_malformed_input_is_refused(opt, what):
    from rumi_slam_amd import capi
    d = _malformed()[what]
    S = d["S"].copy(); stats = np.full(4, 77, np.int32); trace = np.full(4, 55.0)
    rc = opt._lib.rumi_essential_graph(opt._h, len(S), capi.ptr(S), capi.ptr(d["fixed"]), capi.ptr(d["fs"]), len(d["v0"]), capi.ptr(d["v0"]), capi.ptr(d["v1"]),
                                       capi.ptr(d["meas"]), 3, None, capi.ptr(stats), capi.ptr(trace))
    assert rc == capi.RUMI_E_INVALID and opt._lib.rumi_last_error()
    assert S.tobytes() == d["S"].tobytes() and np.all(stats == 77) and np.all(trace == 55.0)


def test_capacity(opt):
    from rumi_slam_amd import capi
    sc = es.make_scene(n_free=300, seed=1, isolated=False)
    with pytest.raises(capi.RumiError) as e:
        opt.essential_graph(*sc.args(), n_iterations=1)
    assert e.value.code == capi.RUMI_E_CAPACITY


@pytest.mark.parametrize("mode", [0, 1])
def test_point_correction(opt, mode):
    X, ref, t8, t7 = es.correction_case()
    A, B = t8 if mode == 0 else t7
    got = opt.correct_points(X, ref, A, B, mode=mode)
    want = es.oracle_correct_points(mode, X, ref, A, B)
    print("mode", mode, rel(got, want))
    assert got[ref < 0].tobytes() == X[ref < 0].tobytes() and not np.array_equal(got[ref >= 0], X[ref >= 0])
    assert rel(got, want) < 1e-4


def test_point_correction_refuses_malformed(opt):
    from rumi_slam_amd import capi
    X, ref, (A, B), _ = es.correction_case()
    for bad in ("ref", "X", "tab"):
        x, r, a = X.copy(), ref.copy(), A.copy()
        if bad == "ref":
            r[5] = len(A)
        elif bad == "X":
            x[7, 1] = np.nan
        else:
            a[2, 3] = 3.0
        keep = x.copy()
        rc = opt._lib.rumi_sim3_correct_points(opt._h, 0, len(x), capi.ptr(x), capi.ptr(r), len(a), capi.ptr(a), capi.ptr(B))
        assert rc == capi.RUMI_E_INVALID and x.tobytes() == keep.tobytes()
