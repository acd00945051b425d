"""The scalar oracle of the Sim3 pose graph (tests/cpp/essential_oracle.cc) against independent restatements, and the committed scenes'
margins.  No GPU."""
import numpy as np
import pytest

import essential_scene as es


# ---- an independent restatement: Sim3 as a 4 x 4 matrix [sR t; 0 1], logarithm and exponential through scipy's matrix functions ----
def mat_of(S):
    from scipy.spatial.transform import Rotation
    M = np.eye(4)
    M[:3, :3] = S[7] * Rotation.from_quat(S[:4]).as_matrix()
    M[:3, 3] = S[4:7]
    return M


def log_of(M):
    """(omega, upsilon, sigma) of a similarity matrix by the matrix logarithm: log [sR t; 0 1] = [Omega + sigma I, upsilon; 0 0]."""
    from scipy.linalg import logm
    Lg = np.real(logm(M))
    sigma = np.trace(Lg[:3, :3]) / 3
    Om = Lg[:3, :3] - sigma * np.eye(3)
    return np.array([Om[2, 1], Om[0, 2], Om[1, 0], *Lg[:3, 3], sigma])


def exp_of(u):
    from scipy.linalg import expm
    G = np.zeros((4, 4))
    G[:3, :3] = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]]) + u[6] * np.eye(3)
    G[:3, 3] = u[3:6]
    return expm(G)


def py_error(C, S0, S1):
    return log_of(mat_of(C) @ mat_of(S0) @ np.linalg.inv(mat_of(S1)))


def oracle_error(C, S0, S1):
    e = np.zeros(7)
    es.oracle().ego_error(es._p(np.ascontiguousarray(C)), es._p(np.ascontiguousarray(S0)), es._p(np.ascontiguousarray(S1)), es._p(e))
    return e


def test_error_matches_matrix_logarithm():
    # Rotation angles above sqrt(2e-5) and scale logarithms above 1e-5: the general branch of Sim3::log, where it is the true logarithm.
    # (Below that angle upstream's coefficient B is not the series limit; the oracle restates upstream there)
    # Measured on the CPU: 4e-15 absolute on errors of order 1e-1; asserted with a tenfold margin.
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(50):
        S0 = es.sim3(rng.normal(0, 0.6, 3), rng.normal(0, 2, 3), np.exp(rng.normal(0, 0.2)))
        S1 = es.sim3(rng.normal(0, 0.6, 3), rng.normal(0, 2, 3), np.exp(rng.normal(0, 0.2)))
        Cm = es.smul(es.sim3(rng.normal(0, 0.05, 3), rng.normal(0, 0.1, 3), np.exp(rng.normal(0, 0.05))), es.smul(S1, es.sinv(S0)))
        worst = max(worst, np.abs(oracle_error(Cm, S0, S1) - py_error(Cm, S0, S1)).max())
    print("error vs matrix logarithm:", worst)
    assert worst < 4e-14


def py_system(sc):
    """H and b of one Gauss-Newton step from py_error, perturbing by exp_of(delta) on the left, delta = 1e-6 (central differences)."""
    free = [v for v in range(sc.n_v) if not sc.fixed[v] and (np.any(sc.v0 == v) or np.any(sc.v1 == v))]
    col = {v: k for k, v in enumerate(free)}
    n = 7 * len(free)
    H = np.zeros((n, n)); b = np.zeros(n)
    M = [mat_of(S) for S in sc.S]
    d = 1e-6
    for e in range(sc.n_e):
        a, c = int(sc.v0[e]), int(sc.v1[e])
        if sc.fixed[a] and sc.fixed[c]:
            continue
        Cm = mat_of(sc.meas[e])
        r = log_of(Cm @ M[a] @ np.linalg.inv(M[c]))
        J = {}
        for end, v in ((0, a), (1, c)):
            if v not in col:
                continue
            Jv = np.zeros((7, 7))
            for k in range(7):
                if k == 6 and sc.fix_scale[v]:
                    continue
                u = np.zeros(7); u[k] = d
                Mp, Mm = exp_of(u) @ M[v], exp_of(-u) @ M[v]
                ep = log_of(Cm @ (Mp if end == 0 else M[a]) @ np.linalg.inv(Mp if end == 1 else M[c]))
                em = log_of(Cm @ (Mm if end == 0 else M[a]) @ np.linalg.inv(Mm if end == 1 else M[c]))
                Jv[:, k] = (ep - em) / (2 * d)
            J[v] = Jv
        for v, Jv in J.items():
            b[7 * col[v]:7 * col[v] + 7] -= Jv.T @ r
            for w, Jw in J.items():
                H[7 * col[v]:7 * col[v] + 7, 7 * col[w]:7 * col[w] + 7] += Jv.T @ Jw
    return H, b


@pytest.mark.parametrize("name", ["free9", "two_free", "fix_scale_small_residual"])
def test_gauss_newton_step_matches_python(name):
    # The oracle's Jacobians are central differences of 1e-9 on errors of order 1e-1: their entries carry ~1e-16 / 1e-9 = 1e-7 of noise.
    # Measured on the CPU: H within 4e-7, b within 6e-7, the step within 1.1e-5 of their largest entries; asserted with a tenfold margin.
    sc = es.scene(name)
    lam = 1e-6        # keeps the fix_scale rows (zero but for lambda) solvable in both
    H, b, col, x = es.oracle_linear_system(sc, lam)
    Hp, bp = py_system(sc)
    xp = np.linalg.solve(Hp + lam * np.eye(len(bp)), bp)
    dH, db, dx = np.abs(H - Hp).max() / np.abs(Hp).max(), np.abs(b - bp).max() / np.abs(bp).max(), np.abs(x - xp).max() / np.abs(xp).max()
    print(name, "H", dH, "b", db, "x", dx)
    assert dH < 4e-6 and db < 6e-6 and dx < 1.1e-4


def test_same_minimum_as_scipy_least_squares():
    # fix_scale on every vertex keeps every error on the branch of Sim3::log that is the true logarithm (sigma == 0 exactly), so the
    # oracle's residuals are smooth and scipy can minimise the very same function.  Both run to convergence (20 iterations).
    # Measured on the CPU: final chi2 within 1.2e-10 relative, poses within 5e-6; asserted with a tenfold margin.
    from scipy.optimize import least_squares
    sc = es.scene("fix_scale_small_residual")
    ref = es.run_oracle(sc, 20)
    free = [v for v in range(sc.n_v) if not sc.fixed[v] and v != sc.isolated]

    def states(p):
        S = sc.S.copy()
        for k, v in enumerate(free):
            u = np.concatenate([p[6 * k:6 * k + 6], [0.0]]); E = np.zeros(8); o = np.zeros(8)
            es.oracle().ego_exp(es._p(u), es._p(E)); es.oracle().ego_mul(es._p(E), es._p(np.ascontiguousarray(sc.S[v])), es._p(o))
            S[v] = o
        return S

    def resid(p):
        S = states(p)
        return np.concatenate([oracle_error(sc.meas[e], S[sc.v0[e]], S[sc.v1[e]]) for e in range(sc.n_e)])

    sol = least_squares(resid, np.zeros(6 * len(free)), method="lm", xtol=1e-14, ftol=1e-14, gtol=1e-14)
    chi_s, chi_o = float(sol.fun @ sol.fun), float(ref["trace"][ref["stats"][0]])
    dpose = np.abs(states(sol.x) - ref["S"]).max()
    print("chi2 scipy", chi_s, "oracle", chi_o, "poses", dpose)
    assert abs(chi_s - chi_o) <= 1.2e-9 * chi_o
    assert dpose < 5e-5


@pytest.mark.parametrize("name", list(es.SCENES))
def test_committed_scenes_are_not_marginal(name):
    """The device's iteration and trial counts are compared with the oracle's on exactly these scenes: no trial's gain ratio may sit near
    zero and no iteration's improvement ratio within a factor of two of the 1e-3 threshold of the three-bad-iterations rule."""
    r = es.oracle_result(name)
    ratios = r["ratios"][~np.isnan(r["ratios"])]
    print(name, r["stats"], r["min_abs_rho"], ratios)
    assert r["stats"][0] >= 1
    assert r["min_abs_rho"] >= 1e-3
    assert not np.any((ratios > 0.5) & (ratios < 2.0))


def test_scene_has_what_the_kernels_need():
    for name in ("merge", "merge_short"):
        assert int(es.oracle_result(name)["stats"][3]) == (2 if name == "merge" else 1)        # both ways a run of 20 can end early
    assert all(int(es.oracle_result(k)["stats"][3]) == 2 and int(es.oracle_result(k)["stats"][0]) >= 4 for k in ("fix_scale_all", "fix_scale_some"))
    sc = es.scene("merge")
    ff = sc.fixed[sc.v0].astype(bool) & sc.fixed[sc.v1].astype(bool)
    f1 = sc.fixed[sc.v0].astype(bool) ^ sc.fixed[sc.v1].astype(bool)
    assert ff.any() and f1.any() and (~ff & ~f1).any()
    assert (sc.fixed[sc.v0] & ~sc.fixed[sc.v1]).any() and (~sc.fixed[sc.v0] & sc.fixed[sc.v1] & 1).any()      # a fixed end on either side
    sc = es.scene("free65")
    pairs = [tuple(sorted(p)) for p in zip(sc.v0.tolist(), sc.v1.tolist())]
    assert len(set(pairs)) < len(pairs)                                        # duplicated vertex pairs
    assert (sc.v0 < sc.v1).any() and (sc.v0 > sc.v1).any()                     # both orientations
    assert sc.isolated is not None and not np.any(sc.v0 == sc.isolated) and not np.any(sc.v1 == sc.isolated)
    assert sc.n_e % 4 != 0 and es.scene("one_free").n_e < 4                   # a partly empty wave at the end; fewer than four edges


def test_point_correction_oracle_matches_numpy():
    X, ref, (A8, B8), (A7, B7) = es.correction_case()
    got = es.oracle_correct_points(0, X, ref, A8, B8)
    want = X.copy()
    for i, v in enumerate(ref):
        if v >= 0:
            want[i] = es.smap(B8[v], es.smap(A8[v], X[i].astype(np.float64))).astype(np.float32)
    assert np.array_equal(got[ref < 0], X[ref < 0])
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    got = es.oracle_correct_points(1, X, ref, A7, B7)
    want = X.copy()
    for i, v in enumerate(ref):
        if v >= 0:
            a, b = np.concatenate([A7[v].astype(np.float64), [1.0]]), np.concatenate([B7[v].astype(np.float64), [1.0]])
            want[i] = es.smap(es.smul(a, es.sinv(b)), X[i].astype(np.float64)).astype(np.float32)
    assert np.array_equal(got[ref < 0], X[ref < 0])
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
