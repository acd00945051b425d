"""The CreateNewMapPoints oracle (tests/cpp/newpoints_oracle.cc) against numpy, and the conditions the scenes of tests/newpoints_scene.py must
meet so that no GPU test of include/rumi_mapping.h passes on an empty case.  Needs no GPU.

Null vector.  The oracle defines Triangulate's null vector by Jacobi rotations on A^T A in double (rumi_mapping.h); numpy.linalg.svd of the same A
(float entries, taken to double) is the independent answer.  Pairs are compared when the two smallest singular values are SEPARATED:
s[2] - s[3] >= 1e-3 * s[0].  Reason for 1e-3: A's entries are float32, i.e. known to 2^-24 ~ 6e-8 of s[0]; the null direction moves by about
(perturbation) / (s[2] - s[3]), so below a separation of 1e-3 * s[0] the input's own rounding already moves the point by more than 6e-5, the
order of the project's 1e-4 bar, and neither answer is "the" point.  Measured on the nine scenes below (25 401 pairs that reach the
triangulation, all of them separated): the largest |x_oracle - x_numpy| / |x_numpy| is 5.9e-8, half a float32 ulp -- the two double results
differ by something of order 1e-16 * (s[0] / s[2])^2, far below float32, so what is measured is how often the final cast to float lands on
different neighbours.  The assertion is 4x the measured value, 2.4e-7: a cast that differs by one ulp in every coordinate moves the point by
up to sqrt(3) * 2^-23 = 2.1e-7 of its norm, which other seeds may reach and which is still the same point; 4x admits that and nothing else -- a wrong
eigenvector, which shows as an error of order 1."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from newpoints_scene import GATES, K_TUM3, SCENES, SF, TH_FAR, NewPointsScene, build_oracle, cut_kept_scene, median_depth, params, run_oracle

SEPARATION = 1e-3
NULLVEC_MEASURED = 5.9e-8
NULLVEC_TOL = 4 * NULLVEC_MEASURED

@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("newpoints"))


@pytest.fixture(scope="module")
def runs(oracle):
    out = []
    for seed, nn, nf, coarse, ori, far in SCENES:
        s = NewPointsScene(seed, nn, nf)
        out.append((s, run_oracle(oracle, s.cur, s.neigh, params(coarse, ori, far, TH_FAR)), (coarse, ori, far)))
    return out


def test_null_vector_against_numpy_svd(runs):
    worst, n_sep, n_all = 0.0, 0, 0
    for _, r, _ in runs:
        tr = r["trace"]
        tr = tr[(tr["gate"] != GATES.index("parallax")) & (tr["gate"] != GATES.index("w0"))]
        A = tr["A"].reshape(-1, 4, 4).astype(np.float64)
        _, s, vt = np.linalg.svd(A)
        v = vt[:, 3, :]
        x = v[:, :3] / v[:, 3:4]
        sep = (s[:, 2] - s[:, 3]) >= SEPARATION * s[:, 0]
        n_all += len(sep); n_sep += int(sep.sum())
        rel = np.linalg.norm(tr["x3D"].astype(np.float64) - x, axis=1) / np.linalg.norm(x, axis=1)
        worst = max(worst, float(rel[sep].max()))
    print(f"null vector: {n_sep} separated pairs of {n_all}, largest relative difference {worst:.3e}")
    assert n_sep > 5000 and n_sep > 0.9 * n_all
    assert worst <= NULLVEC_TOL


def test_triangulate_recovers_a_known_point(oracle):
    """Exact rays of a known point through two poses: the oracle's Triangulate returns it (the definition is a null vector, not just any vector)."""
    s = NewPointsScene(11, 7, 500)
    T1, T2 = s.views[0]["Tcw"], s.views[5]["Tcw"]
    for X in s.land[:50]:
        rays = []
        for T in (T1, T2):
            Xc = T[:, :3].astype(np.float64) @ X + T[:, 3]
            rays.append(np.array([Xc[0] / Xc[2], Xc[1] / Xc[2], 1.0], np.float32))
        A, x = np.zeros(16, np.float32), np.zeros(3, np.float32)
        assert oracle.npo_triangulate(O._p(rays[0]), O._p(rays[1]), O._p(np.ascontiguousarray(T1)), O._p(np.ascontiguousarray(T2)), O._p(A), O._p(x)) == 1
        assert np.linalg.norm(x - X) / np.linalg.norm(X) < 1e-3           # float32 rays over a baseline of a few percent of the depth


def test_median_depth_against_numpy_sort(oracle, runs):
    for s, _, _ in runs:
        for v, view in zip(s.views[1:], s.neigh):
            T = v["Tcw"]
            P = v["mp_pos"][v["kf_mp"] >= 0]
            z = ((T[2, 0] * P[:, 0] + T[2, 1] * P[:, 1]) + T[2, 2] * P[:, 2]) + T[2, 3]
            assert z.dtype == np.float32 and len(z) > 0
            want = np.sort(z)[(len(z) - 1) // 2]
            assert np.float32(median_depth(oracle, view)) == want


def _numpy_gates(C1, N2, idx1, idx2, prm):
    """LocalMapping.cc:506-626 in numpy float32 for arrays of pairs, the triangulation by numpy.linalg.svd.  Returns the gate per pair."""
    f = np.float32
    k1, k2 = C1["keys"][idx1], N2["keys"][idx2]
    T1, T2 = C1["Tcw"], N2["Tcw"]
    fx, fy, cx, cy = K_TUM3
    xn1 = np.stack([(k1["x"] - cx) / fx, (k1["y"] - cy) / fy, np.ones(len(k1), f)], 1)
    xn2 = np.stack([(k2["x"] - cx) / fx, (k2["y"] - cy) / fy, np.ones(len(k2), f)], 1)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    ray1 = np.stack([dot(T1[:, i], xn1) for i in range(3)], 1)
    ray2 = np.stack([dot(T2[:, i], xn2) for i in range(3)], 1)
    cos = dot(ray1, ray2) / (np.sqrt(dot(ray1, ray1)) * np.sqrt(dot(ray2, ray2)))
    gate = np.zeros(len(k1), np.int64)
    par = ~((cos > 0) & (cos.astype(np.float64) < 0.9998))
    A = np.stack([xn1[:, 0:1] * T1[2] - T1[0], xn1[:, 1:2] * T1[2] - T1[1], xn2[:, 0:1] * T2[2] - T2[0], xn2[:, 1:2] * T2[2] - T2[1]], 1)
    v = np.linalg.svd(A.astype(np.float64))[2][:, 3, :]
    X = (v[:, :3] / v[:, 3:4]).astype(f)
    cam = lambda T, r: dot(T[r, :3], X) + T[r, 3]
    z1, z2 = cam(T1, 2), cam(T2, 2)
    s1, s2 = SF[k1["octave"]], SF[k2["octave"]]
    with np.errstate(all="ignore"):
        e1 = (fx * cam(T1, 0) / z1 + cx - k1["x"]) ** 2 + (fy * cam(T1, 1) / z1 + cy - k1["y"]) ** 2
        e2 = (fx * cam(T2, 0) / z2 + cx - k2["x"]) ** 2 + (fy * cam(T2, 1) / z2 + cy - k2["y"]) ** 2
        d1 = np.sqrt(dot(X - C1["Ow"], X - C1["Ow"]))
        d2 = np.sqrt(dot(X - N2["Ow"], X - N2["Ow"]))
        rd, ro = d2 / d1, s1 / s2
    rf = f(prm.ratio_factor)
    tests = [("scale", (rd * rf < ro) | (rd > ro * rf)), ("far", bool(prm.far_points) & ((d1 >= f(prm.th_far_points)) | (d2 >= f(prm.th_far_points)))),
             ("dist0", (d1 == 0) | (d2 == 0)), ("reproj2", e2.astype(np.float64) > 5.991 * (s2 * s2).astype(np.float64)),
             ("reproj1", e1.astype(np.float64) > 5.991 * (s1 * s1).astype(np.float64)), ("z2", z2 <= 0), ("z1", z1 <= 0), ("parallax", par)]
    for name, hit in tests:                       # the earliest test in the reference's order wins: applied last
        gate = np.where(hit, GATES.index(name), gate)
    return gate


def test_gates_against_numpy(oracle):
    """The oracle's decision per evaluated pair against the numpy restatement, on a small scene: the same accepted set, and the same rejecting
    gate wherever numpy's SVD point and the oracle's agree on the side of the threshold (all pairs of this scene)."""
    s = NewPointsScene(21, 7, 500)
    prm = params(1, 0, 1, TH_FAR)
    r = run_oracle(oracle, s.cur, s.neigh, prm)
    tr = r["trace"]
    assert len(tr) > 300
    got = np.zeros(len(tr), np.int64)
    for k in range(7):
        sel = tr["neigh"] == k
        if sel.any():
            got[sel] = _numpy_gates(s.views[0], s.views[1 + k], tr["idx1"][sel], tr["idx2"][sel], prm)
    assert np.array_equal(got == 0, tr["gate"] == 0)
    assert np.array_equal(got, tr["gate"])
    acc = tr[tr["gate"] == 0]
    assert np.array_equal(acc["idx1"], r["points"]["idx1"]) and np.array_equal(acc["neigh"], r["points"]["neigh"])


def test_scene_conditions(runs):
    """What the scenes must contain for the GPU comparison to mean something (asserted on the oracle's output)."""
    assert any(len(s.neigh) == 30 for s, _, _ in runs)
    rejects = {g: 0 for g in GATES}
    for s, r, (coarse, ori, far) in runs:
        if len(s.neigh) >= 7:
            assert r["skipped"][3] == 1 and r["skipped"].sum() < len(s.neigh)          # the baseline test skips one neighbour and not the others
            assert r["per_neigh"][5] < r["per_neigh"][4]                               # nearly parallel rays next to it
        for g in GATES:
            rejects[g] += int((r["trace"]["gate"] == GATES.index(g)).sum())
        assert len(r["points"]) > 40 and r["per_neigh"].sum() == len(r["points"])
        assert np.array_equal(r["points"]["neigh"], np.sort(r["points"]["neigh"]))
        for k in range(len(s.neigh)):                                                  # vMatchedIndices order inside a neighbour
            i1 = r["points"]["idx1"][r["points"]["neigh"] == k]
            assert np.all(np.diff(i1) > 0)
        assert len(np.unique(r["points"]["idx1"])) == len(r["points"])               # a feature receives one point
    for g in ("parallax", "z1", "z2", "reproj1", "reproj2", "scale", "far"):          # x3Dh(3) == 0 and dist == 0 are exempt
        assert rejects[g] > 0, g
    # ... and every gate passes at least one pair: a pair stopped by a LATER gate, or accepted, went through it.  Per scene for the far-point gate,
    # which only exists where it is enabled: there it must reject a pair and let another through to the scale test.
    order = ["parallax", "w0", "z1", "z2", "reproj1", "reproj2", "dist0", "far", "scale", "ok"]
    for s, r, (coarse, ori, far) in runs:
        g = r["trace"]["gate"]
        if far:
            assert (g == GATES.index("far")).any(), "far rejects nothing in a far-enabled scene"
            assert np.isin(g, [GATES.index("scale"), GATES.index("ok")]).any(), "far passes nothing in a far-enabled scene"
        else:
            assert not (g == GATES.index("far")).any()
    allg = np.concatenate([r["trace"]["gate"] for _, r, _ in runs])
    for i, name in enumerate(order[:-1]):
        later = [GATES.index(x) for x in order[i + 1:]]
        assert np.isin(allg, later).any(), f"no pair passes {name}"


def test_sequential_skip_matters(oracle, runs):
    """At least 5 % of the features that create a point also have a candidate in a LATER neighbour (found with the flags of before the call):
    without the replay of the flags those would create a second point."""
    for s, r, (coarse, ori, far) in runs:
        n = len(s.neigh)
        if n < 7:
            continue
        c, v0 = s.views[0], s.cur
        cand = np.full((n, v0.frame.n), -1, np.int64)
        for k, v in enumerate(s.views[1:]):
            _, pairs = O.search_for_triangulation(c["keys"], c["desc"], c["kf_mp"], c["fv"], v["keys"], v["desc"], v["kf_mp"], v["fv"], SF, v["F12"], v["ep"],
                                                  False, coarse, False)
            cand[k, pairs[:, 0]] = pairs[:, 1]
        cand[r["skipped"] != 0] = -1
        later = sum(1 for p in r["points"] if (cand[p["neigh"] + 1:, p["idx1"]] >= 0).any())
        assert later >= 0.05 * len(r["points"]), (later, len(r["points"]))
        # and the loop did skip them: the flags a later neighbour starts from contain every earlier point
        fb = r["flags_before"]
        for p in r["points"]:
            assert fb[p["neigh"], p["idx1"]] < 0 and (p["neigh"] + 1 == n or fb[p["neigh"] + 1, p["idx1"]] >= 0)


def test_histogram_removes_pairs(runs):
    hit = 0
    for s, r, (coarse, ori, far) in runs:
        if ori:
            assert (r["hist_removed"] > 0).sum() >= min(2, len(s.neigh)), r["hist_removed"]
            hit += 1
        else:
            assert r["hist_removed"].sum() == 0
    assert hit >= 2


def test_histogram_on_its_first_cut(oracle):
    """10 / 1 / 1 / 1 pairs in bins 2 / 5 / 8 / 10: the oracle keeps the second and third bin (1 < 0.1f * 10 is false) and drops the fourth."""
    s, pairs, bins = cut_kept_scene(oracle)
    off = run_oracle(oracle, s.cur, s.neigh, params(0, 0, 0, TH_FAR))
    on = run_oracle(oracle, s.cur, s.neigh, params(0, 1, 0, TH_FAR))
    want = np.full(s.cur.frame.n, -1, np.int32)
    want[pairs[:, 0]] = pairs[:, 1]
    assert not on["skipped"][0] and np.array_equal(off["matches"][0], want), "the 13 constructed pairs are what the search finds"
    want[pairs[bins == 10, 0]] = -1
    assert np.array_equal(on["matches"][0], want) and on["hist_removed"][0] == 1 and (on["matches"][0] >= 0).sum() == 12


def test_empty_neighbour_and_no_neighbours(oracle):
    """A neighbour none of whose features holds a map point (the reference indexes an empty vDepths there): the median depth is -1, the
    neighbour is skipped, the others are unaffected.  Zero neighbours: nothing."""
    s = NewPointsScene(31, 7, 500, empty_neigh=(1,))
    assert (s.neigh[1].kf_mp < 0).all()
    assert median_depth(oracle, s.neigh[1]) == -1.0
    r = run_oracle(oracle, s.cur, s.neigh, params())
    assert r["skipped"][1] == 1 and r["per_neigh"][1] == 0 and r["per_neigh"][0] > 0 and r["per_neigh"][2] > 0
    ref = run_oracle(oracle, s.cur, [s.neigh[0]] + s.neigh[2:], params())
    keep = r["points"][r["points"]["neigh"] != 1]
    assert np.array_equal(keep["idx1"], ref["points"]["idx1"]) and np.array_equal(keep["x3D"], ref["points"]["x3D"])
    r0 = run_oracle(oracle, s.cur, [], params())
    assert len(r0["points"]) == 0 and len(r0["per_neigh"]) == 0
