"""rumi_create_new_map_points (include/rumi_mapping.h) on the GPU against the C++ oracle (tests/cpp/newpoints_oracle.cc), which runs
LocalMapping::CreateNewMapPoints as the reference writes it: one search per neighbour with the flags the earlier neighbours left.

The list (neigh, idx1, idx2) must be identical, order included; counts and skip flags identical.  x3D: the project's bar is 1e-4 relative
(DESIGN.md §2); both sides run the same float / double operations in the same order with correctly rounded division and square root, so the
points are expected bit for bit, and that is what is asserted (measured on the MI355X: 0 of the points of every case below differ)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from newpoints_scene import SCENES, SF, TH_FAR, NewPointsScene, build_oracle, cut_kept_scene, params, run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# the CPU tests' scenes (every count of neighbours and features, every switch both ways) and further seeds of the large ones
CASES = SCENES + [(40, 30, 2000, 0, 1, 0), (41, 30, 1000, 1, 0, 0), (42, 7, 500, 0, 0, 1), (43, 30, 500, 0, 1, 1), (44, 1, 2000, 0, 1, 0)]


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("newpoints"))


def matcher(ori, **kw):
    from rumi_slam_amd.matcher import ORBmatcher
    return ORBmatcher(0.6, bool(ori), **kw)


def gpu_call(m, s, neigh, coarse, far, **kw):
    from rumi_slam_amd.mapping import CreateNewMapPoints
    from newpoints_scene import RATIO_FACTOR
    return CreateNewMapPoints(m, s.cur, neigh, RATIO_FACTOR, bool(coarse), bool(far), TH_FAR, **kw)


def assert_same(got, want):
    pts, per, skipped = got
    assert np.array_equal(skipped, want["skipped"])
    assert np.array_equal(per, want["per_neigh"])
    for f in ("neigh", "idx1", "idx2"):
        assert np.array_equal(pts[f], want["points"][f]), f
    a, b = pts["x3D"], want["points"]["x3D"]
    rel = np.linalg.norm(a.astype(np.float64) - b, axis=1) / np.linalg.norm(b.astype(np.float64), axis=1) if len(b) else np.zeros(0)
    ndiff = int((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum()) if len(b) else 0
    print(f"x3D: {len(b)} points, {ndiff} differ in a bit, largest relative difference {rel.max() if len(rel) else 0.0:.3e}")
    assert (rel <= 1e-4).all()
    assert ndiff == 0


def test_symbols():
    from rumi_slam_amd import capi
    L = capi.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rumi_mapping.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rumi_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(capi.MAPPING_SYMBOLS)
    for name in declared:
        getattr(L, name)


@pytest.mark.parametrize("seed,nn,nf,coarse,ori,far", CASES)
def test_against_oracle(oracle, seed, nn, nf, coarse, ori, far):
    s = NewPointsScene(seed, nn, nf)
    want = run_oracle(oracle, s.cur, s.neigh, params(coarse, ori, far, TH_FAR))
    assert len(want["points"]) > 40
    m = matcher(ori)
    assert_same(gpu_call(m, s, s.neigh, coarse, far), want)
    m.close()


def test_nodes_of_more_than_64_features(oracle):
    """A coarse FeatureVector (10 nodes of 80 to 110 features a side): k_newpts_match walks the current node in tiles of 64 features and
    the neighbour's in chunks of 64 candidates, carrying the best key across chunks."""
    for coarse, ori in ((0, 1), (1, 0)):
        s = NewPointsScene(60, 7, 1000, levelsup=2)
        assert np.diff(s.cur.fv.offsets).min() > 64 and all(np.diff(nb.fv.offsets).min() > 64 for nb in s.neigh)     # every node: two chunks a side
        want = run_oracle(oracle, s.cur, s.neigh, params(coarse, ori, 0, TH_FAR))
        assert len(want["points"]) > 100
        m = matcher(ori)
        assert_same(gpu_call(m, s, s.neigh, coarse, 0), want)
        m.close()


def test_histogram_on_its_first_cut(oracle):
    """newpoints_scene.cut_kept_scene: 10 / 1 / 1 / 1 pairs in four rotation bins.  The pairs of the second and third bin stay, the fourth goes."""
    from rumi_slam_amd.mapping import last_matches
    s, pairs, bins = cut_kept_scene(oracle)
    want = run_oracle(oracle, s.cur, s.neigh, params(0, 1, 0, TH_FAR))
    m = matcher(1)
    assert_same(gpu_call(m, s, s.neigh, 0, 0), want)
    got = last_matches(m, 1, s.cur.frame.n)
    assert np.array_equal(got, want["matches"])
    assert np.array_equal(got[0][pairs[:, 0]], np.where(bins == 10, -1, pairs[:, 1]))
    m.close()


def test_more_than_2048_features(oracle):
    """Key-frames of more than 2048 features: k_newpts_depth ranks over more than one LDS tile, k_newpts_replay over three chunks."""
    s = NewPointsScene(61, 7, 2600)
    assert s.cur.frame.n > 2048 and all(nb.frame.n > 2048 and (nb.kf_mp >= 0).sum() > 1100 for nb in s.neigh)
    want = run_oracle(oracle, s.cur, s.neigh, params(0, 1, 1, TH_FAR))
    assert want["skipped"][3] == 1 and want["skipped"].sum() == 1 and len(want["points"]) > 300
    m = matcher(1)
    assert_same(gpu_call(m, s, s.neigh, 0, 1), want)
    m.close()


@pytest.mark.parametrize("seed,nn,nf,coarse,ori", [(0, 30, 1000, 0, 0), (1, 30, 1000, 0, 1), (4, 7, 1000, 1, 1)])
def test_stages_against_search_for_triangulation(oracle, seed, nn, nf, coarse, ori):
    """The path of before this entry, composed here: rumi_search_for_triangulation neighbour by neighbour, each with the flags the oracle's loop
    had reached, gives the matches the new call's search + replay hold for that neighbour."""
    from rumi_slam_amd.mapping import last_matches
    from rumi_slam_amd.matcher import SearchForTriangulation
    s = NewPointsScene(seed, nn, nf)
    want = run_oracle(oracle, s.cur, s.neigh, params(coarse, ori, 0, TH_FAR))
    m = matcher(ori)
    gpu_call(m, s, s.neigh, coarse, 0)
    got = last_matches(m, nn, s.cur.frame.n)
    assert np.array_equal(got, want["matches"])
    total = 0
    for k, nb in enumerate(s.neigh):
        if want["skipped"][k]:
            assert (got[k] < 0).all()
            continue
        n, pairs = SearchForTriangulation(m, s.cur.frame, s.cur.fv, want["flags_before"][k], nb.frame, nb.fv, nb.kf_mp, nb.F12, nb.epipole2, False, bool(coarse))
        mine = np.nonzero(got[k] >= 0)[0]
        assert n == len(mine) and np.array_equal(pairs[:, 0], mine) and np.array_equal(pairs[:, 1], got[k][mine])
        total += n
    assert total > 200
    m.close()


def test_two_runs_are_byte_identical(oracle):
    s = NewPointsScene(3, 30, 2000)
    m = matcher(1)
    a = gpu_call(m, s, s.neigh, 0, 1)
    b = gpu_call(m, s, s.neigh, 0, 1)
    m2 = matcher(1)
    c = gpu_call(m2, s, s.neigh, 0, 1)
    for x, y in ((a, b), (a, c)):
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))
    assert len(a[0]) > 500
    m.close(); m2.close()


@pytest.mark.parametrize("prefix", [1, 4, 6, 17])
def test_truncated_list_gives_the_prefix(prefix):
    """A caller that stops at `if (i > 0 && CheckNewKeyFrames()) return;` applies a prefix: the first neighbours' results do not depend on the rest."""
    s = NewPointsScene(1, 30, 1000)
    m = matcher(1)
    full = gpu_call(m, s, s.neigh, 0, 1)
    part = gpu_call(m, s, s.truncated(prefix), 0, 1)
    n = int(full[1][:prefix].sum())
    assert n == len(part[0]) and (prefix < 2 or n > 50)
    assert part[0].tobytes() == full[0][:n].tobytes()
    assert np.array_equal(part[1], full[1][:prefix]) and np.array_equal(part[2], full[2][:prefix])
    m.close()


def test_empty_neighbour_and_no_neighbours(oracle):
    s = NewPointsScene(31, 7, 500, empty_neigh=(1,))
    m = matcher(0)
    want = run_oracle(oracle, s.cur, s.neigh, params(0, 0, 0, TH_FAR))
    got = gpu_call(m, s, s.neigh, 0, 0)
    assert got[2][1] == 1 and got[1][1] == 0
    assert_same(got, want)
    pts, per, skipped = gpu_call(m, s, [], 0, 0)
    assert len(pts) == 0 and len(per) == 0 and len(skipped) == 0
    m.close()


def test_statuses(oracle):
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import MAX_NEIGH, CreateNewMapPoints, _lib, pack
    from newpoints_scene import RATIO_FACTOR
    s = NewPointsScene(2, 7, 500)
    want = run_oracle(oracle, s.cur, s.neigh, params(0, 1, 0, TH_FAR))
    m = matcher(1)
    # an output list that is too short: RUMI_E_CAPACITY, and the next call is unaffected
    with pytest.raises(capi.RumiError) as e:
        gpu_call(m, s, s.neigh, 0, 0, cap=10)
    assert e.value.code == capi.RUMI_E_CAPACITY
    assert_same(gpu_call(m, s, s.neigh, 0, 0), want)
    m.close()
    # key-frames larger than the matcher's arenas
    small = matcher(1, max_features=256, max_queries=4096)
    with pytest.raises(capi.RumiError) as e:
        gpu_call(small, s, s.neigh, 0, 0)
    assert e.value.code == capi.RUMI_E_CAPACITY
    small.close()
    m = matcher(1)
    L = _lib()
    c, arr = pack(s.cur, s.neigh)
    prm = params(0, 1, 0, TH_FAR)
    out = np.zeros(500, np.dtype([("a", "<i4", 3), ("b", "<f4", 3)]))
    per, sk, n = np.zeros(64, np.int32), np.zeros(64, np.uint8), C.c_int32()
    call = lambda h, cur, nb, nn, p, o, cap, no: L.rumi_create_new_map_points(h, cur, nb, nn, p, o, cap, no, capi.ptr(per), capi.ptr(sk))
    good = (m._h, C.byref(c), C.byref(arr), 7, C.byref(prm), capi.ptr(out), 500, C.byref(n))
    assert call(*good) == capi.RUMI_OK and n.value == len(want["points"])
    for i, bad in [(0, None), (1, None), (2, None), (3, -1), (3, MAX_NEIGH + 1), (4, None), (5, None), (6, -1), (7, None)]:
        a = list(good)
        a[i] = bad
        assert call(*a) == capi.RUMI_E_INVALID, i
    # a FeatureVector that points outside the key-frame, an octave outside mvScaleFactors: refused before anything reaches the device
    fv = s.neigh[2].fv
    keep = int(fv.indices[5])
    fv.indices[5] = 100000
    assert call(*good) == capi.RUMI_E_INVALID
    fv.indices[5] = keep
    fv.indices[5] = fv.indices[6]                       # a feature listed twice
    assert call(*good) == capi.RUMI_E_INVALID
    fv.indices[5] = keep
    ids = s.cur.fv.node_ids                             # node ids out of order: the kernels search them by bisection
    ids[[2, 3]] = ids[[3, 2]]
    assert call(*good) == capi.RUMI_E_INVALID
    ids[[2, 3]] = ids[[3, 2]]
    keys = s.neigh[4].frame.keys
    keys["octave"][7] = 8
    assert call(*good) == capi.RUMI_E_INVALID
    keys["octave"][7] = 0
    assert call(*good) == capi.RUMI_OK
    m.close()
