"""rumi_submap_match (include/rumi_match.h) on the GPU against the C++ oracle (tests/cpp/submap_oracle.cc): the constructed cases of
tests/submap_scene.py, the seeded scenes, the sizes and batching, device-resident key-points.  Indices and counts: every comparison is exact."""
import numpy as np
import pytest

from submap_scene import SEEDS, TOL, batch40_scene, build_oracle, constructed_cases, device_frames, run_oracle, seeded_scene, sizes_scene
from test_submap_cpu import check_refusals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("submap"))


@pytest.fixture(scope="module")
def matcher():
    from rumi_slam_amd.submap import SubmapMatcher
    m = SubmapMatcher()
    yield m
    m.close()


def device(matcher, scene, on_device=False, tol=TOL):
    r = matcher.match(device_frames(scene, on_device), scene.pairs, tol)
    best2 = np.concatenate(r.best2) if r.best2 else np.zeros(0, np.int32)
    matches = np.concatenate(r.matches).reshape(-1, 2) if r.matches else np.zeros((0, 2), np.int32)
    assert r.total == len(matches) and np.array_equal(r.counts, np.diff(r.pair_start))
    return best2, r.pair_start, matches


def check(got, want):
    for name, g, w in zip(("best2", "pair_start", "matches"), got, want):
        diff = np.nonzero(np.asarray(g).ravel() != np.asarray(w).ravel())[0] if np.shape(g) == np.shape(w) else None
        print(f"{name}: shapes {np.shape(g)} {np.shape(w)}" + ("" if diff is None or not len(diff) else f", {len(diff)} differ, first at {diff[0]}"))
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("case", constructed_cases(), ids=lambda c: c[0].name)
def test_constructed_cases(oracle, matcher, case):
    """Tie order, thresholds, mvKeysUn gate against mvKeys distance, NULL slots, many-to-one, grid edges, double distance."""
    s, expect = case
    got = device(matcher, s)
    check(got, run_oracle(oracle, s))
    for i1, i2 in expect.items():
        assert got[0][i1] == i2, (s.name, i1)


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_scenes(oracle, matcher, seed):
    s = seeded_scene(seed)
    check(device(matcher, s), run_oracle(oracle, s))


def test_sizes_in_one_call(oracle, matcher):
    """n of 0, 1, 63, 64, 65 and 2000 in one call, one key-frame 2 shared by three pairs, an empty key-frame 2; the list in ascending i1."""
    s = sizes_scene()
    got, want = device(matcher, s), run_oracle(oracle, s)
    check(got, want)
    for p in range(len(s.pairs)):
        i1 = got[2][got[1][p]:got[1][p + 1], 0]
        assert (np.diff(i1) > 0).all()
    assert got[1][-1] > 1000


def test_a_pair_alone_and_inside_the_batch(oracle, matcher):
    """n_pairs = 40 against the oracle, and every fifth pair alone (n_pairs = 1): the same best2 and list as inside the batch."""
    s = batch40_scene()
    got = device(matcher, s)
    check(got, run_oracle(oracle, s))
    q = s.q_start()
    for p in range(0, 40, 5):
        alone = device(matcher, s.only(p))
        assert np.array_equal(alone[0], got[0][q[p]:q[p + 1]]) and np.array_equal(alone[2], got[2][got[1][p]:got[1][p + 1]])
        assert alone[1].tolist() == [0, got[1][p + 1] - got[1][p]]


@pytest.mark.parametrize("which", ["seed2", "sizes"])
def test_device_resident_key_points(matcher, which):
    """The key-point arrays as torch tensors on the GPU, read in place: identical to the host-array call."""
    s = seeded_scene(2) if which == "seed2" else sizes_scene()
    check(device(matcher, s, on_device=True), device(matcher, s))


def test_two_calls_and_a_fresh_handle_agree(matcher):
    from rumi_slam_amd.submap import SubmapMatcher
    s = seeded_scene(1)
    a, b = device(matcher, s), device(matcher, s)
    fresh = SubmapMatcher()
    c = device(fresh, s)
    fresh.close()
    check(b, a)
    check(c, a)


def test_refusals_with_a_live_handle(matcher):
    check_refusals(matcher._h)
    s = seeded_scene(0)
    r = matcher.match(device_frames(s), [], TOL)                       # no pairs: nothing to do
    assert r.total == 0 and r.pair_start.tolist() == [0]
