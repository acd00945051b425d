"""rumi_common_regions_bow on the GPU: every comparison is exact.  A pair is checked by the oracle's SearchByBoW(KF, KF), a group's union by the
restatement of LoopClosing.cc:635-651 in common_regions_scene; constructed scenes also carry their results written down by hand."""
import numpy as np
import pytest

import oracle_lib as O
from common_regions_scene import (CONTENDED_NODE, NODE_SIZES, SEEDS, contended_scene, cur_size_scene, describe, empty_member_scene, expect_tuple, expected, from_case, gpu_pair, hand_cases,
                                  mixed_groups, node_size_scene, run_gpu, same, seeded_scene, views)
from match_cases import all_cases

pytestmark = pytest.mark.gpu

BOW_KF_CASES = [c for c in all_cases() if c.member == "BOW_KF"]


@pytest.fixture(scope="module")
def M():
    from rumi_slam_amd import matcher
    return matcher


@pytest.fixture(scope="module")
def h(M):
    return M.ORBmatcher(0.9, True)


@pytest.fixture(scope="module")
def seeded():
    """seed -> (scene, the literal loop's results), computed once."""
    out = {}
    for seed in SEEDS:
        s = seeded_scene(seed)
        out[seed] = (s, expected(O, s))
    return out


def check(M, h, scene, want=None):
    want = expected(O, scene) if want is None else want
    got = run_gpu(M, h, scene)
    assert same(got, want), scene.name + ": " + describe(got, want)
    return got


@pytest.mark.parametrize("case", BOW_KF_CASES, ids=lambda c: c.id)
def test_constructed_pair_cases_as_a_group_of_one(M, h, case):
    """Ties, best == second, bestDist1 of 49 and 50, the ratio on and off its boundary, two current features that want one member feature, the
    histograms, node sizes 63 .. 257: the expectation is the case's own, written down from the rule."""
    m12, nm, pt, mem, num, most = run_gpu(M, h, from_case(case))
    assert np.array_equal(m12[0], case.arr) and nm[0] == case.count
    assert np.array_equal(pt[0], case.arr) and np.array_equal(mem[0], np.where(case.arr >= 0, 0, -1))           # member feature i holds point i
    assert num[0] == case.count and most.tolist() == [[0, case.count]]


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0].name)
def test_hand_written_scenes(M, h, case):
    """Gated member features that would have been best and second best; cur_good = 0; nodes on one side only; rotation bin 30 -> 0; a histogram
    that removes matches the union must then not see."""
    scene, e = case
    check(M, h, scene, expect_tuple(e))


@pytest.mark.parametrize("size", NODE_SIZES)
def test_member_node_sizes(M, h, size):
    """0, 1, 15, 16, 17, 33 and 512 features in the member's node keep a lane's `taken` flags in a register; from 513 on they lie in LDS words
    (1024: the last size of two words a lane, 1025: the first of three).  No size leaves the device: same results."""
    check(M, h, node_size_scene(size))


def test_contended_node_above_512(M, h):
    """A member node of 1100 features in which, in every 512-position stretch, two current features want the member feature at the stretch's last
    position: the first takes it, the second must find it taken and settles for the stretch's first.  A lane that lost a `taken` bit past
    position 511 would hand the same feature out twice."""
    size = CONTENDED_NODE
    m12 = check(M, h, contended_scene())[0]
    for i, s0 in enumerate(range(0, size, 512)):
        last = min(s0 + 511, size - 1)
        assert m12[0][2 * i] == size - 1 - last and m12[0][2 * i + 1] == (size - 1 - s0 if last != s0 else -1), (size, s0)


def test_malformed_angle_stays_inside_the_histogram(M, h):
    """An angle no key-point has (930 degrees against 0: round(930 / 30) = 31, past the 30 bins) is counted in the last bin, 29, where the entry
    keeps it: eleven matches in bin 2 and this one in bin 29, 1 < 0.1f * 11 drops it (ORBmatcher.cc:1820).  The reference indexes past rotHist
    here, so the expectation is written down by hand, not asked of the oracle."""
    from common_regions_scene import Build
    from match_cases import desc_at
    s = Build(6)
    for k, a1 in enumerate([60.0] * 11 + [930.0]):
        b = s.base()
        s.cur(b, 3 + 2 * k, angle=a1); s.feat(0, desc_at(b, 3, s.rng), 3 + 2 * k, k, angle=0.0)
    keep = list(range(11)) + [-1]
    e = dict(matches12=[keep], nmatches=[11], matched_point=[keep], matched_member=[[0] * 11 + [-1]], num=[11], most=[[0, 11]])
    check(M, h, s.scene("angle_930", [[0]], 12, ori=True), expect_tuple(e))


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_current_keyframe_sizes(M, h, n):
    check(M, h, cur_size_scene(n))


def test_member_without_features(M, h):
    got = check(M, h, empty_member_scene())
    assert got[1][1] == 0


def test_nothing_to_search(M, h):
    """No groups; a group without members; a current key-frame without features."""
    s = cur_size_scene(64)
    m12, nm, pt, mem, num, most = run_gpu(M, h, s.sub([]))
    assert m12.shape == (0, 64) and pt.shape == (0, 64) and num.shape == (0,)
    got = check(M, h, s.sub([[], [1]]))
    assert got[4][0] == 0 and (got[2][0] == -1).all() and got[5][0].tolist() == [0, 0]
    e = empty_member_scene()
    empty = e.kfs[1]
    from common_regions_scene import KF, Scene
    none = Scene("cur_0", KF(np.zeros(0), np.zeros((0, 32), np.uint8), {}), np.zeros(0, np.uint8), e.kfs, e.mp_bad, [[0, 2]], 0.9, False)
    m12, nm, pt, mem, num, most = run_gpu(M, h, none)
    assert m12.shape == (2, 0) and nm.tolist() == [0, 0] and num.tolist() == [0] and most.tolist() == [[0, 0]] and empty.n == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_scene(M, h, seeded, seed):
    """3 groups x 11 members of 300 features against the oracle and the union restatement; one group at or above 20 BoW matches, one below."""
    s, want = seeded[seed]
    assert (want[4] >= 20).any() and (want[4] < 20).any()
    check(M, h, s, want)
    flat = s.sub(s.groups)
    flat.ori = False
    check(M, h, flat)


def test_groups_of_1_2_and_11_with_a_shared_keyframe(M, h, seeded):
    s, _ = seeded[SEEDS[0]]
    mixed = mixed_groups(s)
    assert [len(g) for g in mixed.groups] == [1, 2, 11] and mixed.members.count(0) == 2
    got = check(M, h, mixed)
    assert np.array_equal(got[0][0], got[0][2]), "the shared key-frame's two member rows differ"


def test_every_pair_alone_equals_the_pair_inside_the_batch(M, h, seeded):
    """rumi_search_by_bow_kf on (current key-frame, member) against that member's row of the batch."""
    s, want = seeded[SEEDS[1]]
    got = run_gpu(M, h, s)
    v = views(M, s)
    for row, k in enumerate(s.members):
        n1, m1 = gpu_pair(M, h, s, k, v)
        assert n1 == got[1][row] and np.array_equal(m1, got[0][row]), (row, k)


def test_a_group_alone_equals_the_group_inside_the_batch(M, h, seeded):
    s, _ = seeded[SEEDS[0]]
    full = run_gpu(M, h, s)
    m = 0
    for g, grp in enumerate(s.groups):
        alone = run_gpu(M, h, s.sub([grp]))
        assert np.array_equal(alone[0], full[0][m:m + len(grp)]) and np.array_equal(alone[1], full[1][m:m + len(grp)])
        for a in (2, 3, 4, 5):
            assert np.array_equal(alone[a][0], full[a][g]), (g, a)
        m += len(grp)


def test_handle_reuse_and_buffer_growth(M, seeded):
    """Twice on a fresh handle, then a larger call, then the first again: the same results (grown buffers, cleared tables)."""
    h = M.ORBmatcher(0.9, True)
    small, big = cur_size_scene(65), seeded[SEEDS[0]][0]
    want_small = expected(O, small)
    first = check(M, h, small, want_small)
    assert same(check(M, h, small, want_small), first)
    check(M, h, big, seeded[SEEDS[0]][1])
    assert same(check(M, h, small, want_small), first)
    # a call that keeps its `taken` flags in LDS (513) between two calls that keep them in a register leaves the handle as it was
    check(M, h, node_size_scene(513))
    assert same(check(M, h, small, want_small), first)
    h.close()


def test_refusals_with_a_handle(h):
    from test_common_regions_cpu import check_refusals
    check_refusals(h)
