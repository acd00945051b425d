"""rumi_common_regions_bow_resident on the GPU: every comparison is exact.  A pair is checked by the oracle's SearchByBoW(KF, KF), a group's union
by the restatement of LoopClosing.cc:635-651 in common_regions_scene, and every scene also by rumi_common_regions_bow on the same key-frames by
host pointers; constructed scenes carry their results written down by hand."""
import numpy as np
import pytest

import oracle_lib as O
from common_regions_scene import KF, Scene, cur_size_scene, describe, expect_tuple, from_case, hand_cases, run_gpu, same
from common_regions_resident_scene import (CUR_SLOT, RES_NODE_SIZES, WHOLE_MEMBER, contended_node_scene, expected_resident, new_store, run_resident,
                                           self_member_scene, slot_groups, slot_of, small_seeded, union_scene)
from match_cases import all_cases

pytestmark = pytest.mark.gpu

BOW_KF_CASES = [c for c in all_cases() if c.member == "BOW_KF"]
SEEDS = [21, 22]


@pytest.fixture(scope="module")
def M():
    from rumi_slam_amd import matcher
    return matcher


@pytest.fixture(scope="module")
def MP():
    from rumi_slam_amd import mapping
    return mapping


@pytest.fixture(scope="module")
def h(M):
    return M.ORBmatcher(0.9, True)


@pytest.fixture(scope="module")
def seeded():
    """seed -> (scene, the literal loop's results, a filled store), computed once."""
    out = {}
    for seed in SEEDS:
        s = small_seeded(seed)
        out[seed] = (s, expected_resident(O, s), new_store(s)[0])
    return out


def check(M, MP, h, scene, want=None, kf_bad=(), store=None):
    """By slot against the expectation, and against the host-pointer entry where no member is bad (that entry has no such notion)."""
    want = expected_resident(O, scene, kf_bad) if want is None else want
    cov = store if store is not None else new_store(scene, kf_bad)[0]
    got = run_resident(MP, h, cov, scene)
    assert same(got, want), scene.name + ": " + describe(got, want)
    if not kf_bad:
        by_pointer = run_gpu(M, h, scene)
        assert same(got, by_pointer), scene.name + " against rumi_common_regions_bow: " + describe(got, by_pointer)
    if store is None:
        cov.close()
    return got


@pytest.mark.parametrize("case", BOW_KF_CASES, ids=lambda c: c.id)
def test_constructed_pair_cases_as_a_group_of_one(M, MP, h, case):
    """Ties, best == second, bestDist1 of 49 and 50, the ratio on and off its boundary, two current features that want one member feature, the
    histograms, node sizes 63 .. 257: the expectation is the case's own, written down from the rule."""
    scene = from_case(case)
    m12, nm, pt, mem, num, most = check(M, MP, h, scene)
    assert np.array_equal(m12[0], case.arr) and nm[0] == case.count
    assert np.array_equal(pt[0], case.arr) and np.array_equal(mem[0], np.where(case.arr >= 0, 0, -1))           # member feature i holds point i
    assert num[0] == case.count and most.tolist() == [[0, case.count]]


@pytest.mark.parametrize("size", RES_NODE_SIZES + [WHOLE_MEMBER])
def test_member_node_sizes(M, MP, h, size):
    """0, 1, 15, 16, 17, 512 and 513 features in the member's node, and a node that holds a whole member of 1100 (three LDS words a lane); two
    current features contend for one member feature in every 512-position stretch.  No size leaves the device."""
    s = contended_node_scene(size)
    m12 = check(M, MP, h, s)[0]
    for i, s0 in enumerate(range(0, size, 512)):
        last = min(s0 + 511, size - 1)
        assert m12[0][2 * i] == size - 1 - last and m12[0][2 * i + 1] == (size - 1 - s0 if last != s0 else -1), (size, s0)


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0].name)
def test_hand_written_scenes(M, MP, h, case):
    """Both gates on both sides (a member feature without a point and one with a bad point that would have been best and second best; a
    current feature without a good point on a perfect twin); nodes on one side only; rotation bin 30 -> 0; a histogram that removes matches
    the union must then not see."""
    scene, e = case
    check(M, MP, h, scene, expect_tuple(e))


def test_current_side_gates_both_kinds(M, MP, h):
    """Not-good current features of both kinds -- a NULL row entry and a point whose bad bit is set -- on twins that would match."""
    s = cur_size_scene(65)
    s.cur_good[[3, 4, 10, 11, 40, 41]] = 0
    cov, sent = new_store(s)
    row = sent["rows"][CUR_SLOT]
    assert (row[[3, 10, 40]] == -1).all() and (row[[4, 11, 41]] >= 0).all() and sent["pt_bad"][row[[4, 11, 41]]].all()
    got = check(M, MP, h, s, store=cov)
    assert (got[0][:, [3, 4, 10, 11, 40, 41]] == -1).all() and got[1].sum() > 0
    cov.close()


def test_bad_bit_flipped_between_two_calls(M, MP, h):
    """case_gates: member feature 2 (point 1, 20 bits) matches.  Point 1 goes bad: feature 3 (point 2, 40 bits, alone among the good ones) matches
    instead.  Back: feature 2 again.  Then the current feature's own point goes bad: nothing matches.  The expectation is the oracle's on the
    edited scene each time."""
    scene, e = hand_cases()[0]
    assert scene.name == "gates"
    cov, sent = new_store(scene)
    first = check(M, MP, h, scene, expect_tuple(e), store=cov)
    cov.set_bad(pt_ids=[1], pt_bad=[1])
    edited = Scene(scene.name, scene.cur, scene.cur_good, scene.kfs, np.array([1, 1, 0], np.uint8), scene.groups, scene.nnratio, scene.ori)
    got = check(M, MP, h, edited, store=cov)
    assert got[0].tolist() == [[3]] and got[2].tolist() == [[2]]
    cov.set_bad(pt_ids=[1], pt_bad=[0])
    assert same(check(M, MP, h, scene, expect_tuple(e), store=cov), first)
    cov.set_bad(pt_ids=[int(sent["rows"][CUR_SLOT][0])], pt_bad=[1])
    none = Scene(scene.name, scene.cur, [0], scene.kfs, scene.mp_bad, scene.groups, scene.nnratio, scene.ori)
    got = check(M, MP, h, none, store=cov)
    assert got[0].tolist() == [[-1]] and got[1].tolist() == [0] and got[4].tolist() == [0]
    cov.close()


def test_member_row_replaced_between_two_calls(M, MP, h):
    """set_keyframes gives the member of case_gates another row: feature 2 loses its point, feature 0 (2 bits) gains point 2."""
    scene, e = hand_cases()[0]
    cov, sent = new_store(scene)
    check(M, MP, h, scene, expect_tuple(e), store=cov)
    K = scene.kfs[0]
    row = np.array([2, 0, -1, 2], np.int32)
    cov.set_keyframes([slot_of(0)], [9000 + 3 * slot_of(0)], [0], [0], [row], [[]], [-1], [[]])
    edited = Scene(scene.name, scene.cur, scene.cur_good, [KF(K.keys["angle"], K.desc, K.fv, row)], scene.mp_bad, scene.groups, scene.nnratio, scene.ori)
    got = check(M, MP, h, edited, store=cov)
    assert got[0].tolist() == [[0]] and got[2].tolist() == [[2]]
    cov.close()


def test_bad_member_in_the_middle_of_a_group(M, MP, h, seeded):
    """The union scene's three key-frames as one group with the middle one bad, then the first one: -1 row, -1 count, the later members keep
    their j; and a seeded group with its second member bad."""
    scene, _ = union_scene()
    mid = scene.sub([[0, 1, 2], [1]])
    got = check(M, MP, h, mid, kf_bad=[1])
    assert got[1].tolist() == [2, -1, 2, -1] and (got[0][1] == -1).all() and got[3].tolist() == [[2, 0, -1, -1], [-1] * 4] and got[5].tolist() == [[0, 2], [0, 0]]
    got = check(M, MP, h, mid, kf_bad=[0])
    assert got[3][0].tolist() == [2, 1, 1, -1] and got[5][0].tolist() == [1, 3]
    s, want, _ = seeded[SEEDS[0]]
    bad = s.groups[0][1]
    got = check(M, MP, h, s, kf_bad=[bad])
    assert got[1][1] == -1 and not same(got, want)


def test_union_cases(M, MP, h):
    """One point matched by two members at the same k and at different k; two first-seen points at one k; the same point in two groups; a
    key-frame shared by two groups; a tie in most_matches: written down by hand in union_scene."""
    scene, e = union_scene()
    check(M, MP, h, scene, expect_tuple(e))


def test_current_keyframe_as_a_member(M, MP, h):
    """cur_slot named among the members.  Alone in its group (the only member searched there) and behind another member: every good feature
    matches itself, as rumi_common_regions_bow answers for a copy of the key-frame.  Then a current key-frame of 1100 features in one node next
    to a 4-feature member: the `taken` words follow the current key-frame, the largest member of the call, and the gated copies past list
    position 511 stay gated."""
    s = self_member_scene()
    assert slot_groups(s) == [[CUR_SLOT], [slot_of(0), CUR_SLOT]]
    got = check(M, MP, h, s)
    assert got[1].tolist() == [4, 2, 4] and got[5].tolist() == [[0, 4], [1, 4]] and got[4].tolist() == [4, 6]
    big = self_member_scene(1100)
    assert slot_groups(big) == [[slot_of(0), CUR_SLOT], [CUR_SLOT]]
    got = check(M, MP, h, big)
    n_good = int(np.count_nonzero(big.cur_good))
    assert got[1].tolist() == [4, n_good, n_good] and np.array_equal(got[0][1], np.where(big.cur_good != 0, np.arange(1100), -1))


def test_stamps_of_an_earlier_call_do_not_reach_the_next(M, MP, seeded):
    """Two calls on one handle: the first stamps every point of the second with other (j, k) -- the groups in another order, the members
    reversed, and once with far larger keys from a seeded scene sharing the point ids.  The second result equals a fresh handle's."""
    scene, e = union_scene()
    cov = new_store(scene)[0]
    used, fresh = M.ORBmatcher(0.9, True), M.ORBmatcher(0.9, True)
    other = scene.sub([[0, 2, 1], [1, 0]])
    first = run_resident(MP, used, cov, other)
    assert same(first, expected_resident(O, other))
    second = run_resident(MP, used, cov, scene)
    assert same(second, run_resident(MP, fresh, cov, scene)) and same(second, expect_tuple(e))
    big, want_big, cov_big = seeded[SEEDS[1]]
    assert same(run_resident(MP, used, cov_big, big), want_big)             # points 0 .. 3 stamped with keys of another n, more groups
    assert same(run_resident(MP, used, cov, scene), second)
    assert same(run_resident(MP, used, cov, other), first)
    used.close(); fresh.close(); cov.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_scene(M, MP, h, seeded, seed):
    """3 groups x 4 members of 200 features against the oracle, the union restatement and the host-pointer entry; with and without the
    rotation histogram."""
    s, want, cov = seeded[seed]
    check(M, MP, h, s, want, store=cov)
    flat = s.sub(s.groups)
    flat.ori = False
    check(M, MP, h, flat, store=cov)


def test_every_pair_alone_equals_the_pair_inside_the_batch(MP, h, seeded):
    s, want, cov = seeded[SEEDS[1]]
    got = run_resident(MP, h, cov, s)
    for row, k in enumerate(s.members):
        alone = run_resident(MP, h, cov, s, [[k]])
        assert alone[1][0] == got[1][row] and np.array_equal(alone[0][0], got[0][row]), (row, k)


def test_a_group_alone_equals_the_group_inside_the_batch(MP, h, seeded):
    s, _, cov = seeded[SEEDS[0]]
    full = run_resident(MP, h, cov, s)
    m = 0
    for g, grp in enumerate(s.groups):
        alone = run_resident(MP, h, cov, s, [grp])
        assert np.array_equal(alone[0], full[0][m:m + len(grp)]) and np.array_equal(alone[1], full[1][m:m + len(grp)])
        for a in (2, 3, 4, 5):
            assert np.array_equal(alone[a][0], full[a][g]), (g, a)
        m += len(grp)


def test_null_matches12_leaves_the_other_five_unchanged(MP, h, seeded):
    s, want, cov = seeded[SEEDS[0]]
    got = run_resident(MP, h, cov, s, want_matches12=False)
    assert got[0] is None and same(got[1:], want[1:])
    ms = MP.common_regions_bow_resident_stage_ms(h)
    assert ms.shape == (3,) and (ms >= 0).all() and ms[1] > 0


def test_empty_inputs(M, MP, h):
    """An empty group beside a full one; no groups; a current key-frame without features (with a bad member: its count is still -1)."""
    s = cur_size_scene(64)
    cov = new_store(s)[0]
    got = check(M, MP, h, s.sub([[], [1]]), store=cov)
    assert got[4][0] == 0 and (got[2][0] == -1).all() and got[5][0].tolist() == [0, 0]
    m12, nm, pt, mem, num, most = run_resident(MP, h, cov, s, [])
    assert m12.shape == (0, 64) and pt.shape == (0, 64) and num.shape == (0,) and most.shape == (0, 2)
    m12, nm, pt, mem, num, most = run_resident(MP, h, cov, s, [[]])
    assert m12.shape == (0, 64) and (pt == -1).all() and num.tolist() == [0] and most.tolist() == [[0, 0]]
    cov.close()
    none = Scene("cur_0", KF(np.zeros(0), np.zeros((0, 32), np.uint8), {}), np.zeros(0, np.uint8), s.kfs, s.mp_bad, [[0, 1]], 0.9, False)
    cov = new_store(none, kf_bad=[1])[0]
    m12, nm, pt, mem, num, most = run_resident(MP, h, cov, none)
    assert m12.shape == (2, 0) and nm.tolist() == [0, -1] and num.tolist() == [0] and most.tolist() == [[0, 0]]
    cov.close()


def test_handle_reuse_and_buffer_growth(M, MP, seeded):
    """Twice on a fresh handle, then a larger call on a larger store, then the first again: the same results (grown buffers, a grown table)."""
    hh = M.ORBmatcher(0.9, True)
    small = cur_size_scene(65)
    cov = new_store(small)[0]
    first = check(M, MP, hh, small, store=cov)
    assert same(check(M, MP, hh, small, store=cov), first)
    big, want, cov_big = seeded[SEEDS[0]]
    check(M, MP, hh, big, want, store=cov_big)
    assert same(check(M, MP, hh, small, store=cov), first)
    hh.close(); cov.close()


def test_refusals_with_a_handle(h):
    """Each writes nothing: the outputs are pre-filled with a pattern."""
    from test_common_regions_resident_cpu import check_refusals
    check_refusals(h)
