"""rumi_common_regions_bow without a GPU: the union restatement (common_regions_scene.union, LoopClosing.cc:635-651) against expectations written
down by hand; the hand-written scenes against the CPU oracle; what the seeded scenes must contain; the host-side refusals of the entry; the
facade test binary compiles."""
import numpy as np
import pytest

import oracle_lib as O
from common_regions_scene import (CONTENDED_NODE, NODE_SIZES, SEEDS, Scene, contended_scene, cur_size_scene, empty_member_scene, expect_tuple, expected, from_case, hand_cases, mixed_groups,
                                  most_matches, node_size_scene, same, describe, seeded_scene, union)
from match_cases import all_cases


# ---- the union restatement against hand-written expectations ----------------------------------------------------------------------------
def test_same_point_from_two_members_at_different_slots():
    """Point 7 at (0, 1) and again at (1, 3): the first counts, the second writes nothing."""
    pt, mem, num = union(4, [[-1, 7, -1, -1], [-1, -1, -1, 7]])
    assert pt.tolist() == [-1, 7, -1, -1] and mem.tolist() == [-1, 0, -1, -1] and num == 1


def test_two_new_points_at_one_slot_the_later_stands():
    """Points 7 (j = 0) and 9 (j = 2) both new at slot 1: the later one overwrites, the count keeps both."""
    pt, mem, num = union(3, [[-1, 7, -1], [-1, -1, -1], [-1, 9, -1]])
    assert pt.tolist() == [-1, 9, -1] and mem.tolist() == [-1, 2, -1] and num == 2


def test_point_seen_again_at_the_same_slot():
    """Point 7 at (0, 1) and at (2, 1): seen already, slot 1 keeps member 0."""
    pt, mem, num = union(3, [[-1, 7, -1], [5, -1, -1], [-1, 7, 6]])
    assert pt.tolist() == [5, 7, 6] and mem.tolist() == [1, 0, 2] and num == 3


def test_same_point_twice_in_one_member():
    """k ascending inside a member: the lower slot inserts the point."""
    pt, mem, num = union(3, [[-1, 4, 4]])
    assert pt.tolist() == [-1, 4, -1] and mem.tolist() == [-1, 0, -1] and num == 1


def test_an_overwritten_point_stays_seen():
    """Point 7 is overwritten at slot 0 by point 9 (j = 1); member 2 brings 7 again at slot 1: nothing is written, 7 is in no slot any more."""
    pt, mem, num = union(2, [[7, -1], [9, -1], [-1, 7]])
    assert pt.tolist() == [9, -1] and mem.tolist() == [1, -1] and num == 2


def test_tie_for_most_matches_goes_to_the_first():
    assert most_matches([3, 5, 5, 2]) == (1, 5)
    assert most_matches([0, 0]) == (0, 0) and most_matches([]) == (0, 0) and most_matches([0, 1]) == (1, 1)


def test_empty_group_and_member_without_matches():
    pt, mem, num = union(3, [])
    assert pt.tolist() == [-1] * 3 and mem.tolist() == [-1] * 3 and num == 0
    pt, mem, num = union(3, [[-1, -1, -1], [2, -1, -1]])
    assert pt.tolist() == [2, -1, -1] and mem.tolist() == [1, -1, -1] and num == 1


# ---- the scenes against the CPU oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0].name)
def test_hand_written_scenes_agree_with_the_oracle(case):
    scene, e = case
    got, want = expected(O, scene), expect_tuple(e)
    assert same(got, want), describe(got, want)


def test_match_cases_as_groups_of_one():
    cases = [c for c in all_cases() if c.member == "BOW_KF"]
    assert len(cases) >= 25
    for c in cases:
        m12, nm, pt, mem, num, most = expected(O, from_case(c))
        assert np.array_equal(m12[0], c.arr) and nm[0] == c.count, c.id
        assert np.array_equal(pt[0], c.arr) and num[0] == c.count and most.tolist() == [[0, c.count]], c.id       # member feature i holds point i


def test_node_size_scenes_match_where_they_should():
    for size in NODE_SIZES:
        s = node_size_scene(size)
        K = s.kfs[0]
        a = list(K.fv[0]).index(9)
        assert K.fv[1][a + 1] - K.fv[1][a] == size and K.n == size
        m12, nm, *_ = expected(O, s)
        assert m12[0][3] == -1
        if size >= 1:
            assert m12[0][0] == 0, size                                 # the twin at the LAST list position holds feature index 0
        if size >= 15:
            assert m12[0][1] == size - 1 and m12[0][2] == size - 1 - 5, size          # the tie goes to the earlier list entry; the NULL best is passed over


def test_contended_scene_contends():
    """In every 512-position stretch of the 1100-feature node the first of the two current features takes the stretch's last position and the
    second the stretch's first."""
    size, s = CONTENDED_NODE, contended_scene()
    K = s.kfs[0]
    a = list(K.fv[0]).index(9)
    assert K.n == size and K.fv[1][a + 1] - K.fv[1][a] == size
    m12, nm, *_ = expected(O, s)
    for i, s0 in enumerate(range(0, size, 512)):
        last = min(s0 + 511, size - 1)
        assert m12[0][2 * i] == size - 1 - last and m12[0][2 * i + 1] == size - 1 - s0, (size, s0)
    assert nm[0] == 2 * len(range(0, size, 512))


def test_size_scenes():
    for n in (1, 63, 64, 65):
        s = cur_size_scene(n)
        assert s.cur.n == n and expected(O, s)[4][0] >= 1
    s = empty_member_scene()
    assert [s.kfs[k].n for k in s.groups[0]] == [40, 0, 40]
    m12, nm, *_ = expected(O, s)
    assert nm[1] == 0 and nm[0] > 0 and nm[2] > 0


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_scenes_cannot_pass_empty(seed):
    s = seeded_scene(seed)
    assert len(s.groups) == 3 and all(len(g) == 11 for g in s.groups) and s.cur.n == 300 and all(k.n == 300 for k in s.kfs)
    assert len(s.kfs) < 33 and len(set(s.groups[0]) & set(s.groups[1])) >= 1                      # a key-frame serves two groups
    m12, nm, pt, mem, num, most = expected(O, s)
    assert (num >= 20).any() and (num < 20).any(), num
    assert num[0] > nm[:11].max(), "the union of group 0 should add points beyond its best member"
    # a point first seen at a later member overwrites an earlier point of the same slot somewhere: the count exceeds the filled slots
    assert num[0] > np.count_nonzero(pt[0] >= 0)
    assert (mem[0] > 0).any() and most[0][1] == nm[:11].max()
    # the histogram removed matches in some member
    s2 = Scene(s.name, s.cur, s.cur_good, s.kfs, s.mp_bad, s.groups, s.nnratio, False)
    assert expected(O, s2)[1].sum() > nm.sum()
    mixed = mixed_groups(s)
    assert [len(g) for g in mixed.groups] == [1, 2, 11] and mixed.members.count(0) == 2


# ---- host-side refusals ------------------------------------------------------------------------------------------------------------------
def refusals():
    """(name, keyword overrides of a well-formed call, a word of the message)."""
    return [("Cur NULL", dict(Cur=None), "NULL"), ("cur_fv NULL", dict(cur_fv=None), "NULL"), ("cur_good NULL", dict(cur_good=None), "NULL"),
            ("kfs NULL", dict(kfs=None), "NULL"), ("mp_bad NULL", dict(mp_bad=None), "NULL"), ("groups NULL", dict(groups=None), "NULL"),
            ("a member's mp NULL", dict(null_mp=True), "NULL"),
            ("group_start descends", dict(groups=([0, 2, 1], [0, 1])), "not ascending"),
            ("group_start does not begin at 0", dict(groups=([1, 2], [0, 1])), "begin at 0"),
            ("member index past the table", dict(groups=[[0, 2]]), "outside the key-frame table"),
            ("negative member index", dict(groups=[[-1]]), "outside the key-frame table"),
            ("map-point id == nmp", dict(mp_id=8), "not below nmp"),
            ("feature index past the key-frame", dict(fv_index=4), "malformed")]


def check_refusals(handle):
    """Shared with the GPU file.  Every refusal is RUMI_E_INVALID with its message, and no output byte changes."""
    from rumi_slam_amd import capi, matcher as M
    rng = np.random.default_rng(0)
    for name, over, word in refusals():
        keys = np.zeros(4, M.KP_DTYPE)
        desc = rng.integers(0, 256, (4, 32), dtype=np.uint8)
        F = M.FrameView(keys, desc, 640, 480, np.ones(8, np.float32))
        fv = M.FeatureVector({3: [0, 1], 5: [2, 3]})
        mp = np.array([0, 1, over.get("mp_id", 2), -1], np.int32)
        bad_fv = M.FeatureVector({3: [0, over["fv_index"]]}) if "fv_index" in over else fv
        kfs = [(F, fv, None if over.get("null_mp") else mp), (F, bad_fv, mp)]
        a = dict(Cur=F, cur_fv=fv, cur_good=np.ones(4, np.uint8), kfs=kfs, mp_bad=np.zeros(8, np.uint8), groups=[[0, 1]])
        a.update({k: v for k, v in over.items() if k in a})
        rc, *out = M.CommonRegionsBoW_status(handle, a["Cur"], a["cur_fv"], a["cur_good"], a["kfs"], a["mp_bad"], a["groups"], 0.9, True, fill=0x77777777)
        msg = capi.lib().rumi_last_error().decode()
        assert rc == capi.RUMI_E_INVALID and word in msg and "rumi_common_regions_bow" in msg, (name, rc, msg)
        for o in out:
            assert o.tobytes() == bytes([0x77]) * o.nbytes, name


def test_refused_before_any_device_work():
    """Without a matcher handle: a malformed call is refused for its own defect; a well-formed one gets as far as the handle."""
    from rumi_slam_amd import capi, matcher as M
    check_refusals(None)
    F = M.FrameView(np.zeros(4, M.KP_DTYPE), np.zeros((4, 32), np.uint8), 640, 480, np.ones(8, np.float32))
    fv = M.FeatureVector({3: [0, 1], 5: [2, 3]})
    rc, *out = M.CommonRegionsBoW_status(None, F, fv, np.ones(4, np.uint8), [(F, fv, np.arange(4, dtype=np.int32))], np.zeros(4, np.uint8), [[0]], 0.9, True,
                                         fill=0x77777777)
    assert rc == capi.RUMI_E_INVALID and "handle" in capi.lib().rumi_last_error().decode()
    assert all(o.tobytes() == bytes([0x77]) * o.nbytes for o in out)


def test_symbols_are_exported():
    from rumi_slam_amd import capi, matcher
    for name in ("rumi_common_regions_bow", "rumi_common_regions_bow_profile"):
        assert name in capi.MATCH_SYMBOLS and name in matcher.MATCH_SYMBOLS
        getattr(capi.lib(), name)


def test_common_regions_facade_compiles(tmp_path):
    from test_common_regions_facade_gpu import build_facade_test
    build_facade_test(str(tmp_path / "test_common_regions_facade"))
