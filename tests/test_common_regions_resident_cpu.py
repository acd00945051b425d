"""rumi_common_regions_bow_resident without a GPU: the symbols and their mirror; what fill_store puts into a store, checked on host arrays; the
constructed scenes against the CPU oracle; every refusal that needs no device; the facade test binary compiles."""
import numpy as np
import pytest

import oracle_lib as O
from common_regions_scene import describe, expect_tuple, hand_cases, same
from common_regions_resident_scene import (CUR_SLOT, RES_NODE_SIZES, WHOLE_MEMBER, contended_node_scene, cur_row, expected_resident, new_store, slot_of,
                                           small_seeded, union_scene)

PATTERN = 0x77777777


def test_symbols_are_exported_and_mirrored():
    from rumi_slam_amd import capi, mapping
    for name in ("rumi_common_regions_bow_resident", "rumi_common_regions_bow_resident_stage_ms"):
        assert name in capi.MAPPING_SYMBOLS
        getattr(capi.lib(), name)
    for name in ("CommonRegionsBoWResident", "CommonRegionsBoWResident_status", "common_regions_bow_resident_stage_ms"):
        assert callable(getattr(mapping, name))


@pytest.mark.parametrize("case", hand_cases() + [union_scene()], ids=lambda c: c[0].name)
def test_fill_store_reproduces_the_scene(case):
    """Read back from the store (its host mirror, staged edits included): the current row's gate equals cur_good; a good feature's point is
    held by no member; every member's row is the scene's mp and its points' bad bits are the scene's mp_bad; the key-frame bad bits; the
    store holds features for every slot."""
    scene, _ = case
    cov, _ = new_store(scene, kf_bad=[0])
    nmp = len(scene.mp_bad)
    row, bad, kf_bad = cov.read_row(CUR_SLOT)
    assert len(row) == scene.cur.n and kf_bad == 0
    assert np.array_equal((row >= 0) & (bad == 0), scene.cur_good != 0)
    assert (row[row >= 0] >= nmp).all() and len(set(row[row >= 0].tolist())) == np.count_nonzero(row >= 0)
    assert np.array_equal(row, cur_row(scene)[0])
    for k, K in enumerate(scene.kfs):
        row, bad, kf_bad = cov.read_row(slot_of(k))
        assert np.array_equal(row, K.mp) and kf_bad == (1 if k == 0 else 0)
        assert np.array_equal(bad, np.where(K.mp >= 0, scene.mp_bad[np.maximum(K.mp, 0)], 0))
    assert cov.feature_stats()["slots"] == len(scene.kfs) + 1
    cov.close()


def test_not_good_features_alternate_between_null_and_a_bad_point():
    from common_regions_scene import cur_size_scene
    s = cur_size_scene(8)
    s.cur_good[[1, 2, 5, 6]] = 0
    row, ids, bad = cur_row(s)
    nmp = len(s.mp_bad)
    assert row.tolist() == [nmp, -1, nmp + 2, nmp + 3, nmp + 4, -1, nmp + 6, nmp + 7]
    assert dict(zip(ids.tolist(), bad.tolist())) == {nmp: 0, nmp + 2: 1, nmp + 3: 0, nmp + 4: 0, nmp + 6: 1, nmp + 7: 0}


def test_constructed_scenes_agree_with_the_oracle():
    scene, e = union_scene()
    got, want = expected_resident(O, scene), expect_tuple(e)
    assert same(got, want), describe(got, want)
    # a bad member in the middle: -1 row, -1 count, the later member keeps j = 2
    mid = scene.sub([[0, 1, 2]])
    m12, nm, pt, mem, num, most = expected_resident(O, mid, kf_bad=[1])
    assert nm.tolist() == [2, -1, 2] and (m12[1] == -1).all() and pt.tolist() == [[3, 1, -1, -1]] and mem.tolist() == [[2, 0, -1, -1]]
    assert num.tolist() == [3] and most.tolist() == [[0, 2]]
    mid2 = expected_resident(O, mid, kf_bad=[0])
    assert mid2[3].tolist() == [[2, 1, 1, -1]] and mid2[5].tolist() == [[1, 3]]


@pytest.mark.parametrize("size", RES_NODE_SIZES + [WHOLE_MEMBER])
def test_contended_nodes_contend(size):
    """In every 512-position stretch the first of the two current features takes the stretch's last position (feature size - 1 - last) and the
    second the stretch's first, or nothing in a stretch of one."""
    s = contended_node_scene(size)
    K = s.kfs[0]
    assert K.n == size and K.fv[1][list(K.fv[0]).index(9) + 1] - K.fv[1][list(K.fv[0]).index(9)] == size
    m12, nm, *_ = expected_resident(O, s)
    for i, s0 in enumerate(range(0, size, 512)):
        last = min(s0 + 511, size - 1)
        assert m12[0][2 * i] == size - 1 - last, (size, s0)
        assert m12[0][2 * i + 1] == (size - 1 - s0 if last != s0 else -1), (size, s0)
    assert m12[0][-1] == -1 and nm[0] == np.count_nonzero(m12[0] >= 0)


def test_small_seeded_scene_is_within_the_size_limit_and_not_empty():
    s = small_seeded(21)
    assert len(s.groups) == 3 and all(len(g) == 4 for g in s.groups) and s.cur.n <= 300 and all(K.n <= 300 for K in s.kfs)
    assert len(set(s.groups[0]) & set(s.groups[1])) == 1
    m12, nm, pt, mem, num, most = expected_resident(O, s)
    assert num[0] > nm[:4].max() and (mem[0] > 0).any() and num[0] >= 20


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
NO_FEATURES, SHORT_ROW, DEAD = 4, 5, 6            # slots beside the union scene's 0 .. 3


def refusal_store():
    """The union scene plus a live slot without features, a live slot whose row is one shorter than its features, and a slot never set."""
    from rumi_slam_amd import matcher as M
    from match_cases import SF
    scene, _ = union_scene()
    cov, sent = new_store(scene, spare_kf=3)
    K = scene.kfs[1]
    cov.set_keyframes([NO_FEATURES, SHORT_ROW], [801, 802], [0, 0], [0, 0], [K.mp, K.mp[:-1]], [[]] * 2, [-1] * 2, [[]] * 2)
    fr, fv = M.FrameView(K.keys, K.desc, 640, 480, SF), M.FeatureVector.from_csr(*K.fv)
    cov.set_keyframe_features(SHORT_ROW, fr, fv, [500.0, 500.0, 320.0, 240.0])
    sent["keep"].append((fr, fv))
    return cov, sent


def refusals():
    """(name, keyword overrides of a well-formed call, a word of the message)."""
    return [("store NULL", dict(store=None), "store is NULL"), ("group_start NULL", dict(groups=None), "group_start is NULL"),
            ("member_slot NULL", dict(groups=([0, 2], None)), "member_slot is NULL"),
            ("nmatches NULL", dict(null_out=1), "output array is NULL"), ("matched_point NULL", dict(null_out=2), "output array is NULL"),
            ("matched_member NULL", dict(null_out=3), "output array is NULL"), ("num_bow_matches NULL", dict(null_out=4), "output array is NULL"),
            ("most_matches NULL", dict(null_out=5), "output array is NULL"),
            ("group_start descends", dict(groups=([0, 2, 1], [1, 2])), "not ascending"),
            ("group_start does not begin at 0", dict(groups=([1, 2], [1, 2])), "begin at 0"),
            ("member slot past the store", dict(groups=[[1, 99]]), "not live"), ("negative member slot", dict(groups=[[-1]]), "not live"),
            ("member slot never set", dict(groups=[[1, DEAD]]), "not live"),
            ("current slot never set", dict(cur_slot=DEAD), "not live"), ("current slot past the store", dict(cur_slot=99), "not live"),
            ("member without features", dict(groups=[[1], [NO_FEATURES]]), "holds no features"),
            ("current slot without features", dict(cur_slot=NO_FEATURES), "holds no features"),
            ("member whose row does not fit its features", dict(groups=[[SHORT_ROW, 1]]), "differs from the length")]


def check_refusals(handle):
    """Shared with the GPU file.  Every refusal is RUMI_E_INVALID with its message, and no output byte changes."""
    from rumi_slam_amd import capi, mapping as MP
    cov, sent = refusal_store()
    for name, over, word in refusals():
        a = dict(store=cov, cur_slot=CUR_SLOT, groups=[[1, 2], [3, 1]], null_out=None)
        a.update(over)
        rc, *out = MP.CommonRegionsBoWResident_status(handle, a["store"], a["cur_slot"], a["groups"], 0.9, True, fill=PATTERN, n=4, null_out=a["null_out"])
        msg = capi.lib().rumi_last_error().decode()
        assert rc == capi.RUMI_E_INVALID and word in msg and "rumi_common_regions_bow_resident" in msg, (name, rc, msg)
        for o in out:
            assert o.tobytes() == bytes([0x77]) * o.nbytes, name
    cov.close()


def test_refused_before_any_device_work():
    """Without a matcher handle: a malformed call is refused for its own defect; a well-formed one gets as far as the handle."""
    from rumi_slam_amd import capi, mapping as MP
    check_refusals(None)
    cov, sent = refusal_store()
    rc, *out = MP.CommonRegionsBoWResident_status(None, cov, CUR_SLOT, [[1, 2], [3, 1]], 0.9, True, fill=PATTERN)
    assert rc == capi.RUMI_E_INVALID and "handle" in capi.lib().rumi_last_error().decode()
    assert all(o.tobytes() == bytes([0x77]) * o.nbytes for o in out)
    cov.close()


def test_a_union_key_that_does_not_fit_is_refused():
    """j * n + k: 65535 members in one group and a current key-frame of 32800 features pass 2^31 - 1."""
    from rumi_slam_amd import capi, mapping as MP, matcher as M
    from rumi_slam_amd.covis import Covisibility
    from match_cases import KP_DTYPE, SF
    n = 32800
    cov = Covisibility(2, 8)
    cov.set_keyframes([0, 1], [1, 2], [0, 0], [0, 0], [[-1] * n, [-1] * 4], [[]] * 2, [-1] * 2, [[]] * 2)
    big = (M.FrameView(np.zeros(n, KP_DTYPE), np.zeros((n, 32), np.uint8), 640, 480, SF), M.FeatureVector({}))
    small = (M.FrameView(np.zeros(4, KP_DTYPE), np.zeros((4, 32), np.uint8), 640, 480, SF), M.FeatureVector({3: [0, 1]}))
    cov.set_keyframe_features(0, *big, [1.0, 1.0, 0.0, 0.0]); cov.set_keyframe_features(1, *small, [1.0, 1.0, 0.0, 0.0])
    L = MP._lib()
    start, member = np.array([0, 65535], np.int32), np.ones(65535, np.int32)
    out = [np.full(4, PATTERN, np.int32) for _ in range(5)]
    rc = L.rumi_common_regions_bow_resident(None, cov._h, 0, 1, capi.ptr(start), capi.ptr(member), 0.9, 1, None, *[capi.ptr(o) for o in out])
    assert rc == capi.RUMI_E_INVALID and "key range" in capi.lib().rumi_last_error().decode()
    assert all((o == PATTERN).all() for o in out)
    start[1] = 65000                                                 # 65000 x 32800 fits: the call gets as far as the handle
    rc = L.rumi_common_regions_bow_resident(None, cov._h, 0, 1, capi.ptr(start), capi.ptr(member), 0.9, 1, None, *[capi.ptr(o) for o in out])
    assert rc == capi.RUMI_E_INVALID and "handle" in capi.lib().rumi_last_error().decode()
    cov.close()


def test_stage_ms_needs_a_call():
    from rumi_slam_amd import capi, mapping as MP
    out = np.zeros(3, np.float32)
    assert MP._lib().rumi_common_regions_bow_resident_stage_ms(None, capi.ptr(out)) == capi.RUMI_E_INVALID


def test_common_regions_resident_facade_compiles(tmp_path):
    from test_common_regions_resident_facade_gpu import build_facade_test
    build_facade_test(str(tmp_path / "test_common_regions_resident_facade"))
