"""rumi_create_new_map_points_resident (include/rumi_mapping.h): CreateNewMapPoints over key-frames that live in the covisibility store
(features by rumi_covis_set_keyframe_features, map-point rows and point positions as the store keeps them), against the block entry
rumi_create_new_map_points on the same matcher and against the C++ oracle (tests/cpp/newpoints_oracle.cc).  Both entries instantiate the same
kernels, so the contract is bytes: neighbour, idx1, idx2, counts, skip flags equal and the x3D bits identical."""
import ctypes as C

import numpy as np
import pytest

from newpoints_scene import RATIO_FACTOR, SCENES, TH_FAR, NewPointsScene, build_oracle, params, run_oracle
from resident_scene import ResidentScene, slot_of, view_pose

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("newpoints_resident"))


def matcher(ori, **kw):
    from rumi_slam_amd.matcher import ORBmatcher
    return ORBmatcher(0.6, bool(ori), **kw)


def block_call(m, cur, neigh, coarse, far, **kw):
    from rumi_slam_amd.mapping import CreateNewMapPoints
    return CreateNewMapPoints(m, cur, neigh, RATIO_FACTOR, bool(coarse), bool(far), TH_FAR, **kw)


def assert_oracle(got, want):
    pts, per, skipped = got
    assert np.array_equal(skipped, want["skipped"])
    assert np.array_equal(per, want["per_neigh"])
    assert pts.tobytes() == want["points"].tobytes()


def assert_bytes(a, b):
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


# ---- 1. parity ----
@pytest.mark.parametrize("seed,nn,nf,coarse,ori,far", SCENES)
def test_parity(oracle, seed, nn, nf, coarse, ori, far):
    s = NewPointsScene(seed, nn, nf)
    want = run_oracle(oracle, s.cur, s.neigh, params(coarse, ori, far, TH_FAR))
    assert len(want["points"]) > 40
    m = matcher(ori)
    rs = ResidentScene(s)
    block = block_call(m, s.cur, s.neigh, coarse, far)
    got = rs.call(m, coarse, far)
    assert_bytes(got, block)
    assert_oracle(got, want)
    m.close()


# ---- 2. the tiling paths of the new instantiations ----
def test_nodes_of_more_than_64_features(oracle):
    s = NewPointsScene(60, 7, 1000, levelsup=2)
    assert np.diff(s.cur.fv.offsets).min() > 64
    rs = ResidentScene(s)
    for coarse, ori in ((0, 1), (1, 0)):
        want = run_oracle(oracle, s.cur, s.neigh, params(coarse, ori, 0, TH_FAR))
        assert len(want["points"]) > 100
        m = matcher(ori)
        assert_oracle(rs.call(m, coarse, 0), want)
        m.close()


def test_more_than_2048_features(oracle):
    s = NewPointsScene(61, 7, 2600)
    assert s.cur.frame.n > 2048 and all(nb.frame.n > 2048 for nb in s.neigh)
    want = run_oracle(oracle, s.cur, s.neigh, params(0, 1, 1, TH_FAR))
    assert want["skipped"][3] == 1 and len(want["points"]) > 300
    m = matcher(1)
    assert_oracle(ResidentScene(s).call(m, 0, 1), want)
    m.close()


# ---- 3. arena growth under live data ----
def test_arena_grows_device_to_device(oracle):
    s = NewPointsScene(2, 7, 500)
    prm = params(0, 1, 0, TH_FAR)
    rs = ResidentScene(s, reserve=64 << 10, sync=False)
    m = matcher(1)
    for k in (0, 1, 2):
        rs.sync(k)
    assert_oracle(rs.call(m, neigh=[1, 2]), run_oracle(oracle, s.cur, s.neigh[:2], prm))     # three key-frames are on the device now
    first = rs.store.feature_stats()
    assert first["last_upload_bytes"] == first["used"] > 64 << 10 and first["growths"] >= 1
    for k in range(3, 8):                                                                    # one by one; the arena has to grow again
        rs.sync(k)
    st = rs.store.feature_stats()
    assert st["growths"] > first["growths"] and st["capacity"] > first["capacity"] and st["slots"] == 8
    want = run_oracle(oracle, s.cur, s.neigh, prm)
    got = rs.call(m)
    assert_oracle(got, want)
    assert rs.store.feature_stats()["last_upload_bytes"] == st["used"] - first["used"]        # only the five new key-frames travelled
    again = rs.call(m)
    assert rs.store.feature_stats()["last_upload_bytes"] == 0
    assert_bytes(again, got)
    m.close()


# ---- 4. edits reach the call ----
def test_edits_reach_the_call(oracle):
    s = NewPointsScene(2, 7, 500)
    prm = params(0, 1, 0, TH_FAR)
    rs = ResidentScene(s)
    m = matcher(1)
    got = rs.call(m)
    assert_oracle(got, run_oracle(oracle, s.cur, s.neigh, prm))
    # a point (with attributes) on a feature of the current key-frame that created one
    f = int(got[0]["idx1"][len(got[0]) // 2])
    assert rs.rows[0][f] < 0
    pid = rs.next_id
    rs.next_id += 1
    row = rs.rows[0].copy()
    row[f] = pid
    cs = slot_of(0)
    rs.store.set_keyframes([cs], [1000 + 7 * cs], [0], [0], [row], [[]], [-1], [[]])
    rs.store.set_points([pid], [0], [[cs]])
    rs.set_positions(np.int32([pid]), np.float32([[0, 0, 8]]))
    kf_mp = s.cur.kf_mp.copy()
    kf_mp[f] = 1
    cur2 = rs.edited_view(0, kf_mp=kf_mp)
    got2 = rs.call(m)
    assert_oracle(got2, run_oracle(oracle, cur2, s.neigh, prm))
    assert f not in got2[0]["idx1"] and len(got2[0]) < len(got[0])
    # every point of one neighbour 1000 x further from its camera: the baseline test now skips it
    k = int(np.nonzero((got2[2] == 0) & (got2[1] > 0))[0][0])
    v = s.neigh[k]
    have = np.nonzero(v.kf_mp >= 0)[0]
    far = (v.Ow + np.float32(1000) * (v.mp_pos[have] - v.Ow)).astype(np.float32)
    rs.set_positions(rs.rows[1 + k][have], far)
    mp_pos = v.mp_pos.copy()
    mp_pos[have] = far
    neigh2 = list(s.neigh)
    neigh2[k] = rs.edited_view(1 + k, mp_pos=mp_pos)
    want3 = run_oracle(oracle, cur2, neigh2, prm)
    got3 = rs.call(m)
    assert want3["skipped"][k] == 1 and got3[2][k] == 1 and got3[1][k] == 0
    assert_oracle(got3, want3)
    m.close()


# ---- 5. replace and drop ----
def test_replace_and_drop(oracle):
    from rumi_slam_amd import capi
    s = NewPointsScene(2, 7, 500)
    other = NewPointsScene(12, 2, 650)
    prm = params(0, 1, 0, TH_FAR)
    rs = ResidentScene(s)
    m = matcher(1)
    rs.call(m)
    new = other.neigh[1]
    assert new.frame.n != s.neigh[2].frame.n
    rs.views[3] = new
    rs.set_row(3, new)
    rs.sync(3)
    neigh2 = list(s.neigh)
    neigh2[2] = new
    want = run_oracle(oracle, s.cur, neigh2, prm)
    got = rs.call(m)
    assert_oracle(got, want)
    assert_bytes(got, block_call(m, s.cur, neigh2, 0, 0))
    assert rs.store.feature_stats()["slots"] == 8
    rs.store.drop_keyframe_features([slot_of(3)])
    with pytest.raises(capi.RumiError) as e:
        rs.call(m)
    assert e.value.code == capi.RUMI_E_INVALID and "holds no features" in str(e.value)
    assert_oracle(rs.call(m, neigh=[1, 2]), run_oracle(oracle, s.cur, s.neigh[:2], prm))      # the others are still there
    m.close()


# ---- 6. further refusals ----
FILL = 0xAB


def raw_call(m, rs, neigh, cap=500, cur=0):
    """(status, out, per, skipped, n_out): the C entry with every output pre-filled."""
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import NEWPOINT_DTYPE, _lib, pack_poses
    L = _lib()
    out = np.frombuffer(bytes([FILL]) * (500 * NEWPOINT_DTYPE.itemsize), NEWPOINT_DTYPE).copy()
    per = np.frombuffer(bytes([FILL]) * 64 * 4, np.int32).copy()
    sk = np.full(64, FILL, np.uint8)
    n_out = C.c_int32(-77)
    slots = np.int32([slot_of(k) for k in neigh])
    cp, arr = pack_poses(view_pose(rs.views[cur]), [view_pose(rs.views[k]) for k in neigh])
    prm = params(0, 1, 0, TH_FAR)
    rc = L.rumi_create_new_map_points_resident(m._h, rs.store._h, slot_of(cur), C.byref(cp), capi.ptr(slots) if len(neigh) else None,
                                               C.byref(arr) if len(neigh) else None, len(neigh), C.byref(prm), capi.ptr(out), cap, C.byref(n_out),
                                               capi.ptr(per), capi.ptr(sk))
    return rc, out, per, sk, n_out.value, capi.lib().rumi_last_error().decode()


def untouched(r):
    _, out, per, sk, n_out, _ = r
    return n_out == -77 and (out.view(np.uint8) == FILL).all() and (per.view(np.uint8) == FILL).all() and (sk == FILL).all()


def test_refusals(oracle):
    from rumi_slam_amd import capi
    s = NewPointsScene(2, 7, 500)
    rs = ResidentScene(s)
    m = matcher(1)
    want = run_oracle(oracle, s.cur, s.neigh, params(0, 1, 0, TH_FAR))
    everyone = list(range(1, 8))
    good = raw_call(m, rs, everyone)
    assert good[0] == capi.RUMI_OK and good[4] == len(want["points"]) and good[1][:good[4]].tobytes() == want["points"].tobytes()
    for neigh in ([1, 2, 3, 2], [1, 0, 2]):                                       # a slot twice; cur_slot among the neighbours
        r = raw_call(m, rs, neigh)
        assert r[0] == capi.RUMI_E_INVALID and "twice" in r[5] and untouched(r)
    r = raw_call(m, rs, everyone, cap=10)                                          # the prefix and RUMI_E_CAPACITY, as the block entry does
    assert r[0] == capi.RUMI_E_CAPACITY and r[4] == len(want["points"]) and r[1][:10].tobytes() == want["points"][:10].tobytes()
    assert (r[1][10:].view(np.uint8) == FILL).all() and np.array_equal(r[2][:7], want["per_neigh"]) and np.array_equal(r[3][:7], want["skipped"])
    r = raw_call(m, rs, [])                                                        # no neighbours: RUMI_OK, nothing created
    assert r[0] == capi.RUMI_OK and r[4] == 0 and (r[1].view(np.uint8) == FILL).all()
    small = matcher(1, max_features=256, max_queries=4096)
    r = raw_call(small, rs, everyone)
    assert r[0] == capi.RUMI_E_CAPACITY and untouched(r)
    small.close()
    # a neighbour's point without attributes: found by k_newpts_gather, the message carries the count
    row = rs.rows[4].copy()
    f = int(np.nonzero(row < 0)[0][3])
    row[f] = rs.next_id
    ns = slot_of(4)
    rs.store.set_keyframes([ns], [1000 + 7 * ns], [0], [0], [row], [[]], [-1], [[]])
    rs.store.set_points([rs.next_id], [0], [[ns]])
    r = raw_call(m, rs, everyone)
    assert r[0] == capi.RUMI_E_INVALID and ": 1 neighbour map point(s) without attributes" in r[5] and untouched(r)
    rs.set_positions(np.int32([rs.next_id]), s.neigh[3].mp_pos[f:f + 1])           # with attributes the call goes through again
    assert raw_call(m, rs, everyone)[0] == capi.RUMI_OK
    # a row that is shorter than the key-frame has features
    rs.store.set_keyframes([ns], [1000 + 7 * ns], [0], [0], [row[:-1]], [[]], [-1], [[]])
    r = raw_call(m, rs, everyone)
    assert r[0] == capi.RUMI_E_INVALID and "differs from the length" in r[5] and untouched(r)
    assert raw_call(m, rs, [1, 2, 3])[0] == capi.RUMI_OK
    # a slot that is not live
    rs.views.append(rs.views[1])
    r = raw_call(m, rs, [1, 8])
    assert r[0] == capi.RUMI_E_INVALID and "not live" in r[5] and untouched(r)
    m.close()


def test_empty_neighbour_is_skipped(oracle):
    s = NewPointsScene(31, 7, 500, empty_neigh=(1,))
    m = matcher(0)
    want = run_oracle(oracle, s.cur, s.neigh, params(0, 0, 0, TH_FAR))
    got = ResidentScene(s).call(m)
    assert got[2][1] == 1 and got[1][1] == 0
    assert_oracle(got, want)
    m.close()


# ---- 7. reuse of freed space ----
def test_freed_space_is_reused(oracle):
    s = NewPointsScene(2, 7, 500)
    rs = ResidentScene(s, reserve=512 << 10)
    m = matcher(1)
    want = run_oracle(oracle, s.cur, s.neigh, params(0, 1, 0, TH_FAR))
    assert_oracle(rs.call(m), want)
    before = rs.store.feature_stats()
    rs.store.drop_keyframe_features([slot_of(3)])
    assert rs.store.feature_stats()["used"] < before["used"]
    rs.sync(3)
    after = rs.store.feature_stats()
    assert after["capacity"] == before["capacity"] and after["growths"] == before["growths"] and after["used"] == before["used"]
    assert_oracle(rs.call(m), want)
    assert 0 < rs.store.feature_stats()["last_upload_bytes"] < before["used"] // 4          # one key-frame travelled
    m.close()


# ---- 8. stability and independence ----
def test_stable_and_independent_of_the_block_entry(oracle):
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import last_matches
    s = NewPointsScene(3, 30, 2000)
    other = NewPointsScene(4, 7, 1000)
    rs = ResidentScene(s)
    m = matcher(1)
    a = rs.call(m, 0, 1)
    b = rs.call(m, 0, 1)
    blk = block_call(m, other.cur, other.neigh, 1, 0)
    c = rs.call(m, 0, 1)
    assert len(a[0]) > 500
    assert_bytes(a, b)
    assert_bytes(a, c)
    assert_bytes(blk, block_call(m, other.cur, other.neigh, 1, 0))
    last_matches(m, 7, other.cur.frame.n)                                          # the hook replays a block call ...
    rs.call(m, 0, 1)
    with pytest.raises(capi.RumiError) as e:                                       # ... and refuses after a resident one
        last_matches(m, 30, s.cur.frame.n)
    assert e.value.code == capi.RUMI_E_INVALID
    m.close()


# ---- the validator is the block entry's ----
@pytest.mark.parametrize("what", ["index", "twice", "nodes", "octave", "offsets"])
def test_both_entries_refuse_with_the_same_message(what):
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import _lib, pack
    s = NewPointsScene(5, 1, 500)
    rs = ResidentScene(s, sync=False)
    v = s.neigh[0]
    if what == "index":
        v.fv.indices[5] = 100000
    elif what == "twice":
        v.fv.indices[5] = v.fv.indices[6]
    elif what == "nodes":
        v.fv.node_ids[[2, 3]] = v.fv.node_ids[[3, 2]]
    elif what == "offsets":
        v.fv.offsets[3] = v.fv.offsets[2] - 1
    else:
        v.frame.keys["octave"][7] = 8
    assert rs.sync(1, check=False) == capi.RUMI_E_INVALID
    mine = capi.lib().rumi_last_error().decode()
    assert rs.store.feature_stats()["slots"] == 0
    m = matcher(0)
    c, arr = pack(s.cur, s.neigh)
    prm = params(0, 0, 0, TH_FAR)
    out = np.zeros(500, np.dtype([("a", "<i4", 3), ("b", "<f4", 3)]))
    per, sk, n = np.zeros(64, np.int32), np.zeros(64, np.uint8), C.c_int32()
    rc = _lib().rumi_create_new_map_points(m._h, C.byref(c), C.byref(arr), 1, C.byref(prm), capi.ptr(out), 500, C.byref(n), capi.ptr(per), capi.ptr(sk))
    assert rc == capi.RUMI_E_INVALID and capi.lib().rumi_last_error().decode() == mine and mine.startswith("key-frame features:")
    m.close()
