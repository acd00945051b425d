"""rumi_covis_set_point_observations and the argument checks of rumi_keyframe_culling_resident, without a device: every refusal leaves the
store as it was, and what the store keeps is observed through a resident call that gets as far as its missing handle."""
import numpy as np
import pytest

from rumi_slam_amd import capi
from rumi_slam_amd.covis import MAX_FEATURES, Covisibility
from rumi_slam_amd.mapping import cull_outputs, cull_resident_status

import culling_resident_scene as rs
from culling_scene import small_batch

_i32, _u8 = np.int32, np.uint8


def last_error():
    return capi.lib().rumi_last_error().decode()


def small_map():
    """The four key-frames and two points of culling_scene.small_batch."""
    octv = np.zeros(3, _i32)
    mp = [np.array([0, 1, -1], _i32), np.array([0, -1, 1], _i32), np.array([-1, 0, 1], _i32), np.array([0, -1, -1], _i32)]
    pts = [(False, 4, [(0, 0), (1, 0), (2, 1), (3, 0)]), (False, 3, [(0, 1), (1, 2), (2, 2)])]
    return rs.MapMirror([(octv, m, False, False, False, False) for m in mp], pts)


@pytest.fixture()
def store():
    m = small_map()
    s = Covisibility(8, 16, arena_entries=256)
    m.load(s)
    yield m, s
    s.close()


def raw_set(s, entry, n, ids, bad, off, obs, feat=None):
    p = lambda a: None if a is None else capi.ptr(a)
    if entry == "rumi_covis_set_points":
        return s._lib.rumi_covis_set_points(s._h, n, p(ids), p(bad), p(off), p(obs))
    return s._lib.rumi_covis_set_point_observations(s._h, n, p(ids), p(bad), p(off), p(obs), p(feat))


def a32(*v):
    return np.array(v, _i32)


# (name, n, ids, off, obs, feature, word of the message): the refusals the two entries share
SHARED = [
    ("id below 0", 1, a32(-1), a32(0, 1), a32(0), a32(0), "a point id outside"),
    ("id at max_points", 1, a32(16), a32(0, 1), a32(0), a32(0), "a point id outside"),
    ("id twice", 2, a32(3, 3), a32(0, 1, 2), a32(0, 1), a32(0, 0), "named twice"),
    ("negative offset", 1, a32(3), a32(-1, 1), a32(0, 0), a32(0, 0), "a negative offset"),
    ("slice backwards", 2, a32(3, 4), a32(2, 1, 2), a32(0, 1), a32(0, 0), "runs backwards"),
    ("slice longer than max_kf", 1, a32(3), a32(0, 9), a32(*range(9)), a32(*[0] * 9), "longer than max_kf"),
    ("observer not live", 1, a32(3), a32(0, 1), a32(5), a32(0), "not a live slot"),
    ("observer outside the slots", 1, a32(3), a32(0, 1), a32(8), a32(0), "not a live slot"),
    ("observer twice", 1, a32(3), a32(0, 2), a32(1, 1), a32(0, 1), "listed twice"),
]


@pytest.mark.parametrize("entry", ["rumi_covis_set_points", "rumi_covis_set_point_observations"])
def test_shared_refusals_leave_the_store_untouched(store, entry):
    m, s = store
    before = s.stats()
    bad = np.zeros(4, _u8)
    for name, n, ids, off, obs, feat, word in SHARED:
        rc = raw_set(s, entry, n, ids, bad, off, obs, feat)
        assert rc == capi.RUMI_E_INVALID and word in last_error() and last_error().startswith(entry + ":"), (name, rc, last_error())
        assert s.stats() == before, name
    for name, args in (("ids", (None, bad, a32(0, 1), a32(0), a32(0))), ("is_bad", (a32(3), None, a32(0, 1), a32(0), a32(0))),
                       ("obs_off", (a32(3), bad, None, a32(0), a32(0))), ("observers", (a32(3), bad, a32(0, 1), None, a32(0)))):
        rc = raw_set(s, entry, 1, *args)
        assert rc == capi.RUMI_E_INVALID and ("missing argument" in last_error() or "has no array" in last_error()), (name, last_error())
        assert s.stats() == before, name
    assert raw_set(s, entry, -1, a32(3), bad, a32(0, 1), a32(0), a32(0)) == capi.RUMI_E_INVALID and "negative count" in last_error()
    assert s.stats() == before
    assert s._lib.rumi_covis_set_points(None, 0, None, None, None, None) == capi.RUMI_E_INVALID
    assert s._lib.rumi_covis_set_point_observations(None, 0, None, None, None, None, None) == capi.RUMI_E_INVALID


def test_feature_range_and_missing_feature_array(store):
    m, s = store
    before = s.stats()
    bad = np.zeros(2, _u8)
    for f in (-1, MAX_FEATURES, 1 << 20):
        rc = raw_set(s, "obs", 1, a32(3), bad, a32(0, 2), a32(0, 1), a32(0, f))
        assert rc == capi.RUMI_E_INVALID and "a feature index outside" in last_error(), (f, last_error())
        assert s.stats() == before
    assert raw_set(s, "obs", 1, a32(3), bad, a32(0, 2), a32(0, 1), None) == capi.RUMI_E_INVALID and "has no array" in last_error()
    assert s.stats() == before
    assert raw_set(s, "obs", 1, a32(3), bad, a32(0, 2), a32(0, 1), a32(0, MAX_FEATURES - 1)) == capi.RUMI_OK     # the last index is inside
    assert raw_set(s, "obs", 1, a32(4), bad, a32(0, 0), None, None) == capi.RUMI_OK                             # no observers, no arrays
    assert raw_set(s, "obs", 0, None, None, None, None, None) == capi.RUMI_OK
    assert s.stats()["live"] > before["live"]


def resident(s, cands, flags=0, fill=0x77, store_handle=True):
    out = cull_outputs(len(cands), fill)
    rc = cull_resident_status(None, s if store_handle else None, cands, flags, out)
    assert all(a.tobytes() == bytes([fill]) * a.nbytes for a in out.values()), "a refused call writes nothing"
    return rc, last_error()


def test_a_point_set_without_features_loses_the_flag(store):
    """Observed without a device: the call is refused for the point that lacks the flag, and for want of a handle once nothing else is wrong."""
    m, s = store
    cands = m.candidates([2, 0, 1])
    rc, msg = resident(s, cands)
    assert rc == capi.RUMI_E_INVALID and "missing handle" in msg, msg
    s.set_points([1], [False], [[k for k, f in m.obs[1]]])
    rc, msg = resident(s, cands)
    assert rc == capi.RUMI_E_INVALID and "without observation features" in msg and " 3 " in msg, msg     # one slot in each of the three rows
    rc, msg = resident(s, m.candidates([3]))                         # key-frame 3 does not hold the point: not among what the loop reads
    assert "missing handle" in msg, msg
    s.set_bad(pt_ids=[0], pt_bad=[1])                                # the bad bit leaves the flag alone
    rc, msg = resident(s, m.candidates([3]))
    assert "missing handle" in msg, msg
    m.set_points(s, [1])
    rc, msg = resident(s, cands)
    assert rc == capi.RUMI_E_INVALID and "missing handle" in msg, msg
    fresh = Covisibility(8, 16)
    m.set_keyframes(fresh, range(m.n_kf))
    for k in range(m.n_kf):
        fr, fv = m.features(k)
        fresh.set_keyframe_features(k, fr, fv, [1.0, 1.0, 0.0, 0.0])
    rc, msg = resident(fresh, cands)                                 # points never set at all
    assert "without observation features" in msg, msg
    fresh.close()


def test_resident_refusals_without_a_device(store):
    m, s = store
    cands = m.candidates([2, 0, 1])
    rc, msg = resident(s, cands, store_handle=False)
    assert rc == capi.RUMI_E_INVALID and "missing argument" in msg
    for flags in (4, 8, -1, 1 << 16):
        rc, msg = resident(s, cands, flags=flags)
        assert rc == capi.RUMI_E_INVALID and "unknown flag" in msg, flags
    for slot in (-1, 4, 7, 8, 1 << 20):                              # 4..7: inside the store, never named; 8 and above: outside it
        rc, msg = resident(s, [(2, 0, 0, 0), (slot, 0, 0, 0)])
        assert rc == capi.RUMI_E_INVALID and "not live" in msg, (slot, msg)
    L = capi.lib()
    rec = np.zeros(1, [("slot", "<i4"), ("f", "u1", 4)])
    out = cull_outputs(1, 0x77)
    names = ["status", "n_mps", "n_redundant", "culled", "n_culled"]
    for missing in names + ["cand"]:
        args = [None if k == missing else capi.ptr(out[k]) for k in names]
        rc = L.rumi_keyframe_culling_resident(None, s._h, None if missing == "cand" else capi.ptr(rec), 1, 0, *args)
        assert rc == capi.RUMI_E_INVALID and "missing argument" in last_error(), missing
    assert L.rumi_keyframe_culling_resident(None, s._h, capi.ptr(rec), -1, 0, *[capi.ptr(out[k]) for k in names]) == capi.RUMI_E_INVALID
    assert all(a.tobytes() == bytes([0x77]) * a.nbytes for a in out.values())
    # a candidate that will be evaluated needs features, and as many as its row is long; a skipped one does not
    s.drop_keyframe_features([0])
    rc, msg = resident(s, cands)
    assert rc == capi.RUMI_E_INVALID and "holds no features" in msg, msg
    rc, msg = resident(s, [(2, 0, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0)])          # key-frame 0 is the initial one: skipped
    assert "missing handle" in msg, msg
    from rumi_slam_amd.matcher import FeatureVector, FrameView
    keys = np.zeros(4, capi.KP_DTYPE)
    s.set_keyframe_features(0, FrameView(keys, np.zeros((4, 32), _u8), 640, 480, np.ones(8, np.float32)), FeatureVector({}), [1.0, 1.0, 0.0, 0.0])
    rc, msg = resident(s, cands)
    assert rc == capi.RUMI_E_INVALID and "feature count differs" in msg, msg


def test_the_block_entry_agrees_on_the_small_map():
    """The mirror builds the batch culling_scene.small_batch builds."""
    a, b = small_map().batch([2, 0, 1]), small_batch()
    assert a.pts.tobytes() == b.pts.tobytes() and a.obs_kf.tobytes() == b.obs_kf.tobytes() and a.obs_feature.tobytes() == b.obs_feature.tobytes()
