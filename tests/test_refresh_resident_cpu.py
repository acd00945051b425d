"""The two store edits behind rumi_refresh_map_points_resident (rumi_covis_set_keyframe_centres, rumi_covis_set_point_reference), the
read-back hook on the host mirror, and every refusal the resident entry decides on the host -- none of which needs a device.

What a refused edit leaves behind is observed through rumi_covis_stats and the mirror hook here; that a refused edit does not change what the
kernels read, and the upload bytes of an accepted one (an upload needs a device), are in tests/test_refresh_resident_gpu.py."""
import numpy as np
import pytest

from rumi_slam_amd import capi
from rumi_slam_amd.covis import Covisibility
from rumi_slam_amd.mapping import (REFRESH_DESCRIPTOR, REFRESH_MAX_OBS, REFRESH_NORMAL_DEPTH, REFRESH_WRITE_BACK, MapPointRefresher,
                                   refresh_resident_outputs)

import refresh_resident_scene as rr

_i32, _f32 = np.int32, np.float32
BOTH = REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH
FILL = 0xC3


def last_error():
    return capi.lib().rumi_last_error().decode()


def tiny_map():
    """Four key-frames of three features (slot 3 bad), three points: two observed, one without observers."""
    rng = np.random.default_rng(9)
    kfs = [(rng.integers(0, 256, (3, 32), dtype=np.uint8), rr.SF, rng.uniform(-4, 4, 3), k == 3) for k in range(4)]
    octs = [np.array([0, 3, 7], _i32)] * 4
    pts = [((0.5, 0.1, 6.0), 1, [(2, 0), (0, 1), (1, 2), (3, 0)]), ((1.0, -0.3, 5.0), 0, [(0, 0), (1, 1)]), ((0.0, 0.0, 4.0), -1, [])]
    return rr.ResidentMap(kfs, octs, pts)


@pytest.fixture()
def loaded():
    m = tiny_map()
    s = Covisibility(8, 16, arena_entries=256)       # slots 4..7 are not live
    m.load(s)
    r = MapPointRefresher()
    yield m, s, r
    r.close()
    s.close()


def p(a):
    return None if a is None else capi.ptr(a)


def test_centre_refusals_leave_the_store_untouched(loaded):
    m, s, _ = loaded
    before, attrs = s.stats(), s.read_attributes([0, 1, 2]).copy()
    L = s._lib
    ok = np.zeros((2, 3), _f32)
    cases = [("slot not live", 1, np.array([5], _i32), ok, "not live"), ("slot below 0", 1, np.array([-1], _i32), ok, "not live"),
             ("slot at max_kf", 1, np.array([8], _i32), ok, "not live"), ("slot twice", 2, np.array([1, 1], _i32), ok, "named twice"),
             ("NaN", 2, np.array([0, 1], _i32), np.array([[0, 0, 0], [0, np.nan, 0]], _f32), "not finite"),
             ("infinity", 1, np.array([0], _i32), np.array([[-np.inf, 0, 0]], _f32), "not finite"),
             ("negative count", -1, np.array([0], _i32), ok, "negative count"), ("no slots", 1, None, ok, "missing argument"),
             ("no centres", 1, np.array([0], _i32), None, "missing argument")]
    for name, n, slots, Ow, word in cases:
        rc = L.rumi_covis_set_keyframe_centres(s._h, n, p(slots), p(Ow))
        assert rc == capi.RUMI_E_INVALID and word in last_error() and last_error().startswith("rumi_covis_set_keyframe_centres:"), (name, last_error())
        assert s.stats() == before and s.read_attributes([0, 1, 2]).tobytes() == attrs.tobytes(), name
    assert L.rumi_covis_set_keyframe_centres(None, 0, None, None) == capi.RUMI_E_INVALID
    assert L.rumi_covis_set_keyframe_centres(s._h, 0, None, None) == capi.RUMI_OK
    assert s.set_keyframe_centres([3, 0], np.ones((2, 3)), check=False) == capi.RUMI_OK        # a bad slot has a pose too
    assert s.stats() == before                                                                 # staged: the edit itself uploads nothing


def test_reference_refusals_and_clear(loaded):
    m, s, _ = loaded
    before = s.stats()
    L = s._lib
    cases = [("id below 0", 1, [-1], [0], "a point id outside"), ("id at max_points", 1, [16], [0], "a point id outside"),
             ("id twice", 2, [1, 1], [0, 1], "named twice"), ("reference not live", 1, [1], [6], "neither -1 nor a live slot"),
             ("reference below -1", 1, [1], [-2], "neither -1 nor a live slot"), ("reference at max_kf", 1, [1], [8], "neither -1 nor a live slot"),
             ("negative count", -1, [1], [0], "negative count")]
    for name, n, ids, ref, word in cases:
        rc = L.rumi_covis_set_point_reference(s._h, n, p(np.array(ids, _i32)), p(np.array(ref, _i32)))
        assert rc == capi.RUMI_E_INVALID and word in last_error() and last_error().startswith("rumi_covis_set_point_reference:"), (name, last_error())
        assert s.stats() == before, name
    for ids, ref in ((None, np.zeros(1, _i32)), (np.zeros(1, _i32), None)):
        assert L.rumi_covis_set_point_reference(s._h, 1, p(ids), p(ref)) == capi.RUMI_E_INVALID and "missing argument" in last_error()
    assert L.rumi_covis_set_point_reference(None, 0, None, None) == capi.RUMI_E_INVALID
    assert s.set_point_reference([0, 1, 15], [3, -1, -1], check=False) == capi.RUMI_OK         # a bad slot may be the reference; -1 clears
    assert s.stats() == before


def test_read_back_hook_on_the_mirror():
    m = tiny_map()
    s = Covisibility(8, 16, arena_entries=256)
    m.set_keyframes(s, range(4))
    m.set_points(s, range(3), attributes=False)
    rc, _ = s.read_attributes([0], check=False)
    assert rc == capi.RUMI_E_INVALID and "no attribute table" in last_error()
    a = m.initial_attributes([2, 0])
    s.set_point_attributes([2, 0], a["pos"], a["normal"], a["min_dist"], a["max_dist"], a["desc"])
    got = s.read_attributes([0, 2, 1])
    want = m.expected_records([2, 0], None, what_desc=False, what_normal=False)
    assert got[0].tobytes() == want[1].tobytes() and got[1].tobytes() == want[0].tobytes()
    assert got[2].tobytes() == bytes(64)                                                       # never set: the table's zeros
    assert got[0, :12].view(_f32).tolist() == [0.5, np.float32(0.1), 6.0]
    for ids in ([-1], [16]):
        rc, _ = s.read_attributes(ids, check=False)
        assert rc == capi.RUMI_E_INVALID and "outside 0..max_points-1" in last_error()
    rc, _ = s.read_attributes([0], from_device=True, check=False)                              # nothing was uploaded, and the hook uploads nothing
    assert rc == capi.RUMI_E_INVALID and "no attribute table" in last_error()
    s.close()


def untouched(out):
    return all(v.tobytes() == bytes([FILL]) * v.nbytes for v in out.values())


def call(r, s, ids, what, flags, out, drop=()):
    a = {k: (None if k in drop else capi.ptr(v)) for k, v in out.items()}
    ids = None if ids is None else np.ascontiguousarray(ids, _i32)
    n = 0 if ids is None else len(ids)
    return r._lib.rumi_refresh_map_points_resident(r._h, s._h if s is not None else None, p(ids), n, what, flags, a["best_obs"], a["best_median"],
                                                   a["desc"], a["normal"], a["min_distance"], a["max_distance"], a["updated"])


def test_resident_host_refusals(loaded):
    m, s, r = loaded
    before, attrs = s.stats(), s.read_attributes([0, 1, 2]).copy()
    out = refresh_resident_outputs(3, FILL)

    def refused(name, rc, word, code=capi.RUMI_E_INVALID):
        assert rc == code and word in last_error() and last_error().startswith("rumi_refresh_map_points_resident:"), (name, rc, last_error())
        assert untouched(out) and s.stats() == before and s.read_attributes([0, 1, 2]).tobytes() == attrs.tobytes(), name

    L = r._lib
    o = [capi.ptr(out[k]) for k in ("best_obs", "best_median", "desc", "normal", "min_distance", "max_distance", "updated")]
    ids = np.array([0, 1, 2], _i32)
    refused("no handle", L.rumi_refresh_map_points_resident(None, s._h, p(ids), 3, BOTH, 0, *o), "missing argument")
    refused("no store", call(r, None, ids, BOTH, 0, out), "missing argument")
    refused("negative count", L.rumi_refresh_map_points_resident(r._h, s._h, p(ids), -1, BOTH, 0, *o), "negative count")
    refused("no ids", L.rumi_refresh_map_points_resident(r._h, s._h, None, 3, BOTH, 0, *o), "missing argument")
    for what, names in ((REFRESH_DESCRIPTOR, ("best_obs", "best_median", "desc")), (REFRESH_NORMAL_DEPTH, ("normal", "min_distance", "max_distance", "updated"))):
        for k in names:
            refused(f"no {k}", call(r, s, ids, what, 0, out, drop=(k,)), "missing argument")
    refused("no mode", call(r, s, ids, 0, 0, out), "without a known mode bit")
    refused("unknown what bit", call(r, s, ids, BOTH | 4, 0, out), "without a known mode bit")
    refused("unknown flag", call(r, s, ids, BOTH, 2, out), "unknown flag")
    refused("unknown flag beside the known one", call(r, s, ids, BOTH, REFRESH_WRITE_BACK | 8, out), "unknown flag")
    refused("id below 0", call(r, s, [0, -1], BOTH, 0, out), "a point id outside")
    refused("id at max_points", call(r, s, [16], BOTH, 0, out), "a point id outside")
    refused("id twice", call(r, s, [1, 0, 1], BOTH, 0, out), "named twice")
    # arrays of a mode not asked for may be NULL: the call passes validation (and stops at the missing device where there is none)
    assert call(r, s, [2], REFRESH_DESCRIPTOR, 0, out, drop=("normal", "min_distance", "max_distance", "updated")) in (capi.RUMI_OK, capi.RUMI_E_NO_DEVICE)


def test_resident_refusals_from_the_mirror():
    m = tiny_map()
    r = MapPointRefresher()
    out = refresh_resident_outputs(3, FILL)
    # observers without observation features
    s = Covisibility(8, 16, arena_entries=256)
    m.load(s)
    s.set_points([1], [0], [[0, 1]])                                                           # rumi_covis_set_points drops the feature indices
    for what in (REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH, BOTH):
        assert call(r, s, [0, 1, 2], what, 0, out) == capi.RUMI_E_INVALID and "1 points have observers but no observation features" in last_error()
        assert untouched(out)
    s.close()
    # no attributes: refused in normal mode and for the write-back, not for a descriptor query
    s = Covisibility(8, 16, arena_entries=256)
    m.set_keyframes(s, range(4)); m.set_features(s, range(4)); m.set_centres(s, range(4))
    m.set_points(s, range(3), attributes=False)
    a = m.initial_attributes([0])
    s.set_point_attributes([0], a["pos"], a["normal"], a["min_dist"], a["max_dist"], a["desc"])
    for what, flags in ((REFRESH_NORMAL_DEPTH, 0), (BOTH, 0), (REFRESH_DESCRIPTOR, REFRESH_WRITE_BACK), (BOTH, REFRESH_WRITE_BACK)):
        assert call(r, s, [0, 1, 2], what, flags, out) == capi.RUMI_E_INVALID and "2 points have no attributes" in last_error(), (what, flags)
        assert untouched(out)
    s.close()
    # the handle and the store on different devices: known without asking either device
    s = Covisibility(8, 16, arena_entries=256, device=1)
    m.load(s)
    r0 = MapPointRefresher(device=0)
    assert call(r0, s, [0, 1], BOTH, 0, out) == capi.RUMI_E_INVALID and "different devices" in last_error()
    assert untouched(out)
    r0.close(); s.close(); r.close()


def test_empty_call_is_ok(loaded):
    m, s, r = loaded
    out = refresh_resident_outputs(1, FILL)
    for what in (REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH, BOTH):
        for flags in (0, REFRESH_WRITE_BACK):
            assert r._lib.rumi_refresh_map_points_resident(r._h, s._h, None, 0, what, flags, *[None] * 7) == capi.RUMI_OK
            assert call(r, s, np.zeros(0, _i32), what, flags, out) == capi.RUMI_OK and untouched(out)


def test_capacity_from_the_mirror():
    """A row of 2049 observers is refused from the mirror: the store holds no features, so nothing could have been launched."""
    n = REFRESH_MAX_OBS + 1
    s = Covisibility(n, 4, arena_entries=8192)
    s.set_keyframes(list(range(n)), list(range(1, n + 1)), [0] * n, [0] * n, [[-1]] * n, [[]] * n, [-1] * n, [[]] * n)
    s.set_point_observations([0, 1], [0, 0], [[(k, 0) for k in range(n)], [(k, 0) for k in range(3)]])
    s.set_point_attributes([0, 1], np.zeros((2, 3)), np.zeros((2, 3)), np.zeros(2), np.zeros(2), np.zeros((2, 32), np.uint8))
    r = MapPointRefresher()
    out = refresh_resident_outputs(2, FILL)
    before, attrs = s.stats(), s.read_attributes([0, 1]).copy()
    for what in (REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH, BOTH):
        for flags in (0, REFRESH_WRITE_BACK):
            assert call(r, s, [1, 0], what, flags, out) == capi.RUMI_E_CAPACITY and "RUMI_REFRESH_MAX_OBS" in last_error()
            assert untouched(out) and s.stats() == before and s.read_attributes([0, 1]).tobytes() == attrs.tobytes()
    r.close(); s.close()
