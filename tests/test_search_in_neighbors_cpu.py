"""The argument rumi_search_in_neighbors_resident rests on (include/rumi_mapping.h), checked on the CPU with the oracle alone:
what the one-call entry answers from the map at the call is all the replay of LocalMapping::SearchInNeighbors ever asks for, with one
exception the model makes visible -- MapPoint::Replace ends with ComputeDistinctiveDescriptors (MapPoint.cc:321), so a point that survives a
Replace may be searched again on its new descriptor.  And the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import search_in_neighbors_scene as S
from rumi_slam_amd import capi

SEEDED = [(seed, 3 + seed % 4) for seed in range(200, 220)]


def run(m):
    fwd, rp, rb = S.expected_call(m)
    ref, nf, nr, searched = S.reference(m)
    return fwd, rp, rb, ref, nf, nr, searched


@pytest.mark.parametrize("seed,nt", S.CONSTRUCTED)
def test_constructed_scenes_take_every_branch(seed, nt):
    m = S.seeded_map(seed, nt)
    assert 3 <= m.n_targets <= 6 and all(64 <= kf.n <= 256 for kf in m.kfs)
    n = S.reference(m)[0].n
    assert n["add"] > 0, "an empty target feature gets an observation"
    assert n["replace_pmp"] > 0, "pMP->Replace(pMPinKF)"
    assert n["replace_inkf"] > 0, "pMPinKF->Replace(pMP)"
    assert n["skip_bad"] > 0, "a forward pair skipped because an earlier target made the point bad"
    assert n["skip_inkf_new"] > 0, "a forward pair skipped because an earlier Replace put the point into a later target"
    assert n["rev_skip_entered"] > 0, "a reverse candidate that entered a target row in the forward pass, skipped by IsInKeyFrame(cur)"
    assert n["rev_dup"] > 0, "a point in two targets' rows"
    assert n["dirty"] > 0, "a Replace that changed the survivor's descriptor"


@pytest.mark.parametrize("seed,nt", S.CONSTRUCTED + SEEDED)
def test_call_time_answers_cover_the_replay(seed, nt):
    m = S.seeded_map(seed, nt)
    fwd, rp, rb, ref, nf, nr, searched = run(m)
    # the superset claim: every reverse candidate the member searches stood in a target row at the call, not bad, not in the current key-frame
    assert set(searched) <= set(rp.tolist())
    assert len(set(rp.tolist())) == len(rp)
    # forward gates only close: a pair gated at the call is gated when its turn comes
    obs0 = m.observations()
    for t in range(m.n_targets):
        for p in m.kfs[0].row:
            if p >= 0 and (m.bad[p] or (1 + t) in obs0[p]):
                assert ref.bad[p] or (1 + t) in ref.obs[p]
    # the replay fed from the call-time answers leaves the member's map and counts
    res, nf2, nr2, missing = S.resident(m, fwd, rp, rb)
    assert missing == []
    assert (nf2, nr2) == (nf, nr) and nf + nr > 20
    assert res.state() == ref.state()


def test_a_changed_descriptor_changes_a_later_search():
    """Point 0 of the current key-frame fuses in target 1 with point 1, which has no more observers than it: point 1 is replaced, point 0
    gains target 1's observation and ComputeDistinctiveDescriptors picks the current key-frame's own descriptor, 60 bits from the one the point
    carried.  Only the new one is within TH_LOW of target 2's feature.  The member finds that match; the call-time answer alone does not."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    b = S.flip_bits(a, 60)
    pts = [S.point_at(200.0, 200.0, 2, a), S.point_at(200.0, 200.0, 2, S.flip_bits(a, 4))]
    feat = lambda d: ([[200.5, 200.0]], [2], [d])
    m = S.tiny_map(pts, [feat(S.flip_bits(a, 4)), feat(S.flip_bits(b, 2))], extra_rows=[[1], None])
    m.kfs[0].row[1] = -1                                          # point 1 lives in target 1 only
    m.kfs[0].desc[0] = b                                          # what the current key-frame sees of point 0
    fwd, rp, rb, ref, nf, nr, searched = run(m)
    assert fwd[0][0] == 0 and fwd[1][0] == -1
    assert ref.n["replace_inkf"] == 1 and 0 in ref.dirty and ref.obs[0].get(2) == 0, "the member fuses point 0 into target 2 as well"
    assert S.resident(m, fwd, rp, rb)[0].state() == ref.state()
    assert S.resident(m, fwd, rp, rb, research=False)[0].state() != ref.state()


# ---- refusals that need no device -------------------------------------------------------------------------------------------------------
class Refusal:
    """The C entry on a machine without a device, where no matcher handle can be created: every refusal below is decided on the host before
    the entry reads the handle (null arguments, counts, th, the records, then the slots against the store's mirror), so a pointer that is
    merely not NULL stands in for it."""

    def __init__(self):
        from rumi_slam_amd import mapping
        self.m = S.seeded_map(5, 3, n_extra=0, n_world=60, n_feat=64)
        self.sc = S.StoreScene(self.m)
        self.L = mapping._lib()
        self.mapping = mapping
        self.fake = C.create_string_buffer(8192)
        self.n_rev = C.c_int32(-5)
        self.fwd = np.full((8, 64), -9, np.int32)
        self.rp, self.rb = np.full(512, -9, np.int32), np.full(512, -9, np.int32)

    def call(self, slots=None, n=None, th=3.0, cur=True, matcher=True, store=True, targets=None, cur_slot=None):
        slots = np.asarray([S.slot_of(k) for k in (1, 2, 3)] if slots is None else slots, np.int32)
        n = len(slots) if n is None else n
        arr = (self.mapping.RumiFuseKF * max(len(slots), 1))(*[self.sc.fuse_kf(1)] * max(len(slots), 1)) if targets is None else targets
        c = self.sc.fuse_kf(0)
        rc = self.L.rumi_search_in_neighbors_resident(C.addressof(self.fake) if matcher else None, self.sc.store._h if store else None,
                                                      S.slot_of(0) if cur_slot is None else cur_slot, C.byref(c) if cur else None, capi.ptr(slots),
                                                      C.byref(arr), n, float(th), capi.ptr(self.fwd), capi.ptr(self.rp), capi.ptr(self.rb), 512,
                                                      C.byref(self.n_rev))
        return rc, capi.lib().rumi_last_error().decode()

    def untouched(self):
        return self.n_rev.value == -5 and (self.fwd == -9).all() and (self.rp == -9).all() and (self.rb == -9).all()


@pytest.fixture(scope="module")
def refusal():
    return Refusal()


@pytest.mark.parametrize("kw", [dict(matcher=False), dict(store=False), dict(cur=False)])
def test_refuses_null_arguments(refusal, kw):
    rc, msg = refusal.call(**kw)
    assert rc == capi.RUMI_E_INVALID and "rumi_search_in_neighbors_resident: missing argument" in msg and refusal.untouched()


def test_refuses_too_many_targets(refusal):
    slots = np.arange(641, dtype=np.int32)
    rc, msg = refusal.call(slots=slots)
    assert rc == capi.RUMI_E_CAPACITY and "RUMI_FUSE_MAX_TARGETS" in msg and refusal.untouched()


def test_refuses_a_slot_named_twice(refusal):
    rc, msg = refusal.call(slots=[S.slot_of(1), S.slot_of(2), S.slot_of(1)])
    assert rc == capi.RUMI_E_INVALID and "a slot named twice" in msg and refusal.untouched()


def test_refuses_the_current_key_frame_among_the_targets(refusal):
    rc, msg = refusal.call(slots=[S.slot_of(1), S.slot_of(0)])
    assert rc == capi.RUMI_E_INVALID and "a slot named twice (the current key-frame is not its own neighbour)" in msg and refusal.untouched()


@pytest.mark.parametrize("th", [0.0, -3.0, float("nan")])
def test_refuses_a_threshold_that_is_not_positive(refusal, th):
    rc, msg = refusal.call(th=th)
    assert rc == capi.RUMI_E_INVALID and "th must be positive" in msg and refusal.untouched()


def test_refuses_a_pose_that_is_not_finite(refusal):
    arr = (refusal.mapping.RumiFuseKF * 3)(*[refusal.sc.fuse_kf(k) for k in (1, 2, 3)])
    arr[1].Tcw7[5] = float("inf")
    rc, msg = refusal.call(targets=arr)
    assert rc == capi.RUMI_E_INVALID and "not finite" in msg and refusal.untouched()


def test_refuses_a_slot_that_is_not_live(refusal):
    rc, msg = refusal.call(slots=[S.slot_of(1), 3])
    assert rc == capi.RUMI_E_INVALID and "a slot that is not live or holds no features" in msg and refusal.untouched()


def test_row_length_is_the_stores(refusal):
    st = refusal.sc.store
    assert [st.row_length(S.slot_of(k)) for k in range(4)] == [64] * 4 and st.row_length(3) == -1 and st.row_length(-1) == -1
    from rumi_slam_amd.mapping import SearchInNeighborsResident

    class NoMatcher:
        _h = None
    with pytest.raises(ValueError, match="slot 3 is not live"):
        SearchInNeighborsResident(NoMatcher(), st, S.slot_of(0), refusal.sc.fuse_kf(0), [3], [refusal.sc.fuse_kf(1)])


def test_the_python_packer_is_the_c_record():
    from rumi_slam_amd.mapping import fuse_kf
    k = fuse_kf(np.arange(7), [7, 8, 9], [10, 11, 12, 13], 14)
    assert np.frombuffer(bytes(k), np.float32).tolist() == list(range(15))
