"""The argument rumi_search_and_fuse_resident rests on (include/rumi_mapping.h), checked on the CPU with the oracle alone: what
the one-call entry answers from the map at the call is all the replay of LoopClosing::SearchAndFuse ever asks for, with one exception the
model makes visible -- MapPoint::Replace ends with ComputeDistinctiveDescriptors on the surviving loop point (MapPoint.cc:321), so a loop point
that survived a Replace is searched again on its new descriptor for the key-frames that follow.

The seeds of search_and_fuse_scene.CONSTRUCTED were picked here, by scanning seeds 100-129 for maps on which the member takes every branch
below and on which at least one of them needs the second search; the GPU tests replay the same maps."""
import numpy as np
import pytest

import search_and_fuse_scene as F
import search_in_neighbors_scene as S

SEEDED = list(range(200, 212))


@pytest.fixture(scope="module")
def runs():
    out = {}
    for seed in F.CONSTRUCTED:
        m = F.seeded_map(seed)
        hits, per = F.expected_call(m)
        out[seed] = (m, hits, per, F.reference(m))
    return out


@pytest.mark.parametrize("seed", F.CONSTRUCTED)
def test_constructed_scenes_take_every_branch(runs, seed):
    m, hits, per, (ref, nf) = runs[seed]
    assert len(m.kfs) <= 8 and all(kf.n <= 160 for kf in m.kfs) and len(m.corrected) == 5
    assert all(float(m.sim3[k][2]) != 1.0 for k in m.corrected), "every corrected pose comes from a Sim3 with scale != 1"
    assert -1 in m.ids and len(set(m.ids)) < len(m.ids) and any(m.bad[p] for p in m.ids if p >= 0)
    n = ref.n
    assert n["add"] > 0, "an empty feature gets an observation"
    assert n["replace"] > n["self_replace"], "pRep->Replace(loop point) after the key-frame"
    assert n["occupant_added"] > 0, "GetMapPoint(bestIdx) returns a loop point added earlier in the same key-frame"
    assert n["skip_inkf_new"] > 0, "a loop point skipped because an earlier key-frame's Replace put it into this key-frame"
    assert n["loop_bad"] > 0, "a loop point that went bad during the member"
    assert n["dirty"] > 0, "a Replace that changed the surviving loop point's descriptor"
    assert len(hits) > 60 and (hits["occupant"] >= 0).any() and (hits["occupant"] < 0).any() and per.sum() == len(hits)


@pytest.mark.parametrize("seed", F.CONSTRUCTED)
def test_the_replay_of_the_call_time_answers_is_the_member(runs, seed):
    m, hits, per, (ref, nf) = runs[seed]
    res, nf2, again = F.resident(m, hits)
    assert again > 0, "second searches were made"
    assert nf2 == nf and nf > 60 and res.state() == ref.state()


def test_without_the_second_search_the_map_differs(runs):
    differs = [seed for seed in F.CONSTRUCTED if F.resident(runs[seed][0], runs[seed][1], research=False)[0].state() != runs[seed][3][0].state()]
    assert differs, "on at least one constructed seed the call-time answers alone do not give the member's map"


@pytest.mark.parametrize("seed", SEEDED)
def test_gates_only_close(seed):
    """A pair gated at the call (bad, or listed by the key-frame) is gated when its turn comes, so the device never has to answer it."""
    m = F.seeded_map(seed, n_corr=3 + seed % 3)
    hits, _ = F.expected_call(m)
    ref, nf = F.reference(m)
    s = F.FuseSim3Model(m)
    for k in m.corrected:
        at_call = F.call_skip(m, k)
        assert not (at_call & ~s.gate(k, m.ids)).any()
        s.fuse_kf(k, m.ids, F.search(m, k, m.ids, s.gate(k, m.ids), s.desc))
    assert s.state() == ref.state()
    res, nf2, _ = F.resident(m, hits)
    assert nf2 == nf and res.state() == ref.state()


def test_a_changed_descriptor_changes_a_later_search():
    """Loop point 0 carries descriptor a; the loop-side key-frame sees it as b, 60 bits away.  In corrected key-frame 1 it fuses with the
    feature that holds point 1, which is replaced; ComputeDistinctiveDescriptors over {b, a'} picks b (equal medians: the first).  Only b is
    within TH_LOW of key-frame 2's feature.  The member finds that match; the call-time answer alone does not."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    b = S.flip_bits(a, 60)
    pts = [S.point_at(200.0, 200.0, 2, a), S.point_at(200.0, 200.0, 2, S.flip_bits(a, 4))]
    feat = lambda xy, d: ([xy], [2], [d])
    m = F.tiny_map(pts, [feat([610.0, 20.0], b), feat([200.5, 200.0], S.flip_bits(a, 4)), feat([200.5, 200.0], S.flip_bits(b, 2))],
                   rows=[[0], [1], None], ids=[0])
    m.corrected = [1, 2]                                          # key-frame 0 is the loop side: it holds point 0 and is not searched
    hits, per = F.expected_call(m)
    assert hits.tolist() == [(0, 0, 0, 1)] and per.tolist() == [1, 0]
    ref, nf = F.reference(m)
    assert nf == 2 and ref.n["replace"] == 1 and 0 in ref.dirty and ref.obs[0] == {0: 0, 1: 0, 2: 0}
    res, nf2, again = F.resident(m, hits)
    assert (nf2, again) == (2, 1) and res.state() == ref.state()
    assert F.resident(m, hits, research=False)[0].state() != ref.state()


def test_an_occupant_added_in_the_same_key_frame_is_replaced_by_the_later_entry():
    """Two loop points project onto one empty feature: the first is added, the second finds it as the occupant (GetMapPoint is read live),
    and the Replace loop merges the FIRST into the second.  An id listed twice meets itself there, and Replace(self) returns at once."""
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    pts = [S.point_at(300.0, 200.0, 2, a), S.point_at(300.0, 200.0, 2, S.flip_bits(a, 1)), S.point_at(100.0, 100.0, 2, S.flip_bits(a, 90))]
    m = F.tiny_map(pts, [([[300.5, 200.0], [100.5, 100.0]], [2, 2], [a, S.flip_bits(a, 90)])], ids=[0, 1, 2, 2])
    hits, per = F.expected_call(m)
    assert hits.tolist() == [(0, 0, 0, -1), (0, 1, 0, -1), (0, 2, 1, -1), (0, 3, 1, -1)], "the occupant previews the row at the call"
    ref, nf = F.reference(m)
    assert nf == 4 and ref.n["add"] == 2 and ref.n["occupant_added"] == 2 and ref.n["self_replace"] == 1
    assert ref.bad.tolist() == [True, False, False] and ref.replaced == {0: 1} and ref.rows[0][:2] == [1, 2]
    assert F.resident(m, hits)[0].state() == ref.state()
