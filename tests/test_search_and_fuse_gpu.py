"""rumi_search_and_fuse_resident (include/rumi_mapping.h): every (corrected key-frame, loop point) search of LoopClosing::SearchAndFuse in one
device call on key-frames and points resident in the covisibility store.  The contract is bytes: the CPU oracle's answer per pair
(oracle_lib.fuse_candidates without the reprojection gate, through tests/search_and_fuse_scene.py) and rumi_fuse_candidates(check_reprojection
= 0) on the same key-frame, pose and points.  The hand-made cases put one property each on the edge where the kernels can go wrong."""
import numpy as np
import pytest

import search_and_fuse_scene as F
import search_in_neighbors_scene as S
from rumi_slam_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    from rumi_slam_amd.matcher import ORBmatcher
    m = ORBmatcher(0.8, True, max_features=2048, max_queries=32768)
    yield m
    m.close()


def check(matcher, m, sc=None):
    """The call against the oracle and, per key-frame, against the single-key-frame entry; returns (scene, hits, per_kf)."""
    sc = F.StoreScene(m) if sc is None else sc
    want_hits, want_per = F.expected_call(m)
    hits, per = sc.call(matcher)
    assert hits.dtype == F.HIT_DTYPE and per.dtype == np.int32
    assert per.tobytes() == want_per.tobytes(), (per.tolist(), want_per.tolist())
    assert hits.tobytes() == want_hits.tobytes(), (len(hits), len(want_hits))
    dense = np.full((len(m.corrected), len(m.ids)), -1, np.int32)
    dense[hits["kf"], hits["point"]] = hits["feature"]
    for kk, k in enumerate(m.corrected):
        one = sc.single(matcher, k, m.ids, F.call_skip(m, k))
        assert dense[kk].tobytes() == one.tobytes(), ("key-frame", kk)
    return sc, hits, per


# ---- 1. whole maps ----
@pytest.mark.parametrize("seed", F.CONSTRUCTED)
def test_parity(matcher, seed):
    m = F.seeded_map(seed)
    sc, hits, per = check(matcher, m)
    assert len(hits) > 60 and (hits["occupant"] >= 0).any() and (hits["occupant"] < 0).any()
    again, per2 = sc.call(matcher)
    assert again.tobytes() == hits.tobytes() and per2.tobytes() == per.tobytes(), "two calls, the same bytes"
    ref, nf = F.reference(m)
    res, nf2, searched_again = F.resident(m, hits)
    assert nf2 == nf and searched_again > 0 and res.state() == ref.state(), "the replay a caller makes of these hits leaves the member's map"


def test_feature_counts_that_are_no_multiple_of_64(matcher):
    m = F.seeded_map(41, n_corr=3, n_world=80, n_feat=97)
    assert all(kf.n == 97 for kf in m.kfs)
    _, hits, per = check(matcher, m)
    assert len(hits) > 30 and (per > 0).all()


# ---- 2. hand-made edges of the gate and the search ----
RNG = np.random.default_rng(78)
D = [RNG.integers(0, 256, 32, dtype=np.uint8) for _ in range(16)]


def one_kf(matcher, points, feats, **kw):
    """The best feature per list entry for one key-frame with the identity pose."""
    m = F.tiny_map(points, [feats], **kw)
    _, hits, per = check(matcher, m)
    out = [-1] * len(m.ids)
    for h in hits:
        out[h["point"]] = int(h["feature"])
    return out


def test_no_reprojection_gate(matcher):
    """A key-point inside the radius whose reprojection error the 5.99 gate of Fuse(pKF, vpMapPoints) rejects (2.45^2 = 6.00 at level 0) is
    found: ORBmatcher.cc:1258-1274 has no such gate.  The same pair through the gated search finds nothing."""
    pts = [S.point_at(300.0, 100.0, 1, D[7])]
    feats = ([[302.45, 100.0]], [0], [D[7]])
    assert float(np.float32(np.float32(300.0) - np.float32(302.45)) ** 2) > 5.99 and 2.45 < F.TH * float(S.SF[1])
    assert one_kf(matcher, pts, feats) == [0]
    sc = F.StoreScene(F.tiny_map(pts, [feats]))
    assert sc.single(matcher, 0, [0], [False], reproj=True).tolist() == [-1]


def test_depth_must_not_be_negative(matcher):
    """p3Dc(2) < 0 is dropped; the mirrored point projects to the same pixel and passes the distance and angle gates."""
    front, behind = S.point_at(200.0, 150.0, 2, D[0]), S.point_at(400.0, 150.0, 2, D[1], z=-1.0)
    u, v = S.pixel_of(behind["pos"])
    assert abs(float(u) - 400.0) < 0.01 and abs(float(v) - 150.0) < 0.01 and behind["pos"][2] < 0
    feats = ([[200.5, 150.0], [400.5, 150.0]], [2, 2], [D[0], D[1]])
    assert one_kf(matcher, [front, behind], feats) == [0, -1]


def test_image_bounds(matcher):
    """KeyFrame::IsInImage is x >= mnMinX && x < mnMaxX: a projection exactly on the minimum is inside, one exactly on the maximum is not."""
    pts = [S.point_at(0.0, 240.0, 2, D[0]), S.point_at(640.0, 100.0, 4, D[1]), S.point_at(639.0, 300.0, 4, D[2]), S.point_at(320.0, 0.0, 2, D[3]),
           S.point_at(100.0, 480.0, 4, D[4])]
    px = [S.pixel_of(p["pos"]) for p in pts]
    assert px[0][0] == 0.0 and px[1][0] == 640.0 and px[3][1] == 0.0 and px[4][1] == 480.0, "the float projection lands on the bound exactly"
    feats = ([[1.0, 240.0], [634.99, 100.0], [634.99, 300.0], [320.0, 1.0], [100.0, 474.99]], [2, 4, 4, 2, 4], [D[0], D[1], D[2], D[3], D[4]])
    assert one_kf(matcher, pts, feats) == [0, -1, 2, 3, -1]


def test_distance_range(matcher):
    """dist3D against 0.8 * min and 1.2 * max (GetMin/MaxDistanceInvariance), a part in a thousand on either side of each."""
    def at(u, v, lo, hi, d):
        p = S.point_at(u, v, 2, d)
        dist = np.sqrt((p["pos"][0] * p["pos"][0] + p["pos"][1] * p["pos"][1]) + p["pos"][2] * p["pos"][2], dtype=np.float32)
        if lo is not None:
            p["min_dist"] = float(dist) / 0.8 * lo
        if hi is not None:
            p["max_dist"], p["min_dist"] = float(dist) / 1.2 * hi, 0.01
        return p, dist
    cases = [at(100.0, 100.0, 0.999, None, D[0]), at(200.0, 100.0, 1.001, None, D[1]), at(300.0, 100.0, None, 1.001, D[2]), at(400.0, 100.0, None, 0.999, D[3])]
    inside = [not (dist < np.float32(0.8) * np.float32(p["min_dist"]) or dist > np.float32(1.2) * np.float32(p["max_dist"])) for p, dist in cases]
    assert inside == [True, False, True, False]
    # max_dist / dist < 1 predicts level 0 for the last two
    feats = ([[100.5, 100.0], [200.5, 100.0], [300.5, 100.0], [400.5, 100.0]], [2, 2, 0, 0], [D[0], D[1], D[2], D[3]])
    assert one_kf(matcher, [p for p, _ in cases], feats) == [0, -1, 2, -1]


def test_viewing_angle_on_its_boundary(matcher):
    """PO.dot(Pn) < 0.5 * dist3D drops the point.  Both points lie on the optical axis at a power of two, so dot = z * Pn.z and dist = z are
    exact: cos = 0.5 is not below the bound, the float just under 0.5 is."""
    def on_axis(z, c, d):
        p = S.point_at(320.0, 240.0, 2, d, z=z)
        assert p["pos"].tolist() == [0.0, 0.0, z]
        p["normal"] = np.float32([np.sqrt(1.0 - float(c) ** 2), 0.0, c])
        return p
    pts = [on_axis(2.0, np.float32(0.5), D[0]), on_axis(4.0, np.nextafter(np.float32(0.5), np.float32(0.0)), D[1])]
    feats = ([[320.5, 240.0], [319.5, 240.0]], [2, 2], [D[0], D[1]])
    assert one_kf(matcher, pts, feats) == [0, -1]
    pts[1]["normal"] = pts[0]["normal"]
    assert one_kf(matcher, pts, feats) == [0, 1]


def test_octave_window(matcher):
    """Levels level - 1 and level are eligible; the better matches two levels below and one above are not."""
    a = D[5]
    pts = [S.point_at(150.0, 150.0, 3, a)]
    xy = [[150.2, 150.0], [150.0, 150.2], [149.8, 150.0], [150.0, 149.8]]
    assert one_kf(matcher, pts, (xy, [1, 2, 3, 4], [a, S.flip_bits(a, 12), S.flip_bits(a, 10), a])) == [2]
    assert one_kf(matcher, pts, (xy, [1, 2, 3, 4], [a, S.flip_bits(a, 10), S.flip_bits(a, 12), a])) == [1]


def test_equal_distances_first_in_area_order_wins(matcher):
    """GetFeaturesInArea walks cell columns, then cell rows, then ascending index inside a cell; Fuse keeps the first of equal distances."""
    a, b, c = D[0], D[1], D[2]
    pts = [S.point_at(95.0, 100.0, 2, a), S.point_at(200.0, 95.0, 2, b), S.point_at(300.0, 300.0, 2, c)]
    feats = ([[96.0, 100.0], [94.0, 100.0], [200.0, 96.0], [200.0, 94.0], [300.5, 300.0], [299.5, 300.0]],
             [2] * 6, [S.flip_bits(a, 7), S.flip_bits(a, 7), S.flip_bits(b, 9), S.flip_bits(b, 9), S.flip_bits(c, 3), S.flip_bits(c, 3)])
    assert one_kf(matcher, pts, feats) == [1, 3, 4]


def test_hamming_threshold(matcher):
    """bestDist <= TH_LOW: 50 is accepted, 51 is not."""
    pts = [S.point_at(100.0, 100.0, 2, D[8]), S.point_at(300.0, 100.0, 2, D[9])]
    feats = ([[100.5, 100.0], [300.5, 100.0]], [2, 2], [S.flip_bits(D[8], S.TH_LOW), S.flip_bits(D[9], S.TH_LOW + 1)])
    assert one_kf(matcher, pts, feats) == [0, -1]


# ---- 3. entries that are passed over ----
def test_skipped_entries(matcher):
    """id -1, a bad point, a point the key-frame lists (spAlreadyFound), and an id twice: the duplicate is answered like the first."""
    pts = [S.point_at(100.0 + 60.0 * i, 120.0, 2, D[i]) for i in range(4)]
    feats = ([[100.5 + 60.0 * i, 120.0] for i in range(4)] + [[50.0, 400.0]], [2] * 5, D[:4] + [D[10]])
    m = F.tiny_map(pts, [feats, feats], rows=[[-1, -1, -1, -1, 2], None], ids=[0, -1, 1, 2, 3, 0])
    m.bad[1] = True
    _, hits, per = check(matcher, m)
    assert hits.tolist() == [(0, 0, 0, -1), (0, 4, 3, -1), (0, 5, 0, -1),
                             (1, 0, 0, -1), (1, 3, 2, -1), (1, 4, 3, -1), (1, 5, 0, -1)] and per.tolist() == [3, 4]


# ---- 4. sizes: the ordered emit across wave and block seams ----
@pytest.mark.parametrize("n_points,n_kfs", [(1, 1), (97, 1), (257, 1), (257, 5), (97, 5)])
def test_hits_across_wave_and_block_seams(matcher, n_points, n_kfs):
    """Hits at list entries 63, 64, 255 and 256 (those the list has; its last entry too), every other entry a point far outside the image or
    -1: the hit list is those entries in order, for every key-frame."""
    at = sorted({i for i in (63, 64, 255, 256, n_points - 1) if i < n_points})
    pts = [S.point_at(80.0 + 90.0 * j, 200.0, 2, D[j]) for j in range(len(at))] + [S.point_at(5000.0, 5000.0, 2, D[15])]
    feats = ([[80.5 + 90.0 * j, 200.0] for j in range(len(at))], [2] * len(at), D[:len(at)])
    ids = [at.index(i) if i in at else (len(at) if i % 3 else -1) for i in range(n_points)]
    m = F.tiny_map(pts, [feats] * n_kfs, rows=[[0] + [-1] * (len(at) - 1)] + [None] * (n_kfs - 1) if n_kfs > 1 else None, ids=ids, pad_to=70 + n_kfs)
    _, hits, per = check(matcher, m)
    want = [(k, i, at.index(i), -1) for k in range(n_kfs) for i in at if not (n_kfs > 1 and k == 0 and i == at[0])]
    assert hits.tolist() == want and per.tolist() == [len(at) - (n_kfs > 1 and k == 0) for k in range(n_kfs)]


def test_more_hits_than_travel_with_the_head(matcher):
    """A list that names four matching points 150 times over, against four key-frames: 2400 hits, more than the first copy carries."""
    pts = [S.point_at(80.0 + 90.0 * j, 200.0, 2, D[j]) for j in range(4)]
    feats = ([[80.5 + 90.0 * j, 200.0] for j in range(4)], [2] * 4, D[:4])
    m = F.tiny_map(pts, [feats] * 4, ids=[0, 1, 2, 3] * 150)
    _, hits, per = check(matcher, m)
    assert per.tolist() == [600] * 4 and hits["feature"].tolist() == [0, 1, 2, 3] * 600


# ---- 5. limits and refusals ----
def test_zero_hits(matcher):
    pts = [S.point_at(5000.0, 100.0, 2, D[0]), S.point_at(100.0, 100.0, 2, D[1])]
    m = F.tiny_map(pts, [([[100.5, 100.0]], [2], [S.flip_bits(D[1], 90)])] * 2)
    _, hits, per = check(matcher, m)
    assert len(hits) == 0 and per.tolist() == [0, 0]
    sc = F.StoreScene(m)
    assert [len(x) for x in sc.call(matcher, corrected=[])] == [0, 0] and [len(x) for x in sc.call(matcher, ids=[])] == [0, 2]


def test_hit_list_one_entry_short(matcher):
    from rumi_slam_amd.mapping import SearchAndFuseResident, search_and_fuse_stage_ms
    m = F.seeded_map(34, n_corr=3)
    want, want_per = F.expected_call(m)
    sc = F.StoreScene(m)
    n = len(want)
    hits, per = np.full(n, -9, F.HIT_DTYPE), np.full(3, -9, np.int32)
    rc, n_hits, msg = sc.raw_call(matcher, hits, n - 1, per)
    assert rc == capi.RUMI_E_CAPACITY and "hit_cap" in msg
    assert n_hits == n and per.tobytes() == want_per.tobytes()
    assert hits[:n - 1].tobytes() == want[:n - 1].tobytes() and hits[n - 1].tolist() == (-9, -9, -9, -9)
    rc, n_hits, _ = sc.raw_call(matcher, hits, n, per)
    assert rc == capi.RUMI_OK and n_hits == n and hits.tobytes() == want.tobytes()
    ms = search_and_fuse_stage_ms(matcher)
    assert ms.shape == (3,) and (ms >= 0).all() and ms[1] > 0
    # the mirror grows its list once and calls again
    grown, per2 = sc.call(matcher, hit_cap=5)
    assert grown.tobytes() == want.tobytes() and per2.tobytes() == want_per.tobytes()


def test_staged_edits_are_seen(matcher):
    m = F.seeded_map(32, n_corr=3)
    sc, hits, per = check(matcher, m)
    free = hits[hits["occupant"] < 0]
    # a point made bad; a point entered into the row at the feature the call found for it; a point moved out of the image
    hb = free[0]
    pb = m.ids[int(hb["point"])]
    ho = next(h for h in free if m.ids[int(h["point"])] != pb)
    po = m.ids[int(ho["point"])]
    hm = next(h for h in free[::-1] if m.ids[int(h["point"])] not in (pb, po))
    pm = m.ids[int(hm["point"])]
    m.bad[pb] = True
    ko = m.corrected[int(ho["kf"])]
    m.kfs[ko].row[int(ho["feature"])] = po
    m.pos[pm] = m.pos[pm] + np.float32([40.0, 0.0, 0.0])
    sc.set_row(ko)
    sc.set_points([pb, po, pm])
    _, hits2, _ = check(matcher, m, sc)
    pairs2 = {(int(h["kf"]), int(h["point"])) for h in hits2}
    assert not any(m.ids[i] in (pb, pm) for _, i in pairs2) and (int(ho["kf"]), int(ho["point"])) not in pairs2
    assert len(hits2) < len(hits)


def test_a_searched_entry_without_attributes(matcher):
    m = F.seeded_map(33, n_corr=3)
    want, _ = F.expected_call(m)
    lone = [p for p in dict.fromkeys(m.ids) if p >= 0 and not m.bad[p]][:3]
    m.has_attr[lone] = False
    entries = sum(m.ids.count(p) for p in lone)
    sc = F.StoreScene(m)
    hits, per = np.full(len(want) + 8, -9, F.HIT_DTYPE), np.full(3, -9, np.int32)
    rc, n_hits, msg = sc.raw_call(matcher, hits, len(hits), per)
    assert rc == capi.RUMI_E_INVALID and "%d searched list entries whose map point has no attributes" % entries in msg, msg
    assert n_hits == -77 and (per == -9).all() and (hits["kf"] == -9).all(), "nothing written"


class Refusals:
    def __init__(self, matcher):
        self.matcher = matcher
        self.m = F.seeded_map(35, n_corr=3, n_world=60, n_feat=70)
        self.sc = F.StoreScene(self.m, max_points=self.m.n_points + 64)
        self.hits, self.per = np.full(64, -9, F.HIT_DTYPE), np.full(700, -9, np.int32)

    def call(self, matcher="own", **kw):
        rc, n_hits, msg = self.sc.raw_call(self.matcher if matcher == "own" else matcher, self.hits, 64, self.per, **kw)
        assert n_hits == -77 and (self.per == -9).all() and (self.hits["kf"] == -9).all(), "nothing written"
        return rc, msg

    def kfs(self, n=3):
        from rumi_slam_amd import mapping
        return (mapping.RumiFuseKF * n)(*[self.sc.fuse_kf(self.m.corrected[k % 3]) for k in range(n)])


@pytest.fixture(scope="module")
def refusals(matcher):
    return Refusals(matcher)


@pytest.mark.parametrize("kw", [dict(matcher=None), dict(store=False), dict(n_hits=False), dict(n_kfs=-1), dict(n_points=-1)])
def test_refuses_missing_arguments(refusals, kw):
    rc, msg = refusals.call(**kw)
    assert rc == capi.RUMI_E_INVALID and "rumi_search_and_fuse_resident: missing argument" in msg


@pytest.mark.parametrize("th", [0.0, -4.0, float("nan")])
def test_refuses_a_threshold_that_is_not_positive(refusals, th):
    rc, msg = refusals.call(th=th)
    assert rc == capi.RUMI_E_INVALID and "th must be positive" in msg


@pytest.mark.parametrize("field,index", [("Tcw7", 5), ("Ow", 1), ("bounds", 2), ("log_scale_factor", None)])
def test_refuses_a_record_that_is_not_finite(refusals, field, index):
    arr = refusals.kfs()
    if index is None:
        setattr(arr[1], field, float("inf"))
    else:
        getattr(arr[1], field)[index] = float("nan")
    rc, msg = refusals.call(kfs=arr)
    assert rc == capi.RUMI_E_INVALID and "not finite" in msg


def test_refuses_empty_bounds(refusals):
    arr = refusals.kfs()
    arr[2].bounds[2] = arr[2].bounds[0]
    rc, msg = refusals.call(kfs=arr)
    assert rc == capi.RUMI_E_INVALID and "empty image bounds" in msg


def test_refuses_slots(refusals):
    r, slot = refusals, [S.slot_of(k) for k in refusals.m.corrected]
    rc, msg = r.call(slots=[slot[0], 3, slot[2]])
    assert rc == capi.RUMI_E_INVALID and "a slot that is not live or holds no features" in msg
    rc, msg = r.call(slots=[slot[0], slot[1], slot[0]])
    assert rc == capi.RUMI_E_INVALID and "a slot named twice" in msg


def test_refuses_a_slot_without_features_and_a_row_of_another_length(matcher):
    m = F.seeded_map(36, n_corr=3, n_world=60, n_feat=70)
    sc = F.StoreScene(m)
    hits, per = np.full(8, -9, F.HIT_DTYPE), np.full(3, -9, np.int32)
    k = m.corrected[1]
    m.kfs[k].row = m.kfs[k].row[:-1]
    sc.set_row(k)
    rc, n_hits, msg = sc.raw_call(matcher, hits, 8, per)
    assert rc == capi.RUMI_E_INVALID and "feature count differs from the length of its map-point row" in msg and n_hits == -77
    sc.store.drop_keyframe_features([S.slot_of(k)])
    rc, n_hits, msg = sc.raw_call(matcher, hits, 8, per)
    assert rc == capi.RUMI_E_INVALID and "holds no features" in msg and n_hits == -77 and (per == -9).all()


def test_refuses_an_id_outside_the_store(refusals):
    cap = refusals.m.n_points + 64
    rc, msg = refusals.call(ids=[0, 1, cap])
    assert rc == capi.RUMI_E_INVALID and "at or above the store's point capacity" in msg
    rc, msg = refusals.call(ids=[0, 1, cap - 1])                              # the last id the tables hold: a point the store never saw
    assert rc == capi.RUMI_E_INVALID and "1 searched list entries whose map point has no attributes" in msg


def test_refuses_what_exceeds_a_capacity(refusals):
    from rumi_slam_amd.matcher import ORBmatcher
    r = refusals
    rc, msg = r.call(slots=np.arange(641, dtype=np.int32), kfs=r.kfs(641))
    assert rc == capi.RUMI_E_CAPACITY and "RUMI_FUSE_MAX_TARGETS" in msg
    rc, msg = r.call(slots=np.arange(640, dtype=np.int32), kfs=r.kfs(640), ids=np.zeros(2 ** 31 // 640 + 1, np.int32))
    assert rc == capi.RUMI_E_CAPACITY and "more pairs than a work item addresses" in msg
    small = ORBmatcher(0.8, True, max_features=64, max_queries=1024)
    try:
        rc, msg = r.call(matcher=small)
        assert rc == capi.RUMI_E_CAPACITY and "exceeds the matcher's max_features" in msg
    finally:
        small.close()


def test_refuses_another_device(refusals):
    """The store is bound to the device of its first consumer; a matcher on another device is refused.  Only a machine with two devices can
    ask for that; on one device there is no second matcher to make."""
    from rumi_slam_amd.matcher import ORBmatcher
    refusals.sc.call(refusals.matcher)
    if capi.lib().rumi_device_count() < 2:
        return
    other = ORBmatcher(0.8, True, max_features=2048, max_queries=32768, device=1)
    try:
        rc, msg = refusals.call(matcher=other)
        assert rc == capi.RUMI_E_INVALID and "different devices" in msg
    finally:
        other.close()
