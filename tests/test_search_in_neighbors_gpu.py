"""rumi_search_in_neighbors_resident (include/rumi_mapping.h): every (target, point) search of LocalMapping::SearchInNeighbors in one device
call on key-frames and points resident in the covisibility store.  The contract is bytes: the CPU oracle's answer per pair
(oracle_lib.fuse_candidates through tests/search_in_neighbors_scene.py) and the merged single-target entry's (rumi_fuse_candidates) on the same
key-frame and points.  The hand-made cases put one property each on the edge where the kernels can go wrong."""
import numpy as np
import pytest

import search_in_neighbors_scene as S
from rumi_slam_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    from rumi_slam_amd.matcher import ORBmatcher
    m = ORBmatcher(0.6, True, max_features=2048, max_queries=32768)
    yield m
    m.close()


def check(matcher, m, sc=None):
    """The call against the oracle and against the single-target entry; returns (scene, fwd, rev_point, rev_best)."""
    sc = S.StoreScene(m) if sc is None else sc
    want = S.expected_call(m)
    got = sc.call(matcher)
    for g, w, name in zip(got, want, ("fwd_best", "rev_point", "rev_best")):
        assert g.dtype == np.int32 and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, int(np.count_nonzero(g != w)))
    obs = m.observations()
    ids = np.asarray(m.kfs[0].row, np.int64)
    for t in range(m.n_targets):
        skip = [p < 0 or m.bad[p] or (1 + t) in obs[p] for p in m.kfs[0].row]
        one = sc.single_target(matcher, 1 + t, ids, skip)
        assert got[0][t].tobytes() == one.tobytes(), ("target", t)
    if len(got[1]):
        assert got[2].tobytes() == sc.single_target(matcher, 0, got[1], np.zeros(len(got[1]), bool)).tobytes()
    return (sc,) + got


# ---- 1. whole maps ----
@pytest.mark.parametrize("seed,nt", S.CONSTRUCTED + [(31, 4)])
def test_parity(matcher, seed, nt):
    m = S.seeded_map(seed, nt)
    sc, fwd, rp, rb = check(matcher, m)
    assert np.count_nonzero(fwd >= 0) > 60 and np.count_nonzero(rb >= 0) > 60 and np.count_nonzero(rb < 0) > 10
    again = sc.call(matcher)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (fwd, rp, rb))), "two calls, the same bytes"
    # the replay a caller makes of these answers leaves the member's map
    ref, nf, nr, _ = S.reference(m)
    res, nf2, nr2, missing = S.resident(m, fwd, rp, rb)
    assert missing == [] and (nf2, nr2) == (nf, nr) and res.state() == ref.state()


def test_feature_counts_that_are_no_multiple_of_64(matcher):
    m = S.seeded_map(41, 3, n_extra=1, n_world=120, n_feat=97)
    assert all(kf.n == 97 for kf in m.kfs)
    _, fwd, rp, rb = check(matcher, m)
    assert np.count_nonzero(fwd >= 0) > 30 and np.count_nonzero(rb >= 0) > 30


def test_staged_edits_are_seen(matcher):
    m = S.seeded_map(32, 4)
    sc, fwd, rp, rb = check(matcher, m)
    cur = m.kfs[0]
    hit = [i for i in range(cur.n) if (fwd[:, i] >= 0).any()]
    # one point made bad
    pb = cur.row[hit[0]]
    m.bad[pb] = True
    # one observation added: a point of the current key-frame enters target 2's row at the feature the call found for it
    i = next(i for i in hit[1:] if fwd[1, i] >= 0 and m.kfs[2].row[fwd[1, i]] < 0)
    po = cur.row[i]
    m.kfs[2].row[int(fwd[1, i])] = po
    # one attribute record moved: a reverse candidate that matched is pushed out of the image
    pm = int(rp[np.nonzero(rb >= 0)[0][0]])
    m.pos[pm] = m.pos[pm] + np.float32([40.0, 0.0, 0.0])
    sc.set_row(2)
    sc.set_points([pb, po, pm])
    _, fwd2, rp2, rb2 = check(matcher, m, sc)
    assert (fwd2[:, hit[0]] == -1).all() and fwd2[1, i] == -1 and (fwd[:, hit[0]] >= 0).any()
    assert rb2[list(rp2).index(pm)] == -1


# ---- 2. hand-made edges ----
RNG = np.random.default_rng(77)
D = [RNG.integers(0, 256, 32, dtype=np.uint8) for _ in range(16)]


def one_target(matcher, points, feats):
    m = S.tiny_map(points, [feats])
    _, fwd, rp, rb = check(matcher, m)
    assert len(rp) == 0
    return fwd[0][:len(points)].tolist()


def test_image_bounds(matcher):
    """KeyFrame::IsInImage (KeyFrame.cc:927-929) is x >= mnMinX && x < mnMaxX: a projection exactly on the minimum is inside, one exactly on the
    maximum is not."""
    pts = [S.point_at(0.0, 240.0, 2, D[0]), S.point_at(640.0, 100.0, 4, D[1]), S.point_at(639.0, 300.0, 4, D[2]), S.point_at(320.0, 0.0, 2, D[3]),
           S.point_at(100.0, 480.0, 4, D[4])]
    px = [S.pixel_of(p["pos"]) for p in pts]
    assert px[0][0] == 0.0 and px[1][0] == 640.0 and px[3][1] == 0.0 and px[4][1] == 480.0, "the float projection lands on the bound exactly"
    # the last grid column ends at x = 635 and the last row at y = 475: at level 4 (radius 6.2, sigma2 4.3) a key-point just inside them is
    # within every gate of a projection on the far bound, so IsInImage alone decides
    feats = ([[1.0, 240.0], [634.99, 100.0], [634.99, 300.0], [320.0, 1.0], [100.0, 474.99]], [2, 4, 4, 2, 4], [D[0], D[1], D[2], D[3], D[4]])
    assert one_target(matcher, pts, feats) == [0, -1, 2, 3, -1]


def test_window_across_a_cell_seam_and_the_last_column(matcher):
    """Cells are 10 px wide and a key-point belongs to cell round(x / 10): 94 and 96 lie in columns 9 and 10.  A key-point at x >= 635 rounds to
    column 64, outside the grid, and is in no cell (Frame::PosInGrid): it is never found, however well it matches."""
    pts = [S.point_at(95.0, 100.0, 2, D[0]), S.point_at(95.0, 200.0, 2, D[1]), S.point_at(633.0, 300.0, 2, D[2]), S.point_at(636.0, 400.0, 2, D[3])]
    feats = ([[96.0, 100.0], [94.0, 200.0], [634.0, 300.0], [637.0, 400.0], [633.0, 400.0]], [2] * 5,
             [D[0], D[1], D[2], D[3], S.flip_bits(D[3], 30)])
    assert one_target(matcher, pts, feats) == [0, 1, 2, 4]


def test_equal_distances_first_in_area_order_wins(matcher):
    """GetFeaturesInArea walks cell columns, then cell rows, then ascending index inside a cell; Fuse keeps the first of equal distances
    (`dist < bestDist`).  The feature indices run against that order."""
    a, b, c = D[0], D[1], D[2]
    pts = [S.point_at(95.0, 100.0, 2, a), S.point_at(200.0, 95.0, 2, b), S.point_at(300.0, 300.0, 2, c)]
    feats = ([[96.0, 100.0], [94.0, 100.0],            # columns 10 and 9: the later index lies in the earlier column
              [200.0, 96.0], [200.0, 94.0],            # rows 10 and 9 of one column (cells are 10 px high)
              [300.5, 300.0], [299.5, 300.0]],         # one cell: the lower index
             [2] * 6, [S.flip_bits(a, 7), S.flip_bits(a, 7), S.flip_bits(b, 9), S.flip_bits(b, 9), S.flip_bits(c, 3), S.flip_bits(c, 3)])
    assert one_target(matcher, pts, feats) == [1, 3, 4]


def test_octave_window(matcher):
    """Levels level - 1 and level are eligible; the better matches two levels below and one above are not."""
    a = D[5]
    pts = [S.point_at(150.0, 150.0, 3, a)]
    feats = ([[150.2, 150.0], [150.0, 150.2], [149.8, 150.0], [150.0, 149.8]], [1, 2, 3, 4],
             [a, S.flip_bits(a, 12), S.flip_bits(a, 10), a])
    assert one_target(matcher, pts, feats) == [2]
    feats = ([[150.2, 150.0], [150.0, 150.2], [149.8, 150.0], [150.0, 149.8]], [1, 2, 3, 4],
             [a, S.flip_bits(a, 10), S.flip_bits(a, 12), a])
    assert one_target(matcher, pts, feats) == [1]


def test_reprojection_gate(matcher):
    """e2 * invSigma2 against 5.99 at level 0 (sigma2 = 1): 2.44^2 = 5.95 passes, 2.45^2 = 6.00 does not."""
    pts = [S.point_at(100.0, 100.0, 1, D[6]), S.point_at(300.0, 100.0, 1, D[7])]
    feats = ([[102.44, 100.0], [302.45, 100.0]], [0, 0], [D[6], D[7]])
    e2 = [float(np.float32(np.float32(100.0) - np.float32(102.44)) ** 2), float(np.float32(np.float32(300.0) - np.float32(302.45)) ** 2)]
    assert e2[0] < 5.99 < e2[1]
    assert one_target(matcher, pts, feats) == [0, -1]


def test_hamming_threshold(matcher):
    """bestDist <= TH_LOW: 50 is accepted, 51 is not."""
    pts = [S.point_at(100.0, 100.0, 2, D[8]), S.point_at(300.0, 100.0, 2, D[9])]
    feats = ([[100.5, 100.0], [300.5, 100.0]], [2, 2], [S.flip_bits(D[8], 50), S.flip_bits(D[9], 51)])
    assert one_target(matcher, pts, feats) == [0, -1]


def test_no_feature_in_the_window(matcher):
    pts = [S.point_at(100.0, 100.0, 2, D[10]), S.point_at(400.0, 300.0, 2, D[11])]
    feats = ([[100.5, 100.0], [420.0, 300.0]], [2, 2], [D[10], D[11]])
    assert one_target(matcher, pts, feats) == [0, -1]


def test_a_target_whose_row_is_empty_gives_no_reverse_candidates(matcher):
    a, b = D[12], D[13]
    pts = [S.point_at(100.0, 100.0, 2, a), S.point_at(601.0, 440.0, 0, b), S.point_at(50.0, 50.0, 2, D[14])]
    f = ([[100.5, 100.0], [400.0, 400.0]], [2, 2], [a, D[15]])
    m = S.tiny_map(pts, [f, f, f], extra_rows=[None, [-1, 1], [2, 1]])
    m.kfs[0].row[1] = m.kfs[0].row[2] = -1                        # points 1 and 2 live in the targets only
    m.kfs[0].desc[0] = b                                          # and point 1 matches feature 0 of the current key-frame (600, 440), one pixel away
    _, fwd, rp, rb = check(matcher, m)
    assert rp.tolist() == [1, 2] and rb.tolist() == [0, -1], "first occurrence in (target, feature) order; point 1 is listed once"
    assert fwd[:, 0].tolist() == [0, 0, 0]


def test_the_view_is_taken_per_call_and_survives_both_arenas_moving(matcher):
    """Between two calls on one matcher the feature arena grows (a new device allocation) and the row arena is rebuilt (every row moves): the
    second call reads the store where it lies then.  The smallest constructed scene, the current key-frame and two targets, in a store whose
    arenas start as small as the entries admit."""
    from rumi_slam_amd.matcher import FeatureVector, FrameView
    a, b = D[12], D[13]
    pts = [S.point_at(100.0, 100.0, 2, a), S.point_at(601.0, 440.0, 0, b), S.point_at(50.0, 50.0, 2, D[14])]
    f = ([[100.5, 100.0], [400.0, 400.0]], [2, 2], [a, D[15]])
    m = S.tiny_map(pts, [f, f], extra_rows=[[-1, 1], [2, 1]])
    m.kfs[0].row[1] = m.kfs[0].row[2] = -1                        # points 1 and 2 live in the targets only
    m.kfs[0].desc[0] = b                                          # and point 1 matches feature 0 of the current key-frame
    sc = S.StoreScene(m, arena_entries=16, reserve_features=4096)
    _, fwd, rp, rb = check(matcher, m, sc)
    assert fwd[:, 0].tolist() == [0, 0] and rp.tolist() == [1, 2] and rb.tolist() == [0, -1]
    # one more key-frame, which no point observes: more features than the feature arena has room left for, a row longer than the row arena
    store, fs, rs = sc.store, sc.store.feature_stats(), sc.store.stats()
    n = max(fs["capacity"] // 60, rs["capacity"]) + 8
    rng = np.random.default_rng(9)
    xy = np.stack([rng.uniform(20, 600, n), rng.uniform(20, 440, n)], 1)
    slot = S.slot_of(len(m.kfs))
    store.set_keyframes([slot], [9000 + 13 * slot], [0], [0], [np.full(n, -1, np.int32)], [[]], [-1], [[]])
    store.set_keyframe_features(slot, FrameView(S.keypoints(xy, np.zeros(n, np.int32)), rng.integers(0, 256, (n, 32), dtype=np.uint8), S.W, S.H, S.SF),
                                FeatureVector({}), S.K4)
    fs2, rs2 = store.feature_stats(), store.stats()
    assert fs2["growths"] > fs["growths"] and fs2["capacity"] > fs["capacity"]
    assert rs2["growths"] + rs2["compactions"] > rs["growths"] + rs["compactions"]
    _, fwd2, rp2, rb2 = check(matcher, m, sc)
    assert fwd2.tobytes() == fwd.tobytes() and rp2.tobytes() == rp.tobytes() and rb2.tobytes() == rb.tobytes()


@pytest.mark.parametrize("nt", [1, 65])
def test_target_counts(matcher, nt):
    """One target, and more targets than a wave has lanes: 65 copies of a 64-feature key-frame under slots of their own."""
    base = S.seeded_map(51, 1, n_extra=0, n_world=50, n_feat=64)
    kfs = [base.kfs[0]] + [S.KeyFrame(base.kfs[1].keys, base.kfs[1].desc, base.kfs[1].Tcw7, base.kfs[1].Ow,
                                     base.kfs[1].row if t == 0 else [-1] * 64) for t in range(nt)]
    m = S.SinMap(kfs, nt, base.pos, base.normal, base.min_dist, base.max_dist, base.desc)
    _, fwd, rp, rb = check(matcher, m)
    assert fwd.shape == (nt, 64) and np.count_nonzero(fwd[0] >= 0) > 10 and np.count_nonzero(rb >= 0) > 5
    if nt > 1:                                                    # an empty copy is searched for the points target 0 already lists, too
        assert all(np.count_nonzero(fwd[t] >= 0) >= np.count_nonzero(fwd[0] >= 0) for t in range(1, nt))
        assert fwd[1:].tobytes() == np.tile(fwd[1], (nt - 1, 1)).tobytes()


# ---- 3. refusals that the device decides, and the capacity of the reverse lists ----
def test_a_searched_point_without_attributes(matcher):
    m = S.seeded_map(33, 3)
    want = S.expected_call(m)
    lone = [p for p in m.kfs[0].row if p >= 0][:2] + [int(want[1][0])]
    m.has_attr[lone] = False
    sc = S.StoreScene(m)
    fwd, rp, rb = np.full(want[0].shape, -9, np.int32), np.full(len(want[1]), -9, np.int32), np.full(len(want[1]), -9, np.int32)
    rc, n_rev = sc.raw_call(matcher, fwd, rp, rb, len(rp))
    msg = capi.lib().rumi_last_error().decode()
    assert rc == capi.RUMI_E_INVALID and "3 searched map point(s) without attributes" in msg, msg
    assert n_rev == -77 and (fwd == -9).all() and (rp == -9).all() and (rb == -9).all(), "nothing written"


def test_reverse_lists_one_entry_short(matcher):
    m = S.seeded_map(34, 3)
    want = S.expected_call(m)
    sc = S.StoreScene(m)
    n = len(want[1])
    fwd, rp, rb = np.full(want[0].shape, -9, np.int32), np.full(n, -9, np.int32), np.full(n, -9, np.int32)
    rc, n_rev = sc.raw_call(matcher, fwd, rp, rb, n - 1)
    assert rc == capi.RUMI_E_CAPACITY and "rev_cap" in capi.lib().rumi_last_error().decode()
    assert n_rev == n and fwd.tobytes() == want[0].tobytes()
    assert rp[:n - 1].tobytes() == want[1][:n - 1].tobytes() and rb[:n - 1].tobytes() == want[2][:n - 1].tobytes() and rp[n - 1] == -9 and rb[n - 1] == -9
    rc, n_rev = sc.raw_call(matcher, fwd, rp, rb, n)
    assert rc == capi.RUMI_OK and n_rev == n and rp.tobytes() == want[1].tobytes() and rb.tobytes() == want[2].tobytes()


def test_no_targets_and_stage_times(matcher):
    from rumi_slam_amd.mapping import search_in_neighbors_stage_ms
    m = S.seeded_map(35, 3)
    sc = S.StoreScene(m)
    fwd, rp, rb = sc.call(matcher, targets=[])
    assert fwd.shape[0] == 0 and len(rp) == 0 and len(rb) == 0
    sc.call(matcher)
    ms = search_in_neighbors_stage_ms(matcher)
    assert ms.shape == (3,) and (ms >= 0).all() and ms[1] > 0
