"""rumi_refresh_map_points_resident (include/rumi_mapping.h) on the GPU: MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth over
the covisibility store, against the block entry (rumi_refresh_map_points) and the C++ oracle (tests/cpp/refresh_oracle.cc) on the same map.

Everything is compared bit for bit, without a tolerance: the descriptor part is integer, and the float part has no transcendental function and
a fixed operation order with correctly rounded division and square root on all three sides."""
import numpy as np
import pytest

import refresh_resident_scene as rr
from refresh_scene import MODES, RefreshScene, build_oracle, run_oracle
from rumi_slam_amd import capi
from rumi_slam_amd.mapping import REFRESH_DESCRIPTOR, REFRESH_MAX_OBS, REFRESH_NORMAL_DEPTH, REFRESH_WRITE_BACK

pytestmark = pytest.mark.gpu
BOTH = REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH
FILL = 0xC3
_i32 = np.int32


def last_error():
    return capi.lib().rumi_last_error().decode()


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("refresh_resident"))


@pytest.fixture(scope="module")
def refresher():
    from rumi_slam_amd.mapping import MapPointRefresher
    r = MapPointRefresher()
    yield r
    r.close()


class Loaded:
    """A map, its store, and the oracle's outputs per mode (computed once, never changed)."""

    def __init__(self, m, oracle):
        self.m, self.store = m, m.store()
        self.batch = m.batch()
        self.want = {what: run_oracle(oracle, self.batch, what, FILL) for what in MODES}
        self.ids = np.arange(m.n_pts, dtype=_i32)


@pytest.fixture(scope="module")
def con(oracle):
    c = Loaded(rr.constructed_map(), oracle)
    yield c
    c.store.close()


@pytest.fixture(scope="module")
def scene(oracle):
    c = Loaded(rr.ResidentMap.from_scene(RefreshScene(0, 360, 500, 400)), oracle)
    yield c
    c.store.close()


def resident(refresher, store, ids, what, flags=0, fill=FILL):
    from rumi_slam_amd.mapping import refresh_resident_outputs
    ids = np.ascontiguousarray(ids, _i32)
    out = refresh_resident_outputs(len(ids), fill)
    capi.check(refresher.status_resident(store, ids, what, flags, out))
    return {k: v[:len(ids)] for k, v in out.items()}


def block(batch, what, fill=FILL):
    from rumi_slam_amd.mapping import RefreshMapPoints
    return RefreshMapPoints(batch, what, out=batch.outputs(fill))


def check_equal(m, got, want, what, ids=None):
    """The resident outputs against the block entry's / the oracle's: the arrays of the modes asked for equal, the others untouched, and desc
    the winning row's bytes where there is a winner (its fill elsewhere)."""
    ids = range(m.n_pts) if ids is None else ids
    for k in ("best_obs", "best_median", "normal", "min_distance", "max_distance", "updated"):
        diff = np.nonzero((got[k].reshape(len(got[k]), -1).view(np.uint8) != want[k].reshape(len(want[k]), -1).view(np.uint8)).any(axis=1))[0]
        print(f"{k}: {len(diff)} of {len(want[k])} entries differ" + (f", first {diff[0]}: {got[k][diff[0]]} vs {want[k][diff[0]]}" if len(diff) else ""))
        assert got[k].tobytes() == want[k].tobytes(), k
    for i, p in enumerate(ids):
        b = int(got["best_obs"][i]) if what & REFRESH_DESCRIPTOR else -1
        if b >= 0:
            k, f = m.points[p][2][b]
            assert got["desc"][i].tobytes() == m.kfs[k][0][f].tobytes(), ("desc", p)
        else:
            assert got["desc"][i].tobytes() == bytes([FILL]) * 32, ("desc untouched", p)


# ---- 1. resident == block entry == oracle ----
@pytest.mark.parametrize("what", MODES)
def test_constructed_set_equals_block_entry_and_oracle(con, refresher, what):
    got = resident(refresher, con.store, con.ids, what)
    blk = block(con.batch, what)
    for k in con.want[what]:
        assert blk[k].tobytes() == con.want[what][k].tobytes(), ("block entry vs oracle", k)
    check_equal(con.m, got, con.want[what], what)


def test_constructed_cases_are_what_they_claim(con):
    """The oracle's own answers show that each constructed case exercises what it is there for."""
    w, c, m = con.want[BOTH], con.m.cases, con.m
    for n in (1, 2, 3, 16, 17, 32, 33, 64, 65, 66, 129, 300):
        assert len(m.points[c[f"len{n}"]][2]) == n and w["best_obs"][c[f"len{n}"]] >= 0
    assert w["best_obs"][c["empty"]] == -1 and w["updated"][c["empty"]] == 0
    assert w["best_obs"][c["all_bad"]] == -1 and w["best_median"][c["all_bad"]] == -1 and w["updated"][c["all_bad"]] == 1
    assert w["best_obs"][c["bad_first"]] >= 1                                                   # the dropped first entry counts
    bad_kf = lambda p: [i for i, (k, _) in enumerate(m.points[p][2]) if m.kfs[k][3]]
    assert bad_kf(c["bad_first"]) == [0] and bad_kf(c["bad_middle"]) == [3] and bad_kf(c["bad_last"]) == [6]
    for name, length, left in (("len17_left16", 17, 16), ("len18_left17", 18, 17), ("len65_left64", 65, 64), ("len66_left65", 66, 65), ("len70_left60", 70, 60)):
        p = c[name]
        assert len(m.points[p][2]) == length and length - len(bad_kf(p)) == left
    assert w["best_obs"][c["two_equal_medians"]] == 1 and w["best_obs"][c["three_equal_medians"]] == 2      # the first of the equal ones, not position 0
    assert w["best_median"][c["identical"]] == 0 and w["best_obs"][c["identical"]] == 0 and w["best_median"][c["identical_wide"]] == 0
    p = c["ref_outside"]
    assert m.points[p][1] not in dict(m.points[p][2])
    assert m.kfs[m.points[c["ref_bad"]][1]][3]
    p = c["ref_top_octave"]
    assert m.octaves[m.points[p][1]][dict(m.points[p][2])[m.points[p][1]]] == 7
    assert [k for k, _ in m.points[c["shared_a"]][2]] == [k for k, _ in m.points[c["shared_b"]][2]]
    assert bad_kf(c["winner_after_bad"]) == [1] and w["best_obs"][c["winner_after_bad"]] == 3  # not 2, its index among the rows left


@pytest.mark.parametrize("what", MODES)
def test_scene_360x500_equals_oracle(scene, refresher, what):
    got = resident(refresher, scene.store, scene.ids, what)
    check_equal(scene.m, got, scene.want[what], what)
    if what & REFRESH_DESCRIPTOR:
        assert (got["best_obs"] >= 0).sum() > 100 and (got["best_obs"] == -1).sum() >= 3
    if what & REFRESH_NORMAL_DEPTH:
        assert got["updated"].sum() == len(got["updated"]) - 1


# ---- 2. independence and determinism ----
def test_batch_order_and_two_calls(con, refresher):
    base = resident(refresher, con.store, con.ids, BOTH)
    again = resident(refresher, con.store, con.ids, BOTH)
    for k in base:
        assert again[k].tobytes() == base[k].tobytes(), ("two calls", k)
    order = np.random.default_rng(5).permutation(con.m.n_pts).astype(_i32)
    got = resident(refresher, con.store, order, BOTH)
    for k in base:
        assert got[k].tobytes() == base[k][order].tobytes(), ("permuted ids", k)
    some = order[:13]                                                                           # a sub-list: other bins, other places in them
    got = resident(refresher, con.store, some, BOTH)
    for k in base:
        assert got[k].tobytes() == base[k][some].tobytes(), ("a sub-list", k)


def test_another_edit_order_gives_the_same_outputs(con, refresher):
    """Points before features, features in reverse order into a small arena that must grow, a third of them dropped and set again so that
    free blocks are reused: the blocks lie elsewhere, the outputs are the same."""
    from rumi_slam_amd.covis import Covisibility
    m = con.m
    s = Covisibility(m.n_kf, m.n_pts, arena_entries=64)
    s.reserve_features(4096)
    m.set_keyframes(s, range(m.n_kf))
    m.set_points(s, range(m.n_pts)[::-1])
    m.set_centres(s, range(m.n_kf)[::-1])
    m.set_features(s, range(m.n_kf)[::-1])
    got_first = resident(refresher, s, con.ids, BOTH)                                           # uploads: the dropped blocks below were on the device
    dropped = list(range(0, m.n_kf, 3))
    s.drop_keyframe_features(dropped)
    used_after_drop = s.feature_stats()["used"]
    m.set_features(s, dropped[::-1])
    st = s.feature_stats()
    assert st["growths"] >= 1 and st["slots"] == m.n_kf and st["used"] > used_after_drop and s.stats()["growths"] + s.stats()["compactions"] >= 1
    got = resident(refresher, s, con.ids, BOTH)
    check_equal(m, got, con.want[BOTH], BOTH)
    for k in got:
        assert got[k].tobytes() == got_first[k].tobytes(), k
    s.close()


# ---- 3. capacity ----
def test_2048_observers_answer(oracle, refresher):
    m = rr.capacity_map(REFRESH_MAX_OBS)
    s = m.store()
    want = run_oracle(oracle, m.batch(), BOTH, FILL)
    check_equal(m, resident(refresher, s, [0, 1], BOTH), want, BOTH)
    assert want["best_obs"][0] >= 0
    s.close()


def test_2049_observers_are_refused_with_nothing_written(refresher):
    from rumi_slam_amd.mapping import refresh_resident_outputs
    m = rr.capacity_map(REFRESH_MAX_OBS + 1)
    s = m.store()
    capi.check(refresher.status_resident(s, np.array([1], _i32), BOTH, 0, refresh_resident_outputs(1)))      # the store is on the device now
    before_dev, before_host, stats = s.read_attributes([0, 1], True).copy(), s.read_attributes([0, 1]).copy(), s.stats()
    for what in MODES:
        for flags in (0, REFRESH_WRITE_BACK):
            out = refresh_resident_outputs(2, FILL)
            assert refresher.status_resident(s, np.array([1, 0], _i32), what, flags, out) == capi.RUMI_E_CAPACITY and "RUMI_REFRESH_MAX_OBS" in last_error()
            assert all(v.tobytes() == bytes([FILL]) * v.nbytes for v in out.values())
    assert s.read_attributes([0, 1], True).tobytes() == before_dev.tobytes() and s.read_attributes([0, 1]).tobytes() == before_host.tobytes()
    assert s.stats() == stats
    s.close()


# ---- 4. write-back ----
def test_write_back_device_and_mirror(con, refresher):
    m = con.m
    s = m.store()
    before = m.expected_records(con.ids, None, False, False)
    # a query first: nothing changes
    resident(refresher, s, con.ids, BOTH)
    assert s.read_attributes(con.ids, True).tobytes() == before.tobytes() and s.read_attributes(con.ids).tobytes() == before.tobytes()
    # descriptor only, then both: device records and mirror equal the expectation built from the oracle's outputs; the position stays
    res = resident(refresher, s, con.ids, REFRESH_DESCRIPTOR, REFRESH_WRITE_BACK)
    check_equal(m, res, con.want[REFRESH_DESCRIPTOR], REFRESH_DESCRIPTOR)
    want = m.expected_records(con.ids, con.want[REFRESH_DESCRIPTOR], True, False)
    assert s.read_attributes(con.ids, True).tobytes() == want.tobytes() and s.read_attributes(con.ids).tobytes() == want.tobytes()
    res = resident(refresher, s, con.ids, BOTH, REFRESH_WRITE_BACK)
    check_equal(m, res, con.want[BOTH], BOTH)
    want = m.expected_records(con.ids, con.want[BOTH], True, True)
    dev, host = s.read_attributes(con.ids, True), s.read_attributes(con.ids)
    assert dev.tobytes() == want.tobytes() and host.tobytes() == want.tobytes()
    assert dev[:, :12].tobytes() == before[:, :12].tobytes()                                    # the position
    e = m.cases["empty"]
    assert dev[e].tobytes() == before[e].tobytes()                                              # a point with an empty row is untouched
    a = m.cases["all_bad"]
    assert dev[a, 32:].tobytes() == before[a, 32:].tobytes() and dev[a, 12:32].tobytes() != before[a, 12:32].tobytes()    # no winner: the descriptor stays
    assert (dev[:, 32:] != before[:, 32:]).any(axis=1).sum() == m.n_pts - 2                    # every other point has a winner
    s.close()


def test_write_back_wins_over_a_stale_staged_edit(con, refresher):
    m = con.m
    s = m.store()
    ids = np.array([m.cases["len3"], m.cases["len33"], m.cases["len66"]], _i32)
    resident(refresher, s, ids, BOTH)                                                           # everything staged so far is on the device
    a = m.initial_attributes(ids)
    s.set_point_attributes(ids, a["pos"], a["normal"] + 100.0, a["min_dist"] + 1.0, a["max_dist"] + 1.0, np.full((3, 32), 0x11, np.uint8))
    resident(refresher, s, ids, BOTH, REFRESH_WRITE_BACK)
    w = {k: v[ids] for k, v in con.want[BOTH].items()}
    want = m.expected_records(ids, w, True, True)
    assert s.read_attributes(ids, True).tobytes() == want.tobytes() and s.read_attributes(ids).tobytes() == want.tobytes()
    resident(refresher, s, ids[:1], REFRESH_DESCRIPTOR)                                         # another flush: nothing stale is left to go up
    assert s.read_attributes(ids, True).tobytes() == want.tobytes()
    s.close()


def test_refused_call_writes_nothing(con, refresher):
    from rumi_slam_amd.covis import Covisibility
    from rumi_slam_amd.mapping import refresh_resident_outputs
    m = con.m
    s = Covisibility(m.n_kf, m.n_pts)
    m.set_keyframes(s, range(m.n_kf)); m.set_features(s, range(m.n_kf))
    lone = m.points[m.cases["len33"]][2][5][0]                                                  # one observer slot of this point gets no centre
    m.set_centres(s, [k for k in range(m.n_kf) if k != lone])
    m.set_points(s, range(m.n_pts))
    ids = np.array([p for p in range(m.n_pts) if lone not in dict(m.points[p][2]) and m.points[p][1] != lone], _i32)
    resident(refresher, s, ids, BOTH)                                                           # the tables are on the device
    before_dev, before_host = s.read_attributes(con.ids, True).copy(), s.read_attributes(con.ids).copy()
    out = refresh_resident_outputs(m.n_pts, FILL)
    rc = refresher.status_resident(s, con.ids, BOTH, REFRESH_WRITE_BACK, out)
    n_missing = sum(1 for p in range(m.n_pts) if lone in dict(m.points[p][2])) + sum(1 for p in range(m.n_pts) if m.points[p][2] and m.points[p][1] == lone)
    assert rc == capi.RUMI_E_INVALID and f"{n_missing} observer or reference slots have no centre" in last_error(), last_error()
    assert all(v.tobytes() == bytes([FILL]) * v.nbytes for v in out.values())
    assert s.read_attributes(con.ids, True).tobytes() == before_dev.tobytes() and s.read_attributes(con.ids).tobytes() == before_host.tobytes()
    # the descriptor part does not read centres
    check_equal(m, resident(refresher, s, con.ids, REFRESH_DESCRIPTOR), con.want[REFRESH_DESCRIPTOR], REFRESH_DESCRIPTOR)
    s.close()


def test_search_in_neighbors_reads_the_written_back_values(oracle, refresher):
    """After the write-back, rumi_search_in_neighbors_resident on that store returns the bytes it returns on a fresh store whose attributes
    the host set from the oracle's values -- with no rumi_covis_set_point_attributes in between."""
    import search_in_neighbors_scene as S
    from rumi_slam_amd.matcher import ORBmatcher
    sm = S.seeded_map(31, 4)
    obs = sm.observations()
    rng = np.random.default_rng(3)
    ref = [sorted(o)[int(rng.integers(0, len(o)))] if o else -1 for o in obs]
    m = rr.ResidentMap([(kf.desc, S.SF, kf.Ow, False) for kf in sm.kfs], [kf.keys["octave"] for kf in sm.kfs],
                       [(sm.pos[p], ref[p], sorted(obs[p].items())) for p in range(sm.n_points)])
    want = run_oracle(oracle, m.batch(), BOTH, FILL)
    ids = np.arange(sm.n_points, dtype=_i32)
    # the store under test: the map as it is, then centres and references by slot, then one refresh with write-back
    a = S.StoreScene(sm)
    a.store.set_keyframe_centres([S.slot_of(k) for k in range(len(sm.kfs))], np.stack([kf.Ow for kf in sm.kfs]))
    a.store.set_point_reference(ids, [S.slot_of(r) if r >= 0 else -1 for r in ref])
    got = resident(refresher, a.store, ids, BOTH, REFRESH_WRITE_BACK)
    check_equal(m, got, want, BOTH)
    # the fresh store: the same map with the oracle's values in its attributes
    sm2 = S.clone(sm)
    for p in range(sm.n_points):
        if want["best_obs"][p] >= 0:
            k, f = m.points[p][2][int(want["best_obs"][p])]
            sm2.desc[p] = sm.kfs[k].desc[f]
        if want["updated"][p]:
            sm2.normal[p], sm2.min_dist[p], sm2.max_dist[p] = want["normal"][p], want["min_distance"][p], want["max_distance"][p]
    assert (sm2.desc != sm.desc).any() and (sm2.normal != sm.normal).any()
    b = S.StoreScene(sm2)
    matcher = ORBmatcher(0.6, True, max_features=2048, max_queries=32768)
    ra, rb = a.call(matcher), b.call(matcher)
    stale = S.StoreScene(sm).call(matcher)
    matcher.close()
    for x, y, name in zip(ra, rb, ("fwd_best", "rev_point", "rev_best")):
        assert x.tobytes() == y.tobytes(), name
    assert any(x.tobytes() != y.tobytes() for x, y in zip(ra, stale)), "the refresh changed nothing the search reads: the test shows nothing"
    for sc in (a, b):
        sc.store.close()


# ---- 5. the refusals counted on the device ----
def small_store(m, skip_features=(), skip_centres=(), references=True):
    from rumi_slam_amd.covis import Covisibility
    s = Covisibility(m.n_kf, m.n_pts)
    m.set_keyframes(s, range(m.n_kf))
    m.set_features(s, [k for k in range(m.n_kf) if k not in skip_features])
    m.set_centres(s, [k for k in range(m.n_kf) if k not in skip_centres])
    m.set_points(s, range(m.n_pts), references=references)
    return s


def tiny_map(nfeat=3):
    rng = np.random.default_rng(9)
    kfs = [(rng.integers(0, 256, (nfeat, 32), dtype=np.uint8), rr.SF, rng.uniform(-4, 4, 3), k == 3) for k in range(5)]
    octs = [np.array([0, 3, 7][:nfeat], _i32)] * 5
    pts = [((0.5, 0.1, 6.0), 1, [(2, 0), (0, 1), (1, 2), (3, 0)]), ((1.0, -0.3, 5.0), 0, [(0, 0), (1, 1)]), ((0.0, 0.0, 4.0), -1, []),
           ((0.3, 0.2, 7.0), 4, [(2, 1), (0, 2)])]
    return rr.ResidentMap(kfs, octs, pts)


def refused(refresher, s, ids, what, word):
    from rumi_slam_amd.mapping import refresh_resident_outputs
    before = s.read_attributes(ids).copy()
    for flags in (0, REFRESH_WRITE_BACK):
        out = refresh_resident_outputs(len(ids), FILL)
        rc = refresher.status_resident(s, np.array(ids, _i32), what, flags, out)
        assert rc == capi.RUMI_E_INVALID and word in last_error() and "inconsistent among what the call reads" in last_error(), last_error()
        assert all(v.tobytes() == bytes([FILL]) * v.nbytes for v in out.values())
        assert s.read_attributes(ids, True).tobytes() == before.tobytes() and s.read_attributes(ids).tobytes() == before.tobytes()


def test_device_counted_refusals(oracle, refresher):
    m = tiny_map()
    ids = [0, 1, 2, 3]
    wants = {what: run_oracle(oracle, m.batch(), what, FILL) for what in MODES}
    s = small_store(m)
    check_equal(m, resident(refresher, s, ids, BOTH), wants[BOTH], BOTH)
    # an observer slot without resident features: slot 2 observes points 0 and 3; a bad observer's features are not read (slot 3)
    s.drop_keyframe_features([2, 3])
    refused(refresher, s, ids, REFRESH_DESCRIPTOR, "2 observers name a slot without resident features")
    check_equal(m, resident(refresher, s, ids, REFRESH_NORMAL_DEPTH), wants[REFRESH_NORMAL_DEPTH], REFRESH_NORMAL_DEPTH)       # the normal part reads no descriptor
    m.set_features(s, [2, 3])
    # an observer feature outside its slot's feature count: point 1 names feature 3 of slot 1, which holds three
    s.set_point_observations([1], [0], [[(0, 0), (1, 3)]])
    refused(refresher, s, ids, REFRESH_DESCRIPTOR, "1 observations name a feature outside")
    m.set_points(s, [1], attributes=False)
    # a reference without a centre (slot 4 observes nothing); an observer without one
    s.close()
    s = small_store(m, skip_centres=(4,))
    refused(refresher, s, ids, REFRESH_NORMAL_DEPTH, "1 observer or reference slots have no centre")
    check_equal(m, resident(refresher, s, ids, REFRESH_DESCRIPTOR), wants[REFRESH_DESCRIPTOR], REFRESH_DESCRIPTOR)
    s.close()
    s = small_store(m, skip_centres=(0,))
    refused(refresher, s, ids, BOTH, "4 observer or reference slots have no centre")            # three observations and one reference
    s.close()
    # no reference slot: never set, then cleared by -1; a point without observers needs none
    s = small_store(m, references=False)
    refused(refresher, s, ids, BOTH, "3 points with observers have no reference slot")
    refused(refresher, s, ids, REFRESH_DESCRIPTOR, "3 points with observers have no reference slot")
    m.set_points(s, ids, attributes=False)
    check_equal(m, resident(refresher, s, ids, BOTH), wants[BOTH], BOTH)
    s.set_point_reference([1, 2], [-1, -1])
    refused(refresher, s, ids, BOTH, "1 points with observers have no reference slot")
    s.set_point_reference([1], [0])
    # a reference slot without features
    s.drop_keyframe_features([4])
    refused(refresher, s, ids, BOTH, "1 reference slots hold no features")
    s.close()


def test_refused_edits_change_nothing_the_kernels_read(oracle, refresher):
    m = tiny_map()
    want = run_oracle(oracle, m.batch(), BOTH, FILL)
    s = small_store(m)
    assert s.set_keyframe_centres([0, 0], np.zeros((2, 3)), check=False) == capi.RUMI_E_INVALID
    assert s.set_keyframe_centres([0, 1], [[0, 0, 0], [np.inf, 0, 0]], check=False) == capi.RUMI_E_INVALID
    assert s.set_point_reference([0, 1], [2, 7], check=False) == capi.RUMI_E_INVALID
    check_equal(m, resident(refresher, s, [0, 1, 2, 3], BOTH), want, BOTH)
    s.close()


def test_upload_bytes_follow_what_changed(refresher):
    m = tiny_map()
    s = small_store(m)
    resident(refresher, s, [0, 1], BOTH)
    resident(refresher, s, [0, 1], BOTH)
    assert s.stats()["last_upload_bytes"] == 0                                                  # nothing staged, nothing sent
    s.set_keyframe_centres([1, 3], np.ones((2, 3)))
    resident(refresher, s, [0, 1], BOTH)
    assert s.stats()["last_upload_bytes"] == 2 * (16 + 16)                                      # a record and 16 bytes a key-frame
    s.set_point_reference([0, 1, 3], [0, 1, 2])
    resident(refresher, s, [0, 1], BOTH)
    assert s.stats()["last_upload_bytes"] == 3 * 16 + 16                                        # a record and a word a point, the payload rounded up to 16 bytes
    resident(refresher, s, [0, 1], BOTH)
    assert s.stats()["last_upload_bytes"] == 0
    s.close()


def test_track_local_map_reads_the_written_back_values(oracle, refresher):
    """After the write-back, rumi_track_local_map (UpdateLocalMap + TrackLocalMap in one call, what TrackLocalMapResident drives) on that store
    returns the bytes it returns on a fresh store whose attributes the host set from the oracle's values, with no
    rumi_covis_set_point_attributes in between."""
    from rumi_slam_amd.covis import Covisibility
    from rumi_slam_amd.matcher import FeatureVector, FrameView
    from test_localmap_gpu import one_call, tracked_frame
    f = tracked_frame()
    sc, w = f["sc"], f["sc"].world
    rng = np.random.default_rng(11)
    sf = np.asarray(f["sf"], np.float32)
    slots = sorted(w.kf)
    assert slots == list(range(len(slots)))
    # what every key-frame holds per entry of its map-point row: the point's descriptor with a few bits flipped, the octave the point's
    # distance range was made for, and a camera centre near the origin (the points lie on a plane in front of it)
    dist = np.linalg.norm(sc.pts["pos"], axis=1)
    level = np.clip(np.rint(np.log(sc.pts["max_dist"] / dist) / np.log(1.2)), 0, 7).astype(np.int32)
    kfs, octs = [], []
    for k in slots:
        mp = w.kf[k]["mp"]
        d = rng.integers(0, 256, (len(mp), 32), dtype=np.uint8)
        o = rng.integers(0, 8, len(mp)).astype(np.int32)
        for i, p in enumerate(mp):
            if p >= 0:
                r = int(sc.row_of_id[p])
                bits = np.unpackbits(sc.pts["desc"][r])
                bits[rng.choice(256, int(rng.integers(0, 9)), replace=False)] ^= 1
                d[i], o[i] = np.packbits(bits), level[r]
        kfs.append((d, sf, rng.uniform(-0.05, 0.05, 3).astype(np.float32), False))
        octs.append(o)
    obs = [[(k, w.kf[k]["mp"].index(int(sc.id_of_row[r]))) for k in w.pt[int(sc.id_of_row[r])]["obs"]] for r in range(sc.n0)]
    m = rr.ResidentMap(kfs, octs, [(sc.pts["pos"][r], obs[r][0][0] if obs[r] else -1, obs[r]) for r in range(sc.n0)])
    want = run_oracle(oracle, m.batch(), BOTH, FILL)
    ids = sc.id_of_row.astype(_i32)
    # the store under test: the scene's store, then what the refresh reads beside it, then one refresh with write-back
    a = sc.store()
    for k in slots:
        keys = np.zeros(len(octs[k]), capi.KP_DTYPE)
        keys["octave"] = octs[k]
        a.set_keyframe_features(k, FrameView(keys, kfs[k][0], 640, 480, sf), FeatureVector({}), rr.K4)
    a.set_keyframe_centres(slots, np.stack([kf[2] for kf in kfs]))
    a.set_point_observations(ids, sc.pts["bad"], obs)
    a.set_point_reference(ids, [p[1] for p in m.points])
    fp, disc = sc.ids(f["rows"]), sc.ids(f["discarded"])
    stale = one_call(f, a, fp, disc)
    got = resident(refresher, a, ids, BOTH, REFRESH_WRITE_BACK)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    ga = one_call(f, a, fp, disc)
    # the fresh store: the scene with the oracle's values in its attributes
    pts = {k: v.copy() for k, v in sc.pts.items()}
    for r in range(sc.n0):
        if want["best_obs"][r] >= 0:
            k, i = obs[r][int(want["best_obs"][r])]
            pts["desc"][r] = kfs[k][0][i]
        if want["updated"][r]:
            pts["normal"][r], pts["min_dist"][r], pts["max_dist"][r] = want["normal"][r], want["min_distance"][r], want["max_distance"][r]
    assert (pts["desc"] != sc.pts["desc"]).any() and (pts["normal"] != sc.pts["normal"]).any()
    b = sc.world.load(Covisibility(sc.world.max_kf, sc.max_points))
    sc.set_attributes(b, pts=pts)
    gb = one_call(f, b, fp, disc)
    same = lambda x, y: np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert sorted(ga) == sorted(gb)
    for k in ga:
        assert same(ga[k], gb[k]), k
    assert ga["nmatches_local"] > 20
    assert any(not same(ga[k], stale[k]) for k in ga), "the refresh changed nothing the tracker reads: the test shows nothing"
    a.close(); b.close()
