"""rumi_search_by_projection_sim3_resident (include/rumi_mapping.h): every SearchByProjection(KeyFrame*, Sim3f&, points, ...) job of a
place-recognition stage in one device call, on key-frames and points resident in the covisibility store.  The contract is bytes, per job:
the CPU oracle's loop (oracle_lib.search_by_projection_sim3 through tests/sim3_projection_scene.py) and rumi_search_by_projection_sim3 on the
same key-frame, pose and points, both from an all -1 vector.  tests/test_sim3_projection_batch_cpu.py shows that the scenes make the list
order matter."""
import numpy as np
import pytest

import search_and_fuse_scene as F
import search_in_neighbors_scene as S
import sim3_projection_scene as P
from rumi_slam_amd import capi

pytestmark = pytest.mark.gpu

MAX_FEATURES = 2048


@pytest.fixture(scope="module")
def matcher():
    from rumi_slam_amd.matcher import ORBmatcher
    m = ORBmatcher(0.8, True, max_features=MAX_FEATURES, max_queries=32768)
    yield m
    m.close()


def call(matcher, st, sc, jobs=None):
    from rumi_slam_amd.mapping import SearchByProjectionSim3Resident
    return SearchByProjectionSim3Resident(matcher, st.store, sc.job_array(jobs), sc.ids)


def check(matcher, sc, st=None, single=True):
    """The call against the oracle and against the single-job entry, job by job; returns (store scene, rows, counts)."""
    st = F.StoreScene(sc.m) if st is None else st
    rows, nm = call(matcher, st, sc)
    assert len(rows) == len(sc.jobs) and nm.dtype == np.int32
    for jj, j in enumerate(sc.jobs):
        n, row = P.oracle_job(sc, j)
        assert rows[jj].dtype == np.int32 and rows[jj].tobytes() == row.tobytes() and nm[jj] == n, ("oracle, job", jj, int(nm[jj]), n)
        if single:
            n1, row1 = P.single_job(matcher, st, sc, j)
            assert rows[jj].tobytes() == row1.tobytes() and nm[jj] == n1, ("rumi_search_by_projection_sim3, job", jj)
    return st, rows, nm


def took(matcher, sc, **kw):
    """Per entry of a one-job scene: the feature it holds."""
    _, rows, nm = check(matcher, sc, **kw)
    out = P.taken(rows[0], sc.jobs[0].count)
    assert nm[0] == (out >= 0).sum()
    return out.tolist()


# ---- 1. seeded scenes ----
@pytest.fixture(scope="module", params=P.SEEDS)
def seeded(request):
    m = P.seeded_map(request.param)
    return P.scenes(m, request.param), F.StoreScene(m)


@pytest.mark.parametrize("shape", ["one", "same_slot", "ten_slots", "overlap"])
def test_seeded(matcher, seeded, shape):
    scenes, st = seeded
    _, rows, nm = check(matcher, scenes[shape], st)
    assert all(200 <= len(r) <= 500 for r in rows) and (nm > 20).all()


def test_seeded_mixed_call_twice(matcher, seeded):
    from rumi_slam_amd.mapping import search_by_projection_sim3_rounds, search_by_projection_sim3_stage_ms
    scenes, st = seeded
    sc = scenes["mixed"]
    _, rows, nm = check(matcher, sc, st, single=False)
    rounds = search_by_projection_sim3_rounds(matcher, len(sc.jobs))
    assert (rounds >= 2).all() and rounds.max() >= 3, "a round past the first: some entry lost a feature to an earlier one"
    ms = search_by_projection_sim3_stage_ms(matcher)
    assert ms.shape == (3,) and (ms >= 0).all() and ms[1] > 0
    rows2, nm2 = call(matcher, st, sc)
    assert nm2.tobytes() == nm.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(rows, rows2)), "two calls, the same bytes"


# ---- 2. hand-made order cases ----
RNG = np.random.default_rng(78)
D = [RNG.integers(0, 256, 32, dtype=np.uint8) for _ in range(16)]


def test_cascade(matcher):
    from rumi_slam_amd.mapping import search_by_projection_sim3_rounds
    assert took(matcher, P.cascade(0)) == list(range(P.CASCADE))
    assert search_by_projection_sim3_rounds(matcher, 1).tolist() == [P.CASCADE + 1], "one entry settles per round, and a round that changes nothing"


@pytest.mark.parametrize("d0", [75, 76])
def test_cascade_whose_first_entry_sits_on_the_threshold(matcher, d0):
    """Entry 0 one bit above TH_LOW * 1.5 matches nothing and blocks nothing: every later entry keeps its first choice."""
    assert took(matcher, P.cascade(d0)) == (list(range(P.CASCADE)) if d0 == 75 else [-1] + list(range(P.CASCADE - 1)))


def test_second_choice_above_the_threshold(matcher):
    a = D[0]
    sc = P.window_scene([a, S.flip_bits(a, 1)], [a, S.flip_bits(a, 77)])
    assert P.hamming(sc.m.desc[1], sc.m.kfs[0].desc[1]) == 76
    assert took(matcher, sc) == [0, -1]


def test_tie_goes_to_the_first_in_area_order(matcher):
    """Feature 0 lies a cell column after feature 1; both are 10 bits from the point."""
    a = D[1]
    sc = P.window_scene([a], [P.flip(a, range(0, 10)), P.flip(a, range(10, 20))], xy=[[P.U0 + 5.0, P.V0], [P.U0 - 5.0, P.V0]])
    assert int(sc.m.kfs[0].keys["x"][0] // 10) == int(sc.m.kfs[0].keys["x"][1] // 10) + 1
    assert took(matcher, sc) == [1]


@pytest.mark.parametrize("th_ratio,bits,found", [(P.STAGE_A, 75, True), (P.STAGE_A, 76, False), (P.STAGE_B, 50, True), (P.STAGE_B, 51, False)])
def test_hamming_threshold(matcher, th_ratio, bits, found):
    sc = P.window_scene([D[2]], [S.flip_bits(D[2], bits)], th_ratio=th_ratio)
    assert took(matcher, sc) == [0 if found else -1]


def test_an_id_listed_twice_takes_two_features(matcher):
    sc = P.window_scene([D[3]], [S.flip_bits(D[3], 5), D[3]], ids=[0, 0])
    assert took(matcher, sc) == [1, 0]


def test_more_candidates_than_the_first_list_arena(matcher):
    """The implementation has no fixed number of slots a pair (count / allocate / fill); what it has is a first arena of 4 candidates a pair + 4096.
    150 entries x 150 in-threshold features = 22500 candidates outgrow 4 * 150 + 4096 = 4696: the lists are sized again and the call repeats
    its launches.  Every feature is contended by every entry."""
    sc = P.crowd()
    out = took(matcher, sc)
    assert sorted(out) == list(range(150))


# ---- 3. gates ----
def gate_scene(points, feats, ids=None, rows=None, th_ratio=P.STAGE_A, variant=0):
    m = P.tiny_map(points, [feats], ids=ids, rows=rows, pad_to=P.PAD)
    return P.Scene(m, m.ids, [P.Job(0, S.IDENT, 0, len(m.ids), th_ratio, variant)])


@pytest.mark.parametrize("variant", [0, 1])
def test_depth_must_not_be_negative(matcher, variant):
    front, behind = S.point_at(200.0, 150.0, 2, D[0]), S.point_at(400.0, 150.0, 2, D[1], z=-1.0)
    feats = ([[200.5, 150.0], [400.5, 150.0]], [2, 2], [D[0], D[1]])
    assert took(matcher, gate_scene([front, behind], feats, variant=variant)) == [0, -1]


def test_image_bounds(matcher):
    pts = [S.point_at(0.0, 240.0, 2, D[0]), S.point_at(640.0, 100.0, 4, D[1]), S.point_at(639.0, 300.0, 4, D[2]), S.point_at(320.0, 0.0, 2, D[3]),
           S.point_at(100.0, 480.0, 4, D[4])]
    px = [S.pixel_of(p["pos"]) for p in pts]
    assert px[0][0] == 0.0 and px[1][0] == 640.0 and px[3][1] == 0.0 and px[4][1] == 480.0, "the float projection lands on the bound exactly"
    feats = ([[1.0, 240.0], [634.99, 100.0], [634.99, 300.0], [320.0, 1.0], [100.0, 474.99]], [2, 4, 4, 2, 4], [D[0], D[1], D[2], D[3], D[4]])
    assert took(matcher, gate_scene(pts, feats)) == [0, -1, 2, 3, -1]


def test_distance_range(matcher):
    """dist3D against 0.8 * min and 1.2 * max, a part in a thousand on either side of each."""
    def at(u, v, lo, hi, d):
        p = S.point_at(u, v, 2, d)
        dist = np.sqrt((p["pos"][0] * p["pos"][0] + p["pos"][1] * p["pos"][1]) + p["pos"][2] * p["pos"][2], dtype=np.float32)
        if lo is not None:
            p["min_dist"] = float(dist) / 0.8 * lo
        if hi is not None:
            p["max_dist"], p["min_dist"] = float(dist) / 1.2 * hi, 0.01
        return p
    pts = [at(100.0, 100.0, 0.999, None, D[0]), at(200.0, 100.0, 1.001, None, D[1]), at(300.0, 100.0, None, 1.001, D[2]), at(400.0, 100.0, None, 0.999, D[3])]
    feats = ([[100.5, 100.0], [200.5, 100.0], [300.5, 100.0], [400.5, 100.0]], [2, 2, 0, 0], [D[0], D[1], D[2], D[3]])
    assert took(matcher, gate_scene(pts, feats)) == [0, -1, 2, -1]


def test_viewing_angle_on_its_boundary(matcher):
    def on_axis(z, c, d):
        p = S.point_at(320.0, 240.0, 2, d, z=z)
        p["normal"] = np.float32([np.sqrt(1.0 - float(c) ** 2), 0.0, c])
        return p
    pts = [on_axis(2.0, np.float32(0.5), D[0]), on_axis(4.0, np.nextafter(np.float32(0.5), np.float32(0.0)), D[1])]
    feats = ([[320.5, 240.0], [319.5, 240.0]], [2, 2], [D[0], D[1]])
    assert took(matcher, gate_scene(pts, feats)) == [0, -1]


def test_level_window(matcher):
    a = D[5]
    pts = [S.point_at(150.0, 150.0, 3, a)]
    xy = [[150.2, 150.0], [150.0, 150.2], [149.8, 150.0], [150.0, 149.8]]
    assert took(matcher, gate_scene(pts, (xy, [1, 2, 3, 4], [a, S.flip_bits(a, 12), S.flip_bits(a, 10), a]))) == [2]
    assert took(matcher, gate_scene(pts, (xy, [1, 2, 3, 4], [a, S.flip_bits(a, 10), S.flip_bits(a, 12), a]))) == [1]


def test_minus_one_bad_and_listed(matcher):
    """id -1 and a bad point are passed over; a point the key-frame already lists is NOT a gate: it matches."""
    pts = [S.point_at(100.0 + 60.0 * i, 120.0, 2, D[i]) for i in range(4)]
    feats = ([[100.5 + 60.0 * i, 120.0] for i in range(4)] + [[50.0, 400.0]], [2] * 5, D[:4] + [D[10]])
    sc = gate_scene(pts, feats, ids=[0, -1, 1, 2, 3], rows=[[-1, -1, -1, -1, 2]])
    sc.m.bad[1] = True
    assert took(matcher, sc) == [0, -1, -1, 2, 3]


# ---- 4. sizes ----
def sized(n_entries, n_feat_pad=P.PAD, n_jobs=1, empty_middle=False):
    """Lists of n_entries over four matching points; the last entry of a list of its length is the one that matches first for its point when the
    earlier entries for that point are -1."""
    pts = [S.point_at(80.0 + 90.0 * j, 200.0, 2, D[j]) for j in range(4)]
    feats = ([[80.5 + 90.0 * j, 200.0] for j in range(4)] + [[80.7 + 90.0 * j, 200.0] for j in range(4)], [2] * 8, D[:4] + [S.flip_bits(D[j], 3) for j in range(4)])
    ids = [(i % 5) - 1 for i in range(n_entries)]
    m = P.tiny_map(pts, [feats] * n_jobs, ids=ids, pad_to=n_feat_pad)
    jobs = [P.Job(k, S.IDENT, 0, 0 if (empty_middle and k == 1) else n_entries, P.STAGE_A, k & 1) for k in range(n_jobs)]
    return P.Scene(m, m.ids, jobs)


# 1024 / 1025: the resolve keeps an entry's state per thread of its 1024-thread workgroup (kS3pResolveThreads); 256 / 257: a gate workgroup
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1024, 1025, 2049])
def test_list_lengths(matcher, n):
    sc = sized(n)
    _, rows, nm = check(matcher, sc)
    if n >= 10:
        assert nm[0] == 8 and rows[0][:8].tolist() == [1, 2, 3, 4, 6, 7, 8, 9], "the first two entries of every point hold its two features"


def test_an_empty_list_between_two_that_are_not(matcher):
    _, rows, nm = check(matcher, sized(65, n_jobs=3, empty_middle=True))
    assert nm.tolist() == [8, 0, 8] and (rows[1] == -1).all()


@pytest.mark.parametrize("n_jobs", [1, 2, 11, 64])
def test_job_counts(matcher, n_jobs):
    _, rows, nm = check(matcher, sized(65, n_jobs=n_jobs), single=n_jobs <= 11)
    assert nm.tolist() == [8] * n_jobs


def test_key_frames_of_one_feature_and_of_max_features(matcher):
    pts = [S.point_at(80.0, 200.0, 2, D[0])]
    m = P.tiny_map(pts, [([[80.5, 200.0]], [2], [D[0]])], pad_to=1)
    one = P.Scene(m, m.ids, [P.Job(0, S.IDENT, 0, 1, P.STAGE_A, 0)])
    assert one.m.kfs[0].n == 1 and took(matcher, one) == [0]
    big = sized(65, n_feat_pad=MAX_FEATURES)
    assert big.m.kfs[0].n == MAX_FEATURES
    _, rows, nm = check(matcher, big)
    assert nm.tolist() == [8] and len(rows[0]) == MAX_FEATURES


# ---- 5. state ----
def test_staged_edits_are_seen(matcher, seeded):
    scenes, _ = seeded
    sc = scenes["same_slot"]
    st, rows, nm = check(matcher, sc, F.StoreScene(sc.m), single=False)
    j0 = sc.jobs[0]
    # a point matched by job 0 whose id no other job's range holds: ids before job 1's and job 2's starts
    lo = min(j.start for j in sc.jobs[1:])
    cand = [int(i) for i in rows[0][rows[0] >= 0] if i < lo and (sc.ids == sc.ids[j0.start + i]).sum() == 1]
    assert cand, "the scene has such an entry"
    p = int(sc.ids[j0.start + cand[0]])
    sc.m.bad[p] = True
    st.set_points([p])
    _, rows2, nm2 = check(matcher, sc, st, single=False)
    assert rows2[0].tobytes() != rows[0].tobytes() and cand[0] not in rows2[0].tolist()
    assert all(rows2[k].tobytes() == rows[k].tobytes() for k in (1, 2)) and nm2[1:].tolist() == nm[1:].tolist()
    sc.m.bad[p] = False


def test_staged_features_are_seen(matcher):
    """Between two calls the key-frame's features are staged again with the descriptor of the one matched feature replaced by a far one: the
    second call flushes them and the entry no longer matches."""
    from rumi_slam_amd.matcher import FrameView
    sc = P.window_scene([D[6]], [S.flip_bits(D[6], 4)])
    st = F.StoreScene(sc.m)
    assert took(matcher, sc, st=st) == [0]
    kf = sc.m.kfs[0]
    kf.desc[0] = S.flip_bits(D[6], 120)
    st.frames[0] = FrameView(kf.keys, kf.desc, S.W, S.H, S.SF)
    st.store.set_keyframe_features(S.slot_of(0), st.frames[0], st.fv, S.K4)
    assert took(matcher, sc, st=st) == [-1]


def test_a_call_without_work_resets_rounds_and_stage_times(matcher):
    from rumi_slam_amd.mapping import search_by_projection_sim3_rounds, search_by_projection_sim3_stage_ms
    sc = sized(65, n_jobs=2)
    st, _, _ = check(matcher, sc, single=False)
    assert search_by_projection_sim3_rounds(matcher, 2).min() >= 1
    sc.jobs[0].count = sc.jobs[1].count = 0
    _, rows, nm = check(matcher, sc, st, single=False)
    assert nm.tolist() == [0, 0] and search_by_projection_sim3_rounds(matcher, 2).tolist() == [0, 0]
    assert search_by_projection_sim3_stage_ms(matcher).tolist() == [0.0, 0.0, 0.0]


# ---- 6. refusals ----
class Refusals:
    def __init__(self, matcher):
        self.matcher = matcher
        self.m = F.seeded_map(35, n_corr=3, n_world=60, n_feat=70)
        self.st = F.StoreScene(self.m, max_points=self.m.n_points + 64)
        ids = np.asarray(self.m.ids, np.int32)
        c = self.m.corrected
        self.sc = P.Scene(self.m, ids, [P.Job(c[0], self.m.poses[c[0]], 0, len(ids), P.STAGE_A, 0), P.Job(c[1], self.m.poses[c[1]], 3, 20, P.STAGE_B, 1)])
        self.rows, self.start, self.nm = np.full(4096, -9, np.int32), np.full(700, -9, np.int32), np.full(700, -9, np.int32)

    def raw(self, jobs=None, ids=None, matcher="own", store=True, n_jobs=None, n_points=None, cap=4096, start=True, nm=True, untouched=True):
        from rumi_slam_amd import mapping
        jobs = self.sc.job_array() if jobs is None else jobs
        ids = np.ascontiguousarray(self.sc.ids if ids is None else ids, np.int32)
        mt = self.matcher if matcher == "own" else matcher
        rc = mapping._lib().rumi_search_by_projection_sim3_resident(mt._h if mt is not None else None, self.st.store._h if store else None, capi.ptr(jobs),
                                                                    len(jobs) if n_jobs is None else n_jobs, capi.ptr(ids),
                                                                    len(ids) if n_points is None else n_points, capi.ptr(self.rows), capi.ptr(self.start) if start else None,
                                                                    cap, capi.ptr(self.nm) if nm else None)
        msg = capi.lib().rumi_last_error().decode()
        if untouched:
            assert (self.rows == -9).all() and (self.start == -9).all() and (self.nm == -9).all(), "nothing written"
        return rc, msg


@pytest.fixture(scope="module")
def refusals(matcher):
    return Refusals(matcher)


@pytest.mark.parametrize("kw", [dict(matcher=None), dict(store=False), dict(start=False), dict(nm=False), dict(n_jobs=-1), dict(n_points=-1), dict(cap=-1)])
def test_refuses_missing_arguments(refusals, kw):
    rc, msg = refusals.raw(**kw)
    assert rc == capi.RUMI_E_INVALID and "rumi_search_by_projection_sim3_resident: missing argument" in msg


@pytest.mark.parametrize("field,value", [("th", 0), ("th", -3), ("ratio_hamming", 0.0), ("ratio_hamming", -1.0), ("ratio_hamming", float("nan")),
                                         ("ratio_hamming", float("inf"))])
def test_refuses_th_and_ratio(refusals, field, value):
    jobs = refusals.sc.job_array()
    jobs[field][1] = value
    rc, msg = refusals.raw(jobs=jobs)
    assert rc == capi.RUMI_E_INVALID and "th and ratio_hamming must be positive" in msg


@pytest.mark.parametrize("field,index", [("Tcw7", 5), ("Ow", 1), ("bounds", 2), ("log_scale_factor", None)])
def test_refuses_a_record_that_is_not_finite(refusals, field, index):
    jobs = refusals.sc.job_array()
    if index is None:
        jobs[field][1] = np.inf
    else:
        jobs[field][1][index] = np.nan
    rc, msg = refusals.raw(jobs=jobs)
    assert rc == capi.RUMI_E_INVALID and "not finite" in msg


def test_refuses_empty_bounds(refusals):
    jobs = refusals.sc.job_array()
    jobs["bounds"][0][2] = jobs["bounds"][0][0]
    rc, msg = refusals.raw(jobs=jobs)
    assert rc == capi.RUMI_E_INVALID and "empty image bounds" in msg


def test_refuses_a_slot_that_is_not_live(refusals):
    jobs = refusals.sc.job_array()
    jobs["kf_slot"][1] = 3
    rc, msg = refusals.raw(jobs=jobs)
    assert rc == capi.RUMI_E_INVALID and "a slot that is not live or holds no features" in msg


def test_refuses_a_slot_without_features(matcher):
    r = Refusals(matcher)
    r.st.store.drop_keyframe_features([S.slot_of(r.sc.jobs[1].k)])
    rc, msg = r.raw()
    assert rc == capi.RUMI_E_INVALID and "holds no features" in msg


@pytest.mark.parametrize("start,count", [(-1, 4), (0, -1), (5, None)])
def test_refuses_a_range_outside_the_ids(refusals, start, count):
    jobs = refusals.sc.job_array()
    jobs["point_start"][1], jobs["point_count"][1] = start, len(refusals.sc.ids) - 4 if count is None else count
    rc, msg = refusals.raw(jobs=jobs)
    assert rc == capi.RUMI_E_INVALID and "a list range outside [0, n_points]" in msg


def test_refuses_an_id_outside_the_store_and_a_point_without_attributes(refusals):
    cap = refusals.m.n_points + 64
    ids = refusals.sc.ids.copy()
    ids[7] = cap
    rc, msg = refusals.raw(ids=ids)
    assert rc == capi.RUMI_E_INVALID and "at or above the store's point capacity" in msg
    ids[7] = cap - 1                                          # the last id the tables hold: a point the store never saw; both jobs list it
    rc, msg = refusals.raw(ids=ids)
    assert rc == capi.RUMI_E_INVALID and "2 searched list entries whose map point has no attributes" in msg, msg


def test_refuses_what_exceeds_a_capacity(refusals):
    from rumi_slam_amd.matcher import ORBmatcher
    r = refusals
    rc, msg = r.raw(jobs=np.repeat(r.sc.job_array()[:1], 641))
    assert rc == capi.RUMI_E_CAPACITY and "RUMI_FUSE_MAX_TARGETS" in msg
    many = np.repeat(r.sc.job_array()[:1], 640)
    many["point_count"] = 2 ** 31 // 640 + 1
    rc, msg = r.raw(jobs=many, ids=np.zeros(2 ** 31 // 640 + 1, np.int32))
    assert rc == capi.RUMI_E_CAPACITY and "more (job, entry) pairs than a work item addresses" in msg
    small = ORBmatcher(0.8, True, max_features=64, max_queries=1024)
    try:
        rc, msg = r.raw(matcher=small)
        assert rc == capi.RUMI_E_CAPACITY and "exceeds the matcher's max_features" in msg
    finally:
        small.close()


def test_matched_cap_one_short_leaves_matched_start_valid(refusals):
    r = refusals
    total = sum(r.m.kfs[j.k].n for j in r.sc.jobs)
    rc, msg = r.raw(cap=total - 1, untouched=False)
    assert rc == capi.RUMI_E_CAPACITY and "matched_cap too small" in msg
    assert r.start[:3].tolist() == [0, r.m.kfs[r.sc.jobs[0].k].n, total] and (r.start[3:] == -9).all() and (r.rows == -9).all() and (r.nm == -9).all()
    rc, msg = r.raw(cap=total, untouched=False)
    assert rc == capi.RUMI_OK
    for jj, j in enumerate(r.sc.jobs):
        n, row = P.oracle_job(r.sc, j)
        assert r.rows[r.start[jj]:r.start[jj + 1]].tobytes() == row.tobytes() and r.nm[jj] == n
    r.rows[:], r.start[:], r.nm[:] = -9, -9, -9


def test_no_jobs_and_empty_lists_make_no_device_call(refusals):
    r = refusals
    rc, _ = r.raw(n_jobs=0, untouched=False)
    assert rc == capi.RUMI_OK and r.start[0] == 0 and (r.start[1:] == -9).all() and (r.rows == -9).all() and (r.nm == -9).all()
    jobs = r.sc.job_array()
    jobs["point_count"] = 0
    rc, _ = r.raw(jobs=jobs, untouched=False)
    n0, n1 = (r.m.kfs[j.k].n for j in r.sc.jobs)
    assert rc == capi.RUMI_OK and r.start[:3].tolist() == [0, n0, n0 + n1] and r.nm[:2].tolist() == [0, 0] and (r.rows[:n0 + n1] == -1).all()
    assert (r.rows[n0 + n1:] == -9).all()
    r.rows[:], r.start[:], r.nm[:] = -9, -9, -9


def test_refuses_another_device(refusals):
    """The store is bound to the device of its first consumer; a matcher on another device is refused.  Only a machine with two devices can
    ask for that; on one device there is no second matcher to make."""
    from rumi_slam_amd.matcher import ORBmatcher
    if capi.lib().rumi_device_count() < 2:
        pytest.skip("one device here: there is no matcher on another device to refuse")
    other = ORBmatcher(0.8, True, max_features=2048, max_queries=32768, device=1)
    try:
        rc, msg = refusals.raw(matcher=other)
        assert rc == capi.RUMI_E_INVALID and "different devices" in msg
    finally:
        other.close()
