"""The projecting kernels against the constructed gate cases of gate_cases.py: every entry that evaluates the gate chain equals the hand-written
expectation and the oracle.  Frustum cases run through the two callers of frustum_gate: k_is_in_frustum (matcher.isInFrustum,
ORBmatcher.SearchLocalPoints) and the tracker's frustum_body (Tracker.local + last_projections), each with its own skip branches and outputs;
search cases through every member's query builder (the RELOC member's gate, reloc_query, is also the relocalisation walk's); the sim3_query
cases also through the resident one-call entry."""
import numpy as np
import pytest

import gate_cases as G
import match_cases as MC
import oracle_lib as O
from test_gate_cases_cpu import check_frustum
from test_matcher_cases_cpu import check

pytestmark = pytest.mark.gpu

ENTRIES = ["MP_FUSED", "MP_FIELDS", "FRUSTUM", "RESIDENT"]


@pytest.fixture(scope="module")
def handles():
    """One matcher handle per member (and per extra entry) for the whole module."""
    from rumi_slam_amd import matcher as M
    hs = {m: M.ORBmatcher(0.8, False, max_features=1024, max_queries=1024) for m in G.SEARCH_MEMBERS + ENTRIES}
    yield M, hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def trackers():
    """One tracker with one extracted synthetic frame per camera: 640 x 480 without distortion (bounds 0, 0, 640, 480), and the 752 x 480 EuRoC
    camera, whose undistorted bounds the I family stands on."""
    from rumi_slam_amd.synth import synth_frame
    from rumi_slam_amd.tracker import Tracker
    plain = Tracker(1000, 1.2, 8, 20, 7, G.W, G.H, 64)
    plain.extract(synth_frame(4242))
    assert plain.undistorted()[1].tolist() == list(G.BOUNDS)
    euroc = Tracker(1000, 1.2, 8, 20, 7, 752, 480, 64)
    euroc.set_distortion(G.EUROC_K, G.EUROC_DIST)
    euroc.extract(synth_frame(321, w=752, h=480))
    assert euroc.undistorted()[1].tolist() == list(G.EUROC_BOUNDS)
    return {G.BOUNDS: plain, G.EUROC_BOUNDS: euroc}


FRUSTUM = G.frustum_cases()


def _frame(M, bounds):
    """A frame of one feature inside the bounds: SearchLocalPoints needs a grid to search."""
    keys = MC._keys([(bounds[0] + 20.0, bounds[1] + 20.0, 0, 0.0)])
    return M.FrameView(keys, np.zeros((1, 32), np.uint8), bounds[2], bounds[3], MC.SF, bounds[0], bounds[1])


def frustum_case(M, h, c):
    p, b = c.pose, c.bounds
    got = M.isInFrustum(h, p.R.ravel(), p.t, p.Ow, c.K, b[2], b[3], c.log_sf or MC.LOG_SF, 8, 0.5, c.pts, min_x=b[0], min_y=b[1])
    check_frustum(c, got, "isInFrustum")
    rows = np.nonzero(c.skip == 0)[0]
    ref = G.oracle_frustum(O, c)
    assert not G.same_bytes(got, ref, rows), f"{c.id}: kernel and oracle differ in {G.same_bytes(got, ref, rows)}"
    # the fused entry: the same kernel with the skip flags, its fields returned
    nto, nm, fm, fields = h.SearchLocalPoints(_frame(M, b), p.R.ravel(), p.t, p.Ow, c.K, c.log_sf or MC.LOG_SF, 8, G.pts_of(c), np.full(1, -1, np.int32), 1.0)
    check_frustum(c, fields, "SearchLocalPoints")
    assert nto == int(c.exp["track_in_view"].sum()), f"{c.id}: nToMatch {nto}"


@pytest.mark.parametrize("family", sorted({c.family for c in FRUSTUM}))
def test_frustum_kernel_equals_expected_and_oracle(handles, family):
    M, hs = handles
    for c in (c for c in FRUSTUM if c.family == family):
        frustum_case(M, hs["FRUSTUM"], c)


def tracker_case(trackers, c):
    trk = trackers[c.bounds]
    n, p = len(c.specs), c.pose
    r = trk.local(c.K, p.T7, np.full(trk.cap, -1, np.int32), G.pts_of(c))
    proj = trk.last_projections(n)
    got = dict(track_in_view=r["in_view"], proj_x=proj[:, 0], proj_y=proj[:, 1], scale_level=proj[:, 2].astype(np.int32), view_cos=proj[:, 3], track_depth=proj[:, 4])
    check_frustum(c, got, "Tracker.local")
    assert r["n_to_match"] == int(c.exp["track_in_view"].sum()), f"{c.id}: n_to_match {r['n_to_match']}"
    # Frame::UpdatePoseMatrices of the case's pose, exactly: Rcw, tcw and Ow = -R^T t
    assert np.array_equal(r["Rcw"].reshape(3, 3), p.R) and np.array_equal(r["tcw"], p.t) and np.array_equal(r["Ow"], p.Ow), f"{c.id}: pose matrices"


@pytest.mark.parametrize("family", sorted({c.family for c in FRUSTUM}))
def test_tracker_frustum_equals_expected(trackers, family):
    """frustum_body, the tracker's caller of frustum_gate: the fields through rumi_track_last_projections, the flags and n_to_match through rumi_track_local."""
    cases = [c for c in G.tracker_cases() if c.family == family]
    assert cases
    for c in cases:
        tracker_case(trackers, c)


@pytest.mark.parametrize("member", G.SEARCH_MEMBERS)
def test_search_kernel_equals_expected_and_oracle(handles, member):
    M, hs = handles
    h = hs[member]
    cases = G.member_cases(member)
    assert cases
    for c in cases:
        search_case(M, hs, c)


def search_case(M, hs, c):
    if c.member == "MP":                                        # the gates are live only in the fused entry
        return mappoint_case(M, hs, c)
    got = MC.call_gpu(M, hs[c.member], c)
    check(c, got, "kernel")
    ref = MC.call_oracle(O, c)
    assert got[0] == ref[0] and np.array_equal(got[1], ref[1]), f"{c.id}: kernel and oracle differ"


def mappoint_case(M, hs, c):
    """An MP case through the fused frustum + search entry (its fields too), and through the search alone on the expected fields."""
    i, sp = c.inp, c.spec
    h = hs["MP_FUSED"]
    h.mfNNratio = c.nnratio
    F = M.FrameView(i["keys"], i["desc"], i["w"], i["h"], MC.SF)
    state = np.full(len(i["keys"]), -1, np.int32)
    pts = dict(MC._pts(i, i["nq"]), obs=np.ones(i["nq"], np.int32))
    th, far, th_far = i["R"] / 4.0, bool(i.get("far", False)), float(i.get("th_far", 50.0))
    nto, nm, fm, fields = h.SearchLocalPoints(F, sp.pose.R.ravel(), sp.pose.t, sp.pose.Ow, MC.K4, MC.LOG_SF, 8, pts, state, th, far, th_far)
    bad = G.same_bytes(fields, c.fields)
    assert not bad, f"{c.id} ({c.cite}): the fused entry's fields differ in {bad}"
    check(c, (nm, fm), "fused entry")
    check(c, MC.call_gpu_fused(M, h, c), "fused entry through match_cases")
    ref = G.call_oracle(O, c)
    assert nm == ref[0] and np.array_equal(fm, ref[1]), f"{c.id}: kernel and oracle differ"
    # the search alone, given the expected fields (k_queries_mappoints -> mappoint_query)
    h2 = hs["MP_FIELDS"]
    h2.mfNNratio = c.nnratio
    check(c, h2.SearchByProjection_MapPoints(F, G.mp_from_fields(c), state, th, far, th_far), "SearchByProjection on the expected fields")


def resident_results(M, hs):
    """Every SIM3P case as one job of one rumi_search_by_projection_sim3_resident call: its key-frame in a slot of a covisibility store, its
    point among the store's points, its pose, th, ratio and overload in the job record.  Returns [(case, (nmatches, row))]."""
    from rumi_slam_amd.covis import Covisibility
    from rumi_slam_amd.mapping import SIM3_PROJ_JOB_DTYPE, SearchByProjectionSim3Resident, sim3_proj_job
    cases = G.sim3_query_cases()
    nk = len(cases)
    assert 0 < nk <= 640
    store = Covisibility(nk + 4, sum(c.inp["nq"] for c in cases) + 64)
    frames, fv = [], M.FeatureVector({})
    jobs, ids, start = np.zeros(nk, SIM3_PROJ_JOB_DTYPE), [], 0
    rows = [np.full(len(c.inp["keys"]), -1, np.int32) for c in cases]
    store.set_keyframes(list(range(nk)), [9000 + 13 * k for k in range(nk)], [0] * nk, [0] * nk, rows, [[]] * nk, [-1] * nk, [[]] * nk)
    for k, c in enumerate(cases):
        i = c.inp
        frames.append(M.FrameView(i["keys"], i["desc"], i["w"], i["h"], MC.SF))
        store.set_keyframe_features(k, frames[k], fv, MC.K4)
        pid = list(range(start, start + i["nq"]))
        store.set_point_observations(pid, np.zeros(len(pid), np.uint8), [[]] * len(pid))
        store.set_point_attributes(pid, i["pos"], i["normal"], i["min_dist"], i["max_dist"], i["qdesc"])
        jobs[k] = sim3_proj_job(k, i.get("Tcw7", MC.IDENT7), i.get("Ow", np.zeros(3, np.float32)), G.BOUNDS, MC.LOG_SF, start, i["nq"], i["R"], i["ratio_hamming"],
                                bool(i["variant"]))
        ids += pid
        start += i["nq"]
    got, nm = SearchByProjectionSim3Resident(hs["RESIDENT"], store, jobs, ids)
    store.close()
    return [(c, (int(nm[k]), got[k])) for k, c in enumerate(cases)]


def test_sim3_query_cases_through_the_resident_entry(handles):
    for c, got in resident_results(*handles):
        check(c, got, "resident entry")
