"""rumi_track_local_map (include/rumi_track.h): Tracking::UpdateLocalMap + TrackLocalMap in one call on a covisibility store that holds the map
points' attributes, the point table built by kernels.  Every comparison is with code that existed before the entry: the two-call path
Covisibility.local_map -> the table gathered on the host (localmap_scene.host_table) -> Tracker.local, which must agree bit for bit (the same
kernels on the same inputs), and the oracle chain of test_localmap_cases_cpu.py with the tolerances of test_track_steps_gpu.py."""
import numpy as np
import pytest

from covis_scene import build_oracle, oracle_local_map
from localmap_scene import LocalMapScene, seam_scene
from rumi_slam_amd.synth import warp_homography
from scene import K_TUM3
from test_localmap_cases_cpu import SEAMS, T0, extras_frame
from test_track_frame_gpu import H, W, _pose_close, _scene
from test_track_steps_gpu import _oracle_local
from test_tracking_loop_gpu import _homography, _pose_gt

pytestmark = pytest.mark.gpu
COUNTS = ("n", "n_to_match", "nmatches_local", "ngood_local", "matches_inliers")


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("covis_oracle"))


def tracked_frame(n_keep=0.6, edit=None):
    """A tracker with one frame resident and TrackWithMotionModel run on it: what UpdateLocalMap + TrackLocalMap start from."""
    from rumi_slam_amd.tracker import Tracker
    img0, sf, inv_sigma2, pts, last = _scene(n_keep=n_keep)
    if edit:
        edit(pts, last)
    sc = LocalMapScene(pts)
    trk = Tracker(1000, 1.2, 8, 20, 7, W, H, 4096)
    _, keys, desc = trk.extract(warp_homography(img0, _homography(*_pose_gt(2))))
    gm = trk.motion(K_TUM3, T0, last["keys"], last["mp"], last["outlier"], sc.pts)
    assert gm["nmatches_motion"] >= 20
    return dict(sc=sc, trk=trk, keys=keys, desc=desc, sf=sf, inv_sigma2=inv_sigma2, rows=gm["frame_mp"], T=gm["Tcw_motion"],
                discarded=np.unique(gm["discarded"][gm["discarded"] >= 0]), last=last)


@pytest.fixture(scope="module")
def frame():
    f = tracked_frame()
    f["cov"] = f["sc"].store()
    return f


def two_calls(f, cov, sc, fp, discarded_ids=(), th_local=1.0, pts=None, stale=None):
    """The path the entry replaces: the store's local map, the table gathered on the host, rumi_track_local."""
    lm = cov.local_map(fp)
    table, fin, seen, points = sc.host_table(lm["local_points"], fp, discarded_ids, pts, stale)
    r = f["trk"].local(K_TUM3, f["T"], fin, points, seen, th_local)
    return lm, table, fin, seen, points, r


def one_call(f, cov, fp, discarded_ids=(), th_local=1.0, stale=None):
    return f["trk"].local_map(cov, K_TUM3, f["T"], fp, discarded_ids, None if stale is None else stale[0], None if stale is None else stale[1], th_local)


def assert_same(got, lm, table, r, what):
    assert np.array_equal(got["local_kf"], lm["local_kf"]) and got["n_k1"] == lm["n_k1"] and got["ref_kf"] == lm["ref_kf"], f"{what}: local key-frames"
    assert np.array_equal(got["frame_point_bad"], lm["frame_point_bad"]), f"{what}: frame_point_bad"
    assert np.array_equal(got["local_points"], lm["local_points"]), f"{what}: local points"
    assert np.array_equal(got["table_ids"], table), f"{what}: table ids {len(got['table_ids'])} vs {len(table)}"
    for k in COUNTS:
        assert got[k] == r[k], f"{what}: {k} {got[k]} vs {r[k]}"
    ids = np.where(r["frame_mp"] >= 0, table[np.maximum(r["frame_mp"], 0)] if len(table) else -1, -1).astype(np.int32)
    assert np.array_equal(got["frame_mp"], ids), f"{what}: frame_mp"
    assert np.array_equal(got["outlier"], r["outlier"]) and np.array_equal(got["in_view"], r["in_view"]), f"{what}: flags"
    for k in ("Tcw", "Rcw", "tcw", "Ow"):
        assert got[k].tobytes() == r[k].tobytes(), f"{what}: {k} differs from the two-call path (the same kernels on the same inputs)"


@pytest.mark.parametrize("th_local", [1.0, 3.0])
def test_equals_the_two_call_path_and_the_oracle_chain(oracle, frame, th_local):
    f, sc, cov = frame, frame["sc"], frame["cov"]
    fp, disc = sc.ids(f["rows"]), sc.ids(f["discarded"])
    lm, table, fin, seen, points, r = two_calls(f, cov, sc, fp, disc, th_local)
    got = one_call(f, cov, fp, disc, th_local)
    assert_same(got, lm, table, r, f"th {th_local}")
    assert len(table) > len(lm["local_points"]) > 300 and lm["frame_point_bad"].sum() >= 1 and got["nmatches_local"] > 20
    # the oracle chain: indices and flags identical, the pose within the tolerance of the step-wise tests
    olm = oracle_local_map(oracle, sc.world, fp)
    otable, ofin, oseen, opoints = sc.host_table(olm["local_points"], fp, disc)
    ref = _oracle_local(f["keys"], f["desc"], f["sf"], f["inv_sigma2"], f["T"], ofin, oseen, opoints, th_local)
    assert np.array_equal(got["table_ids"], otable) and np.array_equal(got["local_kf"], olm["local_kf"]) and got["ref_kf"] == olm["ref_kf"]
    for k in COUNTS[1:]:
        assert got[k] == ref[k], f"oracle: {k} {got[k]} vs {ref[k]}"
    oids = np.where(ref["frame_mp"] >= 0, otable[np.maximum(ref["frame_mp"], 0)], -1)
    assert np.array_equal(got["frame_mp"], oids) and np.array_equal(got["outlier"], ref["outlier"]) and np.array_equal(got["in_view"], ref["in_view"])
    for k in ("Rcw", "tcw", "Ow"):
        assert np.array_equal(got[k], ref[k]), k
    _pose_close(got["Tcw"], ref["Tcw"], "pose after the local map")


@pytest.mark.parametrize("n_local", SEAMS)
def test_table_shapes_at_the_seams(frame, n_local):
    """Local lists of 0, 1, 63, 64, 65 and 257 points: the wave and workgroup boundaries of the prefix and of the gather."""
    f = frame
    sc = seam_scene(f["sc"].pts, f["rows"], n_local)
    cov = sc.store()
    fp = sc.ids(f["rows"]) if n_local else np.full(len(f["rows"]), -1, np.int32)
    lm, table, fin, seen, points, r = two_calls(f, cov, sc, fp)
    got = one_call(f, cov, fp)
    assert len(got["local_points"]) == n_local
    assert_same(got, lm, table, r, f"{n_local} local points")
    if n_local == 0:
        assert len(got["table_ids"]) == 0 and (got["frame_mp"] == -1).all() and got["nmatches_local"] == 0 and got["ngood_local"] == 0
        assert np.array_equal(got["Tcw"], f["T"])


def test_extras_duplicates_bad_points_and_an_appended_discarded_id(frame):
    f, sc, cov = frame, frame["sc"], frame["cov"]
    fp, lone = extras_frame(sc, f["rows"], cov.local_map(sc.ids(f["rows"]))["local_points"])
    lm, table, fin, seen, points, r = two_calls(f, cov, sc, fp, [lone])
    got = one_call(f, cov, fp, [lone])
    assert_same(got, lm, table, r, "extras")
    n_local, t = len(lm["local_points"]), got["table_ids"]
    assert len(set(t.tolist())) == len(t) and t[-1] == lone and len(t) > n_local + 1
    first = {}
    for i, p in enumerate(fp):
        if p >= 0:
            first.setdefault(int(p), i)
    extras = [int(p) for p in t[n_local:-1]]
    assert extras == sorted(extras, key=first.get) and not set(extras) & set(lm["local_points"].tolist()), "extras once each, in order of first feature"
    vals, counts = np.unique(fp[fp >= 0], return_counts=True)
    assert (t == vals[counts > 1][0]).sum() == 1, "a point held by two features has one row"
    badf = np.nonzero(lm["frame_point_bad"])[0]
    # (its feature enters the search as -1: it comes back empty or with a local point the search gave it, never with the bad point)
    assert len(badf) >= 1 and (fin[badf] == -1).all() and not np.isin(fp[badf], t).any() and not np.isin(fp[badf], got["frame_mp"]).any(), "a bad frame point has no row"


def test_discarded_outliers_with_stale_projections():
    """The scene of test_discarded_outliers_with_a_stale_in_view_flag_are_searched_at_their_old_projection through the sparse arguments."""
    rng = np.random.default_rng(11)

    def wrong_points(pts, last):
        wrong = rng.choice(np.nonzero(last["mp"] >= 0)[0], 40, replace=False)
        pts["pos"][wrong, :2] += rng.choice([-1, 1], (40, 2)) * rng.uniform(0.06, 0.09, (40, 2)).astype(np.float32)
    f = tracked_frame(0.6, wrong_points)
    sc, last = f["sc"], f["last"]
    n0 = sc.n0
    cov = sc.store()
    dist = np.linalg.norm(sc.pts["pos"], axis=1).astype(np.float32)
    stale_in = (rng.random(n0) < 0.7).astype(np.uint8)
    stale_proj = np.stack([last["keys"]["x"], last["keys"]["y"], last["keys"]["octave"].astype(np.float32), np.ones(n0, np.float32), dist], 1).astype(np.float32)
    rows = f["discarded"]
    fp, disc, stale = sc.ids(f["rows"]), sc.ids(rows), (stale_in[rows], stale_proj[rows])
    lm, table, fin, seen, points, r = two_calls(f, cov, sc, fp, disc, 3.0, stale=stale)
    got = one_call(f, cov, fp, disc, 3.0, stale)
    assert (r["in_view"] == 2).sum() >= 5, "the scene must discard points that carry the stale flag"
    assert_same(got, lm, table, r, "stale projections")
    plain = one_call(f, cov, fp, disc, 3.0)
    assert (plain["in_view"] == 2).sum() == 0, "without the flags the discarded points are not searched"


def test_attribute_edits_arrive(frame):
    f, sc = frame, frame["sc"]
    cov = sc.store()
    fp, disc = sc.ids(f["rows"]), sc.ids(f["discarded"])
    before = one_call(f, cov, fp, disc)
    searched = set(before["table_ids"][before["in_view"] == 1].tolist())
    moved = sc.row_of_id[[p for p in before["frame_mp"].tolist() if p in searched][:3]]          # three points the local search matched
    assert len(moved) == 3
    pts = dict(sc.pts, pos=sc.pts["pos"].copy(), desc=sc.pts["desc"].copy())
    pts["pos"][moved, :2] += np.float32(0.03)
    pts["desc"][moved] ^= np.uint8(0x5A)
    sc.set_attributes(cov, moved, pts)
    got = one_call(f, cov, fp, disc)
    uploaded = cov.stats()["last_upload_bytes"]
    assert uploaded < sc.max_points * 64, f"{uploaded} bytes for three records: the upload follows what changed"
    lm, table, fin, seen, points, r = two_calls(f, cov, sc, fp, disc, pts=pts)
    assert_same(got, lm, table, r, "after three edits")
    assert got["Tcw"].tobytes() != before["Tcw"].tobytes() or not np.array_equal(got["frame_mp"], before["frame_mp"]), "the edits change the result"


def test_refusals_leave_the_outputs_untouched(frame):
    from rumi_slam_amd import capi
    from rumi_slam_amd.tracker import Tracker
    f, sc = frame, frame["sc"]
    trk = f["trk"]
    fp, disc = sc.ids(f["rows"]), sc.ids(f["discarded"])
    lm0 = frame["cov"].local_map(fp)
    naked = int(sc.row_of_id[lm0["local_points"][5]])
    cov = sc.store(without_attributes=[naked])
    n, kf_cap, cap = len(fp), sc.world.max_kf, 4096
    untouched = lambda o: all(v.tobytes() == bytes([0x77]) * v.nbytes for v in o.values())
    out = Tracker.local_map_outputs(n, kf_cap, cap, 0x77)
    assert trk.local_map_into(cov, K_TUM3, f["T"], fp, out, kf_cap, cap, disc) == capi.RUMI_E_INVALID and untouched(out)
    assert b"1 local or frame point" in capi.lib().rumi_last_error()
    sc.set_attributes(cov, [naked])
    lm, table, fin, seen, points, r = two_calls(f, cov, sc, fp, disc)
    assert_same(one_call(f, cov, fp, disc), lm, table, r, "after the missing attributes were set")
    out = Tracker.local_map_outputs(n, kf_cap, len(table) - 1, 0x77)
    assert trk.local_map_into(cov, K_TUM3, f["T"], fp, out, kf_cap, len(table) - 1, disc) == capi.RUMI_E_CAPACITY and untouched(out)
    out = Tracker.local_map_outputs(n, len(lm["local_kf"]) - 1, cap, 0x77)
    assert trk.local_map_into(cov, K_TUM3, f["T"], fp, out, len(lm["local_kf"]) - 1, cap, disc) == capi.RUMI_E_CAPACITY and untouched(out)
    out = Tracker.local_map_outputs(n, kf_cap, len(table), 0x77)                   # exactly enough
    assert trk.local_map_into(cov, K_TUM3, f["T"], fp, out, kf_cap, len(table), disc) == capi.RUMI_OK and np.array_equal(out["table_ids"], table)
    empty = Tracker(1000, 1.2, 8, 20, 7, W, H, 4096)                              # no frame is resident
    out = Tracker.local_map_outputs(n, kf_cap, cap, 0x77)
    assert empty.local_map_into(cov, K_TUM3, f["T"], fp, out, kf_cap, cap, disc) == capi.RUMI_E_INVALID and untouched(out)
    assert_same(one_call(f, cov, fp, disc), lm, table, r, "after the refusals")


def test_last_projections_follow_the_new_entry(frame):
    f, sc, cov = frame, frame["sc"], frame["cov"]
    fp, disc = sc.ids(f["rows"]), sc.ids(f["discarded"])
    lm, table, fin, seen, points, r = two_calls(f, cov, sc, fp, disc)
    want = f["trk"].last_projections(len(table))
    got = one_call(f, cov, fp, disc)
    proj = f["trk"].last_projections(len(got["table_ids"]))
    assert proj.tobytes() == want.tobytes() and (got["in_view"] == 1).sum() > 50
