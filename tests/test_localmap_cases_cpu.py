"""The constructed cases of rumi_track_local_map (tests/test_localmap_gpu.py) without a GPU: the oracle chain covis_scene.oracle_local_map ->
the table rules of include/rumi_track.h written out in numpy (localmap_scene.host_table) -> test_track_steps_gpu._oracle_local must give
well-formed expectations, and every case must have the property it is there for (extras exist, a duplicate exists, a bad frame point
exists, the local list has exactly 63 / 64 / 65 points ...).  Also the host-side validation of rumi_covis_set_point_attributes."""
import numpy as np
import pytest

from covis_scene import build_oracle, oracle_local_map
from localmap_scene import LocalMapScene, cpu_source, seam_scene
from rumi_slam_amd.synth import warp_homography
from test_track_steps_gpu import _oracle_local, _oracle_motion
from test_tracking_loop_gpu import _homography, _pose_gt

SEAMS = (0, 1, 63, 64, 65, 257)
T0 = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("covis_oracle"))


@pytest.fixture(scope="module")
def frame():
    """One tracked frame from the CPU oracle: the scene, the frame's features, TrackWithMotionModel's vector (table rows) and its outliers."""
    import oracle_lib as O
    img0, sf, inv_sigma2, pts, last = cpu_source(n_keep=0.6)
    sc = LocalMapScene(pts)
    img = warp_homography(img0, _homography(*_pose_gt(2)))
    _, keys, desc = O.OracleExtractor(1000, 1.2, 8, 20, 7).extract(img)
    m = _oracle_motion(keys, desc, sf, inv_sigma2, T0, last, sc.pts)
    assert m["nmatches_motion"] >= 20
    return dict(sc=sc, keys=keys, desc=desc, sf=sf, inv_sigma2=inv_sigma2, rows=m["frame_mp"], T=m["Tcw_motion"],
                discarded=np.unique(m["discarded"][m["discarded"] >= 0]))


def chain(oracle, f, sc, frame_points, discarded_ids=(), th_local=1.0):
    lm = oracle_local_map(oracle, sc.world, frame_points)
    table, fin, seen, points = sc.host_table(lm["local_points"], frame_points, discarded_ids)
    r = _oracle_local(f["keys"], f["desc"], f["sf"], f["inv_sigma2"], f["T"], fin, seen, points, th_local)
    # well-formed: ids once, rows inside the table, a bad or NULL feature holds nothing, the frame keeps what it held
    assert len(set(table.tolist())) == len(table) and (table >= 0).all() and (table < sc.max_points).all()
    assert np.array_equal(table[:len(lm["local_points"])], lm["local_points"])
    assert r["frame_mp"].max(initial=-1) < len(table) and len(r["in_view"]) == len(table)
    held = fin >= 0
    assert not points["bad"][fin[held]].any()
    new = (r["frame_mp"] >= 0) & (r["frame_mp"] != fin)
    assert points["local"][r["frame_mp"][new]].all(), "the search only hands out local points"
    return lm, table, fin, seen, points, r


def test_the_scene_has_what_the_cases_need(oracle, frame):
    f, sc = frame, frame["sc"]
    fp = sc.ids(f["rows"])
    lm, table, fin, seen, points, r = chain(oracle, f, sc, fp, sc.ids(f["discarded"]))
    n_local = len(lm["local_points"])
    assert 2 <= len(lm["local_kf"]) <= 8 and n_local > 300
    assert lm["frame_point_bad"].sum() >= 1, "a bad frame point"
    assert (fin[lm["frame_point_bad"] != 0] == -1).all()
    assert len(table) > n_local, "extras exist"
    extras = table[n_local:]
    assert (sc.pts["obs"][sc.row_of_id[extras]] == 0).any(), "a point without observers among the extras"
    first = {}
    for i, p in enumerate(fp):
        if p >= 0:
            first.setdefault(int(p), i)
    frame_extras = [int(p) for p in extras if int(p) in first]
    assert frame_extras == sorted(frame_extras, key=first.get), "extras in order of first feature"
    assert not np.array_equal(sc.id_of_row[:50], np.arange(50)), "ids are not rows"
    assert r["nmatches_local"] > 20 and r["n_to_match"] > 50 and r["ngood_local"] > 50
    assert len(f["discarded"]) >= 1 and (seen != 0).sum() == len(f["discarded"])


@pytest.mark.parametrize("n_local", SEAMS)
def test_seam_cases_have_their_list_length(oracle, frame, n_local):
    f = frame
    sc = seam_scene(f["sc"].pts, f["rows"], n_local)
    fp = sc.ids(f["rows"]) if n_local else np.full(len(f["rows"]), -1, np.int32)
    lm, table, fin, seen, points, r = chain(oracle, f, sc, fp)
    assert len(lm["local_points"]) == n_local
    if n_local == 0:
        assert len(table) == 0 and (r["frame_mp"] == -1).all() and r["nmatches_local"] == 0 and r["ngood_local"] == 0
    else:
        assert len(table) > n_local + 100, "most of the frame's points are extras"


def test_extras_case(oracle, frame):
    f, sc = frame, frame["sc"]
    fp, lone = extras_frame(sc, f["rows"], oracle_local_map(oracle, sc.world, sc.ids(f["rows"]))["local_points"])
    lm, table, fin, seen, points, r = chain(oracle, f, sc, fp, [lone])
    n_local = len(lm["local_points"])
    vals, counts = np.unique(fp[fp >= 0], return_counts=True)
    dup = vals[counts > 1]
    assert len(dup) >= 1 and (table == dup[0]).sum() == 1 and not (lm["local_points"] == dup[0]).any(), "a point held by two features, an extra"
    assert table[-1] == lone and seen[-1] == 1 and points["local"][-1] == 0, "a discarded id without a row is appended"
    assert lm["frame_point_bad"].sum() >= 1 and len(table) > n_local + 1


def extras_frame(sc, rows, local_points):
    """The frame of the main case with one extra held by a second feature, and a discarded id that neither the frame nor the local list holds."""
    fp = sc.ids(rows).copy()
    local = set(int(p) for p in local_points)
    isbad = lambda p: bool(sc.pts["bad"][sc.row_of_id[p]])
    src = next(i for i, p in enumerate(fp) if p >= 0 and int(p) not in local and not isbad(int(p)))
    dst = next(i for i in range(len(fp) - 1, -1, -1) if fp[i] < 0)
    fp[dst] = fp[src]
    held = set(int(p) for p in fp if p >= 0)
    lone = next(int(sc.id_of_row[r]) for r in range(sc.n0) if int(sc.id_of_row[r]) not in local and int(sc.id_of_row[r]) not in held)
    return fp, lone


def test_set_point_attributes_validation():
    """Plain host code: refused edits leave the handle's state (and its staged upload) as it was."""
    from rumi_slam_amd import capi
    from rumi_slam_amd.covis import Covisibility
    h = Covisibility(4, 16)
    z3, z1, d = np.zeros((2, 3), np.float32), np.zeros(2, np.float32), np.zeros((2, 32), np.uint8)
    assert h.set_point_attributes([3, 5], z3, z3, z1, z1, d) == capi.RUMI_OK
    for ids in ([3, 3], [0, 16], [-1, 2]):
        assert h.set_point_attributes(ids, z3, z3, z1, z1, d, check=False) == capi.RUMI_E_INVALID
    assert h._lib.rumi_covis_set_point_attributes(h._h, 1, None, None, None, None, None, None) == capi.RUMI_E_INVALID
    assert h._lib.rumi_covis_set_point_attributes(h._h, -1, None, None, None, None, None, None) == capi.RUMI_E_INVALID
    assert h.set_point_attributes([], z3[:0], z3[:0], z1[:0], z1[:0], d[:0]) == capi.RUMI_OK
    assert len(h.stats()) == 7
    h.close()
