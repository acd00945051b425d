"""The oracle of the map-point refresh (tests/cpp/refresh_oracle.cc) against plain numpy restatements of MapPoint::ComputeDistinctiveDescriptors
and MapPoint::UpdateNormalAndDepth, the coverage of the scenes (tests/refresh_scene.py), and the host-side validation of
rumi_refresh_map_points.  No GPU."""
import numpy as np
import pytest

from refresh_scene import CASE_COUNTS, MODES, SCENES, SF, RefreshScene, build_oracle, capacity_batch, run_oracle
from rumi_slam_amd.mapping import REFRESH_DESCRIPTOR, REFRESH_MAX_OBS, REFRESH_NORMAL_DEPTH

BOTH = REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("refresh"))


@pytest.fixture(scope="module", params=SCENES, ids=lambda s: f"scene{s[0]}")
def scene(request):
    return RefreshScene(*request.param)


def np_descriptor(s, point):
    """(best_obs, best_median, medians of every kept row) by unpackbits Hamming, np.sort, index (N-1)//2 and a strict-less loop."""
    obs = point[4]
    keep = [j for j, (k, f) in enumerate(obs) if not s.bad[k]]
    if not keep:
        return -1, -1, []
    bits = np.unpackbits(np.stack([s.desc[obs[j][0], obs[j][1]] for j in keep]), axis=1).astype(np.int32)
    n = len(keep)
    dist = (bits[:, None, :] != bits[None, :, :]).sum(2)
    medians = [int(np.sort(dist[i])[(n - 1) // 2]) for i in range(n)]
    best, idx = None, 0
    for i, m in enumerate(medians):
        if best is None or m < best:
            best, idx = m, i
    return keep[idx], best, medians


def np_normal(s, point):
    """(normal, min, max) in float32, in the operation order the header defines; None for a point without observations."""
    pos, ref_kf, _, ref_level, obs = point
    if not obs:
        return None
    f = np.float32

    def norm(d):
        return np.sqrt(f(f(f(d[0] * d[0]) + f(d[1] * d[1])) + f(d[2] * d[2])))
    acc = np.zeros(3, f)
    for k, _ in obs:
        d = (pos - s.Ow[k]).astype(f)
        nrm = norm(d)
        acc = (acc + (d / nrm).astype(f)).astype(f)
    dist = norm((pos - s.Ow[ref_kf]).astype(f))
    mx = f(dist * SF[ref_level])
    mn = f(mx / SF[len(SF) - 1])
    return (acc / f(len(obs))).astype(f), mn, mx


def test_oracle_descriptor_equals_numpy(oracle, scene):
    got = run_oracle(oracle, scene.batch(), REFRESH_DESCRIPTOR)
    for i, p in enumerate(scene.points):
        idx, med, _ = np_descriptor(scene, p)
        assert (int(got["best_obs"][i]), int(got["best_median"][i])) == (idx, med), i


def test_oracle_normal_depth_equals_numpy_bit_for_bit(oracle, scene):
    got = run_oracle(oracle, scene.batch(), REFRESH_NORMAL_DEPTH, fill=0xAB)
    untouched = np.full(3, 0xAB, np.uint8).tobytes() * 4
    for i, p in enumerate(scene.points):
        want = np_normal(scene, p)
        if want is None:
            assert got["updated"][i] == 0 and got["normal"][i].tobytes() == untouched
            continue
        assert got["updated"][i] == 1
        assert got["normal"][i].tobytes() == want[0].tobytes(), i
        assert got["min_distance"][i].tobytes() == want[1].tobytes() and got["max_distance"][i].tobytes() == want[2].tobytes(), i


def test_modes_write_only_their_outputs(oracle, scene):
    b = scene.batch()
    both = run_oracle(oracle, b, BOTH, fill=0x5A)
    blank = b.outputs(0x5A)
    d = run_oracle(oracle, b, REFRESH_DESCRIPTOR, fill=0x5A)
    n = run_oracle(oracle, b, REFRESH_NORMAL_DEPTH, fill=0x5A)
    for k in ("best_obs", "best_median"):
        assert d[k].tobytes() == both[k].tobytes() and n[k].tobytes() == blank[k][:b.n_pts].tobytes()
    for k in ("normal", "min_distance", "max_distance", "updated"):
        assert n[k].tobytes() == both[k].tobytes() and d[k].tobytes() == blank[k][:b.n_pts].tobytes()


def test_scene_coverage(scene):
    s = scene
    good_counts = [sum(not s.bad[k] for k, _ in p[4]) for p in s.points]
    for n in CASE_COUNTS:
        assert n in good_counts, n
    assert max(good_counts) >= 300
    assert max(good_counts) <= REFRESH_MAX_OBS
    # several rows tie for the best median through exact duplicates, with a worse row somewhere (so the choice is a choice)
    ties = 0
    for p in s.points:
        rows = [s.desc[k, f].tobytes() for k, f in p[4] if not s.bad[k]]
        if len(rows) > len(set(rows)):
            idx, med, medians = np_descriptor(s, p)
            ties += medians.count(med) > 1 and [k for k, _ in p[4] if not s.bad[k]][medians.index(med)] == p[4][idx][0]
    assert ties >= 4
    some_bad = [p for p in s.points if p[4] and 0 < sum(s.bad[k] for k, _ in p[4]) < len(p[4])]
    all_bad = [p for p in s.points if p[4] and all(s.bad[k] for k, _ in p[4])]
    assert len(some_bad) >= 4 and len(all_bad) >= 2
    # a dropped entry in front of the winner: best_obs counts the dropped entries
    assert any(np_descriptor(s, p)[0] > 0 and s.bad[p[4][0][0]] for p in some_bad)
    assert any(not p[4] for p in s.points)
    assert any(p[4] and s.bad[p[1]] for p in s.points)
    assert any(p[4] and p[1] not in [k for k, _ in p[4]] for p in s.points)
    assert any(any(a[0] > b[0] for a, b in zip(p[4], p[4][1:])) for p in s.points)
    for p in s.points:                                    # a key-frame observes a point once (std::map keys)
        assert len({k for k, _ in p[4]}) == len(p[4])


def test_all_bad_points_still_update_normal(oracle, scene):
    got = run_oracle(oracle, scene.batch(), BOTH)
    hit = [i for i, p in enumerate(scene.points) if p[4] and all(scene.bad[k] for k, _ in p[4])]
    assert hit and all(got["best_obs"][i] == -1 and got["updated"][i] == 1 for i in hit)


def _status(batch, what, out=None):
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import MapPointRefresher
    try:
        r = MapPointRefresher()
    except (OSError, RuntimeError) as e:
        pytest.skip(f"the library does not load here: {e}")
    out = batch.outputs(0x77) if out is None else out
    rc = r.status(batch, what, out)
    r.close()
    return rc, out


def malformed_batches():
    """(name, batch) with one defect each."""
    def fresh():
        return capacity_batch(6)
    out = []
    b = fresh(); b.obs_kf[2] = b.n_kf; out.append(("key-frame index past the table", b))
    b = fresh(); b.obs_kf[1] = -1; out.append(("negative key-frame index", b))
    b = fresh(); b.obs_feature[4] = 4; out.append(("feature index past its key-frame", b))
    b = fresh(); b.obs_feature[0] = -1; out.append(("negative feature index", b))
    b = fresh(); b.pts["ref_level"][0] = len(SF); out.append(("ref_level past the scale table", b))
    b = fresh(); b.pts["ref_level"][1] = -1; out.append(("negative ref_level", b))
    b = fresh(); b.pts["ref_kf"][0] = b.n_kf; out.append(("reference key-frame past the table", b))
    b = fresh(); b.pts["ref_feature"][1] = 4; out.append(("ref_feature past the reference key-frame", b))
    b = fresh(); b.pts["obs_end"][0] = b.n_obs + 1; out.append(("slice past n_obs", b))
    return out


def check_validation():
    """Shared with the GPU file: every malformed input is RUMI_E_INVALID and writes nothing; so is an unknown mode."""
    from rumi_slam_amd import capi
    for name, b in malformed_batches():
        for what in MODES:
            rc, out = _status(b, what)
            assert rc == capi.RUMI_E_INVALID, name
            assert all(v.tobytes() == bytes([0x77]) * v.nbytes for v in out.values()), name
    good = capacity_batch(6)
    for what in (0, 4, 7):
        assert _status(good, what)[0] == capi.RUMI_E_INVALID
    rc, out = _status(capacity_batch(REFRESH_MAX_OBS + 1), BOTH)
    assert rc == capi.RUMI_E_CAPACITY
    assert all(v.tobytes() == bytes([0x77]) * v.nbytes for v in out.values())


def test_host_side_validation():
    check_validation()
