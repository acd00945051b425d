"""rumi_refresh_map_points (include/rumi_mapping.h) on the GPU against the C++ oracle (tests/cpp/refresh_oracle.cc), which runs
MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth point by point as the reference writes them.

Everything is compared bit for bit, without a tolerance: the descriptor part is integer, and the float part has no transcendental function and
a fixed operation order with correctly rounded division and square root on both sides."""
import numpy as np
import pytest

from refresh_scene import MODES, SCENES, RefreshScene, build_oracle, capacity_batch, run_oracle, same_bytes
from rumi_slam_amd.mapping import REFRESH_DESCRIPTOR, REFRESH_MAX_OBS, REFRESH_NORMAL_DEPTH
from test_refresh_cpu import check_validation

pytestmark = pytest.mark.gpu
BOTH = REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH
FILL = 0xC3


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("refresh"))


@pytest.fixture(scope="module", params=SCENES, ids=lambda s: f"scene{s[0]}")
def scene(request):
    return RefreshScene(*request.param)


def device(batch, what, fill=FILL):
    from rumi_slam_amd.mapping import RefreshMapPoints
    return RefreshMapPoints(batch, what, out=batch.outputs(fill))


def describe(got, want):
    for k in want:
        diff = np.nonzero((got[k].reshape(len(got[k]), -1).view(np.uint8) != want[k].reshape(len(want[k]), -1).view(np.uint8)).any(axis=1))[0]
        print(f"{k}: {len(diff)} of {len(want[k])} entries differ" + (f", first {diff[0]}: {got[k][diff[0]]} vs {want[k][diff[0]]}" if len(diff) else ""))


@pytest.mark.parametrize("what", MODES)
def test_equals_oracle_bit_for_bit(oracle, scene, what):
    """Every output of the modes asked for equals the oracle's, and the arrays of a mode not asked for keep their bytes (the oracle starts
    from the same fill and does not touch them either)."""
    b = scene.batch()
    want, got = run_oracle(oracle, b, what, FILL), device(b, what)
    describe(got, want)
    assert same_bytes(got, want) == []
    if what & REFRESH_DESCRIPTOR:
        assert (got["best_obs"] >= 0).sum() > 100 and (got["best_obs"] == -1).sum() >= 3
    if what & REFRESH_NORMAL_DEPTH:
        assert got["updated"].sum() == len(got["updated"]) - 1


def test_unasked_outputs_untouched(scene):
    b = scene.batch()
    blank = {k: v[:b.n_pts] for k, v in b.outputs(FILL).items()}
    assert same_bytes(device(b, REFRESH_DESCRIPTOR), blank, ("normal", "min_distance", "max_distance", "updated")) == []
    assert same_bytes(device(b, REFRESH_NORMAL_DEPTH), blank, ("best_obs", "best_median")) == []
    assert same_bytes(device(b, REFRESH_DESCRIPTOR), blank, ("best_obs", "best_median")) != []


def test_two_runs_same_bytes(scene):
    b = scene.batch()
    assert same_bytes(device(b, BOTH), device(b, BOTH)) == []


def test_shuffled_batch_same_results(oracle, scene):
    base = device(scene.batch(), BOTH)
    order = np.random.default_rng(5).permutation(len(scene.points))
    got = device(scene.batch(order), BOTH)
    for k in base:
        assert got[k].tobytes() == base[k][order].tobytes(), k


def test_max_obs_works(oracle):
    b = capacity_batch(REFRESH_MAX_OBS)
    want, got = run_oracle(oracle, b, BOTH, FILL), device(b, BOTH)
    describe(got, want)
    assert same_bytes(got, want) == [] and got["best_obs"][0] >= 0


def test_above_max_obs_is_capacity_and_writes_nothing():
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import MapPointRefresher
    b = capacity_batch(REFRESH_MAX_OBS + 1)
    r = MapPointRefresher()
    for what in MODES:
        out = b.outputs(FILL)
        assert r.status(b, what, out) == capi.RUMI_E_CAPACITY
        assert all(v.tobytes() == bytes([FILL]) * v.nbytes for v in out.values())
    r.close()


def test_empty_batch_is_ok():
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import MapPointRefresher, RefreshBatch
    r = MapPointRefresher()
    one_kf = [(np.zeros((4, 32), np.uint8), np.ones(8, np.float32), np.zeros(3, np.float32), False)]
    for b in (RefreshBatch([], []), RefreshBatch(one_kf, [])):
        for what in MODES:
            assert r.status(b, what, b.outputs(FILL)) == capi.RUMI_OK
    r.close()


def test_validation_on_the_device_box():
    check_validation()


def test_handle_reuse_growing_and_shrinking(oracle):
    """One handle over batches of different sizes: its blocks grow and are reused."""
    from rumi_slam_amd.mapping import MapPointRefresher, RefreshMapPoints
    r = MapPointRefresher()
    for b in (capacity_batch(5), capacity_batch(700), capacity_batch(66), capacity_batch(17)):
        got = RefreshMapPoints(b, BOTH, refresher=r, out=b.outputs(FILL))
        assert same_bytes(got, run_oracle(oracle, b, BOTH, FILL)) == []
    r.close()
