"""rumi_keyframe_culling (include/rumi_mapping.h) on the GPU against the C++ oracle (tests/cpp/culling_oracle.cc), which runs
LocalMapping::KeyFrameCulling / CloudKeyFrameCulling candidate by candidate on a mutable copy of the map, SetBadFlag side effects included.

Everything is compared bit for bit: the counts are integers and the verdict is one float multiply and one compare on both sides."""
import numpy as np
import pytest

from culling_scene import SCENES, CullScene, build_oracle, capacity_batch, probe_batch, run_oracle, same_bytes, small_batch
from rumi_slam_amd.mapping import CULL_ABORT_BA, CULL_CLOUD, CULL_CULLED, CULL_KEPT, REFRESH_MAX_OBS
from test_culling_cpu import check_validation

pytestmark = pytest.mark.gpu
FILL = 0xC3


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("culling"))


@pytest.fixture(scope="module", params=SCENES, ids=lambda s: f"scene{s[0]}-{s[1]}")
def scene(request):
    return CullScene(*request.param)


def device(batch, flags, culler=None, fill=FILL):
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import KeyFrameCuller
    own = culler is None
    culler = KeyFrameCuller() if own else culler
    out = batch.outputs(fill)
    capi.check(culler.status(batch, flags, out))
    if own:
        culler.close()
    return out


def describe(got, want):
    for k in want:
        diff = np.nonzero(got[k] != want[k])[0]
        print(f"{k}: {len(diff)} of {len(want[k])} entries differ" + (f", first {diff[0]}: {got[k][diff[0]]} vs {want[k][diff[0]]}" if len(diff) else ""))


@pytest.mark.parametrize("cloud", [False, True], ids=["plain", "cloud"])
def test_equals_oracle_bit_for_bit(oracle, scene, cloud):
    """Status, nMPs, nRedundant, the culled list and its length; what lies behind the list keeps its bytes on both sides."""
    b = scene.batch()
    want, got = run_oracle(oracle, b, scene.flags(cloud), FILL), device(b, scene.flags(cloud))
    describe(got, want)
    assert same_bytes(got, want) == []
    if b.n_cand:
        assert (got["status"][:b.n_cand] == CULL_KEPT).sum() > 5


def test_two_calls_same_bytes(scene):
    from rumi_slam_amd.mapping import KeyFrameCuller
    r = KeyFrameCuller()
    b = scene.batch()
    assert same_bytes(device(b, scene.flags(False), r), device(b, scene.flags(False), r)) == []
    r.close()


@pytest.mark.parametrize("cloud", [False, True], ids=["plain", "cloud"])
def test_permuted_tables_same_results(oracle, scene, cloud):
    """Another order of the points and of every observation list: the outputs are per candidate, and do not move -- on the device, and
    equal to the oracle run on the permuted tables themselves."""
    flags = scene.flags(cloud)
    base = device(scene.batch(), flags)
    order = np.random.default_rng(5).permutation(len(scene.points))
    for b in (scene.batch(order, shuffle_obs=9), scene.batch(None, shuffle_obs=10)):
        got = device(b, flags)
        assert same_bytes(got, base) == []
        assert same_bytes(got, run_oracle(oracle, b, flags, FILL)) == []


def test_handle_grows_and_shrinks(oracle):
    """One handle over calls of different size: its blocks grow and are reused."""
    from rumi_slam_amd.mapping import KeyFrameCuller
    r = KeyFrameCuller()
    for b, flags in ((small_batch(), 0), (CullScene(40, 110).batch(), 0), (CullScene(41, 12).batch(), CULL_CLOUD), (probe_batch(30, 400, (4, 15)), 0),
                     (small_batch(), CULL_ABORT_BA)):
        assert same_bytes(device(b, flags, r), run_oracle(oracle, b, flags, FILL)) == []
    r.close()


def test_probe_workload_culls(oracle):
    """The shape tools/culling_probe.py times, smaller: many culls in one loop."""
    b = probe_batch(40, 600, (4, 40), seed=3, n_rich=24)
    want, got = run_oracle(oracle, b, 0, FILL), device(b, 0)
    describe(got, want)
    assert same_bytes(got, want) == [] and got["n_culled"][0] >= 3


def test_max_obs_works(oracle):
    b = capacity_batch(REFRESH_MAX_OBS)
    assert same_bytes(device(b, 0), run_oracle(oracle, b, 0, FILL)) == []


def test_invalid_and_capacity_leave_outputs_untouched():
    check_validation(must_load=True)


def test_empty_candidate_list_is_ok():
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import CullBatch, KeyFrameCuller
    r = KeyFrameCuller()
    s = CullScene(3, 10)
    for b in (CullBatch([], [], []), CullBatch(s.keyframes(), [], [tuple(p) for p in s.points])):
        out = b.outputs(FILL)
        assert r.status(b, 0, out) == capi.RUMI_OK and out["n_culled"][0] == 0
        assert out["status"].tobytes() == bytes([FILL]) * 4
    r.close()


def test_public_mirror(oracle):
    from rumi_slam_amd.mapping import keyframe_culling
    s = CullScene(*SCENES[3])
    got = keyframe_culling(s.batch(), cloud=True)
    want = run_oracle(oracle, s.batch(), CULL_CLOUD)
    n = int(want["n_culled"][0])
    assert got["culled"].tolist() == want["culled"][:n].tolist() and n >= 1
    assert got["status"].tolist() == want["status"][:len(s.cand)].tolist() and CULL_CULLED in got["status"]
