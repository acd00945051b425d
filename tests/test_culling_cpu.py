"""The oracle of the key-frame culling (tests/cpp/culling_oracle.cc) against an independent Python restatement of
LocalMapping::KeyFrameCulling / CloudKeyFrameCulling that mutates real objects (a dict of observations per point, a list of slots per
key-frame), the coverage of the committed scenes (tests/culling_scene.py), and the host-side validation of rumi_keyframe_culling.  No GPU."""
import numpy as np
import pytest

from culling_scene import SCENES, CullScene, build_oracle, capacity_batch, run_oracle, small_batch
from rumi_slam_amd.mapping import (CULL_ABORT_BA, CULL_CLOUD, CULL_CULLED, CULL_KEPT, CULL_NOT_REACHED, CULL_SKIPPED_BAD, CULL_SKIPPED_CLOUD,
                                   CULL_SKIPPED_INIT, CULL_TO_BE_ERASED, REFRESH_MAX_OBS)


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("culling"))


# ---- the restatement: objects, not arrays ----
class PyMapPoint:
    def __init__(self, bad, n_obs):
        self.bad, self.nObs, self.observations = bool(bad), int(n_obs), {}

    def erase_observation(self, kf):
        if kf in self.observations:
            del self.observations[kf]
            self.nObs -= 1
            if self.nObs <= 2:
                self.set_bad_flag()

    def set_bad_flag(self):
        self.bad = True
        obs, self.observations = self.observations, {}
        for kf, idx in obs.items():
            kf.slots[idx] = None


class PyKeyFrame:
    def __init__(self, octave, bad, init, not_erase, cloud):
        self.octave, self.slots = [int(o) for o in octave], [None] * len(octave)
        self.bad, self.init, self.not_erase, self.cloud, self.to_be_erased = bool(bad), bool(init), bool(not_erase), bool(cloud), False

    def set_bad_flag(self):
        if self.init:
            return
        if self.not_erase:
            self.to_be_erased = True
            return
        for mp in list(self.slots):
            if mp is not None:
                mp.erase_observation(self)
        self.bad = True


def py_world(s):
    kfs = [PyKeyFrame(s.octave[k], s.kf_bad[k], s.kf_init[k], s.not_erase[k], s.cloud[k]) for k in range(s.n_kf)]
    pts = []
    for bad, n, obs in s.points:
        p = PyMapPoint(bad, n)
        for k, f in obs:
            p.observations[kfs[k]] = f
            kfs[k].slots[f] = p
        pts.append(p)
    return kfs, pts


def py_culling(s, cloud, apply=True):
    """(status, nMPs, nRedundant per candidate, culled list, key-frames, points).  apply = False: no SetBadFlag is called, every verdict is
    the one an order-free evaluation gives."""
    kfs, pts = py_world(s)
    status, n_mps, n_red, culled = [CULL_NOT_REACHED] * len(s.cand), [0] * len(s.cand), [0] * len(s.cand), []
    count = 0
    for c, k in enumerate(s.cand):
        count += 1
        kf = kfs[k]
        if cloud and kf.cloud:
            status[c] = CULL_SKIPPED_CLOUD
            continue
        if kf.init or kf.bad:
            status[c] = CULL_SKIPPED_INIT if kf.init else CULL_SKIPPED_BAD
            continue
        for i, mp in enumerate(list(kf.slots)):
            if mp is None or mp.bad:
                continue
            n_mps[c] += 1
            if mp.nObs > 3:
                others = sum(1 for kfi, idx in mp.observations.items() if kfi is not kf and kfi.octave[idx] <= kf.octave[i] + 1)
                n_red[c] += others > 3
        status[c] = CULL_KEPT
        if np.float32(n_red[c]) > np.float32(0.9) * np.float32(n_mps[c]):
            if not apply:
                status[c] = CULL_TO_BE_ERASED if kf.not_erase else CULL_CULLED
            else:
                kf.set_bad_flag()
                status[c] = CULL_CULLED if kf.bad else CULL_TO_BE_ERASED
                if kf.bad:
                    culled.append(c)
        if (count > 20 and s.abort_ba) or count > 100:
            break
    return status, n_mps, n_red, culled, kfs, pts


def check_against_python(oracle, s, cloud):
    b = s.batch()
    out, st = run_oracle(oracle, b, s.flags(cloud), state=True)
    status, n_mps, n_red, culled, kfs, pts = py_culling(s, cloud)
    n = len(s.cand)
    assert out["status"][:n].tolist() == status and out["n_mps"][:n].tolist() == n_mps and out["n_redundant"][:n].tolist() == n_red
    assert out["culled"][:int(out["n_culled"][0])].tolist() == culled
    assert st["kf_bad"][:s.n_kf].tolist() == [int(k.bad) for k in kfs]
    assert st["kf_to_be_erased"][:s.n_kf].tolist() == [int(k.to_be_erased) for k in kfs]
    assert st["pt_bad"][:len(pts)].tolist() == [int(p.bad) for p in pts] and st["pt_nobs"][:len(pts)].tolist() == [p.nObs for p in pts]
    index = {id(p): i for i, p in enumerate(pts)}
    for k, kf in enumerate(kfs):
        assert st["mp_after"][k].tolist() == [-1 if m is None else index[id(m)] for m in kf.slots]
    for i, p in enumerate(pts):
        left = {(kfs.index(kf), f) for kf, f in p.observations.items()} if p.observations else set()
        o0 = int(b.pts["obs_begin"][i])
        assert {s.points[i][2][j] for j in range(len(s.points[i][2])) if st["obs_in_map"][o0 + j]} == left


@pytest.mark.parametrize("seed", range(50))
def test_oracle_equals_python_restatement(oracle, seed):
    s = CullScene(100 + seed, n_cand=(12, 24, 30, 104, 40)[seed % 5], abort_ba=seed % 3 == 1, nfeat=(40, 70))
    for cloud in (False, True):
        check_against_python(oracle, s, cloud)


@pytest.mark.parametrize("scene", SCENES, ids=lambda s: f"scene{s[0]}")
def test_oracle_equals_python_on_committed_scenes(oracle, scene):
    for cloud in (False, True):
        check_against_python(oracle, CullScene(*scene), cloud)


def scene_facts(s, cloud):
    """What a scene shows: flips against the order-free evaluation, statuses, the break taken."""
    seq, free = py_culling(s, cloud)[0], py_culling(s, cloud, apply=False)[0]
    facts = set()
    for a, f in zip(seq, free):
        if f == CULL_CULLED and a == CULL_KEPT:
            facts.add("culled->kept")
        if f == CULL_KEPT and a == CULL_CULLED:
            facts.add("kept->culled")
        facts.add(("status", a))
    reached = [c for c, a in enumerate(seq) if a != CULL_NOT_REACHED]
    if reached and reached[-1] + 1 < len(seq):
        facts.add("break>20" if s.abort_ba else "break>100")
        limit = 20 if s.abort_ba else 100
        if reached[-1] + 1 > limit + 1:
            facts.add("break behind a skipped candidate")
    return facts


def test_committed_seeds_cover_every_branch():
    """Between them the scenes of the GPU test show both flips, a to_be_erased, both breaks, every status, and the special points."""
    facts = set()
    for scene in SCENES:
        s = CullScene(*scene)
        for cloud in (False, True):
            facts |= scene_facts(s, cloud)
    for f in ("culled->kept", "kept->culled", "break>20", "break>100", "break behind a skipped candidate"):
        assert f in facts, f
    for st in (CULL_NOT_REACHED, CULL_SKIPPED_CLOUD, CULL_SKIPPED_INIT, CULL_SKIPPED_BAD, CULL_KEPT, CULL_CULLED, CULL_TO_BE_ERASED):
        assert ("status", st) in facts, st
    assert any(len(CullScene(*sc).cand) == 0 for sc in SCENES)
    assert any(len(CullScene(*sc).cand) > 100 for sc in SCENES)


@pytest.mark.parametrize("scene", [s for s in SCENES if s[1] > 0], ids=lambda s: f"scene{s[0]}")
def test_scene_contents(scene):
    s = CullScene(*scene)
    lens = [len(p[2]) for p in s.points]
    assert 3 in lens and 4 in lens and max(lens) >= 8
    assert all(p[1] == len(p[2]) for p in s.points)
    assert any(p[0] and p[2] for p in s.points)                                 # bad at the call
    cands = set(s.cand)
    assert any((s.mp[k] < 0).all() for k in cands)                             # nMPs = 0: `0 > 0` is false
    status, n_mps = py_culling(s, False)[:2]
    assert any(a == CULL_KEPT and n == 0 for a, n in zip(status, n_mps))
    deltas = set()                                                              # observers at own + 1 and own + 2
    for k in s.cand[:10]:
        for i, p in enumerate(s.mp[k]):
            if p >= 0:
                deltas |= {int(s.octave[kk][f]) - int(s.octave[k][i]) for kk, f in s.points[p][2] if kk != k}
    assert {1, 2} <= deltas
    for k in range(s.n_kf):                                                     # consistency, both ways
        for i, p in enumerate(s.mp[k]):
            assert p < 0 or (k, i) in s.points[p][2]
    for i, p in enumerate(s.points):
        assert all(s.mp[k][f] == i for k, f in p[2]) and len({k for k, _ in p[2]}) == len(p[2])
    assert any(any(a[0] > b[0] for a, b in zip(p[2], p[2][1:])) for p in s.points)             # lists not ascending in the index


def test_variants_differ(oracle):
    """The cloud variant leaves cloud key-frames alone; the plain one judges them."""
    seen = 0
    for scene in SCENES:
        s = CullScene(*scene)
        plain = run_oracle(oracle, s.batch(), s.flags(False))["status"]
        cloud = run_oracle(oracle, s.batch(), s.flags(True))["status"]
        for c, k in enumerate(s.cand):
            if s.cloud[k] and cloud[c] != CULL_NOT_REACHED:
                assert cloud[c] == CULL_SKIPPED_CLOUD
                seen += plain[c] in (CULL_KEPT, CULL_CULLED, CULL_TO_BE_ERASED)
    assert seen >= 3


# ---- validation ----
def _status(batch, flags, out=None, must_load=False):
    from rumi_slam_amd.mapping import KeyFrameCuller
    try:
        r = KeyFrameCuller()
    except (OSError, RuntimeError) as e:
        if must_load:
            raise
        pytest.skip(f"the library does not load here: {e}")
    out = batch.outputs(0x77) if out is None else out
    rc = r.status(batch, flags, out)
    r.close()
    return rc, out


def malformed_batches():
    """(name, batch) with one defect each."""
    out = []
    b = small_batch(); b.cand[1] = 4; out.append(("candidate past the table", b))
    b = small_batch(); b.cand[0] = -1; out.append(("negative candidate", b))
    b = small_batch(); b.obs_kf[2] = 4; out.append(("key-frame index past the table", b))
    b = small_batch(); b.obs_kf[1] = -1; out.append(("negative key-frame index", b))
    b = small_batch(); b.obs_feature[4] = 3; out.append(("feature index past its key-frame", b))
    b = small_batch(); b.obs_feature[0] = -1; out.append(("negative feature index", b))
    b = small_batch(); b.pts["obs_end"][1] = b.n_obs + 1; out.append(("slice past n_obs", b))
    b = small_batch(); b.pts["obs_begin"][0] = -1; out.append(("negative slice", b))
    b = small_batch(); b._keep[1][2] = 2; out.append(("mp past the point table", b))
    b = small_batch(); b._keep[1][2] = -2; out.append(("mp below -1", b))
    b = small_batch(); b._keep[1][2] = 1; out.append(("mp whose point does not list the pair", b))
    b = small_batch(); b._keep[1][0] = -1; out.append(("observation whose slot does not hold the point", b))
    b = small_batch(); b.obs_feature[1] = 1; out.append(("observation of a slot that holds nothing", b))
    b = small_batch(); b._keep[0][1] = 128; out.append(("octave above 127", b))
    b = small_batch(); b._keep[0][1] = -1; out.append(("negative octave", b))
    # a point that lists a key-frame twice: both slots hold it
    # the only defect: point 1 lists key-frame 3 twice, both slots hold it, and no other slot holds it without being listed
    b = small_batch(); b._keep[7][1:3] = 1; b._keep[3][2] = -1; b._keep[5][2] = -1; b.obs_kf[5:7] = 3; b.obs_feature[5:7] = (1, 2)
    out.append(("a point that lists a key-frame twice", b))
    return out


def check_validation(must_load=False):
    """Shared with the GPU file (must_load: a library that does not load is an error there, not a skip): every malformed input is RUMI_E_INVALID and writes nothing; so is an unknown flag; a point above the cap is
    RUMI_E_CAPACITY and writes nothing."""
    from rumi_slam_amd import capi
    for name, b in malformed_batches():
        for flags in (0, CULL_CLOUD | CULL_ABORT_BA):
            rc, out = _status(b, flags, must_load=must_load)
            assert rc == capi.RUMI_E_INVALID, name
            assert all(v.tobytes() == bytes([0x77]) * v.nbytes for v in out.values()), name
    for flags in (4, -1):
        assert _status(small_batch(), flags, must_load=must_load)[0] == capi.RUMI_E_INVALID
    rc, out = _status(capacity_batch(REFRESH_MAX_OBS + 1), 0, must_load=must_load)
    assert rc == capi.RUMI_E_CAPACITY
    assert all(v.tobytes() == bytes([0x77]) * v.nbytes for v in out.values())


def test_host_side_validation():
    check_validation()


def test_small_batch_is_well_formed(oracle):
    """The base of the malformed inputs passes the oracle and the restatement's consistency rules."""
    b = small_batch()
    out = run_oracle(oracle, b, 0)
    assert out["status"][:3].tolist() == [CULL_KEPT] * 3
