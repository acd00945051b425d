"""The evolving map of the resident culling tests, checked on the CPU with the oracle alone (tests/cpp/culling_oracle.cc): the Python mirror
of SetBadFlag() leaves the map the oracle leaves, and the committed sequences show what the GPU tests rely on."""
import numpy as np
import pytest

import culling_resident_scene as rs
from culling_scene import build_oracle, run_oracle
from rumi_slam_amd.mapping import CULL_CULLED, CULL_KEPT, trim


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("culling_resident_oracle"))


def run_sequence(L, seed, n_kf, steps):
    """Per step: (candidates, the oracle's trimmed outputs on the evolved map, the same on the map as it was at the start, edits)."""
    sc, lists = rs.sequence(seed, n_kf, steps)
    m, m0 = rs.MapMirror.from_scene(sc), rs.MapMirror.from_scene(sc)
    out = []
    for step, cand in enumerate(lists):
        grown = rs.before_step(m, step)
        rs.before_step(m0, step)
        b = m.batch(cand)
        raw, st = run_oracle(L, b, 0, state=True)
        res = trim(b, raw)
        b0 = m0.batch(cand)
        res0 = trim(b0, run_oracle(L, b0, 0))
        bad_before = list(m.pt_bad)
        edits = m.apply(cand, res)
        out.append(dict(cand=cand, res=res, res0=res0, edits=edits, grown=grown, turned_bad=[p for p in range(m.n_pts) if m.pt_bad[p] and not bad_before[p]]))
        # the mirror leaves the oracle's map: bad key-frames and points, the observations of the live points, the rows of the live key-frames
        assert [bool(x) for x in st["kf_bad"][:m.n_kf]] == m.kf_bad and [bool(x) for x in st["pt_bad"][:m.n_pts]] == m.pt_bad
        assert all(st["pt_nobs"][p] == len(m.obs[p]) for p in range(m.n_pts) if not m.pt_bad[p])
        for k in range(m.n_kf):
            if not m.kf_bad[k]:
                assert np.array_equal(st["mp_after"][k], m.mp[k]), (seed, k)
        # and stays consistent: mp[k][f] == p exactly when p lists (k, f)
        listed = {(k, f): p for p in range(m.n_pts) for k, f in m.obs[p]}
        held = {(k, int(f)): int(m.mp[k][f]) for k in range(m.n_kf) for f in np.nonzero(m.mp[k] >= 0)[0]}
        assert listed == held
    return out


def test_committed_sequences_show_what_the_gpu_tests_need(oracle):
    steps_with_cull, turned_bad, flips = 0, 0, 0
    for seed, n_kf, steps in rs.SEQUENCES:
        assert len(steps) >= 3
        seq = run_sequence(oracle, seed, n_kf, steps)
        steps_with_cull += sum(len(s["res"]["culled"]) > 0 for s in seq)
        assert sum(len(s["res"]["culled"]) > 0 for s in seq) >= 2, "a cull in at least two steps of every sequence"
        turned_bad += sum(len(s["turned_bad"]) for s in seq)
        for s in seq[1:]:                                            # the same list on the untouched map: a different verdict is the edits' doing
            a, b = s["res"]["status"], s["res0"]["status"]
            flips += int(np.sum(((a == CULL_KEPT) & (b == CULL_CULLED)) | ((a == CULL_CULLED) & (b == CULL_KEPT))))
    assert steps_with_cull >= 2 and turned_bad > 0 and flips > 0, (steps_with_cull, turned_bad, flips)


def test_a_later_list_differs_from_the_first():
    for seed, n_kf, steps in rs.SEQUENCES:
        _, lists = rs.sequence(seed, n_kf, steps)
        assert len({tuple(c) for c in lists}) == len(lists)


def test_store_and_handle_on_different_devices_are_refused_before_either_binds():
    """Known without asking either device: the refusal is RUMI_E_INVALID, not the missing device of a machine without one (the twin of
    test_refresh_resident_cpu.test_resident_refusals_from_the_mirror's last case)."""
    from rumi_slam_amd import capi
    from rumi_slam_amd.covis import Covisibility
    from rumi_slam_amd.mapping import KeyFrameCuller, cull_outputs

    octv = np.zeros(3, np.int32)
    mp = [np.array([0, 1, -1], np.int32), np.array([0, -1, 1], np.int32), np.array([-1, 0, 1], np.int32), np.array([0, -1, -1], np.int32)]
    pts = [(False, 4, [(0, 0), (1, 0), (2, 1), (3, 0)]), (False, 3, [(0, 1), (1, 2), (2, 2)])]
    m = rs.MapMirror([(octv, r, False, False, False, False) for r in mp], pts)
    s = Covisibility(8, 16, arena_entries=256, device=1)
    m.load(s)
    cull = KeyFrameCuller(device=0)
    cands = m.candidates([2, 0, 1])
    out = cull_outputs(len(cands), 0x77)
    before = s.stats()
    rc = cull.status_resident(s, cands, 0, out)
    msg = capi.lib().rumi_last_error().decode()
    assert rc == capi.RUMI_E_INVALID and "different devices" in msg, (rc, msg)
    assert all(a.tobytes() == bytes([0x77]) * a.nbytes for a in out.values()), "a refused call writes nothing"
    assert s.stats() == before
    cull.close(); s.close()


def test_symbols_are_declared():
    from rumi_slam_amd import capi
    assert "rumi_keyframe_culling_resident" in capi.MAPPING_SYMBOLS and "rumi_covis_set_point_observations" in capi.COVIS_SYMBOLS
    for name in ("rumi_keyframe_culling_resident", "rumi_covis_set_point_observations"):
        getattr(capi.lib(), name)
