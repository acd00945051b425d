"""rumi_local_ba_resident without a device: the plain-Python restatement of the reference's window (tests/lba_resident_cases.py) against the
hand-written expectations of every constructed scene, the preconditions that make each scene exercise its case, and the two new setters of the
covisibility store (rumi_covis_set_keyframe_poses, rumi_covis_set_point_maps), which validate and stage on the host."""
import math
import os
import re

import numpy as np
import pytest

import lba_resident_cases as LC
from rumi_slam_amd import capi
from rumi_slam_amd.covis import Covisibility

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def last_error():
    return capi.lib().rumi_last_error().decode()


def _declared(header):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(rumi_[a-z0-9_]+)\s*\(", hdr))


# ---- flatten against the hand-written lists ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LC.ALL))
def test_flatten_matches_the_expectations(name):
    c = LC.ALL[name]()
    w = LC.window(c["scene"], c["cur"], c["neigh"], c["init"])
    e = c["expect"]
    assert w["kf_slots"] == e["kf_slots"] and w["num_OptKF"] == e["num_OptKF"] and w["num_fixedKF"] == e["num_fixedKF"]
    assert w["mp_ids"] == e["mp_ids"]
    if e.get("aborted"):
        assert w["aborted"] and w["args"] is None and LC.flatten(c["scene"], c["cur"], c["neigh"], c["init"]) is None
        return
    kf_pose, kf_fixed, mp_pos, e_mp, e_kf, e_obs, e_w, K4 = w["args"]
    assert len(e_mp) == e["n_edges"] == len(w["edges"])
    assert w["edges"][:len(e.get("first_edges", []))] == e.get("first_edges", [])
    assert (np.diff(e_mp) >= 0).all(), "e_mp is grouped and ascending, as the reference builds it"
    assert kf_pose.shape == (len(e["kf_slots"]), 7) and kf_pose.dtype == np.float32 and mp_pos.shape == (len(e["mp_ids"]), 3)
    init_idx = e["kf_slots"].index(c["init"]) if c["init"] in e["kf_slots"][:e["num_OptKF"]] else -1
    assert kf_fixed.tolist() == [1 if (i >= e["num_OptKF"] or i == init_idx) else 0 for i in range(len(e["kf_slots"]))]
    for (s, p, f), i, k, o, wgt in zip(w["edges"], e_mp, e_kf, e_obs, e_w):
        kp = c["scene"].kfs[s]["keys"][f]
        assert e["mp_ids"][i] == p and e["kf_slots"][k] == s and o[0] == kp["x"] and o[1] == kp["y"]
        assert wgt == np.float32(1.0) / (LC.SF[kp["octave"]] * LC.SF[kp["octave"]])


# ---- each scene still exercises its case ---------------------------------------------------------------------------------------------------
def test_point_order_preconditions():
    c = LC.point_order()
    S = c["scene"]
    locals_ = [c["cur"]] + c["neigh"]
    assert S.kfs[locals_[0]]["row"][20] == 20 and S.kfs[locals_[2]]["row"][0] == 20           # feature 20 of the first row, feature 0 of the third
    assert c["expect"]["mp_ids"].index(20) < c["expect"]["mp_ids"].index(12)                   # listed where the first row has it
    twice = [p for p in S.kfs[2]["row"] if p >= 0 and p in S.kfs[0]["row"]]
    assert twice == [8, 9, 10, 11] and all(c["expect"]["mp_ids"].count(p) == 1 for p in twice)
    row = S.kfs[2]["row"]
    assert -1 in row[:12] and S.pts[row[5]]["bad"] and S.pts[row[7]]["map"] != S.kfs[2]["map"]
    assert row[5] not in c["expect"]["mp_ids"] and row[7] not in c["expect"]["mp_ids"]


def test_key_order_preconditions():
    c = LC.key_order()
    S = c["scene"]
    slots = sorted(S.kfs)
    assert all(S.kfs[a]["key"] > S.kfs[b]["key"] for a, b in zip(slots, slots[1:])), "keys descend while slots ascend"
    key_sorted = lambda p: sorted(S.pts[p]["obs"], key=lambda o: S.kfs[o[0]]["key"])
    assert sum(S.pts[p]["obs"] != key_sorted(p) for p in S.pts) > 30, "the observer rows are given shuffled"
    fixed = c["expect"]["kf_slots"][c["expect"]["num_OptKF"]:]
    assert fixed == [3, 4, 2] and fixed != sorted(fixed) and fixed != sorted(fixed, key=lambda s: S.kfs[s]["key"])
    # the second point's first outside observer in key order (4) is not its first in slot order (2)
    assert [s for s, _ in key_sorted(1) if s in (2, 4)] == [4, 2]
    seen0 = [s for s, _ in S.pts[0]["obs"]]
    assert 6 in seen0 and 7 in seen0 and S.kfs[6]["bad"] and S.kfs[7]["map"] != S.kfs[0]["map"]
    assert S.kfs[5]["bad"] and 5 in c["neigh"] and 5 in [s for s, _ in S.pts[1]["obs"]] and 5 not in c["expect"]["kf_slots"]
    w = LC.window(S, c["cur"], c["neigh"], c["init"])
    assert not any(s in (5, 6, 7) for s, _, _ in w["edges"])


def test_fixed_count_preconditions():
    a, b = LC.fixed_count(), LC.fixed_count(outside=False, init=-1)
    assert a["init"] in [a["cur"]] + a["neigh"] and a["expect"]["num_fixedKF"] == 1 + 1
    locals_b = set([b["cur"]] + b["neigh"])
    assert all(s in locals_b for P in b["scene"].pts.values() for s, _ in P["obs"]) and b["init"] == -1 and b["expect"]["aborted"]
    assert LC.fixed_count(outside=False)["expect"]["num_fixedKF"] == 1


@pytest.mark.parametrize("n_edges", [257, 513])
def test_seams_preconditions(n_edges):
    c = LC.seams(n_edges)
    S = c["scene"]
    w = LC.window(S, c["cur"], c["neigh"], c["init"])
    assert len(w["edges"]) == n_edges and n_edges % 256 == 1                     # one edge past a 256-entry border
    assert len(w["mp_ids"]) % 64 != 0
    per_point = np.bincount(w["args"][3])
    assert per_point[0] == 1 and per_point[1] == 72 > 64
    assert sum(len(S.kfs[s]["row"]) == 8 for s in w["kf_slots"]) == 70
    assert len(S.moved) >= 3 and all((s, p, f) in w["edges"] for s, f, p in S.moved)
    for s, f, p in S.moved:                                                      # 12 px at octave 0: chi2 = 144 at the true point, against 5.991
        assert S.kfs[s]["keys"]["octave"][f] == 0
    assert len(w["kf_slots"]) <= 512


def test_other_path_preconditions():
    c = LC.other_path()
    w = LC.window(c["scene"], c["cur"], c["neigh"], c["init"])
    assert int((w["args"][1] == 0).sum()) == 30 > 29, "one optimised key-frame more than the tile solver takes"


def test_refusal_scenes_preconditions():
    S = LC.point_order(mismatch=True)["scene"]
    assert (0, 2) in S.pts[3]["obs"] and S.kfs[0]["row"][2] != 3
    S = LC.point_order(with_map=False)["scene"]
    assert S.pts[0]["map"] is None and not S.pts[0]["bad"] and [s for s in (2, 0, 1) if 0 in S.kfs[s]["row"]] == [2]
    S = LC.point_order(fixed_pose=False)["scene"]
    assert not S.kfs[3]["has_pose"] and 3 in LC.point_order()["expect"]["kf_slots"]


# ---- the two setters ---------------------------------------------------------------------------------------------------------------------
def test_symbols_declared():
    covis, opt = _declared("rumi_covis.h"), _declared("rumi_opt.h")
    L = capi.covis_lib()
    for name in ("rumi_covis_set_keyframe_poses", "rumi_covis_set_point_maps"):
        assert name in covis and name in capi.COVIS_SYMBOLS
        getattr(L, name)
    assert "rumi_local_ba_resident" in opt and "rumi_local_ba_resident" in capi.OPT_SYMBOLS
    getattr(L, "rumi_local_ba_resident")
    assert "rumi_hook_covis_read_poses" in _declared("rumi_testhooks.h") and "rumi_hook_covis_read_poses" in capi.HOOK_SYMBOLS
    from rumi_slam_amd.optimizer import Optimizer
    assert callable(Optimizer.LocalBundleAdjustmentResident) and callable(Covisibility.set_keyframe_poses) and callable(Covisibility.set_point_maps)


@pytest.fixture
def store():
    s = Covisibility(16, 64)
    s.set_keyframes([2, 3, 4], [11, 12, 13], [0, 0, 0], [0, 0, 0], [[-1] * 8] * 3, [[]] * 3, [-1] * 3, [[]] * 3)
    yield s
    s.close()


def _staged(pose7):
    """What ba_stage_poses makes of seven floats on the host: w >= 0, normalised by 1 / sqrt(sum of squares) in double, a zero behind."""
    q = [float(v) for v in pose7[:4]]
    if q[3] < 0:
        q = [-v for v in q]
    rn = 1.0 / math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [v * rn for v in q] + [float(v) for v in pose7[4:]] + [0.0]


def test_poses_are_staged_as_the_solver_reads_them(store):
    T, has, _, _ = store.read_poses([2, 3, 4])
    assert not has.any() and not T.any()                                        # the table is null until first set
    P = np.float32([[0.1, -0.2, 0.3, 0.9, 1.5, -2.5, 3.25], [0.0, 0.0, 0.6, -0.8, 0.0, 1.0, 2.0]])
    store.set_keyframe_poses([4, 2], P)
    T, has, _, _ = store.read_poses([2, 3, 4])
    assert has.tolist() == [1, 0, 1]
    assert T[2].tolist() == _staged(P[0]) and T[0].tolist() == _staged(P[1]) and not T[1].any()
    assert T[0][3] > 0 and abs(np.linalg.norm(T[0][:4]) - 1) < 1e-15
    store.set_keyframe_poses([2], P[:1])                                        # setting again replaces
    assert store.read_poses([2])[0][0].tolist() == _staged(P[0])
    assert store.set_keyframe_poses([], np.zeros((0, 7), np.float32), check=False) == capi.RUMI_OK


def test_point_maps_are_staged(store):
    _, _, m, has = store.read_poses(ids=[0, 5, 63])
    assert not has.any()
    store.set_point_maps([5, 63], [3, -7])
    _, _, m, has = store.read_poses(ids=[0, 5, 63])
    assert has.tolist() == [0, 1, 1] and m[1:].tolist() == [3, -7]
    store.set_points([5], [1], [[2, 3]])                                        # observers set again: the point keeps its map
    store.set_point_observations([63], [0], [[(2, 1)]])
    _, _, m, has = store.read_poses(ids=[5, 63])
    assert has.tolist() == [1, 1] and m.tolist() == [3, -7]
    store.set_bad(pt_ids=[5], pt_bad=[0])
    assert store.read_poses(ids=[5])[3].tolist() == [1]


@pytest.mark.parametrize("slots,poses,code,msg", [
    ([2, 9], np.zeros((2, 7)) + [0, 0, 0, 1, 0, 0, 0], capi.RUMI_E_INVALID, "a slot that is not live, or named twice"),
    ([2, 2], np.zeros((2, 7)) + [0, 0, 0, 1, 0, 0, 0], capi.RUMI_E_INVALID, "a slot that is not live, or named twice"),
    ([16], np.zeros((1, 7)) + [0, 0, 0, 1, 0, 0, 0], capi.RUMI_E_INVALID, "a slot that is not live, or named twice"),
    ([-1], np.zeros((1, 7)) + [0, 0, 0, 1, 0, 0, 0], capi.RUMI_E_INVALID, "a slot that is not live, or named twice"),
    ([3, 2], np.array([[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, np.inf, 0]]), capi.RUMI_E_INVALID, "a pose that is not finite"),
    ([2], np.array([[np.nan, 0, 0, 1, 0, 0, 0]]), capi.RUMI_E_INVALID, "a pose that is not finite"),
])
def test_pose_refusals_change_nothing(store, slots, poses, code, msg):
    store.set_keyframe_poses([3], np.float32([[0, 0, 0, 1, 1, 2, 3]]))
    before = (store.read_poses([2, 3, 4]), store.stats())
    assert store.set_keyframe_poses(slots, np.float32(poses), check=False) == code
    assert last_error() == "rumi_covis_set_keyframe_poses: " + msg
    after = (store.read_poses([2, 3, 4]), store.stats())
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and before[1] == after[1]


@pytest.mark.parametrize("ids,code,msg", [([64], capi.RUMI_E_INVALID, "a point id outside 0..max_points-1, or named twice"),
                                          ([-1], capi.RUMI_E_INVALID, "a point id outside 0..max_points-1, or named twice"),
                                          ([7, 8, 7], capi.RUMI_E_INVALID, "a point id outside 0..max_points-1, or named twice")])
def test_point_map_refusals_change_nothing(store, ids, code, msg):
    store.set_point_maps([7], [1])
    before = store.read_poses(ids=[7, 8])
    assert store.set_point_maps(ids, [5] * len(ids), check=False) == code
    assert last_error() == "rumi_covis_set_point_maps: " + msg
    assert all(np.array_equal(a, b) for a, b in zip(before, store.read_poses(ids=[7, 8])))


def test_missing_arguments(store):
    L = capi.covis_lib()
    assert L.rumi_covis_set_keyframe_poses(store._h, 1, None, None) == capi.RUMI_E_INVALID
    assert last_error() == "rumi_covis_set_keyframe_poses: missing argument or negative count"
    assert L.rumi_covis_set_point_maps(store._h, -1, None, None) == capi.RUMI_E_INVALID
    assert last_error() == "rumi_covis_set_point_maps: missing argument or negative count"
    assert L.rumi_covis_set_point_maps(None, 0, None, None) == capi.RUMI_E_INVALID


def test_a_scene_loads_into_a_store_without_a_device():
    """to_store makes no device call: every setter it uses stages on the host."""
    c = LC.key_order()
    store = LC.to_store(c["scene"])
    try:
        T, has, m, hm = store.read_poses(sorted(c["scene"].kfs), sorted(c["scene"].pts))
        assert has.all() and hm.all() and not m.any()
        assert T[0].tolist() == _staged(c["scene"].kfs[0]["pose7"])
        row, _, _ = store.read_row(1)
        assert row.tolist() == c["scene"].kfs[1]["row"]
    finally:
        store.close()
