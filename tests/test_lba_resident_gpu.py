"""rumi_local_ba_resident (include/rumi_opt.h) on the GPU: the window assembled on the device from the covisibility store against
rumi_local_ba on the graph the reference builds from the same map (tests/lba_resident_cases.py: flatten), run on a second handle.

Everything is compared with np.array_equal, without a tolerance: the lists and counts are integer work, the raw block the solver starts from
holds the bytes the host path uploads, and the solver is the same code with a fixed order of every sum."""
import numpy as np
import pytest

import lba_resident_cases as LC
from rumi_slam_amd import capi

pytestmark = pytest.mark.gpu
FILL = 0xC3
TAIL = 40            # n_kf .. n_erased and stats[4]: the last ten words of RumiLbaResidentOut


def last_error():
    return capi.lib().rumi_last_error().decode()


@pytest.fixture(scope="module")
def opt():
    from rumi_slam_amd.optimizer import Optimizer
    o = Optimizer(max_kf=128)
    yield o
    o.close()


@pytest.fixture(scope="module")
def ref():
    from rumi_slam_amd.optimizer import Optimizer
    o = Optimizer(max_kf=128)
    yield o
    o.close()


def check_against_flatten(c, res, ref):
    """Lists, counts, poses, positions, stats and the erase list of one resident call against rumi_local_ba on the flatten."""
    w = LC.window(c["scene"], c["cur"], c["neigh"], c["init"])
    stats, kp, mp, erase = ref.LocalBundleAdjustment(*w["args"])
    assert res["status"] == capi.RUMI_OK
    assert res["kf_slots"].tolist() == w["kf_slots"] and res["num_OptKF"] == w["num_OptKF"] and res["num_fixedKF"] == w["num_fixedKF"]
    assert res["mp_ids"].tolist() == w["mp_ids"] and res["num_edges"] == len(w["edges"])
    assert np.array_equal(res["stats"], stats)
    assert np.array_equal(res["kf_pose7"].view(np.uint32), kp[:w["num_OptKF"]].view(np.uint32)), "poses of the local key-frames"
    assert np.array_equal(res["mp_pos3"].view(np.uint32), mp.view(np.uint32)), "positions"
    want = [w["edges"][e] for e in np.flatnonzero(erase)]
    assert res["erased"].tolist() == [list(t) for t in want], "the erase list is the mask's set bits in edge order"
    n = res["num_OptKF"]
    assert (res["raw"]["kf_pose7"][n * 7:].view(np.uint8) == FILL).all() and (res["raw"]["mp_ids"][len(w["mp_ids"]):].view(np.uint8) == FILL).all()
    return w, (stats, kp, mp, erase)


CASES = ["point_order", "key_order", "fixed_count", "fixed_count_init_only", "seams_257", "seams_513"]


@pytest.mark.parametrize("name", CASES)
def test_equals_local_ba_on_the_flatten(opt, ref, name):
    c = LC.ALL[name]()
    store = LC.to_store(c["scene"])
    try:
        res = opt.LocalBundleAdjustmentResident(store, c["cur"], c["neigh"], c["init"], fill=FILL)
        w, (stats, _, _, erase) = check_against_flatten(c, res, ref)
        assert stats[0] > 0 and stats[2] == int((w["args"][1] == 0).sum())
        if name.startswith("seams"):
            # which observations go is the solver's decision (a point with three observers can follow the one that was moved); that the list
            # is not empty and equals the mask's set bits is what this scene is for
            assert len(res["erased"]) > 0 and erase.any()
    finally:
        store.close()


def test_other_path(opt, ref):
    """Thirty optimised key-frames: the tile solver does not take the window, so it is assembled on the device, read back once and handed to the
    single-window host loop.  The branch for windows of more than 512 key-frames takes this same fallback (baw_eligible decides both) and is
    not constructed separately."""
    c = LC.other_path()
    store = LC.to_store(c["scene"])
    try:
        res = opt.LocalBundleAdjustmentResident(store, c["cur"], c["neigh"], c["init"], fill=FILL)
        _, (stats, _, _, _) = check_against_flatten(c, res, ref)
        assert stats[2] == 30
    finally:
        store.close()


def test_two_stores_same_bytes(opt):
    c = LC.key_order()
    out = []
    for _ in range(2):
        store = LC.to_store(c["scene"])
        try:
            r = opt.LocalBundleAdjustmentResident(store, c["cur"], c["neigh"], c["init"], fill=FILL)
            out.append((r["header"][-TAIL:], {k: v.tobytes() for k, v in r["raw"].items()}))
        finally:
            store.close()
    assert out[0] == out[1]


def test_held_to_the_oracle(opt):
    """One scene against g2o on the CPU (oracle_lib.local_ba) at the 1e-4 of test_optimizer_gpu._check_local_ba."""
    import oracle_lib as O
    from test_optimizer_gpu import _check_local_ba
    c = LC.fixed_count()
    store = LC.to_store(c["scene"])
    try:
        res = opt.LocalBundleAdjustmentResident(store, c["cur"], c["neigh"], c["init"])
    finally:
        store.close()
    w = LC.window(c["scene"], c["cur"], c["neigh"], c["init"])
    a = w["args"]
    kp = np.concatenate([res["kf_pose7"], a[0][res["num_OptKF"]:]])
    erase = np.zeros(len(w["edges"]), np.uint8)
    for t in res["erased"].tolist():
        erase[w["edges"].index(tuple(t))] = 1
    _check_local_ba(dict(kf_fixed=a[1], kf_pose=a[0]), (res["stats"], kp, res["mp_pos3"], erase), O.local_ba(*a))


def _device_state(store, c):
    ids, slots = sorted(c["scene"].pts), sorted(c["scene"].kfs)
    return store.read_attributes(ids, from_device=True).tobytes(), store.read_attributes(ids).tobytes(), [a.tobytes() for a in store.read_poses(slots, ids)]


def _untouched(res, written=0):
    """Nothing of `out` was written but the last `written` bytes (stats)."""
    tail = res["header"][-TAIL:]
    return tail[:TAIL - written] == bytes([FILL]) * (TAIL - written) and all((v.view(np.uint8) == FILL).all() for v in res["raw"].values())


def test_no_fixed_keyframe_and_stop_flag(opt):
    c = LC.fixed_count(outside=False, init=-1)
    store = LC.to_store(c["scene"])
    try:
        opt.LocalBundleAdjustmentResident(store, c["cur"], c["neigh"], 1, mp_cap=0, check=False)      # refused for capacity: binds and uploads the store
        before = _device_state(store, c)
        res = opt.LocalBundleAdjustmentResident(store, c["cur"], c["neigh"], -1, fill=FILL, check=False)
        assert res["status"] == capi.RUMI_E_INVALID and last_error() == "LM-LBA: There are 0 fixed KF in the optimizations, LBA aborted"
        assert _untouched(res) and _device_state(store, c) == before
        stop = np.array([1], np.uint8)
        res = opt.LocalBundleAdjustmentResident(store, c["cur"], c["neigh"], 1, stop_flag=stop, fill=FILL, check=False)
        assert res["status"] == capi.RUMI_OK and res["stats"].tolist() == [0, 0, 0, 1]
        assert _untouched(res, written=16) and _device_state(store, c) == before
    finally:
        store.close()


def test_capacities(opt):
    c = LC.point_order()
    store = LC.to_store(c["scene"])
    try:
        for kw in (dict(kf_cap=4), dict(mp_cap=17)):
            res = opt.LocalBundleAdjustmentResident(store, c["cur"], c["neigh"], c["init"], fill=FILL, check=False, **kw)
            assert res["status"] == capi.RUMI_E_CAPACITY and "kf_cap or mp_cap is too small" in last_error() and _untouched(res)
    finally:
        store.close()


@pytest.mark.parametrize("kw,count", [(dict(mismatch=True), "1 observations disagree with their slot's map-point row"),
                                      (dict(with_map=False), "1 points of local rows were never given a map"),
                                      (dict(fixed_pose=False), "18 key-frames or observations of the window have no pose")])
def test_refusals_name_counts(opt, kw, count):
    c = LC.point_order(**kw)
    store = LC.to_store(c["scene"])
    try:
        res = opt.LocalBundleAdjustmentResident(store, c["cur"], c["neigh"], c["init"], fill=FILL, check=False)
        assert res["status"] == capi.RUMI_E_INVALID
        msg = last_error()
        assert msg.startswith("rumi_local_ba_resident: the store is inconsistent among what the call reads: ") and count in msg
        others = [m for m in msg.split(": ", 2)[2].split(", ") if count not in m]
        assert all(m.startswith("0 ") or " 0 " in m for m in others), msg
        assert _untouched(res)
        ids = sorted(c["scene"].pts)
        assert np.array_equal(store.read_attributes(ids, from_device=True), store.read_attributes(ids))
    finally:
        store.close()


def test_store_on_another_device(opt):
    c = LC.point_order()
    store = LC.to_store(c["scene"], device=1)
    try:
        res = opt.LocalBundleAdjustmentResident(store, c["cur"], c["neigh"], c["init"], fill=FILL, check=False)
        assert res["status"] == capi.RUMI_E_INVALID and last_error() == "rumi_local_ba_resident: the store and the handle that reads it are on different devices"
        assert _untouched(res)
    finally:
        store.close()


def test_write_back(opt, ref):
    """After a call the store holds the results: a second call on the map with the erasures applied equals rumi_local_ba on the flatten of the
    updated scene, and the refresh by id reads the new positions where they lie."""
    from rumi_slam_amd.mapping import REFRESH_NORMAL_DEPTH, MapPointRefresher, RefreshBatch, RefreshMapPoints, RefreshMapPointsResident
    c = LC.seams(257)
    S = c["scene"]
    store = LC.to_store(S)
    refresher = MapPointRefresher()
    try:
        res = opt.LocalBundleAdjustmentResident(store, c["cur"], c["neigh"], c["init"])
        assert len(res["erased"]) >= 3
        ids = res["mp_ids"].tolist()
        # ---- the attribute records took the positions, on the device and in the mirror; the poses are staged as the setter would leave them
        for dev in (True, False):
            assert np.array_equal(store.read_attributes(ids, from_device=dev)[:, :12].copy().view(np.float32).view(np.uint32), res["mp_pos3"].view(np.uint32))
        n = res["num_OptKF"]
        twin = LC.to_store(S)
        try:
            twin.set_keyframe_poses(res["kf_slots"][:n], res["kf_pose7"])
            assert np.array_equal(store.read_poses(res["kf_slots"][:n])[0], twin.read_poses(res["kf_slots"][:n])[0])
        finally:
            twin.close()
        # ---- normal and depth by id against the block entry fed with the returned positions
        slots = sorted(S.kfs)
        index = {s: i for i, s in enumerate(slots)}
        kfs = [(np.zeros((len(S.kfs[s]["keys"]), 32), np.uint8), S.kfs[s]["sf"], LC.centre_of(S.kfs[s]["pose7"]), S.kfs[s]["bad"]) for s in slots]
        pts = []
        for i, p in enumerate(ids):
            rs, rf = S.pts[p]["obs"][0]
            pts.append((res["mp_pos3"][i], index[rs], rf, int(S.kfs[rs]["keys"]["octave"][rf]), [(index[s], f) for s, f in S.pts[p]["obs"]]))
        want = RefreshMapPoints(RefreshBatch(kfs, pts), REFRESH_NORMAL_DEPTH, refresher=refresher)
        got = RefreshMapPointsResident(refresher, store, ids, REFRESH_NORMAL_DEPTH, write_back=False)
        for k in ("normal", "min_distance", "max_distance", "updated"):
            assert np.array_equal(got[k], want[k]), k
        # ---- the erasures applied to the scene and the store, then the second window
        for k in range(n):
            S.kfs[int(res["kf_slots"][k])]["pose7"] = res["kf_pose7"][k].copy()
        for i, p in enumerate(ids):
            S.pts[p]["pos"] = res["mp_pos3"][i].copy()
        for s, p, f in res["erased"].tolist():
            assert S.kfs[s]["row"][f] == p
            S.kfs[s]["row"][f] = -1
            S.pts[p]["obs"].remove((s, f))
        LC.set_keyframes(store, S, sorted({s for s, _, _ in res["erased"].tolist()}))
        LC.set_points(store, S, sorted({p for _, p, _ in res["erased"].tolist()}))
        res2 = opt.LocalBundleAdjustmentResident(store, c["cur"], c["neigh"], c["init"], fill=FILL)
        w2, _ = check_against_flatten(c, res2, ref)
        assert len(w2["edges"]) == 257 - len(res["erased"])
    finally:
        refresher.close()
        store.close()
