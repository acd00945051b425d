"""The oracle of the covisibility store (tests/cpp/covis_oracle.cc) against an independent Python restatement of KeyFrame::UpdateConnections
and Tracking::UpdateLocalKeyFrames / UpdateLocalPoints that mutates real objects (a dict of observations per point, dicts walked in key
order, lists, sets), the constructed scenes of tests/covis_scene.py with what each must show, and the host-side validation of the rumi_covis_*
entries where no device is touched.  No GPU."""
import numpy as np
import pytest

from covis_scene import (LM_EXPECTED_POINTS, World, build_oracle, differing, edit_sequence, lm_scenes, oracle_connections, oracle_local_map, random_world,
                         uc_scenes)
from rumi_slam_amd.covis import CONNECTED, EMPTY, MAX_KEYFRAMES

UC = uc_scenes()
LM = lm_scenes()


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("covis"))


# ---- the restatement: objects, not arrays ----
class PyKF:
    def __init__(self, slot, d):
        self.slot, self.key, self.map, self.bad = slot, d["key"], d["map"], d["bad"]
        self.points, self.best, self.parent, self.children = [], [], None, set()
        self.stamp = None

    def __lt__(self, other):                                             # pointer order
        return self.key < other.key


class PyMP:
    def __init__(self, pid, bad):
        self.pid, self.bad, self.observations, self.stamp = pid, bad, {}, None


def py_world(w):
    kfs = {s: PyKF(s, d) for s, d in w.kf.items()}
    pts = {p: PyMP(p, d["bad"]) for p, d in w.pt.items()}
    for p in range(w.max_points):
        pts.setdefault(p, PyMP(p, False))
    for s, d in w.kf.items():
        kfs[s].points = [None if p < 0 else pts[p] for p in d["mp"]]
        kfs[s].best = [kfs[b] for b in d["best"]]
        kfs[s].parent = kfs[d["parent"]] if d["parent"] >= 0 else None
        kfs[s].children = {kfs[c] for c in d["children"]}
    for p, d in w.pt.items():
        for k in d["obs"]:
            pts[p].observations[kfs[k]] = 0
    return kfs, pts


def py_update_connections(kfs, self_kf):
    """(status, KFcounter as [(slot, n)], ordered as [(slot, w)])"""
    counter = {}
    for mp in self_kf.points:
        if mp is None or mp.bad:
            continue
        for kf in sorted(mp.observations):
            if kf.slot == self_kf.slot or kf.bad or kf.map != self_kf.map:
                continue
            counter[kf] = counter.get(kf, 0) + 1
    if not counter:
        return EMPTY, [], []
    nmax, kmax, pairs = 0, None, []
    for kf in sorted(counter):
        if counter[kf] > nmax:
            nmax, kmax = counter[kf], kf
        if counter[kf] >= 15:
            pairs.append((counter[kf], kf))
    if not pairs:
        pairs.append((nmax, kmax))
    pairs.sort(key=lambda t: (t[0], t[1].key))
    kfl, wl = [], []
    for wgt, kf in pairs:
        kfl.insert(0, kf); wl.insert(0, wgt)
    return CONNECTED, [(kf.slot, counter[kf]) for kf in sorted(counter)], [(kf.slot, x) for kf, x in zip(kfl, wl)]


def py_local_map(kfs, pts, frame, frame_id):
    counter = {}
    frame = [None if p < 0 else pts[p] for p in frame]
    nulled = [0] * len(frame)
    for i, mp in enumerate(frame):
        if mp is None:
            continue
        if not mp.bad:
            for kf in mp.observations:
                counter[kf] = counter.get(kf, 0) + 1
        else:
            frame[i] = None
            nulled[i] = 1
    mx, kmax, local = 0, None, []
    for kf in sorted(counter):
        if kf.bad:
            continue
        if counter[kf] > mx:
            mx, kmax = counter[kf], kf
        local.append(kf)
        kf.stamp = frame_id
    k1 = len(local)
    for m in range(k1):
        if len(local) > 80:
            break
        kf = local[m]
        for nb in kf.best[:10]:
            if not nb.bad and nb.stamp != frame_id:
                local.append(nb); nb.stamp = frame_id
                break
        for ch in sorted(kf.children):
            if not ch.bad and ch.stamp != frame_id:
                local.append(ch); ch.stamp = frame_id
                break
        if kf.parent is not None and kf.parent.stamp != frame_id:
            local.append(kf.parent); kf.parent.stamp = frame_id
            break
    points = []
    for kf in reversed(local):
        for mp in kf.points:
            if mp is None or mp.stamp == frame_id:
                continue
            if not mp.bad:
                points.append(mp); mp.stamp = frame_id
    return dict(frame_point_bad=np.array(nulled, np.uint8), local_kf=np.array([k.slot for k in local], np.int32), n_k1=k1,
                ref_kf=-1 if kmax is None else kmax.slot, local_points=np.array([p.pid for p in points], np.int32))


def check_uc(oracle, w, batch):
    o = oracle_connections(oracle, w, batch)
    kfs, _ = py_world(w)
    for b, s in enumerate(batch):
        st, conn, ordl = py_update_connections(kfs, kfs[s])
        assert int(o["status"][b]) == st
        c0, c1, o0, o1 = o["conn_off"][b], o["conn_off"][b + 1], o["ord_off"][b], o["ord_off"][b + 1]
        assert list(zip(o["conn_slot"][c0:c1].tolist(), o["conn_count"][c0:c1].tolist())) == conn
        assert list(zip(o["ord_slot"][o0:o1].tolist(), o["ord_weight"][o0:o1].tolist())) == ordl
    return o


def check_lm(oracle, w, frames):
    kfs, pts = py_world(w)
    outs = []
    for fid, frame in enumerate(frames):
        o = oracle_local_map(oracle, w, frame)
        assert differing(o, py_local_map(kfs, pts, frame, fid + 1)) == []
        outs.append(o)
    return outs


@pytest.mark.parametrize("seed", range(50))
def test_oracle_equals_python_restatement(oracle, seed):
    w, frames = random_world(100 + seed, (8, 20, 33, 50, 90)[seed % 5], nfeat=((30, 50), (60, 90))[seed % 2], n_frames=3)
    rng = np.random.default_rng(seed)
    check_uc(oracle, w, [int(s) for s in rng.choice(sorted(w.kf), min(len(w.kf), 12), replace=False)])
    check_lm(oracle, w, frames)


@pytest.mark.parametrize("scene", UC, ids=[s[0] for s in UC])
def test_oracle_equals_python_on_connection_scenes(oracle, scene):
    check_uc(oracle, scene[1], scene[2])


@pytest.mark.parametrize("scene", LM, ids=[s[0] for s in LM])
def test_oracle_equals_python_on_local_map_scenes(oracle, scene):
    name, w, frames, expect = scene
    outs = check_lm(oracle, w, frames)
    if expect is not None:
        assert outs[0]["local_kf"].tolist() == expect
    if name in LM_EXPECTED_POINTS:
        assert outs[0]["local_points"].tolist() == LM_EXPECTED_POINTS[name]


def test_random_worlds_reach_the_threshold(oracle):
    """The random maps are not all below 15: some lists are thresholded, some fall back to the single maximum."""
    thresholded = single = 0
    for seed in range(10):
        w, _ = random_world(100 + seed, 33, nfeat=(60, 90))
        o = oracle_connections(oracle, w, sorted(w.kf))
        for b in range(len(w.kf)):
            ws = o["ord_weight"][o["ord_off"][b]:o["ord_off"][b + 1]]
            thresholded += len(ws) > 1 and ws.min() >= 15
            single += len(ws) == 1 and ws[0] < 15
    assert thresholded >= 20 and single >= 5


def test_connection_scenes_show_what_they_are_for(oracle):
    by = {s[0]: s for s in UC}

    def run(name):
        _, w, batch = by[name]
        return w, batch, oracle_connections(oracle, w, batch)

    def entry(o, b):
        return (o["conn_slot"][o["conn_off"][b]:o["conn_off"][b + 1]].tolist(), o["conn_count"][o["conn_off"][b]:o["conn_off"][b + 1]].tolist(),
                o["ord_slot"][o["ord_off"][b]:o["ord_off"][b + 1]].tolist(), o["ord_weight"][o["ord_off"][b]:o["ord_off"][b + 1]].tolist())

    w, batch, o = run("empty")
    assert o["status"].tolist() == [EMPTY, EMPTY] and len(w.kf[1]["mp"]) == 0 and o["conn_off"][-1] == 0 and o["ord_off"][-1] == 0
    _, _, o = run("14_and_15")
    assert sorted(entry(o, 0)[1]) == [2, 14, 15] and entry(o, 0)[2:] == ([1], [15])
    _, _, o = run("tie_at_max_below_th")
    assert entry(o, 0) == ([2, 4, 3, 1], [5, 5, 5, 3], [2], [5])          # key order 2, 4, 3, 1; the first of the tied wins
    _, _, o = run("three_equal_weights")
    assert entry(o, 0)[2:] == ([4, 2, 1, 3, 5], [20, 16, 16, 16, 15])     # keys 9, 3, 1 descending among the 16s
    w, _, o = run("filters_and_bad_point")
    assert entry(o, 0)[:2] == ([4, 1], [16, 16]) and o["status"].tolist() == [CONNECTED, EMPTY]
    w, _, o = run("300_observers")
    rest = [s for s in range(1, 301) if s not in (7, 9)]                  # key = 1000 - slot: descending key is ascending slot
    assert entry(o, 0)[2:] == ([7, 9] + rest, [21, 21] + [20] * 298)
    assert entry(o, 1) == ([9, 7, 0], [1, 1, 1], [9], [1])
    w, batch, o = run("row_seams")
    assert [len(w.kf[s]["mp"]) for s in batch] == [1, 63, 64, 65, 255, 256, 257]
    w2 = w.copy(); w2.kf[6]["mp"] = w2.kf[6]["mp"][:-1]
    assert differing(o, oracle_connections(oracle, w2, batch)) != []     # the feature behind the 256th counts
    w, batch, o = run("first_and_last_slot")
    assert w.max_kf == MAX_KEYFRAMES and entry(o, 0) == ([MAX_KEYFRAMES - 1, 0, 4000], [18, 18, 15], [0, MAX_KEYFRAMES - 1, 4000], [18, 18, 15])
    _, batch, o = run("slot_twice")
    assert batch[0] == batch[2] and entry(o, 0) == entry(o, 2)
    assert len(by["B1"][2]) == 1 and len(by["B70"][2]) == 70


def test_local_map_scenes_show_what_they_are_for(oracle):
    by = {s[0]: s for s in LM}
    _, w, frames, _ = by["no_votes"]
    for f in frames:
        o = oracle_local_map(oracle, w, f)
        assert o["n_k1"] == 0 and len(o["local_kf"]) == 0 and o["ref_kf"] == -1 and len(o["local_points"]) == 0
    assert oracle_local_map(oracle, w, frames[2])["frame_point_bad"].tolist() == [1]
    _, w, frames, _ = by["bad_frame_point_and_tie"]
    o = oracle_local_map(oracle, w, frames[0])
    assert o["frame_point_bad"].tolist() == [0, 1, 0, 0, 0] and o["ref_kf"] == 1 and 2 not in o["local_kf"]
    for k1, grown in ((80, 1), (81, 0), (78, 3)):
        _, w, frames, _ = by[f"k1_{k1}"]
        o = oracle_local_map(oracle, w, frames[0])
        assert o["n_k1"] == k1 and len(o["local_kf"]) == k1 + grown
    _, w, frames, expect = by["parent_ends_the_loop"]
    o = oracle_local_map(oracle, w, frames[0])
    assert w.kf[6]["bad"] and 6 in o["local_kf"] and not {7, 8, 9} & set(o["local_kf"].tolist())     # what members 3.. would have added
    _, w, frames, _ = by["consecutive_frames"]
    outs = [oracle_local_map(oracle, w, f) for f in frames]
    assert len(frames) == 3 and any(set(a["local_points"].tolist()) & set(b["local_points"].tolist()) and differing(a, b) for a, b in zip(outs, outs[1:]))
    assert any(set(f) & set(o["local_points"].tolist()) for f, o in zip(frames, outs))              # the frame's own points among the rows


# ---- validation: nothing here reaches a device ----
def _handle(max_kf=8, max_points=16, arena=0, must_load=False):
    from rumi_slam_amd.covis import Covisibility
    try:
        return Covisibility(max_kf, max_points, arena)
    except (OSError, RuntimeError) as e:
        if must_load or getattr(e, "code", None) is not None:
            raise
        pytest.skip(f"the library does not load here: {e}")


def small_world():
    w = World(8, 16)
    for s in range(4):
        w.add_kf(s, 10 + s, mp=[s, s + 1, -1], best=[(s + 1) % 4], parent=(s + 3) % 4, children=[(s + 1) % 4])
    for p in range(6):
        w.add_pt(p, [p % 4, (p + 1) % 4])
    return w


def malformed_edits():
    """(name, function of (handle, world) that returns the status of one refused call)"""
    def kf(slot=1, **over):
        def call(h, w):
            w = w.copy()
            w.kf[slot].update(over)
            return w.put_keyframes(h, [slot], check=False)
        return call

    def pt(ids, obs):
        return lambda h, w: h.set_points(ids, [0] * len(ids), obs, check=False)

    return [("slot past the table", lambda h, w: h.set_keyframes([8], [99], [0], [0], [[]], [[]], [-1], [[]], check=False)),
            ("negative slot", lambda h, w: h.set_keyframes([-1], [99], [0], [0], [[]], [[]], [-1], [[]], check=False)),
            ("slot named twice", lambda h, w: h.set_keyframes([5, 5], [98, 99], [0, 0], [0, 0], [[], []], [[], []], [-1, -1], [[], []], check=False)),
            ("key of another live slot", kf(key=12)),
            ("the same key twice in a call", lambda h, w: h.set_keyframes([5, 6], [99, 99], [0, 0], [0, 0], [[], []], [[], []], [-1, -1], [[], []], check=False)),
            ("mp past the point table", kf(mp=[0, 16])),
            ("mp below -1", kf(mp=[-2])),
            ("best not live", kf(best=[6])),
            ("best past the table", kf(best=[8])),
            ("parent not live", kf(parent=7)),
            ("parent is the key-frame", kf(parent=1)),
            ("child not live", kf(children=[5])),
            ("child is the key-frame", kf(children=[1])),
            ("child listed twice", kf(children=[2, 3, 2])),
            ("point id past the table", pt([16], [[0]])),
            ("negative point id", pt([-1], [[0]])),
            ("point named twice", pt([3, 3], [[0], [1]])),
            ("observer not live", pt([3], [[0, 5]])),
            ("observer past the table", pt([3], [[8]])),
            ("negative observer", pt([3], [[-1]])),
            ("observer listed twice", pt([3], [[1, 2, 1]])),
            ("bad flag of a slot that is not live", lambda h, w: h.set_bad([5], [1], [], [], check=False)),
            ("bad flag of a point past the table", lambda h, w: h.set_bad([], [], [16], [1], check=False)),
            ("map of a slot that is not live", lambda h, w: h.set_maps([1, 6], [1, 1], check=False)),
            ("backward mp slice", lambda h, w: _raw_keyframes(h, mp_off=[2, 0])),
            ("backward observer slice", lambda h, w: _raw_points(h, obs_off=[1, 0]))]


def _raw_keyframes(h, mp_off):
    from rumi_slam_amd import capi
    a = lambda v, dt=np.int32: np.ascontiguousarray(v, dt)
    args = [a([5]), a([99], np.uint64), a([0]), a([0], np.uint8), a(mp_off), a([0, 0, 0]), a([-1] * 10), a([-1]), a([0, 0]), a([0])]
    return h._lib.rumi_covis_set_keyframes(h._h, 1, *[capi.ptr(x) for x in args])


def _raw_points(h, obs_off):
    from rumi_slam_amd import capi
    a = lambda v, dt=np.int32: np.ascontiguousarray(v, dt)
    args = [a([3]), a([0], np.uint8), a(obs_off), a([0, 0])]
    return h._lib.rumi_covis_set_points(h._h, 1, *[capi.ptr(x) for x in args])


def check_edit_validation(must_load=False):
    """Shared with the GPU file: every malformed edit is RUMI_E_INVALID; a handle above the limit is RUMI_E_CAPACITY."""
    from rumi_slam_amd import capi
    from rumi_slam_amd.covis import Covisibility
    w = small_world()
    h = w.load(_handle(must_load=must_load))
    before = h.stats()
    for name, call in malformed_edits():
        assert call(h, w) == capi.RUMI_E_INVALID, name
    after = h.stats()
    assert {k: before[k] for k in ("tail", "live", "replaced")} == {k: after[k] for k in ("tail", "live", "replaced")}
    h.close()
    with pytest.raises(capi.RumiError) as e:
        Covisibility(MAX_KEYFRAMES + 1, 16)
    assert e.value.code == capi.RUMI_E_CAPACITY
    for bad in ((0, 16), (8, 0), (-1, 16)):
        with pytest.raises(capi.RumiError) as e:
            Covisibility(*bad)
        assert e.value.code == capi.RUMI_E_INVALID
    return w


def query_errors(h, w):
    """(name, expected status, call(out) -> status, outputs) for every query error that is decided before a device is touched."""
    from rumi_slam_amd import capi
    from rumi_slam_amd.covis import Covisibility as Cv
    return [("batch entry not live", capi.RUMI_E_INVALID, lambda o: h.update_connections_into([0, 6], o, 64, 64), Cv.connection_outputs(2, 64, 64, 0x77)),
            ("batch entry past the table", capi.RUMI_E_INVALID, lambda o: h.update_connections_into([8], o, 64, 64), Cv.connection_outputs(1, 64, 64, 0x77)),
            ("negative batch entry", capi.RUMI_E_INVALID, lambda o: h.update_connections_into([-1], o, 64, 64), Cv.connection_outputs(1, 64, 64, 0x77)),
            ("frame point past the table", capi.RUMI_E_INVALID, lambda o: h.local_map_into([0, 16], o, 8, 16), Cv.local_map_outputs(2, 8, 16, 0x77)),
            ("frame point below -1", capi.RUMI_E_INVALID, lambda o: h.local_map_into([-2], o, 8, 16), Cv.local_map_outputs(1, 8, 16, 0x77)),
            ("negative capacity", capi.RUMI_E_INVALID, lambda o: h.local_map_into([0], o, -1, 16), Cv.local_map_outputs(1, 8, 16, 0x77))]


def untouched(out):
    return all(v.tobytes() == bytes([0x77]) * v.nbytes for v in out.values())


def test_host_side_validation():
    w = check_edit_validation()
    h = w.load(_handle())
    for name, want, call, out in query_errors(h, w):
        assert call(out) == want, name
        assert untouched(out), name
    h.close()


def test_arena_bookkeeping_without_a_device():
    """A small arena: rows that outgrow their place move to the tail, a full arena is compacted, and one whose live rows pass three
    quarters is doubled.  Only the host's bookkeeping is looked at; the answers are compared on the GPU."""
    w0, edits, _ = edit_sequence(0)
    h = _handle(w0.max_kf, w0.max_points, arena=2048)
    w0.load(h)
    from covis_scene import apply_edit
    for e in edits:
        apply_edit(h, e)
    st = h.stats()
    assert st["replaced"] >= 1 and st["compactions"] + st["growths"] >= 1
    assert st["live"] <= st["tail"] <= st["capacity"]
    h.close()


def test_edit_sequence_contents():
    w0, edits, w1 = edit_sequence(0)
    kinds = [e[0] for e in edits]
    assert len(edits) >= 190 and {"kf", "pt", "bad", "maps"} <= set(kinds)
    grew = shrank = 0
    cur = {p: len(d["obs"]) for p, d in w0.pt.items()}
    for kind, what, snap in edits:
        if kind == "pt":
            for p in what:
                n = len(snap.pt[p]["obs"])
                grew += n > cur.get(p, 0); shrank += n < cur.get(p, 0)
                cur[p] = n
    assert grew >= 10 and shrank >= 10
    assert len(w1.kf) > len(w0.kf)
