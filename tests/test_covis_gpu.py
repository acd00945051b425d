"""rumi_covis_update_connections and rumi_covis_local_map (include/rumi_covis.h) against the scalar oracle (tests/cpp/covis_oracle.cc): every
output byte for byte over the constructed scenes of tests/covis_scene.py and 20 random maps, the same bytes from two calls, invariance
under a relabelling of the points and a shuffle of the observer rows, untouched outputs on every error path, and a handle that went
through 200 edits against a fresh one given the final state."""
import numpy as np
import pytest

from covis_scene import apply_edit, build_oracle, differing, edit_sequence, lm_scenes, oracle_connections, oracle_local_map, random_world, uc_scenes
from rumi_slam_amd import capi
from rumi_slam_amd.covis import Covisibility
from test_covis_cpu import check_edit_validation, query_errors, untouched

pytestmark = pytest.mark.gpu

UC = uc_scenes()
LM = lm_scenes()


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("covis"))


def check_both(oracle, h, w, batch, frames):
    """Both queries of handle h against the oracle on world w; returns the results."""
    flat = w.flat()
    got = [h.update_connections(batch, w.n_live())]
    assert differing(got[0], oracle_connections(oracle, w, batch, flat)) == []
    for f in frames:
        got.append(h.local_map(f))
        assert differing(got[-1], oracle_local_map(oracle, w, f, flat)) == []
    return got


@pytest.mark.parametrize("scene", UC, ids=[s[0] for s in UC])
def test_update_connections_scenes(oracle, scene):
    _, w, batch = scene
    h = w.handle()
    want = oracle_connections(oracle, w, batch)
    first = h.update_connections(batch, w.n_live())
    assert differing(first, want) == []
    assert differing(h.update_connections(batch, w.n_live()), first) == []
    h.close()


@pytest.mark.parametrize("scene", LM, ids=[s[0] for s in LM])
def test_local_map_scenes(oracle, scene):
    _, w, frames, _ = scene
    h = w.handle()
    flat = w.flat()
    for f in frames + frames[:1]:                                        # one handle, consecutive calls; the first frame once more at the end
        want = oracle_local_map(oracle, w, f, flat)
        first = h.local_map(f)
        assert differing(first, want) == []
        assert differing(h.local_map(f), first) == []
    h.close()


@pytest.mark.parametrize("seed", range(20))
def test_random_maps(oracle, seed):
    w, frames = random_world(300 + seed, (10, 33, 70, 130)[seed % 4], nfeat=((30, 50), (60, 90), (250, 300))[seed % 3], n_frames=3)
    rng = np.random.default_rng(seed)
    batch = [int(s) for s in rng.choice(sorted(w.kf), min(len(w.kf), 40), replace=True)]
    h = w.handle()
    check_both(oracle, h, w, batch, frames)
    h.close()


@pytest.mark.parametrize("seed", range(3))
def test_relabelled_points_and_shuffled_observers(oracle, seed):
    w, frames = random_world(400 + seed, 45, nfeat=(60, 90), n_frames=2)
    w2, new_of = w.relabelled(seed)
    batch = sorted(w.kf)
    h, h2 = w.handle(), w2.handle()
    assert differing(h.update_connections(batch, w.n_live()), h2.update_connections(batch, w.n_live())) == []
    for f in frames:
        a, b = h.local_map(f), h2.local_map([-1 if p < 0 else int(new_of[p]) for p in f])
        a["local_points"] = new_of[a["local_points"]].astype(np.int32)
        assert differing(a, b) == []
    h.close(); h2.close()


def test_error_paths_leave_outputs_untouched(oracle):
    w = check_edit_validation(must_load=True)
    h = w.load(Covisibility(w.max_kf, w.max_points))
    for name, want, call, out in query_errors(h, w):
        assert call(out) == want, name
        assert untouched(out), name
    batch, frame = [0, 1, 2, 3], [0, 1, 2, 3, 4, 5]
    uc, lm = oracle_connections(oracle, w, batch), oracle_local_map(oracle, w, frame)
    nc, no, nk, npt = len(uc["conn_slot"]), len(uc["ord_slot"]), len(lm["local_kf"]), len(lm["local_points"])
    assert min(nc, no, nk, npt) >= 1
    for cc, oc in ((nc - 1, no), (nc, no - 1)):
        out = Covisibility.connection_outputs(len(batch), 64, 64, 0x77)
        assert h.update_connections_into(batch, out, cc, oc) == capi.RUMI_E_CAPACITY and untouched(out)
    for kc, pc in ((nk - 1, npt), (nk, npt - 1)):
        out = Covisibility.local_map_outputs(len(frame), 64, 64, 0x77)
        assert h.local_map_into(frame, out, kc, pc) == capi.RUMI_E_CAPACITY and untouched(out)
    out = Covisibility.connection_outputs(len(batch), nc, no, 0x77)      # exactly enough
    assert h.update_connections_into(batch, out, nc, no) == capi.RUMI_OK
    assert differing(h.update_connections(batch, w.n_live()), uc) == [] and differing(h.local_map(frame), lm) == []
    h.close()


def test_edited_handle_equals_fresh_handle(oracle):
    """About 200 edits on a small arena (rows grow, shrink, move to the tail; the arena is compacted or grown), with queries in between so
    that the edits reach the device in many batches; refused edits in between change nothing."""
    w0, edits, w1 = edit_sequence(0)
    _, frames = random_world(40, 24, nfeat=(20, 30), max_kf=40, spare_points=60, n_frames=2)
    h = Covisibility(w0.max_kf, w0.max_points, arena_entries=2048)
    w0.load(h)
    w = w0.copy()
    uploads = []
    for i, e in enumerate(edits):
        apply_edit(h, e)
        w.kf.update({s: e[2].copy_kf(s) for s in e[2].kf})
        w.pt.update({p: dict(bad=d["bad"], obs=list(d["obs"])) for p, d in e[2].pt.items()})
        if i % 25 == 24:
            check_both(oracle, h, w, sorted(w.kf), frames)
            uploads.append(h.stats()["last_upload_bytes"])
    st = h.stats()
    assert st["replaced"] >= 1 and st["compactions"] + st["growths"] >= 1
    assert min(uploads) < 4 * st["live"]                                # 25 edits upload fewer bytes than the live rows hold
    assert differing(dict(a=np.array(sorted(w.kf))), dict(a=np.array(sorted(w1.kf)))) == []
    batch = sorted(w1.kf)
    mine = check_both(oracle, h, w1, batch, frames)
    fresh = w1.handle()
    theirs = check_both(oracle, fresh, w1, batch, frames)
    for a, b in zip(mine, theirs):
        assert differing(a, b) == []
    a, b = batch[0], batch[1]                                            # refused: the answers stay
    clash = w1.copy(); clash.kf[a]["key"] = w1.kf[b]["key"]; clash.kf[a]["mp"] = [0, 1, 2]
    refused = [h.set_keyframes([w1.max_kf], [1], [0], [0], [[0]], [[]], [-1], [[]], check=False), clash.put_keyframes(h, [a], check=False),
               h.set_points([0, 1], [1, 1], [[a], [b, a, b]], check=False), h.set_points([w1.max_points], [1], [[a]], check=False),
               h.set_bad([a, w1.max_kf], [1, 1], [0], [1], check=False), h.set_maps([a, -1], [5, 5], check=False)]
    assert refused == [capi.RUMI_E_INVALID] * len(refused)
    again = check_both(oracle, h, w1, batch, frames)
    for a, b in zip(mine, again):
        assert differing(a, b) == []
    h.close(); fresh.close()
