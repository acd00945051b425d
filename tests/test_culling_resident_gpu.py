"""rumi_keyframe_culling_resident (include/rumi_mapping.h) on the GPU: the covisibility store as the map, against the block entry
(rumi_keyframe_culling) and the C++ oracle (tests/cpp/culling_oracle.cc) on the same map, byte for byte."""
import numpy as np
import pytest

import culling_resident_scene as rs
from culling_scene import SCENES, CullScene, build_oracle, run_oracle, same_bytes

pytestmark = pytest.mark.gpu
FILL = 0xC3


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("culling_resident"))


@pytest.fixture(scope="module")
def culler():
    from rumi_slam_amd.mapping import KeyFrameCuller
    r = KeyFrameCuller()
    yield r
    r.close()


def new_store(m, max_kf=None, arena_entries=0, slot_of=None, spare_kf=0):
    from rumi_slam_amd.covis import Covisibility
    s = Covisibility(max_kf or m.n_kf + spare_kf, m.n_pts + 8, arena_entries=arena_entries)
    m.load(s, slot_of)
    return s


def resident(culler, store, m, cand, flags=0, slot_of=None, expect=0):
    """The raw outputs over FILL; ``expect``: the status code the call must return."""
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import cull_outputs
    out = cull_outputs(len(cand), FILL)
    rc = culler.status_resident(store, m.candidates(cand, slot_of), flags, out)
    assert rc == expect, (rc, capi.lib().rumi_last_error().decode())
    return out


def block(culler, m, cand, flags=0):
    from rumi_slam_amd import capi
    b = m.batch(cand)
    out = b.outputs(FILL)
    capi.check(culler.status(b, flags, out))
    return out


def three_way(oracle, culler, store, m, cand, flags=0, slot_of=None):
    got, blk, want = resident(culler, store, m, cand, flags, slot_of), block(culler, m, cand, flags), run_oracle(oracle, m.batch(cand), flags, FILL)
    assert same_bytes(blk, want) == [], "block entry vs oracle"
    assert same_bytes(got, want) == [], "resident entry vs oracle"
    return got


@pytest.mark.parametrize("params", SCENES, ids=lambda s: f"scene{s[0]}-{s[1]}")
def test_every_scene_both_variants(oracle, culler, params):
    sc = CullScene(*params)
    m = rs.MapMirror.from_scene(sc)
    store = new_store(m)
    for cloud in (False, True):
        got = three_way(oracle, culler, store, m, sc.cand, sc.flags(cloud))
        assert same_bytes(resident(culler, store, m, sc.cand, sc.flags(cloud)), got) == [], "two calls on one state"
    store.close()


@pytest.mark.parametrize("seq", rs.SEQUENCES, ids=lambda s: f"seed{s[0]}")
def test_sequence_with_only_the_edits_staged(oracle, culler, seq):
    from rumi_slam_amd.mapping import trim
    sc, lists = rs.sequence(*seq)
    m = rs.MapMirror.from_scene(sc)
    store = new_store(m, spare_kf=rs.GROW_KFS)
    uploads, culls, replaced0 = [], 0, store.stats()["replaced"]
    for step, cand in enumerate(lists):
        m.stage(store, rs.before_step(m, step))
        got = three_way(oracle, culler, store, m, cand)
        uploads.append(store.stats()["last_upload_bytes"])
        res = trim(m.batch(cand), got)
        culls += len(res["culled"]) > 0
        m.stage(store, m.apply(cand, res))                           # SetBadFlag() in the returned order; nothing else is staged
    st = store.stats()
    print("uploads", uploads, "stats", st)
    assert culls >= 2
    assert st["replaced"] > replaced0, "observer rows that outgrew their place were re-placed at the tail"
    assert all(u < uploads[0] // 4 for u in uploads[1:]), "a later step uploads its edits, not the map"
    store.close()


def check_case(oracle, culler, m, cand, min_culled, slot_of=None, max_kf=None, arena_entries=0):
    store = new_store(m, max_kf=max_kf, arena_entries=arena_entries, slot_of=slot_of)
    got = three_way(oracle, culler, store, m, cand, slot_of=slot_of)
    assert got["n_culled"][0] >= min_culled, got["n_culled"][0]
    return store, got


def test_second_workgroup_row_and_stride_loop(oracle, culler):
    """257 features: one lane in the second workgroup row of the first pass.  1030-1100: the replay's stride loop, after a cull."""
    nfeat = [257, 1030, 300, 1100, 257, 1057, 420, 1024, 1025, 256, 380, 1031]
    m = rs.synthetic_map(nfeat, 6, 11, rich={0, 5, 9})
    store, got = check_case(oracle, culler, m, [0, 9, 5, 1, 3, 4, 7, 8, 11, 2], 2)
    cand = [0, 9, 5, 1, 3, 4, 7, 8, 11, 2]
    later = [k for c, k in enumerate(cand) if c > int(got["culled"][0]) and got["status"][c] >= 4]
    assert any((m.mp[k][1024:] >= 0).any() for k in later), "a row with points behind entry 1024 is evaluated after a cull"
    store.close()


def test_slots_spread_over_the_bit_set(oracle, culler):
    """max_kf = 8192; two culled slots in one 32-bit word of the culled set, one at 8191."""
    m = rs.synthetic_map([70] * 12, 6, 12, rich={0, 1, 9})
    slot_of = [4100, 4127, 4128, 0, 31, 32, 63, 64, 4096, 8191, 8190, 8160]
    assert slot_of[0] >> 5 == slot_of[1] >> 5
    store, got = check_case(oracle, culler, m, [0, 1, 9, 3, 4, 5, 6, 7, 8, 2, 10, 11], 3, slot_of=slot_of, max_kf=8192)
    assert got["culled"][:3].tolist() == [0, 1, 2]
    store.close()


def test_candidate_listed_twice(oracle, culler):
    from rumi_slam_amd.mapping import CULL_CULLED, CULL_SKIPPED_BAD
    m = rs.synthetic_map([80] * 10, 6, 13, rich={4})
    store, got = check_case(oracle, culler, m, [4, 2, 4, 3, 5], 1)
    assert got["status"][0] == CULL_CULLED and got["status"][2] == CULL_SKIPPED_BAD
    store.close()


def test_point_with_many_observers(oracle, culler):
    m = rs.synthetic_map([40] * 70, 5, 14, rich={3, 40}, everywhere=3)
    assert max(len(o) for o in m.obs) >= 65
    store, got = check_case(oracle, culler, m, [3, 40, 0, 10, 69, 33], 2)
    store.close()


def test_compacted_and_grown_arena(oracle, culler):
    m = rs.synthetic_map([90] * 14, 6, 15, rich={2, 7})
    store = new_store(m, arena_entries=64)                           # the load alone doubles the arena several times
    true = m.mp
    for r in range(1, 9):                                            # rows that outgrow their place move to the tail and leave holes behind
        if store.stats()["compactions"] >= 1:
            break
        m.mp = [np.concatenate([a, np.full(40 * r, -1, np.int32)]) for a in true]
        m.set_keyframes(store, range(m.n_kf))
        m.mp = true
        m.set_keyframes(store, range(m.n_kf))
    st = store.stats()
    print(st)
    assert st["growths"] >= 1 and st["compactions"] >= 1 and st["replaced"] >= 1
    got = three_way(oracle, culler, store, m, [2, 7, 0, 1, 3, 8, 9])
    assert got["n_culled"][0] >= 2
    store.close()


def test_device_found_refusals_leave_the_outputs_untouched(oracle, culler):
    from rumi_slam_amd import capi
    m = rs.synthetic_map([60] * 10, 6, 16, rich={1})
    store = new_store(m)
    cand = [1, 0, 2, 3]
    base = resident(culler, store, m, cand)
    p = next(int(q) for q in m.mp[0] if q >= 0 and any(k not in cand for k, f in m.obs[q]))      # a point of candidate 0 ...
    outsider = next(k for k, f in m.obs[p] if k not in cand)                                     # ... with an observer outside the list
    free = int(np.nonzero(m.mp[outsider] != p)[0][0])

    def refused(word, restore):
        out = resident(culler, store, m, cand, expect=capi.RUMI_E_INVALID)
        msg = capi.lib().rumi_last_error().decode()
        assert word in msg and "rumi_keyframe_culling_resident" in msg, msg
        assert all(a.tobytes() == bytes([FILL]) * a.nbytes for a in out.values()), "nothing written"
        restore()
        assert same_bytes(resident(culler, store, m, cand), base) == [], "a correct call on the same handle afterwards"
        return msg

    obs = lambda edit: [edit(k, f) for k, f in m.obs[p]]
    # a point without observation features
    store.set_points([p], [False], [[k for k, f in m.obs[p]]])
    refused("without observation features", lambda: m.set_points(store, [p]))
    # an observer slot without resident features
    store.drop_keyframe_features([outsider])
    msg = refused(" observations name a key-frame without resident features", lambda: store.set_keyframe_features(outsider, *m.features(outsider), [500.0, 500.0, 320.0, 240.0]))
    assert not msg.split("inconsistent among what the loop reads: ")[1].startswith("0 "), msg
    # an observation whose feature lies outside the observer's row, then one whose slot holds another point
    for f_bad in (60, 65535, free):
        store.set_point_observations([p], [False], [obs(lambda k, f: (k, f_bad if k == outsider else f))])
        msg = refused("name a feature outside the key-frame's row or one that does not hold the point", lambda: m.set_points(store, [p]))
        assert ", 0 name a feature" not in msg, msg
    # a candidate slot holding p where p does not list (candidate, slot)
    store.set_point_observations([p], [False], [[(k, f) for k, f in m.obs[p] if k != 0]])
    msg = refused("candidate slots hold a point that does not list", lambda: m.set_points(store, [p]))
    assert ", 0 candidate slots" not in msg, msg
    store.set_point_observations([p], [False], [obs(lambda k, f: (k, (f + 1) % 60 if k == 0 else f))])      # lists the candidate, at another slot
    msg = refused("candidate slots hold a point that does not list", lambda: m.set_points(store, [p]))
    assert ", 0 candidate slots" not in msg and ", 0 name a feature" not in msg, msg
    store.close()


def test_empty_list_makes_no_device_call(culler):
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import cull_outputs
    m = rs.synthetic_map([30] * 5, 4, 17)
    store = new_store(m)
    out = cull_outputs(0, FILL)
    assert culler.status_resident(store, [], 0, out) == capi.RUMI_OK and out["n_culled"][0] == 0
    assert out["status"].tobytes() == bytes([FILL]) * 4
    assert store.stats()["last_upload_bytes"] == 0, "an empty list makes no device call"
    store.close()


def test_the_stores_other_queries_do_not_see_a_culling_call(oracle, culler):
    m = rs.synthetic_map([80] * 12, 6, 18, rich={2, 5})
    store = new_store(m)
    slots = list(range(m.n_kf))
    frame = np.concatenate([m.mp[3][:40], m.mp[6][:40]]).astype(np.int32)
    before = (store.update_connections(slots, n_live=m.n_kf), store.local_map(frame))
    got = three_way(oracle, culler, store, m, [2, 5, 0, 1, 3, 4])
    assert got["n_culled"][0] == 2
    after = (store.update_connections(slots, n_live=m.n_kf), store.local_map(frame))
    for b, a in zip(before, after):
        for k in b:
            assert np.asarray(b[k]).tobytes() == np.asarray(a[k]).tobytes(), k
    assert same_bytes(resident(culler, store, m, [2, 5, 0, 1, 3, 4]), got) == [], "and a second culling call after them"
    store.close()


def test_public_mirror(oracle):
    from rumi_slam_amd.mapping import CULL_CLOUD, KeyFrameCuller, KeyFrameCullingResident, trim
    sc = CullScene(*SCENES[3])
    m = rs.MapMirror.from_scene(sc)
    store = new_store(m)
    r = KeyFrameCuller()
    got = KeyFrameCullingResident(r, store, m.candidates(sc.cand), CULL_CLOUD)
    want = trim(sc.batch(), run_oracle(oracle, sc.batch(), CULL_CLOUD))
    assert all(got[k].tolist() == want[k].tolist() for k in want) and len(got["culled"]) >= 1
    assert r.stage_ms().sum() > 0
    r.close()
    store.close()
