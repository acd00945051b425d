"""rumi_covis_set_keyframe_features and its companions (include/rumi_covis.h) without a device: a set_ call validates and stages on the host, so
every refusal, the stats and the free-space arithmetic are observable here.  The validator is the one rumi_create_new_map_points uses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rumi_slam_amd import capi
from rumi_slam_amd.covis import MAX_FEATURES, Covisibility
from rumi_slam_amd.matcher import FeatureVector, FrameView

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rumi_covis_set_keyframe_features", "rumi_covis_drop_keyframe_features", "rumi_covis_reserve_features", "rumi_covis_feature_stats"]
K4 = np.float32([500, 500, 320, 240])
SF = (np.float32(1.2) ** np.arange(8)).astype(np.float32)


def keyframe(n=40, seed=0, nodes=5):
    rng = np.random.default_rng(seed)
    keys = np.zeros(n, capi.KP_DTYPE)
    keys["x"], keys["y"] = rng.uniform(10, 600, n), rng.uniform(10, 400, n)
    keys["octave"] = rng.integers(0, 8, n)
    keys["angle"] = rng.uniform(0, 360, n)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    perm = rng.permutation(n)
    fv = FeatureVector({10 * (a + 1): perm[a::nodes].tolist() for a in range(nodes)})
    return FrameView(keys, desc, 640, 480, SF), fv


def block_bytes(frame, fv):
    up = lambda b: (b + 15) & ~15
    n, nn = frame.n if hasattr(frame, "n") else len(frame.keys), len(fv.node_ids)
    return 64 + up(n * 28) + up(n * 32) + up(len(SF) * 4) + up(nn * 4) + up((nn + 1) * 4) + up(len(fv.indices) * 4)


@pytest.fixture
def store():
    s = Covisibility(16, 256)
    s.set_keyframes([2, 3, 4], [11, 12, 13], [0, 0, 0], [0, 0, 0], [[-1] * 40] * 3, [[]] * 3, [-1] * 3, [[]] * 3)
    yield s
    s.close()


def last_error():
    return capi.lib().rumi_last_error().decode()


def test_symbols_declared():
    L = capi.covis_lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rumi_covis.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rumi_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in capi.COVIS_SYMBOLS
        getattr(L, name)
    assert "rumi_create_new_map_points_resident" in capi.MAPPING_SYMBOLS
    getattr(L, "rumi_create_new_map_points_resident")


def test_set_stats_drop_and_reuse(store):
    f, v = keyframe()
    b = block_bytes(f, v)
    z = store.feature_stats()
    assert z == dict(capacity=0, used=0, slots=0, growths=0, compactions=0, last_upload_bytes=0)
    store.reserve_features(4096)
    store.set_keyframe_features(2, f, v, K4)
    store.set_keyframe_features(3, f, v, K4)
    st = store.feature_stats()
    assert st["capacity"] == 4096 * 2 and st["growths"] == 1 and st["used"] == 2 * b and st["slots"] == 2      # two blocks of ~2.7 KB pass 4 KiB
    assert store.reserve_features(1 << 20, check=False) == capi.RUMI_E_INVALID                                   # only before the first key-frame
    store.drop_keyframe_features([2, 7, 15])                                                                     # 7, 15 hold nothing: not an error
    assert store.feature_stats()["used"] == b and store.feature_stats()["slots"] == 1
    store.set_keyframe_features(4, f, v, K4)                                                                     # takes the freed block
    store.set_keyframe_features(3, f, v, K4)                                                                     # replaces: frees, then reuses
    st = store.feature_stats()
    assert st["capacity"] == 8192 and st["growths"] == 1 and st["used"] == 2 * b and st["slots"] == 2
    assert store.drop_keyframe_features([16], check=False) == capi.RUMI_E_INVALID
    assert store.drop_keyframe_features([-1], check=False) == capi.RUMI_E_INVALID


def _refusals():
    """(name, mutate(frame, fv, args) -> None, expected code, part of the message)"""
    def dead(f, v, a): a["slot"] = 9
    def outside(f, v, a): a["slot"] = 16
    def too_many(f, v, a): f.c.n = MAX_FEATURES + 1
    def octave(f, v, a): f.keys["octave"][7] = 8
    def octave_neg(f, v, a): f.keys["octave"][0] = -1
    def offsets(f, v, a): v.offsets[2] = v.offsets[1] - 1
    def offsets0(f, v, a): v.offsets[0] = 1
    def index(f, v, a): v.indices[5] = 40
    def nodes(f, v, a): v.node_ids[[2, 3]] = v.node_ids[[3, 2]]
    def nodes_eq(f, v, a): v.node_ids[3] = v.node_ids[2]
    def twice(f, v, a): v.indices[5] = v.indices[6]
    def no_keys(f, v, a): f.c.keys_un = None
    def no_desc(f, v, a): f.c.desc = None
    def no_scale(f, v, a): f.c.scale_factors = None
    def no_idx(f, v, a): v.c.indices = None
    def no_k4(f, v, a): a["K4"] = None
    def levels(f, v, a): f.c.nlevels = 0
    I, Cp = capi.RUMI_E_INVALID, capi.RUMI_E_CAPACITY
    return [("dead slot", dead, I, "not live"), ("slot outside", outside, I, "not live"), ("n above the limit", too_many, Cp, "RUMI_COVIS_MAX_FEATURES"),
            ("octave outside nlevels", octave, I, "octave"), ("negative octave", octave_neg, I, "octave"),
            ("offsets not ascending", offsets, I, "offsets or indices"), ("first offset not 0", offsets0, I, "offsets or indices"),
            ("index out of range", index, I, "offsets or indices"), ("node ids not ascending", nodes, I, "not strictly ascending"),
            ("equal node ids", nodes_eq, I, "not strictly ascending"), ("a feature listed twice", twice, I, "listed twice"),
            ("missing keys", no_keys, I, "missing arrays"), ("missing descriptors", no_desc, I, "missing arrays"),
            ("missing scale factors", no_scale, I, "missing arrays"), ("missing indices", no_idx, I, "missing arrays"),
            ("missing K4", no_k4, I, "missing argument"), ("no levels", levels, I, "bad sizes")]


@pytest.mark.parametrize("name,mutate,code,msg", _refusals(), ids=[r[0] for r in _refusals()])
def test_refusal_leaves_the_store_untouched(store, name, mutate, code, msg):
    good_f, good_v = keyframe(seed=1)
    store.set_keyframe_features(3, good_f, good_v, K4)
    before = store.feature_stats()
    f, v = keyframe(seed=2)
    a = dict(slot=2, K4=K4)
    mutate(f, v, a)
    rc = store._lib.rumi_covis_set_keyframe_features(store._h, a["slot"], C.byref(f.c), C.byref(v.c), None if a["K4"] is None else capi.ptr(a["K4"]))
    assert rc == code and msg in last_error(), last_error()
    assert store.feature_stats() == before
    f2, v2 = keyframe(seed=3)
    store.set_keyframe_features(2, f2, v2, K4)                    # a following valid set is unaffected
    after = store.feature_stats()
    assert after["slots"] == 2 and after["used"] == before["used"] + block_bytes(f2, v2)


def test_missing_handle_and_pointers(store):
    L = store._lib
    f, v = keyframe()
    assert L.rumi_covis_set_keyframe_features(None, 2, C.byref(f.c), C.byref(v.c), capi.ptr(K4)) == capi.RUMI_E_INVALID
    assert L.rumi_covis_set_keyframe_features(store._h, 2, None, C.byref(v.c), capi.ptr(K4)) == capi.RUMI_E_INVALID
    assert L.rumi_covis_set_keyframe_features(store._h, 2, C.byref(f.c), None, capi.ptr(K4)) == capi.RUMI_E_INVALID
    assert L.rumi_covis_feature_stats(store._h, None) == capi.RUMI_E_INVALID
    assert L.rumi_covis_drop_keyframe_features(store._h, 1, None) == capi.RUMI_E_INVALID
    assert L.rumi_covis_reserve_features(store._h, -1) == capi.RUMI_E_INVALID
    assert store.feature_stats()["slots"] == 0


def test_empty_keyframe_and_empty_feature_vector(store):
    f = FrameView(np.zeros(0, capi.KP_DTYPE), np.zeros((0, 32), np.uint8), 640, 480, SF)
    v = FeatureVector({})
    store.set_keyframe_features(2, f, v, K4)
    assert store.feature_stats()["used"] == 64 + 32 + 16 and store.feature_stats()["slots"] == 1      # record, scale factors, one offset


def test_validator_is_shared_with_the_block_entry():
    """One definition, in a header both translation units include; that both entries answer the same malformed key-frame with the same message
    is asserted on the device (tests/test_newpoints_resident_gpu.py: a matcher handle needs one)."""
    csrc = os.path.join(ROOT, "rumi_slam_amd", "csrc")
    defs = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".inc", ".h")) and re.search(r"bool\s+keyframe_features_valid\s*\(", open(os.path.join(csrc, f)).read())]
    assert defs == ["keyframe_features.h"]
    for f in ("mapping.hip", "covis_features.inc"):
        assert "keyframe_features_valid(" in open(os.path.join(csrc, f)).read()
    assert "node ids not strictly ascending" not in open(os.path.join(csrc, "mapping.hip")).read()
