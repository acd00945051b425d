"""One handle, three calls: a small input, one that exceeds every capacity the small one left, the small one again.  The blocks a handle
grows on demand (DevBuf / MirrorBuf, csrc/rumi_common.h) are released and allocated again by the second call and must still serve the third;
every result is held to what the entry's own GPU test holds it to (its oracle and comparison helper), and where that is a tolerance or where
there is no oracle, also to the bytes a fresh handle returns for that input alone.  The sites whose own tests already walk a handle through
growth are not repeated here: culling, refresh, the covisibility arena, the candidate lists of SearchForInitialization."""
import numpy as np
import pytest

import essential_scene as es
import oracle_lib as O
from ba_scene import ba_problem
from kfdb_scene import Scene as KfdbScene
from kfdb_scene import build_oracle as build_kfdb_oracle
from newpoints_scene import TH_FAR, NewPointsScene, params
from newpoints_scene import build_oracle as build_newpoints_oracle
from newpoints_scene import run_oracle as run_newpoints_oracle
from scene import TrackingScene
from submap_scene import Scene as SubmapScene
from submap_scene import build_oracle as build_submap_oracle
from submap_scene import run_oracle as run_submap_oracle
from submap_scene import seeded_scene
from voc_scene import synthetic_vocabulary, synthetic_vocabulary_fast

pytestmark = pytest.mark.gpu


def small_large_small(small, large):
    return (("small", small), ("large", large), ("small again", small))


# ---- CreateNewMapPoints and its match hook: blk, cand / gate / x3D, res, matched ----
def test_create_new_map_points_and_match_hook(tmp_path):
    from rumi_slam_amd.mapping import last_matches
    from test_newpoints_gpu import assert_same, gpu_call, matcher
    oracle = build_newpoints_oracle(tmp_path)
    m = matcher(1)
    for name, s in small_large_small(NewPointsScene(70, 1, 32), NewPointsScene(71, 3, 300)):
        want = run_newpoints_oracle(oracle, s.cur, s.neigh, params(0, 1, 0, TH_FAR))
        assert_same(gpu_call(m, s, s.neigh, 0, 0), want)
        assert np.array_equal(last_matches(m, len(s.neigh), s.cur.frame.n), want["matches"]), name
        if name == "large":
            assert len(want["points"]) > 10
    m.close()


# ---- batched SearchByBoW: bow, bowOut ----
def bow_candidates(K, nodes=60):
    """The frame of scene 40 and K candidate key-frames that share descriptors with it (as test_matcher_gpu builds them)."""
    from rumi_slam_amd.matcher import FeatureVector, FrameView
    scenes = [TrackingScene(40 + k) for k in range(K)]
    base = scenes[0]
    F = FrameView(base.cur_keys, base.cur_desc, base.w, base.h, base.sf)
    _, fv_f0 = base.feature_vectors(nodes)
    b = FeatureVector(fv_f0)
    fnode = {int(i): nd for nd, idxs in fv_f0.items() for i in idxs}
    KFs, fvs, mps, bads = [], [], [], []
    for k, s in enumerate(scenes):
        kdesc = s.last_desc.copy()
        n = min(len(kdesc), len(base.cur_desc))
        take = np.random.default_rng(k).random(n) < 0.5
        kdesc[:n][take] = base.cur_desc[:n][take]
        node_kf, rng = {}, np.random.default_rng(100 + k)
        for i in range(len(kdesc)):
            node_kf.setdefault(fnode[i] if i < n and take[i] else int(rng.integers(0, nodes)) * 7 + 3, []).append(i)
        KFs.append(FrameView(s.last_keys, kdesc, s.w, s.h, s.sf)); fvs.append(FeatureVector(node_kf)); mps.append(s.last_mp)
        bads.append((np.random.default_rng(k).random(len(s.mp_obs)) < 0.05).astype(np.uint8))
    return base, F, b, KFs, fvs, mps, bads


def test_search_by_bow_batch():
    from rumi_slam_amd.matcher import ORBmatcher, SearchByBoW_batch
    base, F, b, KFs, fvs, mps, bads = bow_candidates(4)
    refs = [O.search_by_bow(KFs[k].keys, KFs[k].desc, mps[k], bads[k], (fvs[k].node_ids, fvs[k].offsets, fvs[k].indices), base.cur_keys, base.cur_desc,
                            (b.node_ids, b.offsets, b.indices), 0.75, True) for k in range(4)]
    assert all(n > 30 for n, _ in refs)
    m = ORBmatcher(0.75, True)
    for name, K in small_large_small(1, 4):
        nm, got = SearchByBoW_batch(m, KFs[:K], fvs[:K], mps[:K], bads[:K], F, b)
        for k in range(K):
            assert nm[k] == refs[k][0] and np.array_equal(got[k], refs[k][1]), (name, k)
    m.close()


# ---- sub-map matching: sub, subOut, and the upload block it grows ----
def test_submap_match(tmp_path):
    from rumi_slam_amd.submap import SubmapMatcher
    from test_submap_gpu import check, device
    oracle = build_submap_oracle(tmp_path)
    m = SubmapMatcher()
    two = seeded_scene(31, 2, (150, 200))
    for name, s in small_large_small(SubmapScene(two.frames[:2], two.pairs[:1], "one pair"), seeded_scene(32, 4, (500, 600))):
        print(name)
        check(device(m, s), run_submap_oracle(oracle, s))
    m.close()


# ---- essential graph and point correction: egA, eg ----
def test_essential_graph_and_point_correction():
    from rumi_slam_amd.optimizer import Optimizer
    from test_essential_gpu import check_against_oracle, rel
    sizes = dict(max_pose_edges=64, max_pose_batch=1, max_kf=256, max_mp=4096, max_edges=4096)
    o = Optimizer(**sizes)
    corrections = {"two_free": es.correction_case(3, 4, 30), "merge": es.correction_case(4, 40, 3000)}
    for name, scene in small_large_small("two_free", "merge"):
        got = check_against_oracle(o, scene)
        X, ref, t8, _ = corrections[scene]
        pts = o.correct_points(X, ref, *t8, mode=0)
        assert rel(pts, es.oracle_correct_points(0, X, ref, *t8)) < 1e-4
        fresh = Optimizer(**sizes)                                   # the oracle is held to a tolerance; a handle that has only seen this input, to the bytes
        sc = es.scene(scene)
        want = fresh.essential_graph(*sc.args(), n_iterations=es.SCENES[scene]["n_it"])
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), name
        assert pts.tobytes() == fresh.correct_points(X, ref, *t8, mode=0).tobytes(), name
        fresh.close()
    o.close()


# ---- vocabulary transform: q, word, node, w ----
def test_vocabulary_transform():
    from rumi_slam_amd.vocabulary import ORBVocabulary
    from test_vocabulary_gpu import _features
    voc = synthetic_vocabulary(0, 10, 3)
    g, o = ORBVocabulary(*voc), O.OracleVocabulary(*voc)
    rng = np.random.default_rng(7)
    for name, d in small_large_small(_features(voc, rng, 10), _features(voc, rng, 600)):
        for a, b in zip(g.transform_features(d, 1), o.transform_features(d, 1)):
            assert a.tobytes() == b.tobytes(), name
    g.close()


# ---- key-frame database: the query arrays (a batch of 1, of 8, of 1, both kinds of query) ----
def test_kfdb_query_batches(tmp_path):
    from rumi_slam_amd.vocabulary import ORBVocabulary
    from test_kfdb_gpu import NW, check
    voc = ORBVocabulary(*synthetic_vocabulary_fast(5, 10, 5))
    sc = KfdbScene(23, 12, 1, n_words=NW)
    rng = np.random.default_rng(5)
    script, qid = sc.add_commands() + sc.cov_commands(), 1_000_000
    for batch in (1, 8, 1):                                          # run_gpu puts consecutive queries of one kind into one call
        for kind in "RN":
            for _ in range(batch):
                i = int(rng.integers(len(sc.ids)))
                w, v = sc.query_bow(place=sc.place_of[i])
                script.append(("R", qid, sc.maps[i], w, v) if kind == "R" else ("N", qid, sc.maps[i], 3, [sc.ids[i]] + sc.connected(i), w, v))
                qid += 1
    want = check(voc, build_kfdb_oracle(tmp_path), script, batch=True, max_kf=64, max_entries=20000)
    assert len(want) == 20
    voc.close()


# ---- batched local BA: groupOut ----
def test_local_ba_batch_windows():
    from rumi_slam_amd.optimizer import Optimizer
    probs = [ba_problem(seed=600, n_opt=3, n_fixed=2, n_points=100)] + [ba_problem(seed=601 + i, n_opt=8, n_fixed=2, n_points=300) for i in range(4)]
    wins = [(b["kf_pose"], b["kf_fixed"], b["mp_pos"], b["e_mp"], b["e_kf"], b["e_obs"], b["e_w"], b["K"]) for b in probs]
    o = Optimizer()
    single = [o.LocalBundleAdjustment(*w) for w in wins]
    for name, (w, s) in small_large_small((wins[:1], single[:1]), (wins[1:], single[1:])):
        got = o.LocalBundleAdjustmentBatch(w, 1)
        assert len(got) == len(s)
        for i, (a, b) in enumerate(zip(s, got)):
            assert all(np.array_equal(a[j], b[j]) for j in range(4)), (name, i)
    o.close()
