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


# ---- batched local BA: one batch arena, then four, then one again ----
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


# ---- the optimiser's parts (csrc/opt.hip: pose blocks, arenas, runners, worker contexts): what the handle owns, every route on one handle ----
OPT_SIZES = dict(max_pose_edges=4096, max_pose_batch=4, max_kf=32, max_mp=512, max_edges=8192)


def opt_parts(max_pose_edges, max_pose_batch, max_kf, max_mp, max_edges):
    """(device, pinned) bytes of every part, transcribed from the allocation paragraph of include/rumi_opt.h."""
    PE, PB, K, M, E = max_pose_edges, max_pose_batch, max_kf, max_mp, max_edges
    r16, r256 = (lambda x: (x + 15) // 16 * 16), (lambda x: (x + 255) // 256 * 256)
    NP = min(r16(6 * K + 1), 256)
    S = 48 * E + 32 * M + 80 * K + 1024
    runner = 15616 + 32 * r256(r16(r16(r16(64 * K) + 24 * M) + E) + 16)
    parts = dict(pose=(34 * PE + 64 * PB + 532, 25 * PE + 64 * PB + 532),
                 W=(233 * E + 232 * M + 672 * K + 2560, S + 64),
                 H=(144 * E + (120 + 24 * NP) * M + 8 * NP * NP + 8 * (6 * K + 2) ** 2 + 96 * K + 64, 128),
                 X=(26088000 + 16 * max(192, (M + 31) // 32) + 2 * r256(4 * M + 4) + 6 * r256(4 * E) + r256(8 * E) + r256(E) + r256(128 * (M // 16 + 2)), 24),
                 R=(runner, runner))
    return {k: np.array(v, np.int64) for k, v in parts.items()}


def ba_window(**cfg):
    b = ba_problem(**cfg)
    return (b["kf_pose"], b["kf_fixed"], b["mp_pos"], b["e_mp"], b["e_kf"], b["e_obs"], b["e_w"], b["K"])


def eligible_windows(n, seed=700):
    """Windows the window-batched kernels take, within OPT_SIZES."""
    return [ba_window(seed=seed + i, n_opt=3 + i % 6, n_fixed=2, n_points=100 + 10 * (i % 11)) for i in range(n)]


def same_bytes(a, b):
    flat = lambda r: [np.asarray(x).tobytes() for x in (r if isinstance(r, (tuple, list)) else [r])]
    if isinstance(a, list):
        return len(a) == len(b) and all(same_bytes(x, y) for x, y in zip(a, b))
    return flat(a) == flat(b)


def test_optimizer_footprint_follows_the_header():
    from rumi_slam_amd.optimizer import Optimizer
    p = opt_parts(**OPT_SIZES)
    o = Optimizer(**OPT_SIZES)
    created = np.array(o.footprint())
    assert (created == p["pose"] + p["W"] + p["H"] + p["R"]).all(), (created, p)
    twelve = eligible_windows(12)                                    # the first count that runs as three launch groups
    o.LocalBundleAdjustmentBatch(twelve, 1)
    batch = np.array(o.footprint())
    assert (batch - created == 12 * (p["W"] + p["X"]) + 2 * p["R"]).all(), (batch - created, p)
    o.LocalBundleAdjustmentBatch(twelve, 1)
    assert (np.array(o.footprint()) == batch).all(), "the same batch again"
    o.LocalBundleAdjustmentBatch(twelve[:3], 1)
    assert (np.array(o.footprint()) == batch).all(), "a smaller batch"
    o.LocalBundleAdjustmentBatch([ba_window(seed=720, n_opt=30, n_fixed=2, n_points=200)], 2)      # 30 optimised key-frames: ba_run's host loop
    assert (np.array(o.footprint()) - batch == p["W"] + p["H"] + p["R"]).all(), "one worker context"
    o.close()


def test_optimizer_every_route_on_one_handle():
    """Batch arenas, a worker context, the handle's own window with its batch extras, the pose blocks, Sim3 and the essential graph in turn on ONE
    handle: no route may find a block that another one left in a state it cannot use.  Every result of a route with a fixed summation order is
    held to the bytes a fresh handle returns for that input alone; the window of 30 key-frames (f64 atomics) to the oracle."""
    from ba_scene import pose_problem
    from rumi_slam_amd.optimizer import Optimizer
    from sim3_scene import sim3_pair_problem
    from test_optimizer_gpu import _check_local_ba
    nine, two, big = eligible_windows(9, 730), eligible_windows(2, 750), ba_window(seed=760, n_opt=30, n_fixed=2, n_points=200)
    single, merge, gba = eligible_windows(3, 770)
    poses = [pose_problem(40 + i, 150 + 37 * i, 0.15) for i in range(3)]
    start = np.cumsum([0] + [len(q["inv_sigma2"]) for q in poses]).astype(np.int32)
    pose_args = (start, np.concatenate([q["Xw"] for q in poses]), np.concatenate([q["obs"] for q in poses]), np.concatenate([q["inv_sigma2"] for q in poses]),
                 poses[0]["K"], np.stack([q["T0"] for q in poses]))
    s = sim3_pair_problem(seed=6, n=60)
    sim3_args = (s["S0"], s["P1c"], s["P2c"], s["obs1"], s["obs2"], s["w1"], s["w2"], s["K"], s["K"])
    eg, eg_it = es.scene("two_free"), es.SCENES["two_free"]["n_it"]
    routes = [("batch of 9", lambda h: h.LocalBundleAdjustmentBatch(nine, 1)),
              ("mixed batch", lambda h: h.LocalBundleAdjustmentBatch(two + [big], 2)),
              ("local BA", lambda h: h.LocalBundleAdjustment(*single)),
              ("merge BA", lambda h: h.MergeBundleAdjustment(*merge)),
              ("global BA", lambda h: h.BundleAdjustment(*gba)),
              ("pose batch", lambda h: h.PoseOptimizationBatch(*pose_args)),
              ("Sim3", lambda h: h.OptimizeSim3(*sim3_args)),
              ("essential graph", lambda h: h.essential_graph(*eg.args(), n_iterations=eg_it)),
              ("batch of 9 again", lambda h: h.LocalBundleAdjustmentBatch(nine, 1))]
    o = Optimizer(**OPT_SIZES)
    for name, call in routes:
        got = call(o)
        fresh = Optimizer(**OPT_SIZES)
        want = call(fresh)
        fresh.close()
        if name == "mixed batch":
            _check_local_ba(dict(kf_pose=big[0], kf_fixed=big[1]), got[2], O.local_ba(*big))
            got, want = got[:2], want[:2]
        assert same_bytes(got, want), name
    o.close()


def test_optimizer_destroyed_after_a_batch_and_created_again():
    from rumi_slam_amd.optimizer import Optimizer
    w = eligible_windows(1, 780)[0]
    fresh = Optimizer(**OPT_SIZES)
    want = fresh.LocalBundleAdjustment(*w)
    fresh.close()
    o = Optimizer(**OPT_SIZES)
    o.LocalBundleAdjustmentBatch(eligible_windows(12, 790) + [ba_window(seed=760, n_opt=30, n_fixed=2, n_points=200)], 2)   # arenas, runners and a worker context to release
    o.close()
    o = Optimizer(**OPT_SIZES)
    assert same_bytes(o.LocalBundleAdjustment(*w), want)
    o.close()
