"""The GPU key-frame database (include/rumi_kfdb.h) against the C++ oracle (tests/cpp/kfdb_oracle.cc): the same key-frames, in the same order,
float scores bit-equal, for the same database contents and call sequence."""
import os
import re

import numpy as np
import pytest

from kfdb_scene import Scene, build_oracle, format_nbest, l1_normalise, run_gpu, run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

NW = 100000


@pytest.fixture(scope="module")
def voc():
    from voc_scene import synthetic_vocabulary_fast
    from rumi_slam_amd.vocabulary import ORBVocabulary
    return ORBVocabulary(*synthetic_vocabulary_fast(5, 10, 5))


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("kfdb"))


def new_db(voc, max_kf=6000, max_entries=2_000_000):
    from rumi_slam_amd.kfdb import KeyFrameDatabase
    return KeyFrameDatabase(voc, max_kf, max_entries)


def check(voc, oracle, script, batch=True, **kw):
    want = run_oracle(oracle, script)
    db = new_db(voc, **kw)
    got = run_gpu(db, script, batch=batch)
    db.close()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    return want


def scene_script(sc, n_reloc, n_nbest, n_cand, seed):
    rng = np.random.default_rng(seed)
    s = sc.add_commands() + sc.cov_commands()
    qid = 1_000_000
    for _ in range(n_reloc):
        i = int(rng.integers(len(sc.ids)))
        w, v = sc.query_bow(place=sc.place_of[i])
        s.append(("R", qid, sc.maps[i], w, v)); qid += 1
    for _ in range(n_nbest):                     # a new key-frame near key-frame i, connected to i and its covisibles
        i = int(rng.integers(len(sc.ids)))
        w, v = sc.query_bow(place=sc.place_of[i])
        s.append(("N", qid, sc.maps[i], n_cand, [sc.ids[i]] + sc.connected(i), w, v)); qid += 1
    return s


def test_kfdb_symbols():
    from rumi_slam_amd import capi
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "rumi_kfdb.h")).read()
    declared = set(re.findall(r"\b(rumi_kfdb_\w+)\s*\(", hdr))
    assert declared == set(capi.KFDB_SYMBOLS)
    for name in declared:
        getattr(L, name)


@pytest.mark.parametrize("n_kf,n_maps,n_cand", [(1, 1, 1), (50, 2, 3), (500, 3, 5), (5000, 2, 3)])
def test_queries_against_oracle(voc, oracle, n_kf, n_maps, n_cand):
    sc = Scene(11 + n_kf, n_kf, n_maps, n_words=NW)
    script = scene_script(sc, 12, 12, n_cand, n_kf)
    out = check(voc, oracle, script)
    assert any(len(l.split("|")[1].split()) > 1 for l in out) or n_kf == 1


@pytest.mark.parametrize("n_cand", [1, 3, 5])
def test_nbest_n(voc, oracle, n_cand):
    sc = Scene(3, 400, 3, n_words=NW)
    check(voc, oracle, scene_script(sc, 0, 20, n_cand, 7))


def test_batch_of_64_equals_single_calls(voc, oracle):
    sc = Scene(21, 800, 2, n_words=NW)
    script = scene_script(sc, 32, 32, 3, 9)
    batched = check(voc, oracle, script, batch=True)
    db = new_db(voc)
    single = run_gpu(db, script, batch=False)
    assert single == batched


def test_identical_bow_vectors_keep_list_order(voc, oracle):
    rng = np.random.default_rng(1)
    w, v = l1_normalise(rng.choice(NW, 40, replace=False), rng.uniform(0.1, 2, 40))
    s = [("A", 10 + i, 1 + (i % 2), w, v) for i in range(30)]
    s += [("V", 10 + i, [10 + (i + 1) % 30, 10 + (i + 2) % 30]) for i in range(30)]
    s += [("R", 500, 1, w, v), ("N", 501, 1, 5, [], w, v), ("N", 502, 2, 3, [11, 13], w, v)]
    out = check(voc, oracle, s)
    assert len(out[0].split("|")[1].split()) == 30


def test_empty_and_disjoint_queries(voc, oracle):
    sc = Scene(4, 60, 1, n_words=NW)
    used = set(int(x) for b in sc.bows for x in b[0])
    free = np.array([x for x in range(NW) if x not in used][:20], np.uint32)
    fw, fv = l1_normalise(free, np.ones(20))
    e = (np.zeros(0, np.uint32), np.zeros(0))
    s = sc.add_commands() + sc.cov_commands() + [("R", 7, 1, *e), ("R", 8, 1, fw, fv), ("N", 9, 1, 3, [], *e), ("N", 10, 1, 3, [], fw, fv)]
    out = check(voc, oracle, s)
    assert out == ["R 7 | |", "R 8 | |", "N 9 | | |", "N 10 | | |"]


def test_loop_list_full_merge_continues_and_bad_map(voc, oracle):
    rng = np.random.default_rng(2)
    base = rng.choice(NW, 50, replace=False)
    s = []
    for i in range(40):                          # maps 1..4 interleaved, all near one place
        w = np.concatenate([base[:45], rng.integers(0, NW, 5)])
        s.append(("A", 100 + i, 1 + i % 4, *l1_normalise(w, rng.uniform(0.1, 2, 50))))
    q = l1_normalise(base, rng.uniform(0.1, 2, 50))
    s += [("N", 900, 1, 2, [], *q), ("B", 3, 1), ("N", 901, 1, 5, [], *q), ("N", 902, 2, 3, [], *q), ("B", 3, 0), ("N", 903, 1, 5, [], *q)]
    out = check(voc, oracle, s)
    loop, merge = out[0].split("|")[2].split(), out[0].split("|")[3].split()
    assert len(loop) == 2 and len(merge) == 2
    assert not any(int(x) % 4 == 2 for x in out[1].split("|")[3].split())      # map 3 (ids 102, 106, ...) is bad


def _stale_scene(kind):
    rng = np.random.default_rng(3)
    W1 = rng.choice(NW // 2, 50, replace=False)
    W2 = NW // 2 + rng.choice(NW // 2, 50, replace=False)
    X = l1_normalise(W1, rng.uniform(0.1, 2, 50))
    P = l1_normalise(np.concatenate([W2, W1[:1]]), rng.uniform(0.1, 2, 51))
    B = l1_normalise(np.concatenate([W2[:40], W1[:1], rng.integers(0, NW // 2, 5)]), rng.uniform(0.1, 2, 46))
    s = [("A", 1, 1, *X), ("A", 2, 1, *P), ("V", 2, [1])]
    if kind == "R":
        s += [("R", 100, 1, *X), ("R", 101, 1, *B)]
    else:
        s += [("N", 100, 1, 3, [], *X), ("N", 101, 1, 3, [], *B)]
    return s


@pytest.mark.parametrize("kind", ["R", "N"])
def test_stale_score_sequence(voc, oracle, kind):
    """Query A scores X (si 1); query B marks X below the word threshold, and X is the covisible of the scored P: B takes X's stale score, so its
    best key-frame is X.  A fresh 0 would give P."""
    s = _stale_scene(kind)
    out = check(voc, oracle, s, batch=False)
    b = out[1].split("|")
    assert [p.split(":")[0] for p in b[1].split()] == ["2"]           # only P is scored by B
    assert b[2].split() == ["1"]                                      # ... and the candidate is X, by its stale score
    # the same two queries in one batched call
    out2 = check(voc, oracle, s, batch=True)
    assert out2 == out


def test_visible_below_equals_interleaved_query_then_add(voc, oracle):
    from rumi_slam_amd.kfdb import KeyFrameDatabase
    sc = Scene(8, 300, 2, n_words=NW)
    B = 64
    pre = list(range(len(sc.ids) - B))
    inter = []
    for i in range(len(sc.ids) - B, len(sc.ids)):
        inter.append(("N", sc.ids[i], sc.maps[i], 3, sc.connected(i), sc.bows[i][0], sc.bows[i][1]))
        inter.append(("A", sc.ids[i], sc.maps[i], sc.bows[i][0], sc.bows[i][1]))
    script = sc.add_commands(pre) + sc.cov_commands(pre) + inter
    want = run_oracle(oracle, script)
    db = KeyFrameDatabase(voc, 1000, 200000)
    run_gpu(db, sc.add_commands(pre) + sc.cov_commands(pre))
    base = db.next_seq()
    tail = list(range(len(sc.ids) - B, len(sc.ids)))
    db.add([sc.ids[i] for i in tail], [sc.maps[i] for i in tail], [sc.bows[i] for i in tail])
    res, scored = db.detect_nbest_candidates([sc.ids[i] for i in tail], [sc.maps[i] for i in tail], [sc.bows[i] for i in tail],
                                             [sc.connected(i) for i in tail], 3, visible_below=[base + b for b in range(B)], with_scored=True)
    got = [format_nbest(sc.ids[i], s, lp, mg) for i, s, (lp, mg) in zip(tail, scored, res)]
    assert got == want


def test_erase_clear_map_readd(voc, oracle):
    sc = Scene(9, 400, 3, n_words=NW)
    s = scene_script(sc, 6, 6, 3, 1)
    s += [("E", sc.ids[i]) for i in range(0, 400, 7)]
    s += scene_script(sc, 6, 6, 3, 2)[800:]
    s += [("K", sc.ids[5], 3), ("M", 2)]
    s += scene_script(sc, 6, 6, 3, 3)[800:]
    back = [i for i in range(400) if sc.maps[i] == 2 and i != 5][:50]
    s += sc.add_commands(back) + sc.cov_commands(back) + scene_script(sc, 6, 6, 3, 4)[800:]
    s += [("C",)] + sc.add_commands(range(100)) + sc.cov_commands(range(100)) + scene_script(sc, 6, 6, 3, 5)[800:]
    check(voc, oracle, s, max_kf=500, max_entries=40000)


def test_capacity_and_refusals(voc):
    from rumi_slam_amd import capi
    from rumi_slam_amd.kfdb import KeyFrameDatabase
    from rumi_slam_amd.vocabulary import ORBVocabulary, L2_NORM
    from voc_scene import synthetic_vocabulary
    db = KeyFrameDatabase(voc, 4, 100)
    w, v = l1_normalise(np.arange(30), np.ones(30))
    db.add([1, 2, 3], [1, 1, 1], [(w, v)] * 3)
    with pytest.raises(capi.RumiError) as e:
        db.add([4, 5], [1, 1], [(w, v)] * 2)
    assert e.value.code == capi.RUMI_E_CAPACITY
    with pytest.raises(capi.RumiError) as e:
        db.add([4], [1], [(np.arange(40), np.ones(40) / 40)])
    assert e.value.code == capi.RUMI_E_CAPACITY
    assert db.size() == 3
    with pytest.raises(capi.RumiError) as e:
        db.add([3], [1], [(w, v)])
    assert e.value.code == capi.RUMI_E_INVALID
    with pytest.raises(capi.RumiError) as e:
        db.detect_relocalization_candidates([5, 5], [1, 1], [(w, v)] * 2)
    assert e.value.code == capi.RUMI_E_INVALID
    db.erase([1])
    db.add([4], [1], [(w, v)])                   # room again
    assert db.size() == 3
    l2 = ORBVocabulary(*synthetic_vocabulary(1, 4, 3), scoring=L2_NORM)
    with pytest.raises(capi.RumiError) as e:
        KeyFrameDatabase(l2, 10, 100)
    assert e.value.code == capi.RUMI_E_INVALID


def test_add_batch_device_matches_voc_assemble():
    import torch
    from voc_scene import synthetic_vocabulary_fast
    from rumi_slam_amd.extractor import ORBextractor
    from rumi_slam_amd.kfdb import KeyFrameDatabase
    from rumi_slam_amd.synth import synth_frame
    from rumi_slam_amd.vocabulary import ORBVocabulary
    voc = ORBVocabulary(*synthetic_vocabulary_fast(21, 10, 6))
    ext = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=16)
    frames = torch.from_numpy(np.stack([synth_frame(300 + i) for i in range(16)])).cuda()
    _, desc, counts = ext.extract_batch(frames, (0, 1000), cap=1100)
    word, weight, node = voc.transform_batch(desc, counts)
    torch.cuda.synchronize()
    db = KeyFrameDatabase(voc, 64, 64 * 1200)
    ids = np.arange(1, 17, dtype=np.uint64)
    db.add_batch_device(ids, np.ones(16, np.int32), word, weight, counts)
    wh, vh, nh, ch = word.cpu().numpy().view(np.uint32), weight.cpu().numpy(), node.cpu().numpy().view(np.uint32), counts.cpu().numpy()
    for f in range(16):
        n = int(ch[f, 0])
        (bi, bv), _ = voc.assemble(wh[f, :n], vh[f, :n], nh[f, :n])
        gw, gv = db.bow(ids[f])
        assert np.array_equal(gw, bi)
        assert gv.tobytes() == bv.tobytes()


def test_refresh_between_score_and_select(voc, oracle):
    """The covisibility rows and isBad() flags of the scored key-frames are set between score and select (what the facade does); the result
    equals the oracle's with the new covisibility (and bad flags) in place before the queries, and differs from the stale rows' result."""
    sc = Scene(31, 400, 2, n_words=NW)
    base = scene_script(sc, 0, 0, 3, 0)
    queries = [c for c in scene_script(sc, 0, 24, 3, 5)[len(base):]]
    new_cov = {sc.ids[i]: list(reversed(sc.covisibles(i)))[1:] + ([sc.ids[i + 15]] if i + 15 < len(sc.ids) and sc.maps[i + 15] == sc.maps[i] else [])
               for i in range(len(sc.ids))}
    db = new_db(voc)
    run_gpu(db, base)
    bad = []

    def between(scored):
        ids = sorted(set(int(x) for ids_q, _ in scored for x in ids_q))
        db.set_covisibles(ids, [new_cov[i] for i in ids])
        if not bad and ids:
            bad.append(ids[0])
            db.set_bad([ids[0]], [1])

    res, scored = db.detect_nbest_candidates([q[1] for q in queries], [q[2] for q in queries], [(q[5], q[6]) for q in queries],
                                             [q[4] for q in queries], 3, with_scored=True, between=between)
    got = [format_nbest(q[1], s, lp, mg) for q, s, (lp, mg) in zip(queries, scored, res)]
    assert bad
    want = run_oracle(oracle, base + [("V", i, c) for i, c in new_cov.items()] + [("D", bad[0], 1)] + queries)
    assert got == want
    stale = run_oracle(oracle, base + queries)
    assert want != stale                        # the refresh changes the answer


def test_pool_compaction_with_staged_adds(voc, oracle):
    """A small entry pool: erases leave holes, and the next staged adds only fit after the pool is compacted (flush)."""
    sc = Scene(41, 140, 2, n_words=NW)
    s = sc.add_commands(range(100)) + sc.cov_commands(range(100)) + scene_script(sc, 4, 4, 3, 1)[280:]
    s += [("E", sc.ids[i]) for i in range(0, 100, 2)]
    s += sc.add_commands(range(100, 140)) + sc.cov_commands(range(140)) + [("D", sc.ids[101], 1)] + scene_script(sc, 6, 6, 3, 2)[280:]
    n_entries = sum(len(b[0]) for b in sc.bows[:100])
    check(voc, oracle, s, max_kf=128, max_entries=n_entries + 100)
