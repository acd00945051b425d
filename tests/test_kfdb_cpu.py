"""The C++ key-frame database oracle (tests/cpp/kfdb_oracle.cc) against a tiny pure-Python restatement of KeyFrameDatabase.cc's two queries
(kfdb_cases.PyDB),
on hand-built cases, and the scene generator of tests/kfdb_scene.py.  CPU only."""
import numpy as np
import pytest

from kfdb_cases import PyDB
from kfdb_scene import Scene, build_oracle, l1_normalise, run_oracle, to_text


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return build_oracle(tmp_path_factory.mktemp("kfdb_cpu"))


def bow(words, vals=None):
    return l1_normalise(np.asarray(words), np.ones(len(words)) if vals is None else np.asarray(vals, float))


def same(oracle, script):
    want = run_oracle(oracle, script)
    assert PyDB().run(script) == want
    return want


def test_ties_keep_list_order(oracle):
    b = bow(range(20))
    s = [("A", i, 1, *b) for i in (5, 3, 9, 1)] + [("N", 50, 1, 4, [], *b), ("R", 51, 1, *b)]
    out = same(oracle, s)
    assert out[0].split("|")[2].split() == ["5", "3", "9", "1"]     # add order (same first word), acc ties keep it


def test_list_order_is_first_shared_word_then_add_order(oracle):
    s = [("A", 1, 1, *bow([30, 31, 32])), ("A", 2, 1, *bow([10, 30, 31])), ("A", 3, 1, *bow([20, 30, 32]))]
    s += [("R", 9, 1, *bow([10, 20, 30, 31, 32]))]
    out = same(oracle, s)
    assert [p.split(":")[0] for p in out[0].split("|")[1].split()] == ["2", "3", "1"]


def test_stale_score_and_connected_set(oracle):
    X, P = bow(range(0, 30)), bow(list(range(100, 130)) + [0])
    s = [("A", 1, 1, *X), ("A", 2, 1, *P), ("A", 3, 1, *P), ("V", 2, [1]), ("N", 10, 1, 3, [], *X),
         ("N", 11, 1, 3, [3], *bow(list(range(100, 125)) + [0])), ("N", 12, 1, 3, [1, 2, 3], *X)]
    out = same(oracle, s)
    assert out[1].split("|")[2].split() == ["1"]                     # P's best is X, by X's stale score from query 10
    assert "3:" not in out[1]                                        # 3 is connected: never listed
    assert out[2] == "N 12 | | |"


def test_full_loop_list(oracle):
    b = bow(range(40))
    s = [("A", 10 + i, 1 + i % 2, *b) for i in range(8)] + [("B", 2, 1), ("N", 99, 1, 2, [], *b), ("B", 2, 0), ("N", 98, 1, 2, [], *b)]
    out = same(oracle, s)
    assert out[0].split("|")[2].split() == ["10", "12"] and out[0].split("|")[3].split() == []
    assert out[1].split("|")[3].split() == ["11", "13"]


def test_scene_generator():
    sc = Scene(1, 200, 3, n_words=5000)
    assert len(sc.ids) == 200 and set(sc.maps) == {1, 2, 3}
    for w, v in sc.bows[:20]:
        assert np.all(np.diff(w.astype(np.int64)) > 0) and abs(v.sum() - 1) < 1e-12
    share = [len(set(sc.bows[i][0]) & set(sc.bows[i + 1][0])) for i in range(60) if sc.maps[i] == sc.maps[i + 1]]
    assert np.median(share) > 15                                    # consecutive key-frames share a third of their words or more
    cov = sc.covisibles(10)
    assert 0 < len(cov) <= 10 and all(sc.maps[sc.ids.index(c)] == sc.maps[10] for c in cov)
    assert to_text([("A", 1, 1, np.array([3], np.uint32), np.array([0.5]))]) == "A 1 1 1 3 0x1.0000000000000p-1\n"


def test_scene_queries_python_equals_oracle(oracle):
    sc = Scene(2, 120, 2, n_words=3000)
    s = sc.add_commands() + sc.cov_commands()
    for q in range(10):
        w, v = sc.query_bow(place=sc.place_of[q * 11])
        s.append(("R", 500 + q, sc.maps[q * 11], w, v))
        s.append(("N", 600 + q, sc.maps[q * 11], 3, [sc.ids[q * 11]], w, v))
    same(oracle, s)


def test_oracle_vocabulary_bow_vectors(oracle):
    """BowVectors made by the CPU restatement of DBoW2's transform (oracle_lib.OracleVocabulary) on a voc_scene tree."""
    import oracle_lib
    from voc_scene import synthetic_vocabulary
    voc = oracle_lib.OracleVocabulary(*synthetic_vocabulary(4, 10, 3))
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    s = []
    for i in range(12):
        d = base.copy()
        d[rng.random(300) < 0.3] = rng.integers(0, 256, 32, dtype=np.uint8)
        (w, v), _ = voc.transform(d)
        s.append(("A", i + 1, 1 + i % 2, w, v))
    (w, v), _ = voc.transform(base)
    s += [("V", 1, [2, 3]), ("R", 100, 1, w, v), ("N", 101, 2, 2, [2], w, v)]
    out = same(oracle, s)
    assert len(out[0].split("|")[1].split()) >= 1
