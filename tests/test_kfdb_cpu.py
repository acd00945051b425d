"""The C++ key-frame database oracle (tests/cpp/kfdb_oracle.cc) against a tiny pure-Python restatement of KeyFrameDatabase.cc's two queries,
on hand-built cases, and the scene generator of tests/kfdb_scene.py.  CPU only."""
import numpy as np
import pytest

from kfdb_scene import Scene, build_oracle, l1_normalise, run_oracle, to_text


def f32(x):
    return float(np.float32(x))


def f32hex(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


class PyDB:
    """KeyFrameDatabase.cc:604-708 (N-best) and :733-843 (reloc), float arithmetic through numpy float32."""

    def __init__(self):
        self.kf, self.inv, self.indb, self.badmaps = {}, {}, set(), set()

    def run(self, script):
        out = []
        for c in script:
            op = c[0]
            if op == "A":
                k = self.kf.setdefault(c[1], dict(rq=0, rs=0.0, pq=0, ps=0.0))
                k.update(map=c[2], bow=dict(zip((int(x) for x in c[3]), (float(x) for x in c[4]))), cov=[], bad=False)
                for w in k["bow"]:
                    self.inv.setdefault(w, []).append(c[1])
                self.indb.add(c[1])
            elif op == "E":
                self._erase(c[1])
            elif op == "M":
                for i in [i for i in self.indb if self.kf[i]["map"] == c[1]]:
                    self._erase(i)
            elif op == "B":
                (self.badmaps.add if c[2] else self.badmaps.discard)(c[1])
            elif op == "V":
                if c[1] in self.indb:
                    self.kf[c[1]]["cov"] = [x for x in c[2] if x in self.indb]
            elif op == "R":
                out.append(self._query("R", c[1], c[2], set(), dict(zip((int(x) for x in c[3]), (float(x) for x in c[4]))), None))
            elif op == "N":
                out.append(self._query("N", c[1], c[2], set(c[4]), dict(zip((int(x) for x in c[5]), (float(x) for x in c[6]))), c[3]))
        return out

    def _erase(self, i):
        if i not in self.indb:
            return
        for w in self.kf[i]["bow"]:
            self.inv[w].remove(i)
        self.indb.discard(i)
        for k in self.kf.values():
            if "cov" in k:
                k["cov"] = [x for x in k["cov"] if x != i]

    @staticmethod
    def score(a, b):
        s = 0.0
        for w in sorted(set(a) & set(b)):
            v, u = a[w], b[w]
            s += abs(v - u) - abs(v) - abs(u)
        return f32(-s / 2.0)

    def _query(self, kind, qid, qmap, conn, bow, N):
        q, sc = ("rq", "rs") if kind == "R" else ("pq", "ps")
        listed, words = [], {}
        for w in sorted(bow):
            for i in self.inv.get(w, []):
                k = self.kf[i]
                if k[q] != qid:
                    words[i] = 0
                    if i not in conn:
                        k[q] = qid
                        listed.append(i)
                words[i] = words.get(i, 0) + 1
        line = f"{kind} {qid} |"
        if not listed:
            return line + (" |" if kind == "R" else " | |")
        mx = max(words[i] for i in listed)
        mn = int(f32(np.float32(mx) * np.float32(0.8)))
        scored = []
        for i in listed:
            if words[i] > mn:
                s = self.score(bow, self.kf[i]["bow"])
                self.kf[i][sc] = s
                scored.append((s, i))
        line += "".join(f" {i}:{f32hex(s)}" for s, i in scored) + " |"
        acc = []
        best_acc = np.float32(0)
        for s, i in scored:
            a, b, bi = np.float32(s), np.float32(s), i
            for x in self.kf[i]["cov"]:
                if self.kf[x][q] != qid:
                    continue
                a = np.float32(a + np.float32(self.kf[x][sc]))
                if np.float32(self.kf[x][sc]) > b:
                    b, bi = np.float32(self.kf[x][sc]), x
            acc.append((a, bi))
            best_acc = max(best_acc, a)
        if kind == "R":
            th, seen, out = np.float32(0.75) * best_acc, set(), []
            for a, i in acc:
                if a > th and self.kf[i]["map"] == qmap and i not in seen:
                    out.append(i); seen.add(i)
            return line + "".join(f" {i}" for i in out)
        acc = sorted(acc, key=lambda t: -t[0])        # stable, as std::list::sort
        loop, merge, seen = [], [], set()
        for a, i in acc:
            if not (len(loop) < N or len(merge) < N):
                break
            if i in seen:
                continue
            m = self.kf[i]["map"]
            if m == qmap and len(loop) < N:
                loop.append(i)
            elif m != qmap and len(merge) < N and m not in self.badmaps:
                merge.append(i)
            seen.add(i)
        return line + "".join(f" {i}" for i in loop) + " |" + "".join(f" {i}" for i in merge)


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
