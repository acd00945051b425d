"""Constructed cases for the key-frame database (include/rumi_kfdb.h; the k_q_* kernels and k_bow_assemble of rumi_slam_amd/csrc/kfdb.hip): tiny
hand-made databases in which one value stands ON an edge of one comparison of DetectRelocalizationCandidates or DetectNBestCandidates.

The database takes word values as given (only ascending word ids are checked), so every value here is dyadic: with positive values the L1 score
is the sum of min(v, w) over the common words, exact in double, and every float an output line shows is written down by hand.  Nothing here needs a
GPU or the C++ oracle to BUILD a case.  A case holds a script in the command format of kfdb_scene.py, the expected output lines in the oracle's text
format, the rule it stands on (file:line of the modelled project, never its text) and one sentence naming the edge.

Two additions to the command format: an "R" or "N" command may carry one more element, `visible_below` as a number of adds counted from the start of
the script (the device's visible_below argument); the oracle has no such argument, so such a case also gives `oracle_script`, the same calls with
each query moved in front of the adds it must not see.

``PyDB`` is the plain restatement of the two queries (float arithmetic through numpy float32).  ``PyDB(deviation)`` is the same with one subtle error
a kernel could make (``DEVIATIONS``); ``BITES`` names the cases that must then fail.  Every case is audited when it is built: ``near_edges`` replays
PyDB's trace in exact arithmetic (fractions.Fraction) and reports each float decision that is on or within ``CLEAR_ULPS`` ulps of an edge, and
each sum that rounds; a case must declare exactly the kinds it means to stand on (``edges``), so nothing else is near one by accident.

Rules.  KeyFrameDatabase.cc (KFD below) and DBoW2/ScoringObject.cpp (SO):
  listing      KFD:748-752 (reloc), KFD:623-630 (N-best, connected key-frames left out)
  word gate    KFD:769, :780 (reloc), KFD:648, :659 (N-best)
  score        SO:23-68, called at KFD:783 / :662
  accumulate   KFD:801-820 (reloc), KFD:680-699 (N-best)
  reloc walk   KFD:824-840
  N-best walk  KFD:702 (sort), :709-729

Families (``COVERAGE`` names the cases per family and query kind, ``NOT_APPLICABLE`` the reason where there is none):
  W word threshold   S score   L list order   A covisibility accumulation   R reloc walk   N N-best walk   V visibility   T batching"""
import math
from fractions import Fraction

import numpy as np

NW = 100000                     # words of synthetic_vocabulary_fast(5, 10, 5), the vocabulary of the GPU tests
CLEAR_ULPS = 4
FAMILIES = "WSLARNVT"
DEVIATIONS = ("word_ge", "thr_double", "acc_reverse", "si_pairwise", "best_ge", "sort_unstable", "list_by_id", "vis_le", "max_first256")


def f32(x):
    return float(np.float32(x))


def f32hex(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


def _ulp(x):
    """float32 ulp at |x| (the smallest subnormal at 0)."""
    x = abs(float(x))
    if x == 0.0:
        return Fraction(1, 2 ** 149)
    return Fraction(2) ** (math.frexp(x)[1] - 1 - 23)


def _pairwise(t):
    if len(t) == 0:
        return 0.0
    if len(t) == 1:
        return t[0]
    return _pairwise(t[:len(t) // 2]) + _pairwise(t[len(t) // 2:])


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
class PyDB:
    """KFD:604-708 (N-best) and :733-843 (reloc), float arithmetic through numpy float32.  `deviation`: one of DEVIATIONS, or None for the rule.
    `trace` keeps, per query, what near_edges needs."""

    def __init__(self, deviation=None):
        assert deviation is None or deviation in DEVIATIONS
        self.dev = deviation
        self.kf, self.inv, self.indb, self.badmaps = {}, {}, set(), set()
        self.seq = 0
        self.trace = []

    def run(self, script):
        out = []
        base = self.seq
        for c in script:
            op = c[0]
            if op == "A":
                k = self.kf.setdefault(c[1], dict(rq=0, rs=0.0, pq=0, ps=0.0))
                k.update(map=c[2], bow=dict(zip((int(x) for x in c[3]), (float(x) for x in c[4]))), cov=[], bad=False, seq=self.seq)
                self.seq += 1
                for w in k["bow"]:
                    self.inv.setdefault(w, []).append(c[1])
                self.indb.add(c[1])
            elif op == "E":
                self._erase(c[1])
            elif op == "M":
                for i in [i for i in self.indb if self.kf[i]["map"] == c[1]]:
                    self._erase(i)
            elif op == "C":
                for i in list(self.indb):
                    self._erase(i)
            elif op == "B":
                (self.badmaps.add if c[2] else self.badmaps.discard)(c[1])
            elif op == "K":
                if c[1] in self.indb:
                    self.kf[c[1]]["map"] = c[2]
            elif op == "D":
                if c[1] in self.indb:
                    self.kf[c[1]]["bad"] = bool(c[2])
            elif op == "V":
                if c[1] in self.indb:
                    self.kf[c[1]]["cov"] = [x for x in c[2] if x in self.indb]
            elif op == "R":
                vb = base + c[5] if len(c) > 5 else None
                out.append(self._query("R", c[1], c[2], set(), dict(zip((int(x) for x in c[3]), (float(x) for x in c[4]))), None, vb))
            elif op == "N":
                vb = base + c[7] if len(c) > 7 else None
                out.append(self._query("N", c[1], c[2], set(c[4]), dict(zip((int(x) for x in c[5]), (float(x) for x in c[6]))), c[3], vb))
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

    def _terms(self, a, b):
        return [abs(a[w] - b[w]) - abs(a[w]) - abs(b[w]) for w in sorted(set(a) & set(b))]

    def score(self, a, b):
        t = self._terms(a, b)
        if self.dev == "si_pairwise":
            s = _pairwise(t)
        else:
            s = 0.0
            for x in t:
                s += x
        return f32(-s / 2.0)

    @staticmethod
    def score_exact(a, b):
        s = Fraction(0)
        for w in set(a) & set(b):
            v, u = Fraction(a[w]), Fraction(b[w])
            s += abs(v - u) - abs(v) - abs(u)
        return -s / 2

    def _query(self, kind, qid, qmap, conn, bow, N, vb):
        q, sc = ("rq", "rs") if kind == "R" else ("pq", "ps")
        listed, words, first = [], {}, {}
        for r, w in enumerate(sorted(bow)):
            for i in self.inv.get(w, []):
                k = self.kf[i]
                if vb is not None and (k["seq"] > vb if self.dev == "vis_le" else k["seq"] >= vb):
                    continue
                if k[q] != qid:
                    words[i] = 0
                    if i not in conn:
                        k[q] = qid
                        listed.append(i)
                        first[i] = r
                words[i] = words.get(i, 0) + 1
        if self.dev == "list_by_id":
            listed.sort(key=lambda i: (first[i], i))
        tr = dict(kind=kind, qid=qid, si=[], best=[], acc=[])
        self.trace.append(tr)
        line = f"{kind} {qid} |"
        if not listed:
            return line + (" |" if kind == "R" else " | |")
        mx = max(words[i] for i in listed)
        mn = int(f32(np.float32(mx) * np.float32(0.8)))
        scored = []
        for i in listed:
            if words[i] >= mn if self.dev == "word_ge" else words[i] > mn:
                s = self.score(bow, self.kf[i]["bow"])
                self.kf[i][sc] = s
                scored.append((s, i))
                tr["si"].append((i, s, self.score_exact(bow, self.kf[i]["bow"])))
        line += "".join(f" {i}:{f32hex(s)}" for s, i in scored) + " |"
        acc = []
        for s, i in scored:
            a, b, bi = np.float32(s), np.float32(s), i
            exact = Fraction(float(s))
            cov = self.kf[i]["cov"]
            for x in (reversed(cov) if self.dev == "acc_reverse" else cov):
                if self.kf[x][q] != qid:
                    continue
                v = np.float32(self.kf[x][sc])
                a = np.float32(a + v)
                exact += Fraction(float(v))
                tr["best"].append((i, x, float(v), float(b)))
                if v >= b if self.dev == "best_ge" else v > b:
                    b, bi = v, x
            acc.append((a, bi))
            tr["acc"].append((i, float(a), exact))
        top = acc[:256] if self.dev == "max_first256" else acc
        best_acc = np.float32(0)
        for a, _ in top:
            if a > best_acc:
                best_acc = a
        if kind == "R":
            seen, out = set(), []
            for a, i in acc:
                keep = float(a) > 0.75 * float(best_acc) if self.dev == "thr_double" else a > np.float32(0.75) * best_acc
                if keep and self.kf[i]["map"] == qmap and i not in seen:
                    out.append(i); seen.add(i)
            return line + "".join(f" {i}" for i in out)
        order = sorted(range(len(acc)), key=(lambda j: (-acc[j][0], -j)) if self.dev == "sort_unstable" else (lambda j: -acc[j][0]))   # stable, as std::list::sort
        loop, merge, seen = [], [], set()
        for j in order:
            i = acc[j][1]
            if not (len(loop) < N or len(merge) < N):
                break
            if self.kf[i]["bad"]:
                continue
            if i in seen:
                continue
            m = self.kf[i]["map"]
            if m == qmap and len(loop) < N:
                loop.append(i)
            elif m != qmap and len(merge) < N and m not in self.badmaps:
                merge.append(i)
            seen.add(i)
        return line + "".join(f" {i}" for i in loop) + " |" + "".join(f" {i}" for i in merge)


def near_edges(trace):
    """The kinds of float edge the queries of a PyDB trace stand on or within CLEAR_ULPS ulps of, in exact arithmetic:
    si_round   an L1 score whose exact value is no float (the fold order and the final rounding show)
    acc_round  an accumulated score whose exact sum is no float (the association shows)
    best_tie   a covisible's score within reach of the running best score
    thr        reloc: an accumulated score within reach of 0.75 x the best one
    acc_tie    N-best: two list entries whose accumulated scores are within reach of each other"""
    kinds = set()
    for tr in trace:
        if any(Fraction(s) != e for _, s, e in tr["si"]):
            kinds.add("si_round")
        if any(Fraction(a) != e for _, a, e in tr["acc"]):
            kinds.add("acc_round")
        if any(abs(Fraction(v) - Fraction(b)) <= CLEAR_ULPS * _ulp(b) for _, _, v, b in tr["best"]):
            kinds.add("best_tie")
        accs = [e for _, _, e in tr["acc"]]
        if tr["kind"] == "R" and accs:
            th = Fraction(3, 4) * max(max(accs), Fraction(0))
            if th > 0 and any(abs(a - th) <= CLEAR_ULPS * _ulp(float(th)) for a in accs):
                kinds.add("thr")
        if tr["kind"] == "N":
            s = sorted(accs)
            if any(y - x <= CLEAR_ULPS * _ulp(float(y)) for x, y in zip(s, s[1:])):
                kinds.add("acc_tie")
    return kinds


# ---------------------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------------------
W16 = list(range(100, 116))     # the 16 words most cases share


def vec(words, vals):
    """(word ids, values); a scalar value goes to every word."""
    w = np.asarray(list(words), np.uint32)
    v = np.full(len(w), vals, np.float64) if np.isscalar(vals) else np.asarray(list(vals), np.float64)
    assert len(w) == len(v) and np.all(np.diff(w.astype(np.int64)) > 0), "BowVector words must ascend"
    return w, v


def A(kid, kmap, words, vals):
    return ("A", kid, kmap, *vec(words, vals))


def Rq(qid, qmap, words, vals, vb=None):
    return ("R", qid, qmap, *vec(words, vals)) + (() if vb is None else (vb,))


def Nq(qid, qmap, n, conn, words, vals, vb=None):
    return ("N", qid, qmap, n, list(conn), *vec(words, vals)) + (() if vb is None else (vb,))


def rline(qid, scored, cand):
    """scored: "id:bits id:bits"; cand: "id id"."""
    return f"R {qid} |" + (" " + scored if scored else "") + " |" + (" " + cand if cand else "")


def nline(qid, scored, loop, merge):
    return f"N {qid} |" + (" " + scored if scored else "") + " |" + (" " + loop if loop else "") + " |" + (" " + merge if merge else "")


def ids(seq):
    return " ".join(str(i) for i in seq)


def pairs(seq, bits):
    return " ".join(f"{i}:{bits}" for i in seq)


class Case:
    def __init__(self, name, family, script, expect, rule, edge, edges=(), oracle_script=None):
        assert family in FAMILIES and name.startswith(family + "_")
        self.name, self.family, self.script, self.expect, self.rule, self.edge = name, family, script, expect, rule, edge
        self.edges = set(edges)
        self.oracle_script = script if oracle_script is None else oracle_script
        self.kinds = {c[0] for c in script if c[0] in "RN"}
        db = PyDB()
        db.run(script)
        got = near_edges(db.trace)
        assert got == self.edges, (name, "stands near", sorted(got), "but declares", sorted(self.edges))

    def __repr__(self):
        return self.name


CASES = []


def case(*a, **kw):
    CASES.append(Case(*a, **kw))


Q16 = (W16, 1 / 16)                                             # the usual query: si of an identical key-frame is 1.0
V1 = (W16, 1 / 16)                                              # si 1.0     3f800000
V9375 = (W16, [1 / 16] * 14 + [1 / 32] * 2)                     # si 0.9375  3f700000
V875 = (W16, [1 / 16] * 12 + [1 / 32] * 4)                      # si 0.875   3f600000
V75 = (W16, [1 / 16] * 8 + [1 / 32] * 8)                        # si 0.75    3f400000
V6875 = (W16, [1 / 16] * 6 + [1 / 32] * 10)                     # si 0.6875  3f300000
V5 = (W16, 1 / 32)                                              # si 0.5     3f000000
V25 = (W16, 1 / 64)                                             # si 0.25    3e800000
V125 = (W16, 1 / 128)                                           # si 0.125   3e000000

# ---------------------------------------------------------------------------------------------------------------------------------
# W: the word threshold.  Values 1/32 everywhere, so si = (common words) / 32.
# ---------------------------------------------------------------------------------------------------------------------------------
_W = {  # maxCommonWords: (minCommonWords, bits of (min + 1) / 32, bits of max / 32)
    1: (0, "3d000000", "3d000000"), 4: (3, "3e000000", "3e000000"), 5: (4, "3e200000", "3e200000"), 6: (4, "3e200000", "3e400000"),
    9: (7, "3e800000", "3e900000"), 10: (8, "3e900000", "3ea00000"), 16: (12, "3ed00000", "3f000000")}
for _m, (_mn, _ha, _hm) in _W.items():
    _s = ([A(1, 1, range(100, 100 + _mn), 1 / 32)] if _mn else []) + [A(2, 1, range(100, 101 + _mn), 1 / 32), A(3, 1, range(100, 100 + _m), 1 / 32)]
    _s += [Rq(50, 1, range(100, 100 + _m), 1 / 32), Nq(51, 1, 3, [], range(100, 100 + _m), 1 / 32)]
    _tie = _mn + 1 == _m
    case(f"W_max{_m}", "W", _s, [rline(50, f"2:{_ha} 3:{_hm}", "2 3"), nline(51, f"2:{_ha} 3:{_hm}", "2 3" if _tie else "3 2", "")],
         "KFD:769,780 / KFD:648,659", f"key-frame 1 shares exactly minCommonWords = {_mn} of {_m} words and is not scored, key-frame 2 shares one more and is",
         edges={"acc_tie"} if _tie else ())

case("W_connected_max", "W",
     [A(1, 1, range(100, 105), 1 / 32), A(2, 1, range(100, 104), 1 / 32), A(3, 1, range(100, 110), 1 / 32),
      Rq(50, 1, range(100, 110), 1 / 32), Nq(51, 1, 3, [3], range(100, 110), 1 / 32)],
     [rline(50, "3:3ea00000", "3"), nline(51, "1:3e200000", "1", "")],
     "KFD:623-630,641-645", "the connected key-frame 3 shares 10 words and is not listed: the N-best maximum is 5, so key-frame 1 (5 words) is scored, "
     "key-frame 2 (4 = minCommonWords) is not; reloc lists 3 and its maximum is 10")

case("W_marked_max", "W",
     [A(1, 1, range(300, 310), 1 / 32), A(2, 1, range(100, 105), 1 / 32),
      Rq(7, 1, range(300, 310), 1 / 32), Rq(7, 1, list(range(100, 105)) + list(range(300, 310)), 1 / 32),
      Nq(8, 1, 3, [], range(300, 310), 1 / 32), Nq(8, 1, 3, [], list(range(100, 105)) + list(range(300, 310)), 1 / 32)],
     [rline(7, "1:3ea00000", "1"), rline(7, "2:3e200000", "2"), nline(8, "1:3ea00000", "1", ""), nline(8, "2:3e200000", "2", "")],
     "KFD:748-752,762-766 / KFD:623-630", "the second call repeats the query id: key-frame 1 is already marked, is not listed again and its 10 words "
     "do not raise the maximum, so key-frame 2 (5 words) is scored")

# ---------------------------------------------------------------------------------------------------------------------------------
# S: the score
# ---------------------------------------------------------------------------------------------------------------------------------
_fold = np.zeros(130)
_fold[0] = 0.5 + 2.0 ** -25
_fold[[1, 2, 63, 64, 65, 127, 128, 129]] = 2.0 ** -55
case("S_fold_order", "S", [A(1, 1, range(1000, 1130), _fold), Rq(60, 1, range(1000, 1130), _fold), Nq(61, 1, 1, [], range(1000, 1130), _fold)],
     [rline(60, "1:3f000000", "1"), nline(61, "1:3f000000", "1", "")],
     "SO:23-68", "the in-order double fold loses each 2^-54 term against 1 + 2^-24, and -s/2 is the float midpoint 0.5 + 2^-25, which rounds to even; "
     "a fold that adds the small terms to each other first crosses the midpoint (3f000001)", edges={"si_round"})

for _n, _pos, _h in [(1, [0], "3c800000"), (63, [62], "3c800000"), (64, [63], "3c800000"), (65, [63, 64], "3d000000"),
                     (128, [63, 64, 127], "3d400000"), (129, [63, 64, 127, 128], "3d800000")]:
    _kw = [1000 + 2 * j for j in range(_n)]
    _qw = sorted([_kw[p] for p in _pos] + [999, 1001, 1000 + 2 * _n + 1])
    case(f"S_chunk{_n}", "S", [A(1, 1, _kw, 2.0 ** -6), Rq(60, 1, _qw, 2.0 ** -4), Nq(61, 1, 1, [], _qw, 2.0 ** -4)],
         [rline(60, f"1:{_h}", "1"), nline(61, f"1:{_h}", "1", "")],
         "SO:23-68", f"a key-frame vector of {_n} words whose only common words are at positions {_pos}: the ends of the 64-word chunks of k_q_si")

case("S_one_word_query", "S", [A(1, 1, [400, 500, 600], 0.25), Rq(60, 1, [500], 0.5), Nq(61, 1, 1, [], [500], 0.5)],
     [rline(60, "1:3e800000", "1"), nline(61, "1:3e800000", "1", "")], "SO:23-68", "a query of one word")

case("S_query_ends", "S", [A(1, 1, [50, 100, 119, 200], 2.0 ** -6), Rq(60, 1, range(100, 120), 2.0 ** -5), Nq(61, 1, 1, [], range(100, 120), 2.0 ** -5)],
     [rline(60, "1:3d000000", "1"), nline(61, "1:3d000000", "1", "")],
     "SO:23-68", "the common words are the first and the last entry of the query: both ends of the search in the query's words")

case("S_word_id_extremes", "S", [A(1, 1, [0, NW - 1], 0.25), Rq(60, 1, [0, 5000, NW - 1], 0.5), Nq(61, 1, 1, [], [0, 5000, NW - 1], 0.5)],
     [rline(60, "1:3f000000", "1"), nline(61, "1:3f000000", "1", "")], "SO:23-68", "word ids 0 and nWords - 1: the ends of the inverted file")

case("S_zero_common", "S", [A(1, 1, [100, 101, 102, 103, 200], [0, 0, 0, 0, 1]), Rq(60, 1, range(100, 104), 0.25), Nq(61, 1, 1, [], range(100, 104), 0.25)],
     [rline(60, "1:80000000", ""), nline(61, "1:80000000", "1", "")],
     "SO:23-68 / KFD:819-820,831", "every common value of the key-frame is 0: si = -(+0)/2 = -0, the key-frame is scored and listed, bestAccScore stays 0 "
     "and reloc retains nothing (-0 > 0 fails); N-best has no such gate and returns it")

# ---------------------------------------------------------------------------------------------------------------------------------
# L: list order = (rank of the first shared query word, add sequence)
# ---------------------------------------------------------------------------------------------------------------------------------
_lq = ([10, 20, 30, 31, 32], 1 / 8)
case("L_rank_then_sequence", "L",
     [A(9, 1, [30, 31, 32], 1 / 8), A(8, 1, [10, 30, 31], 1 / 8), A(7, 1, [20, 30, 32], 1 / 8), A(6, 1, [10, 30, 32], 1 / 8), A(12, 1, [30, 31, 32], 1 / 8),
      ("E", 9), A(9, 1, [30, 31, 32], 1 / 8), Rq(60, 1, *_lq), Nq(61, 1, 5, [], *_lq)],
     [rline(60, pairs([8, 6, 7, 12, 9], "3ec00000"), "8 6 7 12 9"), nline(61, pairs([8, 6, 7, 12, 9], "3ec00000"), "8 6 7 12 9", "")],
     "KFD:741-755 / KFD:615-633", "8 and 6 are met on the first query word (ids descend, sequences ascend), 7 on the second, 12 and 9 on the third; 9 was "
     "erased and re-added, so it holds the lowest slot and the latest sequence; every score ties, so N-best keeps the list order", edges={"acc_tie"})

_pw = [([1000, 2000] if i % 2 else [2000]) for i in range(1, 130)]
_odd = list(range(1, 130, 2))
case("L_postings_65_129", "L",
     [A(i, 1, _pw[i - 1], 0.25) for i in range(1, 130)] +
     [Rq(60, 1, [1000, 2000], 0.25), Nq(61, 1, 5, [], [1000, 2000], 0.25), Rq(62, 1, [2000], 0.25), Nq(63, 1, 5, [], [2000], 0.25)],
     [rline(60, pairs(_odd, "3f000000"), ids(_odd)), nline(61, pairs(_odd, "3f000000"), "1 3 5 7 9", ""),
      rline(62, pairs(range(1, 130), "3e800000"), ids(range(1, 130))), nline(63, pairs(range(1, 130), "3e800000"), "1 2 3 4 5", "")],
     "KFD:741-755 / KFD:615-633", "word 1000 is in 65 key-frames and word 2000 in 129: posting lists one longer than one and two lane strides of k_q_count; "
     "a posting missed leaves an odd key-frame at 1 word = minCommonWords", edges={"acc_tie"})

# ---------------------------------------------------------------------------------------------------------------------------------
# A: accumulation over the covisibles
# ---------------------------------------------------------------------------------------------------------------------------------
_s1234 = "1:3f800000 2:3f800000 3:33800000 4:33800000"
case("A_association", "A",
     [A(1, 1, *V1), A(2, 1, *V1), A(3, 1, W16, 2.0 ** -28), A(4, 1, W16, 2.0 ** -28), ("V", 2, [3, 4]), Rq(70, 1, *Q16), Nq(71, 1, 4, [], *Q16)],
     [rline(70, _s1234, "1 2"), nline(71, _s1234, "1 2 3 4", "")],
     "KFD:801-820 / KFD:680-699", "acc(2) = (1 + 2^-24) + 2^-24 stays 1.0f when summed in covisibility order and ties acc(1), so the list order holds; "
     "adding the covisibles to each other first gives 3f800001 and puts 2 first", edges={"acc_round", "acc_tie"})

_q22 = (W16, [1 / 16] * 15 + [1 / 16 + 2.0 ** -22])
_s2134 = "2:3f800000 1:3f800002 3:34000000 4:33800000"
case("A_order", "A",
     [A(2, 1, *V1), A(1, 1, *_q22), A(3, 1, W16, 2.0 ** -27), A(4, 1, W16, 2.0 ** -28), ("V", 2, [3, 4]), Rq(70, 1, *_q22), Nq(71, 1, 4, [], *_q22)],
     [rline(70, _s2134, "2 1"), nline(71, _s2134, "2 1 3 4", "")],
     "KFD:801-820 / KFD:680-699", "acc(2) = (1 + 2^-23) + 2^-24 rounds to even, 3f800002, and ties acc(1), so 2 (listed first) stays first; in reverse "
     "covisibility order (1 + 2^-24) + 2^-23 = 3f800001 and 1 comes first", edges={"acc_round", "acc_tie"})

case("A_cov_equal", "A", [A(1, 1, *V5), A(2, 1, *V5), ("V", 1, [2]), Rq(70, 1, *Q16), Nq(71, 1, 1, [], *Q16)],
     [rline(70, "1:3f000000 2:3f000000", "1"), nline(71, "1:3f000000 2:3f000000", "1", "")],
     "KFD:811 / KFD:690", "the covisible's score is bit-equal to the parent's: the comparison is strict and the parent stays the best key-frame", edges={"best_tie"})

_v5up = (W16, [1 / 32 + 2.0 ** -24] + [1 / 32] * 15)
case("A_cov_one_ulp", "A", [A(1, 1, *V5), A(2, 1, *_v5up), ("V", 1, [2]), Rq(70, 1, *Q16), Nq(71, 1, 1, [], *Q16)],
     [rline(70, "1:3f000000 2:3f000001", "2"), nline(71, "1:3f000000 2:3f000001", "2", "")],
     "KFD:811 / KFD:690", "the covisible's score is one ulp above the parent's: the covisible becomes the best key-frame", edges={"best_tie", "acc_round"})

_s124 = "1:3e800000 2:3e000000 4:3f000000"
case("A_hole", "A",
     [A(1, 1, *V25), A(2, 1, *V125), A(3, 1, *V25), A(4, 1, *V5), ("V", 1, [2, 3, 4]), ("E", 3), Rq(70, 1, *Q16), Nq(71, 1, 3, [], *Q16)],
     [rline(70, _s124, "4"), nline(71, _s124, "4 2", "")],
     "KFD:801-820 / KFD:680-699", "erasing covisible 3 leaves a hole in the middle of key-frame 1's row: the walk goes on past it and 4 becomes the best")

case("A_cov_other_map", "A", [A(1, 1, *V25), A(2, 2, *V5), ("V", 1, [2]), Rq(70, 1, *Q16), Nq(71, 1, 2, [], *Q16)],
     [rline(70, "1:3e800000 2:3f000000", ""), nline(71, "1:3e800000 2:3f000000", "", "2")],
     "KFD:801-820,834 / KFD:680-699,717-724", "the covisible is of another map: it still adds its score and becomes the best key-frame, which reloc then "
     "drops and N-best files under merge")

case("A_cov_connected", "A", [A(1, 1, *V25), A(2, 1, *V5), ("V", 1, [2]), Nq(71, 1, 2, [], *Q16), Nq(72, 1, 2, [2], *Q16)],
     [nline(71, "1:3e800000 2:3f000000", "2", ""), nline(72, "1:3e800000", "1", "")],
     "KFD:686-687", "in the second query covisible 2 is connected, so it does not carry the query id and is skipped, although its score of the first "
     "query (0.5) is still there")

case("A_cov_unscored", "A", [A(1, 1, *V5), A(2, 1, range(100, 112), 1 / 32), A(3, 1, *V75), ("V", 1, [2]), Rq(70, 1, *Q16), Nq(71, 1, 2, [], *Q16)],
     [rline(70, "1:3f000000 3:3f400000", "3"), nline(71, "1:3f000000 3:3f400000", "3 1", "")],
     "KFD:807-810 / KFD:686-689", "covisible 2 shares 12 = minCommonWords words: it carries the query id but was never scored and adds its initial 0, not "
     "the 0.375 a scoring would give")

_covs = " ".join(f"{1 + k}:{h}" for k, h in zip(range(1, 11), ["3e000000", "3d800000", "3d000000", "3c800000", "3c000000", "3b800000", "3b000000", "3a800000",
                                                              "3a000000", "39800000"]))
_rival = (W16, [1 / 16] * 11 + [1 / 128] * 4 + [253 * 2.0 ** -13])        # si 0.75 - 3 * 2^-13: between the sum over nine covisibles and over ten
case("A_ten_covisibles", "A",
     [A(20, 1, *_rival), A(1, 1, *V5)] + [A(1 + k, 1, W16, 2.0 ** -(6 + k)) for k in range(1, 11)] + [("V", 1, list(range(2, 12))), Rq(70, 1, *Q16), Nq(71, 1, 2, [], *Q16)],
     [rline(70, "20:3f3fe800 1:3f000000 " + _covs, "20 1"), nline(71, "20:3f3fe800 1:3f000000 " + _covs, "1 20", "")],
     "KFD:801-820 / KFD:680-699", "ten covisibles, all scored: acc(1) = 0.75 - 2^-12 beats key-frame 20 only if the tenth (2^-12) is added")

# ---------------------------------------------------------------------------------------------------------------------------------
# R: the reloc walk
# ---------------------------------------------------------------------------------------------------------------------------------
_f8 = (list(range(200, 208)), [1 / 32] * 8)


def _with_foreign(v, bump=0.0):
    return W16 + _f8[0], list(v[1][:15]) + [v[1][15] + bump] + _f8[1]


case("R_equal_075", "R", [A(1, 1, *V1), A(2, 1, *_with_foreign(V75)), Rq(70, 1, *Q16)], [rline(70, "1:3f800000 2:3f400000", "1")],
     "KFD:824,831", "acc(2) is exactly 0.75f * bestAccScore: the comparison is strict and 2 is dropped", edges={"thr"})
case("R_one_ulp_above_075", "R", [A(1, 1, *V1), A(2, 1, *_with_foreign(V75, 2.0 ** -24)), Rq(70, 1, *Q16)], [rline(70, "1:3f800000 2:3f400001", "1 2")],
     "KFD:824,831", "acc(2) is one ulp above 0.75f * bestAccScore and is retained", edges={"thr"})
case("R_above_075", "R", [A(1, 1, *V1), A(2, 1, *_with_foreign(V75, 2.0 ** -20)), Rq(70, 1, *Q16)], [rline(70, "1:3f800000 2:3f400010", "1 2")],
     "KFD:824,831", "acc(2) is 16 ulps above the threshold and is retained")

_q23 = (W16, [1 / 16] * 15 + [1 / 16 + 2.0 ** -23])
_v23 = (W16, [1 / 16] * 8 + [1 / 32] * 7 + [1 / 32 + 2.0 ** -23])
case("R_float_threshold", "R", [A(1, 1, *_q23), A(2, 1, *_v23), Rq(70, 1, *_q23)], [rline(70, "1:3f800001 2:3f400002", "1")],
     "KFD:824,831", "0.75f * 3f800001 is a float midpoint and rounds to even, 3f400002 = acc(2): dropped; the same product in double lies below acc(2)", edges={"thr"})

case("R_best_in_other_map", "R", [A(1, 2, *V1), A(2, 1, *V9375), Rq(70, 1, *Q16)], [rline(70, "1:3f800000 2:3f700000", "2")],
     "KFD:831,834", "the best entry passes the threshold and is then dropped because its key-frame is of another map")

case("R_best_from_three_entries", "R",
     [A(2, 1, *V9375), A(4, 1, *V9375), A(1, 1, *V1), A(3, 1, *V9375), A(5, 1, *V875), ("V", 2, [1]), ("V", 3, [1]), ("V", 4, [5]), Rq(70, 1, *Q16)],
     [rline(70, "2:3f700000 4:3f700000 1:3f800000 3:3f700000 5:3f600000", "1 4")],
     "KFD:836-840", "key-frame 1 is the best of the entries of 2 and 3 and of its own (which fails the threshold): it is emitted once, where 2 stands, before 4")


def _r_max(n, at):
    """n entries of acc 0.6875, the unique maximum 1.0 at list index `at` and one retained entry (0.875) beyond index 255."""
    ret = n - 1 if at != n - 1 else 0
    vecs = {at: (V1, "3f800000"), ret: (V875, "3f600000")}
    script = [A(i + 1, 1, *vecs.get(i, (V6875, "3f300000"))[0]) for i in range(n)] + [Rq(70, 1, *Q16)]
    scored = " ".join(f"{i + 1}:{vecs.get(i, (None, '3f300000'))[1]}" for i in range(n))
    return script, [rline(70, scored, ids(sorted([at + 1, ret + 1])))]


for _n, _at in [(257, 0), (257, 255), (257, 256), (300, 0), (300, 255), (300, 256), (300, 299)]:
    case(f"R_max_n{_n}_at{_at}", "R", *_r_max(_n, _at), "KFD:819-820,824,831",
         f"{_n} scored entries; the unique maximum stands at list index {_at}; a maximum taken over 256 entries only retains the 0.6875 entries as well")

# ---------------------------------------------------------------------------------------------------------------------------------
# N: the N-best walk
# ---------------------------------------------------------------------------------------------------------------------------------
_long = (W16 + [200, 201, 202, 203], 1 / 16)
_lid = [1000 - i for i in range(300)]
case("N_long_tie_list", "N", [A(1000 - i, 1 + i % 2, *_long) for i in range(300)] + [Rq(70, 2, *Q16), Nq(71, 2, 3, [], *Q16)],
     [rline(70, pairs(_lid, "3f800000"), ids(range(999, 700, -2))), nline(71, pairs(_lid, "3f800000"), "999 997 995", "1000 998 996")],
     "KFD:702", "300 bit-equal accumulated scores: the sort is stable, so the walk meets them in list order (ids descend, maps alternate)", edges={"acc_tie"})

_b255 = {256: (V1, "3f800000"), 299: (V875, "3f600000")}
_s255 = " ".join(f"{i + 1}:{_b255.get(i, (None, '3f300000'))[1]}" for i in range(300))
case("N_best_beyond_255", "N", [A(i + 1, 1, *_b255.get(i, (V6875,))[0]) for i in range(300)] + [Nq(71, 1, 3, [], *Q16)], [nline(71, _s255, "257 300 1", "")],
     "KFD:702", "300 entries; the two largest accumulated scores stand at list indices 256 and 299, behind the first 256-entry pass of the rank sort; the "
     "third place goes to the first of 298 ties", edges={"acc_tie"})

_eight = [A(i, 1 + (i - 1) % 2, *V1) for i in range(1, 9)]
_s8 = pairs(range(1, 9), "3f800000")
case("N_one_and_five", "N", _eight + [Nq(71, 1, 1, [], *Q16), Nq(72, 1, 5, [], *Q16)],
     [nline(71, _s8, "1", "2"), nline(72, _s8, "1 3 5 7", "2 4 6 8")],
     "KFD:709-729", "N = 1 stops after one of each kind; N = 5 finds only four of each", edges={"acc_tie"})

case("N_fewer_than_n", "N", [A(1, 1, *V1), A(2, 1, *V5), A(3, 2, *V25), Nq(71, 1, 5, [], *Q16)],
     [nline(71, "1:3f800000 2:3f000000 3:3e800000", "1 2", "3")], "KFD:709", "three scored entries and N = 5: the walk ends with the list")

case("N_loop_full_merge_goes_on", "N", [A(i, m, *V1) for i, m in zip(range(1, 7), [1, 1, 1, 2, 1, 2])] + [Nq(71, 1, 2, [], *Q16)],
     [nline(71, pairs(range(1, 7), "3f800000"), "1 2", "4 6")],
     "KFD:709,717-725", "the loop list is full after two entries; 3 and 5 are consumed without a place while merge fills up", edges={"acc_tie"})

_s3 = pairs([1, 2, 3], "3f800000")
case("N_bad_key_frame", "N", [A(1, 1, *V1), A(2, 1, *V1), A(3, 1, *V1), ("D", 2, 1), Nq(71, 1, 2, [], *Q16), ("D", 2, 0), Nq(72, 1, 2, [], *Q16)],
     [nline(71, _s3, "1 3", ""), nline(72, _s3, "1 2", "")],
     "KFD:712-713", "an isBad() key-frame is scored, then skipped by the walk, which advances (the database's stated departure from the rule's "
     "non-advancing continue); with the flag cleared it is back", edges={"acc_tie"})

_s5 = pairs(range(1, 6), "3f800000")
case("N_bad_map", "N", [A(i, m, *V1) for i, m in zip(range(1, 6), [1, 2, 3, 2, 3])] + [("B", 2, 1), Nq(71, 1, 2, [], *Q16), ("B", 2, 0), Nq(72, 1, 2, [], *Q16)],
     [nline(71, _s5, "1", "3 5"), nline(72, _s5, "1", "2 3")],
     "KFD:721", "key-frames of a bad map are consumed but not filed under merge", edges={"acc_tie"})

case("N_repeated_best", "N", [A(2, 1, *V9375), A(3, 1, *V9375), A(1, 1, *V1), A(4, 1, *V5), ("V", 2, [1]), ("V", 3, [1]), Nq(71, 1, 3, [], *Q16)],
     [nline(71, "2:3f700000 3:3f700000 1:3f800000 4:3f000000", "1 4", "")],
     "KFD:715,725", "key-frame 1 is the best of three entries and is filed once", edges={"acc_tie"})

# ---------------------------------------------------------------------------------------------------------------------------------
# V: visibility (visible_below): a key-frame is visible to a query iff its add sequence is below the bound
# ---------------------------------------------------------------------------------------------------------------------------------
_vq = (list(range(100, 110)), 1 / 32)
_va = [A(1, 1, range(100, 105), 1 / 32), A(2, 1, range(100, 105), 1 / 32), A(3, 1, range(100, 110), 1 / 32)]
case("V_bound", "V",
     _va + [Rq(80, 1, *_vq, vb=2), Nq(81, 1, 3, [], *_vq, vb=2), Rq(82, 1, *_vq), Nq(83, 1, 3, [], *_vq)],
     [rline(80, "1:3e200000 2:3e200000", "1 2"), nline(81, "1:3e200000 2:3e200000", "1 2", ""), rline(82, "3:3ea00000", "3"), nline(83, "3:3ea00000", "3", "")],
     "include/rumi_kfdb.h (visible_below) over KFD:741-755 / KFD:615-633", "bound 2: sequence 1 (bound - 1) is visible, sequence 2 (= bound) is hidden and its "
     "10 words do not raise the maximum of 5; without a bound key-frame 3 is seen and alone passes the word gate", edges={"acc_tie"},
     oracle_script=_va[:2] + [Rq(80, 1, *_vq), Nq(81, 1, 3, [], *_vq)] + _va[2:] + [Rq(82, 1, *_vq), Nq(83, 1, 3, [], *_vq)])

# ---------------------------------------------------------------------------------------------------------------------------------
# T: batching: eight queries of each kind, consecutive, so that they go in one call (and in two tiles where max_batch() is 4)
# ---------------------------------------------------------------------------------------------------------------------------------
_B16 = list(range(200, 216))
_ta = [A(1, 1, *V1), A(2, 2, W16, V75[1][:15] + [1 / 32 + 2.0 ** -24]), A(3, 1, *V5), A(11, 1, _B16, 1 / 32), A(12, 2, _B16, 1 / 64)]
_tq = [((W16, 1 / 16) if j % 2 == 0 else (_B16, 1 / 16)) for j in range(8)]
_sa, _sb = "1:3f800000 2:3f400001 3:3f000000", "11:3f000000 12:3e800000"
case("T_eight_queries", "T",
     _ta + [Rq(100 + j, 1 + (j // 2) % 2, *_tq[j]) for j in range(8)] + [Nq(200 + j, 1 + (j // 2) % 2, 1 + j % 3, [], *_tq[j]) for j in range(8)],
     [rline(100, _sa, "1"), rline(101, _sb, "11"), rline(102, _sa, "2"), rline(103, _sb, ""), rline(104, _sa, "1"), rline(105, _sb, "11"), rline(106, _sa, "2"),
      rline(107, _sb, ""),
      nline(200, _sa, "1", "2"), nline(201, _sb, "11", "12"), nline(202, _sa, "2", "1 3"), nline(203, _sb, "12", "11"), nline(204, _sa, "1 3", "2"),
      nline(205, _sb, "11", "12"), nline(206, _sa, "2", "1"), nline(207, _sb, "12", "11")],
     "KFD:733-843 / KFD:604-708, call by call", "eight queries in one call, alternating between two sets of key-frames, maps and N: every query has its own "
     "row of counters, and a split into two tiles changes nothing", edges={"thr"})

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

COVERAGE = {(f, k): [c.name for c in CASES if c.family == f and k in c.kinds] for f in FAMILIES for k in "RN"}
NOT_APPLICABLE = {
    ("R", "N"): "N-best forms neither bestAccScore nor the 0.75 gate (KFD:702-729 sorts instead); its walk over a long list is N_long_tie_list",
}
assert not any(COVERAGE[k] for k in NOT_APPLICABLE)

# the cases that must fail under each deviation of PyDB
BITES = {
    # key-frames AT minCommonWords become scored (W_max1 has none: minCommonWords is 0 there)
    "word_ge": ["W_max4", "W_max5", "W_max6", "W_max9", "W_max10", "W_max16", "W_connected_max", "L_postings_65_129", "A_cov_unscored"],
    "thr_double": ["R_float_threshold"],
    "acc_reverse": ["A_order"],
    "si_pairwise": ["S_fold_order"],
    "best_ge": ["A_cov_equal"],
    # every N-best query whose walk meets two bit-equal accumulated scores of different key-frames
    "sort_unstable": ["W_max1", "W_max4", "W_max5", "L_rank_then_sequence", "L_postings_65_129", "A_association", "A_order", "N_long_tie_list",
                      "N_best_beyond_255", "N_one_and_five", "N_loop_full_merge_goes_on", "N_bad_key_frame", "N_bad_map", "V_bound"],
    # every list in which a larger id was added before a smaller one and met on the same query word
    "list_by_id": ["L_rank_then_sequence", "A_order", "A_ten_covisibles", "R_best_from_three_entries", "N_long_tie_list", "N_repeated_best"],
    "vis_le": ["V_bound"],
    "max_first256": ["R_max_n257_at256", "R_max_n300_at256", "R_max_n300_at299"],
}
assert set(BITES) == set(DEVIATIONS)


def shifted(case_, kf_off, q_off):
    """The case's script and expected lines with every key-frame id raised by kf_off and every query id by q_off: on one long-lived database a
    key-frame keeps its query state by id across erase and re-add, as the rule's KeyFrame object does, so each case needs ids of its own."""
    s = []
    for c in case_.script:
        op = c[0]
        if op in ("A", "E", "K", "D"):
            s.append((op, c[1] + kf_off) + tuple(c[2:]))
        elif op == "V":
            s.append((op, c[1] + kf_off, [x + kf_off for x in c[2]]))
        elif op == "R":
            s.append((op, c[1] + q_off) + tuple(c[2:]))
        elif op == "N":
            s.append((op, c[1] + q_off, c[2], c[3], [x + kf_off for x in c[4]]) + tuple(c[5:]))
        else:
            s.append(c)
    lines = []
    for ln in case_.expect:
        parts = [p.split() for p in ln.split("|")]
        sc = " ".join(f"{int(p.split(':')[0]) + kf_off}:{p.split(':')[1]}" for p in parts[1])
        groups = [ids(int(x) + kf_off for x in p) for p in parts[2:]]
        lines.append((rline if parts[0][0] == "R" else nline)(int(parts[0][1]) + q_off, sc, *groups))
    return s, lines


# ---------------------------------------------------------------------------------------------------------------------------------
# BowVector assembly (k_bow_assemble): per-feature rows as rumi_voc_transform_batch_device leaves them, and the vector a TF_IDF vocabulary's
# addWeight (TemplatedVocabulary.h:1147-1190) and BowVector::normalize(L1) make of them.  The vocabulary of the tests weighs TF_IDF, so a repeated
# word SUMS its weights in feature order (it would be first-value-wins under IDF or BINARY).
# ---------------------------------------------------------------------------------------------------------------------------------
_T = 2.0 ** -53
ASSEMBLY_CAP = 320
ASSEMBLY = [  # (name, words per feature, weights per feature, counts[f][0], expected words, expected values, what it stands on)
    ("sum_in_feature_order", [7, 7, 7, 9], [1.0, _T, _T, 1.0], 4, [7, 9], [0.5, 0.5],
     "(1 + 2^-53) + 2^-53 stays 1.0 in feature order"),
    ("sum_reverse_order", [7, 7, 7, 9], [_T, _T, 1.0, 1.0], 4, [7, 9], [0.5 + 2.0 ** -53, 0.5],
     "the same weights in reverse: (2^-53 + 2^-53) + 1 = 1 + 2^-52; the norm 2 + 2^-52 rounds to 2"),
    ("zero_and_negative_dropped", [5, 5, 6, 8, 8], [0.0, -1.0, 1.0, -2.0, 3.0], 5, [6, 8], [0.25, 0.75], "weights of 0 and below are stopped words"),
    ("all_zero", [5, 6, 7], [0.0, 0.0, 0.0], 3, [], [], "every weight 0: an empty vector"),
    ("count_0", [5, 6, 7], [1.0, 1.0, 1.0], 0, [], [], "no feature"),
    ("count_1", [5, 6, 7], [4.0, 1.0, 1.0], 1, [5], [1.0], "one feature"),
    ("count_256", [1000 - i for i in range(256)], [2.0 ** -8] * 256, 256, list(range(745, 1001)), [2.0 ** -8] * 256,
     "one full pass of the 256-thread rank sort, words descending"),
    ("count_257", [1000 - i for i in range(257)], [1.0] * 257, 257, list(range(744, 1001)), [1.0 / 257.0] * 257, "one feature more than the workgroup"),
    ("same_word_far_apart", [42] + [1000 + i for i in range(298)] + [42], [0.5] + [0.25] * 298 + [0.25], 300, [42] + [1000 + i for i in range(298)],
     [0.75 / 75.25] + [0.25 / 75.25] * 298, "word 42 at feature 0 and at feature 299"),
    ("norm_fold_order", [1, 2, 3, 4, 5], [1.0] + [2.0 ** -54] * 4, 5, [1, 2, 3, 4, 5], [1.0] + [2.0 ** -54] * 4,
     "the norm in word order is 1.0 (each 2^-54 is lost); summed together first it is 1 + 2^-52 and every value changes"),
]
ASSEMBLY_CLAMP = ("count_above_cap", 4, [3, 3, 2, 1], [1.0, 1.0, 1.0, 1.0], 7, [1, 2, 3], [0.25, 0.25, 0.5], "counts above cap is clamped to cap")
