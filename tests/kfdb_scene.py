"""Synthetic key-frame databases for the tests of include/rumi_kfdb.h, and the script both the C++ oracle (tests/cpp/kfdb_oracle.cc) and the
GPU database run.

A script is a list of commands (tuples): ("A", id, map, words, vals), ("E", id), ("M", map), ("C",), ("B", map, bad), ("K", id, map),
("D", id, bad), ("V", id, [covisible ids]), ("R", qid, map, words, vals), ("N", qid, map, n_cand, [connected ids], words, vals).
"R" and "N" may carry one more element: visible_below, as a number of adds counted from the start of the script; only run_gpu and kfdb_cases.PyDB
read it (the oracle has no such argument, to_text leaves it out)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def l1_normalise(words, vals):
    """(sorted unique words, L1-normalised values): BowVector::normalize(L1) on a sparse vector (norm summed in word order)."""
    o = np.argsort(words, kind="stable")
    w, v = np.asarray(words, np.uint32)[o], np.asarray(vals, np.float64)[o]
    keep = np.concatenate([[True], w[1:] != w[:-1]]) if len(w) else np.zeros(0, bool)
    w, v = w[keep], v[keep]
    norm = 0.0
    for x in v:
        norm += abs(float(x))
    if norm > 0:
        v = v / norm
    return w, v


class Scene:
    """Trajectories through "places" (word pools) in several maps.  Consecutive key-frames of a trajectory share most of their words; a
    trajectory revisits places, so loop and merge candidates exist.  Covisibility comes from shared words within a map."""

    def __init__(self, seed, n_kf, n_maps=1, n_words=20000, words_per_kf=60, n_places=None, pool=None, share=0.8, window=12, id_base=1):
        rng = np.random.default_rng(seed)
        n_places = n_places or max(4, n_kf // 8)
        pool = pool or words_per_kf * 2
        self.places = [rng.choice(n_words, pool, replace=False) for _ in range(n_places)]
        self.ids, self.maps, self.bows, self.place_of = [], [], [], []
        per_map = [n_kf // n_maps + (1 if m < n_kf % n_maps else 0) for m in range(n_maps)]
        kid = id_base
        for m in range(n_maps):
            p = int(rng.integers(n_places))
            for _ in range(per_map[m]):
                if rng.random() < 0.15:
                    p = int(rng.integers(n_places))          # jump (revisits an earlier place now and then)
                n_in = int(words_per_kf * share)
                w = np.concatenate([rng.choice(self.places[p], n_in, replace=False), rng.integers(0, n_words, words_per_kf - n_in)])
                v = rng.uniform(0.1, 5.0, len(w))
                self.bows.append(l1_normalise(w, v))
                self.ids.append(kid); self.maps.append(m + 1); self.place_of.append(p)
                kid += 1
        self.n_words = n_words
        self.rng = rng
        self.window = window
        self._sets = [set(int(x) for x in b[0]) for b in self.bows]

    def covisibles(self, i):
        """GetBestCovisibilityKeyFrames(10) of key-frame i: same map, within the window, by shared words (ties: lower id first)."""
        cand = []
        for j in range(max(0, i - self.window), min(len(self.ids), i + self.window + 1)):
            if j == i or self.maps[j] != self.maps[i]:
                continue
            s = len(self._sets[i] & self._sets[j])
            if s >= 15:
                cand.append((-s, self.ids[j]))
        cand.sort()
        return [c[1] for c in cand[:10]]

    def connected(self, i):
        return self.covisibles(i)

    def query_bow(self, place=None, words=None):
        rng = self.rng
        p = int(rng.integers(len(self.places))) if place is None else place
        n = words or len(self.bows[0][0])
        w = np.concatenate([rng.choice(self.places[p], int(n * 0.8), replace=False), rng.integers(0, self.n_words, n - int(n * 0.8))])
        return l1_normalise(w, rng.uniform(0.1, 5.0, len(w)))

    def add_commands(self, idx=None):
        idx = range(len(self.ids)) if idx is None else idx
        return [("A", self.ids[i], self.maps[i], self.bows[i][0], self.bows[i][1]) for i in idx]

    def cov_commands(self, idx=None):
        idx = range(len(self.ids)) if idx is None else idx
        return [("V", self.ids[i], self.covisibles(i)) for i in idx]


# ---- script text (oracle input) and outputs ----
def _bow_text(w, v):
    return f"{len(w)} " + " ".join(f"{int(a)} {float(b).hex()}" for a, b in zip(w, v))


def to_text(script):
    out = []
    for c in script:
        op = c[0]
        if op == "A":
            out.append(f"A {c[1]} {c[2]} " + _bow_text(c[3], c[4]))
        elif op in ("E", "M"):
            out.append(f"{op} {c[1]}")
        elif op == "C":
            out.append("C")
        elif op in ("B", "K", "D"):
            out.append(f"{op} {c[1]} {int(c[2])}")
        elif op == "V":
            out.append(f"V {c[1]} {len(c[2])} " + " ".join(str(x) for x in c[2]))
        elif op == "R":
            out.append(f"R {c[1]} {c[2]} " + _bow_text(c[3], c[4]))
        elif op == "N":
            out.append(f"N {c[1]} {c[2]} {c[3]} {len(c[4])} " + " ".join(str(x) for x in c[4]) + " " + _bow_text(c[5], c[6]))
    return "\n".join(out) + "\n"


def build_oracle(out_dir):
    exe = os.path.join(str(out_dir), "kfdb_oracle")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "kfdb_oracle.cc"), "-o", exe])
    return exe


def run_oracle(exe, script):
    r = subprocess.run([exe], input=to_text(script), capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def _f32hex(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


def format_reloc(qid, scored, cand):
    s = " ".join(f"{int(i)}:{_f32hex(x)}" for i, x in zip(*scored)) if scored is not None else ""
    return f"R {qid} |" + (" " + s if s else "") + " |" + "".join(f" {int(i)}" for i in cand)


def format_nbest(qid, scored, loop, merge):
    s = " ".join(f"{int(i)}:{_f32hex(x)}" for i, x in zip(*scored)) if scored is not None else ""
    return f"N {qid} |" + (" " + s if s else "") + " |" + "".join(f" {int(i)}" for i in loop) + " |" + "".join(f" {int(i)}" for i in merge)


def run_gpu(db, script, batch=True):
    """Runs a script on a rumi_slam_amd.kfdb.KeyFrameDatabase; consecutive adds go in one call, and with batch=True consecutive queries of one
    kind (distinct ids) go in one batched call.  Returns the output lines in the oracle's format."""
    out = []
    i = 0
    base = db.next_seq()

    def bounds(qs, at):
        return [base + q[at] if len(q) > at else (1 << 62) for q in qs] if any(len(q) > at for q in qs) else None

    while i < len(script):
        c = script[i]
        op = c[0]
        if op == "A":
            j = i
            while j < len(script) and script[j][0] == "A":
                j += 1
            db.add([x[1] for x in script[i:j]], [x[2] for x in script[i:j]], [(x[3], x[4]) for x in script[i:j]])
            i = j
            continue
        if op in ("R", "N"):
            j, seen = i, set()
            while j < len(script) and script[j][0] == op and script[j][1] not in seen and (batch or j == i):
                seen.add(script[j][1]); j += 1
            qs = script[i:j]
            if op == "R":
                cands, scored = db.detect_relocalization_candidates([q[1] for q in qs], [q[2] for q in qs], [(q[3], q[4]) for q in qs], visible_below=bounds(qs, 5),
                                                                      with_scored=True)
                out += [format_reloc(q[1], s, cd) for q, s, cd in zip(qs, scored, cands)]
            else:
                res, scored = db.detect_nbest_candidates([q[1] for q in qs], [q[2] for q in qs], [(q[5], q[6]) for q in qs], [q[4] for q in qs],
                                                         [q[3] for q in qs], visible_below=bounds(qs, 7), with_scored=True)
                out += [format_nbest(q[1], s, lp, mg) for q, s, (lp, mg) in zip(qs, scored, res)]
            i = j
            continue
        if op == "E":
            db.erase([c[1]])
        elif op == "M":
            db.clear_map(c[1])
        elif op == "C":
            db.clear()
        elif op == "B":
            db.set_map_bad(c[1], c[2])
        elif op == "K":
            db.set_maps([c[1]], [c[2]])
        elif op == "D":
            db.set_bad([c[1]], [c[2]])
        elif op == "V":
            db.set_covisibles([c[1]], [c[2]])
        i += 1
    return out
