"""Times the key-frame database (include/rumi_kfdb.h) against the one-core C++ oracle (tests/cpp/kfdb_oracle.cc).

Databases of 1k / 10k / 30k key-frames of about 1000 words on the k = 10, L = 6 tree (synthetic_vocabulary_fast); one reloc query, and batches of
64 and 1024 N-best queries.  Prints one JSON line per size and a digest of every candidate list (two runs must print the same digests).
    python tools/kfdb_probe.py [--sizes 1000,10000,30000] [--out FILE]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from kfdb_scene import Scene, build_oracle, format_nbest, to_text  # noqa: E402


def oracle_ms(exe, setup, queries):
    """ms the oracle spends in the given queries' functions alone (its own clock, KFDB_ORACLE_TIMING: script parsing excluded), and its output."""
    r = subprocess.run([exe], input=to_text(setup + queries), capture_output=True, text=True, timeout=3600, env=dict(os.environ, KFDB_ORACLE_TIMING="1"))
    assert r.returncode == 0, r.stderr
    ms = sum(float(l.split()[1]) for l in [l for l in r.stderr.splitlines() if l.startswith("query_ms ")][-len(queries):])
    return ms, r.stdout.splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,30000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401
    from voc_scene import synthetic_vocabulary_fast
    from rumi_slam_amd.kfdb import KeyFrameDatabase
    from rumi_slam_amd.vocabulary import ORBVocabulary
    voc = ORBVocabulary(*synthetic_vocabulary_fast(7, 10, 6))
    nw = voc.size()
    exe = build_oracle(tempfile.mkdtemp())
    lines = []
    for n in (int(x) for x in a.sizes.split(",")):
        sc = Scene(n, n, 3, n_words=nw, words_per_kf=1000, n_places=max(8, n // 20), window=8)
        setup = sc.add_commands() + sc.cov_commands()
        db = KeyFrameDatabase(voc, n + 16, n * 1000 + 4096)
        t = time.perf_counter()
        db.add(sc.ids, sc.maps, sc.bows)
        db.set_covisibles(sc.ids, [sc.covisibles(i) for i in range(n)])
        build_ms = (time.perf_counter() - t) * 1e3
        rng = np.random.default_rng(n)
        res = {"n_kf": n, "build_ms": round(build_ms, 2)}
        digest = hashlib.sha256()
        # one reloc query through the C entry
        i = int(rng.integers(n))
        qb = sc.query_bow(place=sc.place_of[i])
        db.detect_relocalization_candidates([10**9], [sc.maps[i]], [qb])          # warm
        reps = []
        for r in range(5):
            t = time.perf_counter()
            cand = db.detect_relocalization_candidates([10**9 + 1 + r], [sc.maps[i]], [qb])
            reps.append((time.perf_counter() - t) * 1e3)
        res["reloc1_ms"] = round(float(np.median(reps)), 3)
        res["reloc1_oracle_ms"] = round(oracle_ms(exe, setup, [("R", 10**9 + 1, sc.maps[i], *qb)])[0], 3)
        digest.update(repr([list(map(int, c)) for c in cand]).encode())
        qid = 2 * 10**9
        done = []                                       # the N-best queries so far: the oracle replays them (stale scores carry over)
        for B in (1, 1, 64, 1024):                      # (the first one-query call pays first-use allocations: the second is reported)
            idx = rng.integers(n, size=B)
            qs = [(qid + k, sc.maps[j], sc.query_bow(place=sc.place_of[j]), [sc.ids[j]] + sc.connected(j)) for k, j in enumerate(idx)]
            qid += B
            t = time.perf_counter()
            out, scored = db.detect_nbest_candidates([q[0] for q in qs], [q[1] for q in qs], [q[2] for q in qs], [q[3] for q in qs], 3, with_scored=True)
            gpu_ms = (time.perf_counter() - t) * 1e3
            got = [format_nbest(q[0], s, lp, mg) for q, s, (lp, mg) in zip(qs, scored, out)]
            new = [("N", q[0], q[1], 3, q[3], *q[2]) for q in qs]
            o_ms, want = oracle_ms(exe, setup + done, new)
            want = want[-B:]
            done += new
            res[f"nbest{B}_ms"] = round(gpu_ms, 3)                        # (B = 1: the second call overwrites the first)
            res[f"nbest{B}_oracle_ms"] = round(o_ms, 3)
            res[f"nbest{B}_speedup"] = round(o_ms / gpu_ms, 2) if gpu_ms > 0 else None
            res[f"nbest{B}_equal"] = got == want
            digest.update("\n".join(got).encode())
        res["digest"] = digest.hexdigest()[:16]
        db.close()
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
