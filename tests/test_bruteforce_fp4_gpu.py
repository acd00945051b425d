"""What the FP4 form of k_bruteforce_mfma adds over tests/test_bruteforce_mfma_gpu.py, against the CPU oracle, bit for bit on best index, best
distance and second distance: the edges of its blocking (64 queries per wave as two accumulators, the workgroup, the train stage), the extremes of
its f32 key X + index / 65536 (X = -256, 255 and 256, odd indices), an index above 15 bits, ties between the tiles and stages a wave walks, and a
ring that wraps over an empty frame.  Every launch goes through _run_batch / _run_ring, so the inputs can be checked against their own assertions
on a CPU by pointing those two at the oracle (_oracle_batch / _oracle_ring)."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu


def _run_batch(q, cq, t, ct):
    import torch
    from rumi_slam_amd.matcher import bruteforce_batch
    out = bruteforce_batch(torch.from_numpy(q).cuda(), torch.from_numpy(cq).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(ct).cuda())
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def _run_ring(d, c):
    import torch
    from rumi_slam_amd.matcher import bruteforce_ring
    out = bruteforce_ring(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda())
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def _oracle_pair(q, nq, t, nt, cap):
    out = [np.full(cap, -7, np.int32) for _ in range(3)]
    for o, r in zip(out, O.bruteforce_match(np.ascontiguousarray(q[:nq]), np.ascontiguousarray(t[:nt]))):
        o[:nq] = r
    return out


def _oracle_batch(q, cq, t, ct):
    cap = q.shape[1]
    rows = [_oracle_pair(q[b], min(int(cq[b, 0]), cap), t[b], min(int(ct[b, 0]), cap), cap) for b in range(len(q))]
    return [np.stack([r[k] for r in rows]) for k in range(3)]


def _oracle_ring(d, c):
    return _oracle_batch(d, c, np.roll(d, -1, axis=0), np.roll(c, -1, axis=0))


def _check(got, q, nq, t, nt, tag):
    bi, bd, sd = got
    rbi, rbd, rsd = O.bruteforce_match(np.ascontiguousarray(q[:nq]), np.ascontiguousarray(t[:nt]))
    assert np.array_equal(bi[:nq], rbi), (tag, "best index")
    assert np.array_equal(bd[:nq], rbd), (tag, "best distance")
    assert np.array_equal(sd[:nq], rsd), (tag, "second distance")


def _counts(n):
    return np.stack([np.asarray(n, np.int32), np.zeros(len(n), np.int32)], 1)


def _ham(a, b):
    return int(np.unpackbits(a ^ b).sum())


def _shape():
    from rumi_slam_amd.matcher import bruteforce_shape
    return bruteforce_shape()                                 # kBfmWaveQueries, kBfmQueries, kBfmStage of match.hip


def test_blocking_edges():
    """nq and nt one below, at and one above the queries per wave, the queries per workgroup and the train stage (and 63, 64, 65 whatever those
    are), every combination, eight pairs a launch; and nq = nt = 1."""
    wave_q, wg_q, stage = _shape()
    edges = sorted({e + d for e in (wave_q, wg_q, stage, 64) for d in (-1, 0, 1)})
    pairs = [(a, b) for a in edges for b in edges] + [(1, 1)]
    cap = max(edges) + 7
    rng = np.random.default_rng(41)
    for k in range(0, len(pairs), 8):
        chunk = pairs[k:k + 8]
        q = rng.integers(0, 256, (len(chunk), cap, 32), dtype=np.uint8)
        t = rng.integers(0, 256, (len(chunk), cap, 32), dtype=np.uint8)
        for b, (nq, nt) in enumerate(chunk):                 # near-ties in the last rows and columns: the last train is a few bits from the last query
            t[b, nt - 1] = q[b, nq - 1]
            t[b, nt - 1, 5] ^= 0x11
        got = _run_batch(q, _counts([p[0] for p in chunk]), t, _counts([p[1] for p in chunk]))
        for b, (nq, nt) in enumerate(chunk):
            _check([g[b] for g in got], q[b], nq, t[b], nt, (nq, nt))
            assert [got[0][b, nq - 1], got[1][b, nq - 1]] == [nt - 1, 2], (nq, nt)


def test_key_extremes():
    """The ends of the key's range.  X = Ham - popcount(query) runs from -256 (all-ones query, all-ones train) to 256 (all-zero query, all-ones
    train); the index sits in the 16 fraction bits, so an odd index next to |X| = 256, or distances 255 and 1 next to 256, show a rounded key."""
    rng = np.random.default_rng(43)
    cap = 1096
    q = rng.integers(0, 256, (7, cap, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (7, cap, 32), dtype=np.uint8)
    nq = [70, 70, 70, 70, 40, 40, 40]
    nt = [130, cap, cap, cap, cap, cap, 999]
    # 0: one query repeated, every train its exact complement: Ham = 256 everywhere
    q[0] = q[0, 0].copy(); t[0] = ~q[0, 0]
    # 1: the same with the all-zero query and all-ones trains (X = 256 at every index up to 1095), 2: all-ones query, all-zero trains (X = 0)
    q[1] = 0; t[1] = 255
    q[2] = 255; t[2] = 0
    # 3: exact copies at the last train index and at index 0; all-ones query with all-ones trains (X = -256) at the odd index 1093
    t[3, cap - 1] = q[3, 0]
    t[3, 0] = q[3, 1]
    q[3, 2] = 255; t[3, 1093] = 255
    q[3, 3] = 255; q[3, 3, 0] = 0xFE                          # popcount 255: X = -255 on the all-ones train would be Ham 1; its own copy is at 1091
    t[3, 1091] = q[3, 3]
    # 4: trains all complements of query 0 (256) but one at distance 255 (odd index) and, for query 1 = query 0, nothing else; second = 256
    q[4] = q[4, 0].copy(); t[4] = ~q[4, 0]
    t[4, 777, 9] ^= 0x40
    # 5: distance 1 and distance 255 among 256s: best 1 at index 1001, second 255
    q[5] = q[5, 0].copy(); t[5] = ~q[5, 0]
    t[5, 333, 31] ^= 0x80
    t[5, 1001] = q[5, 0]; t[5, 1001, 0] ^= 0x01
    # 6: the all-zero query (popcount 0: the only one whose X reaches 256): all-ones trains, one with a bit cleared (255) at odd index 777
    q[6] = 0; t[6] = 255
    t[6, 777, 17] = 0xEF
    got = _run_batch(q, _counts(nq), t, _counts(nt))
    for b in range(7):
        _check([g[b] for g in got], q[b], nq[b], t[b], nt[b], b)
    for b in (0, 1):
        assert (got[0][b, :nq[b]] == -1).all() and (got[1][b, :nq[b]] == 256).all() and (got[2][b, :nq[b]] == 256).all()
    assert (got[0][2, :70] == -1).all() and (got[1][2, :70] == 256).all()
    assert sum(_ham(q[3, 0], t[3, j]) == 0 for j in range(cap)) == 1 and sum(_ham(q[3, 1], t[3, j]) == 0 for j in range(cap)) == 1
    assert [got[0][3, 0], got[1][3, 0]] == [cap - 1, 0] and [got[0][3, 1], got[1][3, 1]] == [0, 0]
    assert [got[0][3, 2], got[1][3, 2], got[2][3, 2]] == [1093, 0, 1]
    assert [got[0][3, 3], got[1][3, 3], got[2][3, 3]] == [1091, 0, 1]
    assert (got[0][4, :40] == 777).all() and (got[1][4, :40] == 255).all() and (got[2][4, :40] == 256).all()
    assert (got[0][5, :40] == 1001).all() and (got[1][5, :40] == 1).all() and (got[2][5, :40] == 255).all()
    assert (got[0][6, :40] == 777).all() and (got[1][6, :40] == 255).all() and (got[2][6, :40] == 256).all()


def test_wide_index():
    """cap = nt = 40 000, three queries: duplicates of query 0 at 5 and 39 999 (the first wins, second distance 0), the only copy of query 1 at
    32 768 and of query 2 at 39 998: the index field holds more than 15 bits."""
    rng = np.random.default_rng(47)
    cap = 40000
    q = rng.integers(0, 256, (1, cap, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (1, cap, 32), dtype=np.uint8)
    t[0, 5] = q[0, 0]; t[0, 39999] = q[0, 0]
    t[0, 32768] = q[0, 1]
    t[0, 39998] = q[0, 2]
    got = _run_batch(q, _counts([3]), t, _counts([cap]))
    _check([g[0] for g in got], q[0], 3, t[0], cap, "wide")
    tb = np.unpackbits(t[0], axis=1)
    for i, where in enumerate([[5, 39999], [32768], [39998]]):
        d = (tb != np.unpackbits(q[0, i])[None]).sum(1)
        assert np.flatnonzero(d == 0).tolist() == where
    assert [got[0][0, 0], got[1][0, 0], got[2][0, 0]] == [5, 0, 0]
    assert [got[0][0, 1], got[1][0, 1]] == [32768, 0] and got[2][0, 1] > 0
    assert [got[0][0, 2], got[1][0, 2]] == [39998, 0] and got[2][0, 2] > 0


def test_wide_index_odd_at_the_precision_edge():
    """cap = nt = 40 000 again, now with the keys whose magnitude is largest: the all-ones query against all-ones trains (X = -256, where an f32
    has exactly 16 fraction bits left) at the odd indices 32 769 and 39 997, and a popcount-255 query whose only copy sits at the odd index
    39 999 (X = -255): a key that lost its lowest fraction bit would report an even index."""
    rng = np.random.default_rng(61)
    cap = 40000
    q = rng.integers(0, 256, (1, cap, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (1, cap, 32), dtype=np.uint8)
    q[0, 0] = 255
    t[0, 32769] = 255; t[0, 39997] = 255
    q[0, 1] = 255; q[0, 1, 13] = 0x7F
    t[0, 39999] = q[0, 1]
    got = _run_batch(q, _counts([3]), t, _counts([cap]))
    _check([g[0] for g in got], q[0], 3, t[0], cap, "wide odd")
    assert [got[0][0, 0], got[1][0, 0], got[2][0, 0]] == [32769, 0, 0]
    assert [got[0][0, 1], got[1][0, 1], got[2][0, 1]] == [39999, 0, 1]


def test_two_accumulator_ties():
    """Identical trains in the two 32-row tiles of one stage, in consecutive stages and in the two lane halves of a tile, asked for by queries
    of both accumulators of a wave (columns 0-31 and 32-63) and of a later wave: the lower index wins and the second distance equals the best,
    for exact copies (0, 0) and for copies three bits away (3, 3)."""
    wave_q, wg_q, stage = _shape()
    rng = np.random.default_rng(53)
    cap = 3 * stage + wg_q + 40
    nq, nt = wave_q * 2 + 9, 3 * stage + 5
    q = rng.integers(0, 256, (2, cap, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (2, cap, 32), dtype=np.uint8)
    places = [(3, 3 + 32), (10, 10 + stage), (stage + 7, stage + 7 + 32), (stage + 31, 2 * stage), (2 * stage - 1, 2 * stage + 36), (17, 21),
              (40, 2 * stage + 40)]
    cols = [0, 31, 32, wave_q - 1, wave_q, wave_q + 33, 2 * wave_q + 8]
    for f, flip in enumerate([0, 3]):
        for (lo, hi), c in zip(places, cols):
            t[f, hi] = t[f, lo]
            q[f, c] = t[f, lo]
            for k in range(flip):
                q[f, c, 7 * k + 1] ^= 1 << k
    got = _run_batch(q, _counts([nq, nq]), t, _counts([nt, nt]))
    for f, flip in enumerate([0, 3]):
        _check([g[f] for g in got], q[f], nq, t[f], nt, flip)
        for (lo, hi), c in zip(places, cols):
            assert [got[0][f, c], got[1][f, c], got[2][f, c]] == [lo, flip, flip], (flip, lo, hi, c)


def test_ring_wraps_over_an_empty_frame():
    """Three frames of 65, 0 and 1 descriptors: 0 -> 1 has no train, 1 has no query, 2 -> 0 wraps to the first frame."""
    rng = np.random.default_rng(59)
    cap = 72
    d = rng.integers(0, 256, (3, cap, 32), dtype=np.uint8)
    d[0, 64] = d[2, 0]                                        # the wrapping query finds its copy in the last row of frame 0
    c = _counts([65, 0, 1])
    got = _run_ring(d, c)
    assert (got[0][0, :65] == -1).all() and (got[1][0, :65] == 256).all() and (got[2][0, :65] == 256).all()
    _check([g[2] for g in got], d[2], 1, d[0], 65, "wrap")
    assert [got[0][2, 0], got[1][2, 0]] == [64, 0]
