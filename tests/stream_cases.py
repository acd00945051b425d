"""Constructed descriptor pairs for the one-pair brute-force kernel (k_bruteforce_pair), with hand-written expectations.  The kernel splits the
train rows into slices of R rows that run on different workgroups and merges their (best, second) pairs, so the cases sit on the slice
boundaries: `build(rows)` places them for a given R = rows per slice (rumi_match_bruteforce_pair_shape).  A case is a dict

    name, q [CAP,32] u8, nq, t [CAP,32] u8, nt, expect {query row: (best index, best distance, second distance or None)}

Background rows are random (Hamming distance to anything about 128 +- 8, never below 60 for these seeds), constructed rows are copies at most
three bits apart, so the expectations follow from the placement alone.  tests/test_stream_cases_cpu.py checks every expectation against the CPU
oracle; the GPU tests compare whole result arrays.  Needs neither GPU nor library."""
import numpy as np

CAP = 1096
STAGE = 64                      # train rows per stage of the brute-force kernels (rumi_match_bruteforce_shape()[2]; the CPU test checks it)
NQ_LIST = [1, 63, 64, 65, 256, 257, CAP]


def max_slices(cap=CAP):
    """The largest slice count the entry accepts: a slice is at least one stage, and the scratch holds 64 partials a query."""
    return min((cap + STAGE - 1) // STAGE, 64)


def nt_list(rows):
    return sorted({min(max(n, 0), CAP) for n in (0, 1, rows - 1, rows, rows + 1, 2 * rows + 31, CAP)})


def flip(d, nbits, start=0):
    """A copy of descriptor d with `nbits` bits flipped, one per byte from byte `start` on."""
    d = d.copy()
    for k in range(nbits):
        d[(start + 3 * k) % 32] ^= np.uint8(1 << (k % 8))
    return d


def placement(rows):
    """(Rp, Sp): the slice length the cases are placed on and the number of such slices in CAP rows.  A kernel run as ONE slice has no
    boundary: the cases then sit on the stage boundaries it walks."""
    rp = rows if rows < CAP else STAGE
    return rp, (CAP + rp - 1) // rp


def _random_pair(seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (CAP, 32), dtype=np.uint8), rng.integers(0, 256, (CAP, 32), dtype=np.uint8), rng


def build(rows):
    rp, sp = placement(rows)
    assert sp >= 2
    last0 = (sp - 1) * rp                                    # first row of the last slice; its last row is CAP - 1
    assert CAP - last0 >= 8
    cases = []

    # equal minima in different slices: last row of slice 0 / first row of slice 1, last slice / slice 0; copies three bits away across a boundary
    q, t, rng = _random_pair(101)
    d, e, f = (rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(3))
    q[0], t[rp - 1], t[rp] = d, d, d
    q[1], t[CAP - 1], t[0] = e, e, e
    q[2], t[rp - 2], t[rp + 1] = flip(f, 3), f, f
    q[300] = q[0]                                            # the same from another wave and the second accumulator
    cases.append(dict(name="equal_minima_across_slices", q=q, nq=301, t=t, nt=CAP,
                      expect={0: (rp - 1, 0, 0), 1: (0, 0, 0), 2: (rp - 2, 3, 3), 300: (rp - 1, 0, 0)}))

    # best and second in one slice while the others hold worse rows; best in slice a, runner-up in slice b, both orders
    q, t, rng = _random_pair(102)
    d, e, f, g = (rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(4))
    q[0], t[5], t[9] = d, flip(d, 1), flip(d, 2, 1)
    q[1], t[last0 + 4], t[last0 + 2] = e, flip(e, 1), flip(e, 2, 1)            # both in the last slice, the better one at the higher row
    q[2], t[11], t[last0 + 6] = f, flip(f, 1), flip(f, 2, 1)                   # best in slice 0, runner-up in the last slice
    q[3], t[last0 + 1], t[13] = g, flip(g, 1), flip(g, 2, 1)                   # best in the last slice, runner-up in slice 0
    cases.append(dict(name="best_and_second_placement", q=q, nq=70, t=t, nt=CAP,
                      expect={0: (5, 1, 2), 1: (last0 + 4, 1, 2), 2: (11, 1, 2), 3: (last0 + 1, 1, 2)}))

    # an exact duplicate of the best inside the same slice and in another slice at once: the multiset's second is a tie
    q, t, rng = _random_pair(103)
    d, e = (rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(2))
    q[0], t[3], t[40], t[rp + 6] = d, d, d, d
    q[1], t[rp + 3], t[rp + 41], t[7] = e, e, e, e
    cases.append(dict(name="duplicate_best_in_and_across_slices", q=q, nq=2, t=t, nt=CAP, expect={0: (3, 0, 0), 1: (7, 0, 0)}))

    # all-zero queries against all-one train rows: Ham 256, index -1, both distances 256 -- alone, and mixed with one row at distance 255 at a
    # slice's first row, at a slice's last row, and with two such rows in different slices
    ones = np.full((CAP, 32), 255, np.uint8)
    zq = np.zeros((CAP, 32), np.uint8)
    cases.append(dict(name="ham256_everywhere", q=zq.copy(), nq=65, t=ones.copy(), nt=CAP, expect={i: (-1, 256, 256) for i in (0, 31, 32, 64)}))
    for name, where, exp in (("ham256_and_255_at_slice_first_row", [rp], (rp, 255, 256)), ("ham256_and_255_at_slice_last_row", [rp - 1], (rp - 1, 255, 256)),
                             ("ham256_and_255_in_two_slices", [last0 + 1, 17], (17, 255, 255)), ("ham256_and_255_at_last_row", [CAP - 1], (CAP - 1, 255, 256))):
        t = ones.copy()
        for k, r in enumerate(where):
            t[r, 5 + k] = 0xEF
        cases.append(dict(name=name, q=zq.copy(), nq=65, t=t, nt=CAP, expect={i: exp for i in (0, 33, 64)}))

    # train counts on the slice edges: the only copy of query 0 in the last valid row, a copy of query 1 just behind it (must not be seen)
    for nt in nt_list(rows):
        q, t, rng = _random_pair(200 + nt)
        exp = {0: (-1, 256, 256), 1: (-1, 256, 256)} if nt == 0 else {0: (nt - 1, 0, None)}
        if nt > 0:
            t[nt - 1] = q[0]
        if nt < CAP:
            t[nt] = q[1]
        cases.append(dict(name=f"train_count_{nt}", q=q, nq=65, t=t, nt=nt, expect=exp))

    # query counts on the wave and workgroup edges: the last query's only copy in the last train row
    for nq in NQ_LIST:
        q, t, rng = _random_pair(300 + nq)
        t[CAP - 1] = q[nq - 1]
        cases.append(dict(name=f"query_count_{nq}", q=q, nq=nq, t=t, nt=CAP, expect={nq - 1: (CAP - 1, 0, None)}))
    return cases


def check_expectations(case, best_idx, best_dist, second_dist):
    for row, (bi, bd, sd) in case["expect"].items():
        assert row < case["nq"], (case["name"], row)
        got = (int(best_idx[row]), int(best_dist[row]), int(second_dist[row]))
        assert got[:2] == (bi, bd) and (sd is None or got[2] == sd), (case["name"], row, got, (bi, bd, sd))
        if sd is None:
            assert got[2] >= 60, (case["name"], row, got)      # a lone copy: the runner-up is a background row
