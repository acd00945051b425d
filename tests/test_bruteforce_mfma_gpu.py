"""The brute-force matcher on the int8 matrix cores (k_bruteforce_mfma) against the CPU oracle, bit for bit on best index, best
distance and second distance: every tile edge, ties across lane halves and train tiles, single-bit descriptors (a wrong MFMA fragment
map shows up as wrong distances), strided and ring layouts at 4 and 8 mod 16, extractor output, and near-ties in seeded batches."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 31, 32, 33, 255, 256, 257, 1000, 1096]


def _run_batch(q, cq, t, ct):
    import torch
    from rumi_slam_amd.matcher import bruteforce_batch
    out = bruteforce_batch(torch.from_numpy(q).cuda(), torch.from_numpy(cq).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(ct).cuda())
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def _check(got, q, nq, t, nt, tag):
    bi, bd, sd = got
    rbi, rbd, rsd = O.bruteforce_match(np.ascontiguousarray(q[:nq]), np.ascontiguousarray(t[:nt]))
    assert np.array_equal(bi[:nq], rbi), (tag, "best index")
    assert np.array_equal(bd[:nq], rbd), (tag, "best distance")
    assert np.array_equal(sd[:nq], rsd), (tag, "second distance")


def _counts(n):
    return np.stack([np.asarray(n, np.int32), np.zeros(len(n), np.int32)], 1)


def test_all_tile_edges():
    """Every (nq, nt) of SIZES in one launch, and counts above cap (clamped to it)."""
    rng = np.random.default_rng(5)
    cap = 1096
    pairs = [(a, b) for a in SIZES for b in SIZES] + [(5000, 1096), (1096, 70000), (2000, 300)]
    B = len(pairs)
    q = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    got = _run_batch(q, _counts([p[0] for p in pairs]), t, _counts([p[1] for p in pairs]))
    for b, (nq, nt) in enumerate(pairs):
        nq, nt = min(nq, cap), min(nt, cap)
        if nt == 0 and nq:
            assert (got[0][b, :nq] == -1).all() and (got[1][b, :nq] == 256).all() and (got[2][b, :nq] == 256).all()
        _check([g[b] for g in got], q[b], nq, t[b], nt, (nq, nt))


def test_ties_duplicates_complements():
    rng = np.random.default_rng(9)
    cap = 1096
    q = rng.integers(0, 256, (4, cap, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (4, cap, 32), dtype=np.uint8)
    # frame 0: duplicates across the lane halves of a tile (rows r and r + 4), across train tiles, at low and high indices
    for lo, hi in [(0, 4), (2, 6), (9, 13), (3, 40), (31, 32), (64, 1050), (100, 1095), (500, 503)]:
        t[0, hi] = t[0, lo]
        q[0, lo] = t[0, lo]                                  # a query equal to both copies: distance 0 at the lower index, second 0
    for k in range(120, 160):                                 # near-duplicates: one bit away from a train, in both halves of its tile
        q[0, k] = t[0, k + 5]
        q[0, k, k % 32] ^= 1 << (k % 8)
    # frame 1: every descriptor identical
    t[1] = t[1, 0].copy(); q[1] = t[1, 0].copy()
    # frame 2: one train, the bitwise complement of query 0 (distance 256 never wins)
    t[2] = ~q[2]
    # frame 3: only complements of query 0, and one exact copy of query 1 late in the list
    t[3] = ~q[3, 0].copy(); t[3, 1077] = q[3, 1]
    cq = _counts([cap, cap, 900, 50]); ct = _counts([cap, 1000, 1, cap])
    got = _run_batch(q, cq, t, ct)
    for b in range(4):
        _check([g[b] for g in got], q[b], int(cq[b, 0]), t[b], int(ct[b, 0]), b)
    assert [got[0][0, 3], got[1][0, 3], got[2][0, 3]] == [3, 0, 0]
    assert [got[0][0, 64], got[1][0, 64], got[2][0, 64]] == [64, 0, 0]
    assert (got[0][1, :cap] == 0).all() and (got[1][1, :cap] == 0).all() and (got[2][1, :cap] == 0).all()
    assert [got[0][2, 0], got[1][2, 0], got[2][2, 0]] == [-1, 256, 256]
    assert got[0][3, 1] == 1077 and got[1][3, 1] == 0


def test_single_bit_descriptors():
    """Train j holds only bit j (j < 256), then 32 zero rows: a query with bits S has distance |S| - 1 to the trains of S, |S| to the zero
    rows and |S| + 1 to the rest.  Any disagreement between the A and B fragment maps, or a wrong row / column map, moves these distances."""
    rng = np.random.default_rng(13)
    nt, nq = 288, 300
    t = np.zeros((1, 320, 32), np.uint8)
    for j in range(256):
        t[0, j, j >> 3] = 1 << (j & 7)
    q = np.zeros((1, 320, 32), np.uint8)
    for i in range(256):
        q[0, i, i >> 3] = 1 << (i & 7)                        # single bits: train i at distance 0, every other at 2
    for i in range(256, nq):                                  # a few chosen bits each
        for k in rng.choice(256, size=int(rng.integers(2, 9)), replace=False):
            q[0, i, k >> 3] |= 1 << (k & 7)
    got = _run_batch(q, _counts([nq]), t, _counts([nt]))
    _check([g[0] for g in got], q[0], nq, t[0], nt, "single bit")
    assert np.array_equal(got[0][0, :256], np.arange(256)) and (got[1][0, :256] == 0).all() and (got[2][0, :256] == 1).all()


@pytest.mark.parametrize("mod", [4, 8])
def test_strided_and_ring_misaligned(mod):
    """Frames at a stride of 4 or 8 mod 16 from a base at the same offset (the records layout of the N > 1 path)."""
    import torch
    from rumi_slam_amd.matcher import bruteforce_batch, bruteforce_ring
    rng = np.random.default_rng(17 + mod)
    B, cap = 5, 1096
    stride = cap * 32 + 48 + mod                              # == mod (mod 16)
    raw = torch.from_numpy(rng.integers(0, 256, B * stride + 64, dtype=np.uint8)).cuda()
    desc = raw[mod:].as_strided((B, cap, 32), (stride, 32, 1))
    assert desc.data_ptr() % 16 == mod and desc.stride(0) % 16 == mod
    counts = torch.from_numpy(_counts([1096, 1000, 257, 33, 1005])).cuda()
    ri, rd, rs = [x.cpu().numpy() for x in bruteforce_ring(desc, counts)]
    bi, bd, sd = [x.cpu().numpy() for x in bruteforce_batch(desc[:-1], counts[:-1], desc[1:], counts[1:])]
    torch.cuda.synchronize()
    d, c = desc.cpu().numpy(), counts.cpu().numpy()
    for b in range(B):
        tb = (b + 1) % B
        _check((ri[b], rd[b], rs[b]), d[b], int(c[b, 0]), d[tb], int(c[tb, 0]), ("ring", b))
        if b < B - 1:
            _check((bi[b], bd[b], sd[b]), d[b], int(c[b, 0]), d[tb], int(c[tb, 0]), ("strided", b))


def test_ring_on_extractor_records():
    """Consecutive warped frames through the extractor's records and the ring launch: many near-ties, as in the benchmark."""
    import torch
    from rumi_slam_amd import rumination as R
    from rumi_slam_amd.extractor import ORBextractor
    from rumi_slam_amd.matcher import bruteforce_ring
    from rumi_slam_amd.synth import synth_frame, warp_frame
    img0 = synth_frame(91)
    frames = [img0] + [warp_frame(img0, 200 + i)[0] for i in range(5)]
    ext = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=len(frames))
    cap = 1000 + 4 * 8 + 64
    rec = ext.extract_batch_records(torch.from_numpy(np.stack(frames)).cuda(), cap=cap)
    ext.sync()
    kp, desc, counts = R.record_views(rec, cap)
    ri, rd, rs = [x.cpu().numpy() for x in bruteforce_ring(desc, counts)]
    torch.cuda.synchronize()
    d, c = desc.cpu().numpy(), counts.cpu().numpy()
    B = len(frames)
    for b in range(B):
        tb = (b + 1) % B
        _check((ri[b], rd[b], rs[b]), d[b], int(c[b, 0]), d[tb], int(c[tb, 0]), b)
    assert (rd[1, :int(c[1, 0])] < 40).sum() > 300


def test_seeded_batch_and_ring_vs_oracle():
    """Six frames of 1096 descriptors, every third train a few bits from its query (near-ties), counts (1096, 1000, 0, 33, 257, 1005)
    against the flipped counts, and the ring launch over the trains."""
    import torch
    from rumi_slam_amd.matcher import bruteforce_ring
    rng = np.random.default_rng(23)
    q = rng.integers(0, 256, (6, 1096, 32), dtype=np.uint8)
    t = q.copy()
    t[:, ::3] ^= rng.integers(0, 4, (6, 366, 32), dtype=np.uint8)
    c = _counts([1096, 1000, 0, 33, 257, 1005])
    ct = np.ascontiguousarray(c[::-1])
    got = _run_batch(q, c, t, ct)
    for b in range(6):
        _check([g[b] for g in got], q[b], int(c[b, 0]), t[b], int(ct[b, 0]), ("batch", b))
    ri, rd, rs = [x.cpu().numpy() for x in bruteforce_ring(torch.from_numpy(t).cuda(), torch.from_numpy(c).cuda())]
    torch.cuda.synchronize()
    for b in range(6):
        tb = (b + 1) % 6
        _check((ri[b], rd[b], rs[b]), t[b], int(c[b, 0]), t[tb], int(c[tb, 0]), ("ring", b))
