"""k_bruteforce_pair (one pair, train rows split over workgroups, last-arriver merge) on the device: the constructed cases of
tests/stream_cases.py at forced slice counts 1, 2, 3, the maximum and the automatic one, bit for bit against the written expectations, the CPU
oracle and the batch kernel at nbatch = 1; rows at or past the query count untouched; descriptor blocks that are only 4-byte aligned; one scratch
reused without clearing; one random 1000 x 1000 pair."""
import numpy as np
import pytest

import oracle_lib as O
import stream_cases as SC

pytestmark = pytest.mark.gpu

FILL = -7


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _count(n):
    return _dev(np.array([n, 0], np.int32))


def _run_pair(q, nq, t, nt, slices, scratch=None, misaligned=False):
    import torch
    from rumi_slam_amd.matcher import bruteforce_pair
    cap = q.shape[0]
    if misaligned:                       # the descriptor block of a per-frame record {n, mono, kp[cap], desc[cap][32]}: 8 + 28 cap bytes into an aligned block
        off = 8 + 28 * cap
        assert off % 4 == 0 and off % 16 != 0
        bq, bt = (torch.zeros(8 + 60 * cap, dtype=torch.uint8, device="cuda") for _ in range(2))
        assert bq.data_ptr() % 16 == 0 and bt.data_ptr() % 16 == 0
        dq, dt = bq[off:].view(cap, 32), bt[off:].view(cap, 32)
        dq.copy_(_dev(q)); dt.copy_(_dev(t))
    else:
        dq, dt = _dev(q), _dev(t)
    out = [torch.full((cap,), FILL, dtype=torch.int32, device="cuda") for _ in range(3)]
    bruteforce_pair(dq, _count(nq), dt, _count(nt), slices=slices, scratch=scratch, out=out)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def _run_batch1(q, nq, t, nt):
    import torch
    from rumi_slam_amd.matcher import bruteforce_batch
    out = bruteforce_batch(_dev(q[None]), _count(nq)[None], _dev(t[None]), _count(nt)[None])
    torch.cuda.synchronize()
    return [x.cpu().numpy()[0] for x in out]


def _oracle(q, nq, t, nt):
    return O.bruteforce_match(np.ascontiguousarray(q[:nq]), np.ascontiguousarray(t[:nt]))


def _check_case(c, got, tag):
    nq = c["nq"]
    SC.check_expectations(c, *got)
    for g, r, b, what in zip(got, _oracle(c["q"], nq, c["t"], c["nt"]), _run_batch1(c["q"], nq, c["t"], c["nt"]), ("best index", "best distance", "second distance")):
        assert np.array_equal(g[:nq], r), (tag, c["name"], what, "oracle")
        assert np.array_equal(g[:nq], b[:nq]), (tag, c["name"], what, "batch kernel")
        assert (g[nq:] == FILL).all(), (tag, c["name"], what, "rows past nq written")


@pytest.mark.parametrize("slices", [1, 2, 3, SC.max_slices(), 0])
def test_constructed_cases(slices):
    from rumi_slam_amd.matcher import bruteforce_pair_scratch, bruteforce_pair_shape
    used, rows = bruteforce_pair_shape(SC.CAP, SC.CAP, slices)
    assert used >= 1 and (slices == 0 or used == slices)
    scratch = bruteforce_pair_scratch(SC.CAP, "cuda")        # one scratch for the whole run: every call leaves its tickets at zero
    for c in SC.build(rows):
        _check_case(c, _run_pair(c["q"], c["nq"], c["t"], c["nt"], slices, scratch=scratch), (slices, rows))


@pytest.mark.parametrize("slices", [1, 3, 0])
def test_misaligned_descriptor_bases(slices):
    """Both descriptor blocks 4-byte but not 16-byte aligned, at a record's offset 8 + 28 cap."""
    from rumi_slam_amd.matcher import bruteforce_pair_shape
    rows = bruteforce_pair_shape(SC.CAP, SC.CAP, slices)[1]
    for c in SC.build(rows)[:3]:
        _check_case(c, _run_pair(c["q"], c["nq"], c["t"], c["nt"], slices, misaligned=True), ("misaligned", slices))


def test_scratch_reuse_without_clearing():
    """Three calls with different (nq, nt, slices) on one scratch, then the first again: equal to fresh-scratch runs, so every merging
    workgroup has put its ticket back."""
    from rumi_slam_amd.matcher import bruteforce_pair_scratch
    rng = np.random.default_rng(7)
    q = rng.integers(0, 256, (SC.CAP, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (SC.CAP, 32), dtype=np.uint8)
    t[500], t[900] = q[3], q[3]
    calls = [(700, 1000, SC.max_slices()), (257, 130, 2), (SC.CAP, SC.CAP, 3), (700, 1000, SC.max_slices())]
    scratch = bruteforce_pair_scratch(SC.CAP, "cuda")
    shared = [_run_pair(q, nq, t, nt, s, scratch=scratch) for nq, nt, s in calls]
    for (nq, nt, s), got in zip(calls, shared):
        fresh = _run_pair(q, nq, t, nt, s)
        for g, f, r in zip(got, fresh, _oracle(q, nq, t, nt)):
            assert np.array_equal(g, f), (nq, nt, s)
            assert np.array_equal(g[:nq], r), (nq, nt, s)
    assert [shared[0][0][3], shared[0][1][3], shared[0][2][3]] == [500, 0, 0]
    assert all(np.array_equal(a, b) for a, b in zip(shared[0], shared[3]))
    tickets = (SC.max_slices() * SC.CAP * 8 + 15) // 16 * 16                   # the scratch: [slices][cap][2] f32, then a ticket per query block
    assert int(scratch[:tickets].count_nonzero()) > 0 and int(scratch[tickets:].count_nonzero()) == 0   # partials stay, tickets are back at zero


def test_random_1000_by_1000():
    rng = np.random.default_rng(20251)
    cap = 1000
    q = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
    got = _run_pair(q, cap, t, cap, 0)
    for g, r, b in zip(got, _oracle(q, cap, t, cap), _run_batch1(q, cap, t, cap)):
        assert np.array_equal(g, r) and np.array_equal(g, b)
