"""What the streaming front-end (k_bruteforce_pair, RumiOrbStream) can be asked without a device: the constructed cases of tests/stream_cases.py
against the CPU oracle, so that no GPU test passes on an empty case; the host-only shape and scratch entries; the argument refusals; the
exports."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import stream_cases as SC
from rumi_slam_amd import capi
from rumi_slam_amd.matcher import bruteforce_pair_scratch_bytes, bruteforce_pair_shape, bruteforce_shape, _lib


_max_slices = SC.max_slices


def slice_settings(cap=SC.CAP):
    """The slice counts the GPU tests force (1, 2, 3, the maximum) and the automatic one (0), each with its rows per slice."""
    return [(s, bruteforce_pair_shape(cap, cap, s)[1]) for s in (1, 2, 3, _max_slices(cap), 0)]


def test_stage_constant_is_the_kernels():
    assert bruteforce_shape()[2] == SC.STAGE


@pytest.mark.parametrize("slices", [1, 2, 3, SC.max_slices(), 0])
def test_oracle_gives_the_written_expectations(slices):
    rows = bruteforce_pair_shape(SC.CAP, SC.CAP, slices)[1]
    cases = SC.build(rows)
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    assert {f"train_count_{n}" for n in SC.nt_list(rows)} <= set(names) and {f"query_count_{n}" for n in SC.NQ_LIST} <= set(names)
    for c in cases:
        assert c["expect"] and 1 <= c["nq"] <= SC.CAP and 0 <= c["nt"] <= SC.CAP
        bi, bd, sd = O.bruteforce_match(np.ascontiguousarray(c["q"][:c["nq"]]), np.ascontiguousarray(c["t"][:c["nt"]]))
        SC.check_expectations(c, bi, bd, sd)


def test_cases_sit_on_the_slice_boundaries():
    """For a kernel of several slices the constructed rows straddle ITS boundaries (rows R - 1 and R, the last slice against slice 0)."""
    for slices, rows in slice_settings():
        rp, sp = SC.placement(rows)
        assert rp % SC.STAGE == 0 and sp >= 2
        if rows < SC.CAP:
            assert rp == rows
        c = SC.build(rows)[0]
        assert c["expect"][0][0] == rp - 1 and np.array_equal(c["t"][rp - 1], c["t"][rp])


def test_pair_shape_is_consistent():
    stage = bruteforce_shape()[2]
    for cap in (1, 63, 64, 65, 500, SC.CAP, 5000, 65535):
        mx = _max_slices(cap)
        for nt in (0, 1, stage - 1, stage, stage + 1, cap // 2, cap, cap + 100):
            for slices in [0, 1, 2, 3, mx]:
                if slices > mx:
                    continue
                used, rows = bruteforce_pair_shape(cap, nt, slices)
                assert used >= 1 and rows >= stage and rows % stage == 0, (cap, nt, slices)
                assert used * rows >= min(max(nt, 1), cap), (cap, nt, slices)
                assert slices == 0 or used == slices, (cap, nt, slices)          # a forced count is honoured ...
                assert used <= mx
        for bad in (-1, mx + 1, 10 ** 6):                                         # ... or refused
            assert bruteforce_pair_shape(cap, cap, bad) == (0, 0), (cap, bad)
    for cap in (0, -5, 65536):
        assert bruteforce_pair_shape(cap, 10, 0) == (0, 0)
    assert bruteforce_pair_shape(SC.CAP) == bruteforce_pair_shape(SC.CAP, SC.CAP, 0)


def test_scratch_bytes_monotone():
    prev = 0
    for cap in list(range(1, 700)) + [1000, SC.CAP, 4096, 20000, 65535]:
        b = bruteforce_pair_scratch_bytes(cap)
        assert b >= prev and b > 0 and b % 16 == 0, cap
        used, rows = bruteforce_pair_shape(cap, cap, _max_slices(cap))
        assert b >= used * cap * 8 + 4 * ((cap + bruteforce_shape()[1] - 1) // bruteforce_shape()[1]), cap   # [S][cap][2] f32 and a ticket per query block
        prev = b
    assert bruteforce_pair_scratch_bytes(0) == 0 and bruteforce_pair_scratch_bytes(65536) == 0


def test_pair_entry_refuses_without_a_device():
    L = _lib()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16          # a 16-byte aligned address: never dereferenced, every call below is refused first
    good = dict(q=p, nq=p, t=p, nt=p, cap=16, slices=1, scratch=p, bi=p, bd=p, sd=p)

    def call(**kw):
        a = dict(good, **kw)
        return L.rumi_match_bruteforce_pair_device(a["q"], a["nq"], a["t"], a["nt"], a["cap"], a["slices"], a["scratch"], a["bi"], a["bd"], a["sd"], None)
    for name in ("q", "nq", "t", "nt", "scratch", "bi", "bd", "sd"):
        assert call(**{name: None}) == capi.RUMI_E_INVALID, name
    for kw in (dict(cap=0), dict(cap=-1), dict(cap=65536), dict(slices=-1), dict(slices=2), dict(cap=SC.CAP, slices=_max_slices(SC.CAP) + 1),
               dict(q=p + 2), dict(t=p + 1), dict(scratch=p + 4)):
        assert call(**kw) == capi.RUMI_E_INVALID, kw
    assert b"rumi_match_bruteforce_pair_device" in L.rumi_last_error()


def test_stream_entries_refuse_null():
    L = capi.lib()
    s, f = C.c_void_p(), capi.RumiStreamFrame()
    assert L.rumi_orb_stream_create(None, C.byref(s)) == capi.RUMI_E_INVALID and not s.value
    assert L.rumi_orb_stream_create(None, None) == capi.RUMI_E_INVALID
    assert L.rumi_orb_stream_reset(None) == capi.RUMI_E_INVALID
    assert L.rumi_orb_stream_push(None, None, 0, 0, 0, 0, 1000, C.byref(f)) == capi.RUMI_E_INVALID and f.mono == -1 and f.n == 0
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.rumi_orb_stream_resident(None, C.byref(a), C.byref(b), C.byref(c)) == capi.RUMI_E_INVALID
    L.rumi_orb_stream_destroy(None)


def test_new_symbols_exported():
    L = capi.lib()
    new = ["rumi_match_bruteforce_pair_scratch_bytes", "rumi_match_bruteforce_pair_shape", "rumi_match_bruteforce_pair_device",
           "rumi_orb_stream_create", "rumi_orb_stream_destroy", "rumi_orb_stream_reset", "rumi_orb_stream_push", "rumi_orb_stream_resident"]
    for name in new:
        assert hasattr(L, name), name
    assert set(new[:3]) <= set(capi.MATCH_SYMBOLS) and set(new[3:]) <= set(capi.ORB_SYMBOLS)
