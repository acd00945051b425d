"""The byte compare of k_fast_cells' quick test (fast_score_cell_bytes), restated on the CPU over every byte pair: v_lerp_u8 computes
(a + b + (r & 1)) >> 1 per byte, so bit 7 of lerp(p, ~x, 0) is [p > x] and bit 7 of lerp(p, ~y, 1) is [p >= y]; with x = sat(v + T),
y = sat(v - T) these are cv::FAST's strict brighter / darker tests.  Also the multiplication that turns the flag bits into the ring mask."""
import numpy as np

from test_fast_bytes_gpu import RING_CAP, level0_step_entries, make_frame, quick_entries


def _lerp_u8(a, b, r):
    return (a.astype(np.int32) + b.astype(np.int32) + (r & 1)) >> 1


def test_lerp_compare_identity_all_pairs():
    p, x = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    gt = (_lerp_u8(p, 255 - x, 0) >> 7) & 1
    ge = (_lerp_u8(p, 255 - x, 1) >> 7) & 1
    assert np.array_equal(gt, (p > x).astype(np.int32))
    assert np.array_equal(ge, (p >= x).astype(np.int32))
    # results stay bytes: (a + b + 1) >> 1 <= 255
    assert _lerp_u8(p, 255 - x, 1).max() <= 255


def test_saturated_thresholds_match_strict_fast_tests():
    """~sat(v + T) = sat(~v - T) and ~sat(v - T) = sat(~v + T) (the packed 16-bit clamp forms), and the compares built on them are
    cv::FAST's p > v + T / p < v - T for every (p, v) and the thresholds the tests use."""
    p, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for T in (1, 7, 20, 254):
        nb = np.maximum(255 - v - T, 0)
        nd = np.minimum(255 - v + T, 255)
        assert np.array_equal(nb, 255 - np.minimum(v + T, 255))
        assert np.array_equal(nd, 255 - np.maximum(v - T, 0))
        brighter = (_lerp_u8(p, nb, 0) >> 7) & 1
        not_darker = (_lerp_u8(p, nd, 1) >> 7) & 1
        assert np.array_equal(brighter, (p > v + T).astype(np.int32)), T
        assert np.array_equal(1 - not_darker, (p < v - T).astype(np.int32)), T


def test_high_byte_clamp_arithmetic():
    """The thresholds travel in the HIGH byte of 16-bit halves with arbitrary low bytes: a clamped add / subtract of T << 8 leaves
    sat(h + T) / sat(h - T) there."""
    h, lo = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    x = (h << 8) | lo
    for T in (1, 7, 20, 254):
        assert np.array_equal(np.minimum(x + (T << 8), 0xFFFF) >> 8, np.minimum(h + T, 255))
        assert np.array_equal(np.maximum(x - (T << 8), 0) >> 8, np.maximum(h - T, 0))


def test_ring_mask_multiplication():
    """fast_bytes_ringmask: flags at bits 8 q + 6 (darker) and 8 q + 7 (brighter) times 0x41041 land, and only they, in bits 24 + 2 q and
    25 + 2 q, for every combination."""
    for bits in range(256):
        f = 0
        for q in range(4):
            f |= ((bits >> (2 * q)) & 1) << (8 * q + 6) | ((bits >> (2 * q + 1)) & 1) << (8 * q + 7)
        assert ((f * 0x41041) & 0xFFFFFFFF) >> 24 == bits, bits


def test_split_append_is_taken_by_ramp():
    """The ramp frame of tests/test_fast_bytes_gpu.py at T = 1: most level-0 steps of k_fast_cells append more than the ring holds, so
    the two-halves append is taken whatever (< 128) entries wait from the step before; no step exceeds 64 items x 8 pixels x 2."""
    steps = level0_step_entries(make_frame("ramp"), 1)
    assert (steps > RING_CAP).sum() > len(steps) // 2, (steps.max(), (steps > RING_CAP).sum(), len(steps))
    assert steps.max() <= 1024


def test_quick_entries_restatement():
    """The restated quick test on hand-made neighbourhoods: a pixel on the ramp passes in both polarities, a flat one in neither, a dot
    brighter than all its ring passes darker-ring only; contrasts of exactly T do not count."""
    y, x = np.mgrid[0:16, 0:16]
    assert (quick_entries(((2 * x + y) % 256).astype(np.uint8), 1)[4:12, 4:12] == 2).all()
    flat = np.full((16, 16), 100, np.uint8)
    assert (quick_entries(flat, 1) == 0).all()
    dot = flat.copy(); dot[8, 8] = 102
    e = quick_entries(dot, 1)
    assert e[8, 8] == 1 and quick_entries(dot, 2)[8, 8] == 0
