"""IC_Angle by rows (k_disc_angle, csrc/orb_orient_desc.inc) on the CPU: rumi_hook_disc_moments evaluates the kernel's own chunk function
(disc_chunk_moments, csrc/orb_math.h: the eight dot products of a row's 16-byte half against its weight and mask vectors, the two moments) on the
2 x 16 bytes a row's two lanes load, and the vectors the launch code builds from the umax table (make_disc_vectors, csrc/orb_geom.h).  The
reference is the direct double loop of lib_src/ORBextractor.cc:73-97 written in numpy over the 31 x 31 neighbourhood: m_10 = sum of u * I(v, u),
m_01 = sum of v * I(v, u) over |u| <= umax[|v|].

A staged row is the 36 bytes of the level from (x - 15) & ~3 on; the disc's column u = -15 sits in byte s = 0..3 of it (s = (x - 15) & 3) and the
kernel loads the 32 bytes from there.  Bytes [0, s) and [s + 31, 36) belong to the neighbours and must contribute nothing: byte s + 31 (u = 16)
is loaded and masked, the others are never read."""
import ctypes as C

import numpy as np
import pytest

from rumi_slam_amd import capi
from rumi_slam_amd.extractor import tables

ROWS, ROWB, HALF = 31, 36, 15
UMAX = np.ascontiguousarray(tables()["umax"], np.int32)


def hook(rows, s, want_vectors=False):
    rows = np.ascontiguousarray(rows, np.uint8)
    assert rows.shape == (ROWS, ROWB)
    m01, m10 = C.c_int32(), C.c_int32()
    W, M = np.zeros((ROWS, 8), np.uint32), np.zeros((ROWS, 8), np.uint32)
    rc = capi.hooks().rumi_hook_disc_moments(capi.ptr(rows), s, capi.ptr(UMAX), C.byref(m01), C.byref(m10), capi.ptr(W) if want_vectors else None,
                                             capi.ptr(M) if want_vectors else None)
    assert rc == 0
    return (m01.value, m10.value, W, M) if want_vectors else (m01.value, m10.value)


def direct(rows, s):
    """ORBextractor.cc:73-97: the double loop, v outside, u inside."""
    disc = rows[:, s:s + ROWS].astype(np.int64)
    m01 = m10 = 0
    for v in range(-HALF, HALF + 1):
        for u in range(-int(UMAX[abs(v)]), int(UMAX[abs(v)]) + 1):
            m10 += u * int(disc[v + HALF, u + HALF])
            m01 += v * int(disc[v + HALF, u + HALF])
    return m01, m10


def test_umax_is_symmetric():
    """The row formulation sums the pixels of the column one only because the disc is its own transpose: |u| <= umax[|v|]  <=>  |v| <= umax[|u|]."""
    assert UMAX.shape == (16,) and UMAX[0] == HALF
    for u in range(HALF + 1):
        for v in range(HALF + 1):
            assert (u <= UMAX[v]) == (v <= UMAX[u]), (u, v)


@pytest.mark.parametrize("s", range(4))
def test_vectors(s):
    """W: byte u + 15 of row v holds u + 15 inside the disc, M: 1 there; 0 everywhere else, byte 31 included."""
    _, _, W, M = hook(np.zeros((ROWS, ROWB), np.uint8), s, True)
    Wb, Mb = W.view(np.uint8).reshape(ROWS, 32), M.view(np.uint8).reshape(ROWS, 32)
    for r in range(ROWS):
        inside = np.abs(np.arange(32) - HALF) <= UMAX[abs(r - HALF)]
        inside[31] = False
        assert np.array_equal(Mb[r], inside.astype(np.uint8)), r
        assert np.array_equal(Wb[r], np.where(inside, np.arange(32), 0).astype(np.uint8)), r


@pytest.mark.parametrize("s", range(4))
def test_constant_and_random_neighbourhoods(s):
    rng = np.random.default_rng(100 + s)
    full = np.full((ROWS, ROWB), 255, np.uint8)
    assert hook(full, s) == direct(full, s) == (0, 0)
    # the largest magnitudes: everything right of / below the centre at 255, the rest 0 (and the mirror images)
    for sl, sign in (((slice(None), slice(s + HALF + 1, None)), 1), ((slice(None), slice(None, s + HALF)), -1)):
        img = np.zeros((ROWS, ROWB), np.uint8)
        img[sl] = 255
        assert hook(img, s) == direct(img, s)
        assert hook(img, s)[0] == 0 and sign * hook(img, s)[1] > 0
    for sl in ((slice(HALF + 1, None), slice(None)), (slice(None, HALF), slice(None))):
        img = np.zeros((ROWS, ROWB), np.uint8)
        img[sl] = 255
        assert hook(img, s) == direct(img, s) and hook(img, s)[1] == 0 and hook(img, s)[0] != 0
    zero = np.zeros((ROWS, ROWB), np.uint8)
    assert hook(zero, s) == (0, 0)
    for _ in range(40):
        img = rng.integers(0, 256, (ROWS, ROWB), dtype=np.uint8)
        assert hook(img, s) == direct(img, s)


@pytest.mark.parametrize("s", range(4))
def test_single_pixel_at_every_staged_position(s):
    """A lone 255 at each of the 31 x 36 staged bytes pins every weight and every mask byte: (v, u) inside the disc gives (255 v, 255 u), the
    corners outside the disc and the bytes left and right of the 31 columns give (0, 0)."""
    for r in range(ROWS):
        for b in range(ROWB):
            img = np.zeros((ROWS, ROWB), np.uint8)
            img[r, b] = 255
            v, u = r - HALF, b - s - HALF
            want = (255 * v, 255 * u) if abs(u) <= HALF and abs(u) <= UMAX[abs(v)] else (0, 0)
            assert hook(img, s) == want, (r, b)
    # (the expectation above is the double loop's: spot-checked against it)
    for r, b in ((0, s), (0, s + HALF), (4, s + 1), (30, s + 30), (15, s), (15, ROWB - 1)):
        img = np.zeros((ROWS, ROWB), np.uint8)
        img[r, b] = 255
        assert hook(img, s) == direct(img, s)
