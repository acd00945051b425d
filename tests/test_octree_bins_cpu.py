"""The batch quadtree's coordinate tables (csrc/orb_octree.h: oct_level_tabs, oct_coord_bin, oct_make_bins -- what set_geometry uploads and
k_compact / k_oct_select index), read through rumi_hook_octree_bins, against a numpy restatement of DivideNode's halving rule:

  a key belongs to root r = min(int(x / hX), nIni - 1) with hX = float32(W) / nIni, the root spans [int(hX r), int(hX (r + 1))) x [0, H), and a
  node [lo, hi) is cut at lo + ceil((hi - lo) / 2): the right / lower child takes v >= that.  The x half of a key's depth-D path is
  root << 2 D | bit 2 (D - 1 - d) for a right turn at depth d, the y half bit 2 (D - 1 - d) + 1 for a lower one."""
import numpy as np
import pytest

from rumi_slam_amd import capi

H = capi.hooks()
F32 = np.float32

# (width, height, nfeatures, scale factor, levels)
GEOMETRIES = [(640, 480, 1000, 1.2, 8), (320, 240, 1000, 1.2, 4), (1118, 112, 500, 1.2, 1), (71, 71, 30, 1.2, 1)]


def hook(w, h, nfeat, sf, nl, level):
    info = np.zeros(6, np.int32)
    bins = np.zeros(w + h + 8, np.uint16)
    n = capi.C.c_int32(0)
    rc = H.rumi_hook_octree_bins(w, h, nfeat, F32(sf), nl, level, capi.ptr(info), capi.ptr(bins), len(bins), capi.C.byref(n))
    assert rc == capi.RUMI_OK, rc
    return [int(v) for v in info], bins[:n.value].copy()


def tab_depth(n_ini, N):
    D = 4 if N <= 256 else 5 if N <= 1024 else 6 if N <= 1152 else 5
    while D > 1 and (n_ini << (2 * D)) > 4096:
        D -= 1
    return D


def halves(lo, hi, v, D):
    bits = 0
    for _ in range(D):
        mid = lo + ((hi - lo + 1) >> 1)
        right = v >= mid
        lo, hi = (mid, hi) if right else (lo, mid)
        bits = bits * 4 + int(right)
    return bits


def restated(W, Hh, n_ini, D):
    hX = F32(W) / F32(n_ini)
    xs, ys = [], []
    for v in range(W + 1):
        r = min(int(F32(v) / hX), n_ini - 1)
        xs.append((r << (2 * D)) | halves(int(hX * F32(r)), int(hX * F32(r + 1)), v, D))
    for v in range(Hh + 1):
        ys.append(halves(0, Hh, v, D) << 1)
    return np.array(xs, np.uint16), np.array(ys, np.uint16)


def levels_of(g):
    return [pytest.param(g, l, id="%dx%d-L%d" % (g[0], g[1], l)) for l in range(g[4])]


@pytest.mark.parametrize("g,level", [p for g in GEOMETRIES for p in levels_of(g)])
def test_tables_follow_the_halving_rule(g, level):
    w, h, nfeat, sf, nl = g
    (W, Hh, n_ini, D, cells, N), bins = hook(w, h, nfeat, sf, nl, level)
    assert n_ini == int(np.floor(F32(W) / F32(Hh) + F32(0.5))) and 1 <= n_ini <= 16     # roundf of a positive value
    assert D == tab_depth(n_ini, N) and cells == n_ini << (2 * D) and cells <= 4096
    assert len(bins) == W + 1 + Hh + 1
    xs, ys = restated(W, Hh, n_ini, D)
    assert np.array_equal(bins[:W + 1], xs), np.nonzero(bins[:W + 1] != xs)[0][:8]
    assert np.array_equal(bins[W + 1:], ys), np.nonzero(bins[W + 1:] != ys)[0][:8]
    # the two halves never share a bit, and every cell index lies inside the level's tables
    assert not (int(np.bitwise_or.reduce(xs)) & int(np.bitwise_or.reduce(ys)) & ((1 << (2 * D)) - 1))
    assert int(xs.max()) | int(ys.max()) < cells
    # the paths are monotone in the coordinate: the cells of a level tile its area in order
    assert np.all(np.diff(xs.astype(np.int32)) >= 0)


def test_more_than_one_root():
    (W, Hh, n_ini, D, cells, _), bins = hook(1118, 112, 500, 1.2, 1, 0)
    assert n_ini == 14 and D == 4 and cells == 14 * 256
    roots = bins[:W] >> (2 * D)
    assert roots[0] == 0 and roots[-1] == n_ini - 1 and len(np.unique(roots)) == n_ini


def test_hook_refuses_bad_arguments():
    info = np.zeros(6, np.int32)
    n = capi.C.c_int32(0)
    assert H.rumi_hook_octree_bins(640, 480, 1000, F32(1.2), 8, 8, capi.ptr(info), None, 0, capi.C.byref(n)) == capi.RUMI_E_INVALID
    assert H.rumi_hook_octree_bins(640, 480, 1000, F32(1.2), 8, 0, capi.ptr(info), None, 0, capi.C.byref(n)) == capi.RUMI_E_CAPACITY
    assert n.value == (640 - 32) + 1 + (480 - 32) + 1


def hist_lds(w, h, nfeat, sf, nl):
    info = np.zeros(4, np.int32)
    assert H.rumi_hook_compact_hist_lds(w, h, nfeat, F32(sf), nl, capi.ptr(info)) == capi.RUMI_OK
    return [int(v) for v in info]


# the bench geometry; the large ones whose table would push k_compact past 64 KiB of LDS (prefix 34 336 B + table 32 768 B at 2560 x 1440 with 5000
# features); a large frame with few features, whose table still fits
LDS_GEOMETRIES = [(640, 480, 1000, 1.2, 8), (2560, 1440, 5000, 1.2, 8), (2560, 1440, 4000, 1.2, 8), (3000, 1500, 4000, 1.2, 8),
                  (2560, 1440, 1000, 1.2, 8), (1118, 112, 500, 1.2, 1)]


@pytest.mark.parametrize("g", LDS_GEOMETRIES, ids=["%dx%d-n%d" % g[:3] for g in LDS_GEOMETRIES])
def test_compact_lds_sizing_rule(g):
    """k_compact's count table is taken only when prefix + table + static LDS stays within the 64 KiB a launch gets without an opt-in; otherwise
    the geometry has no pipeline (table 0) and the launch needs the prefix alone, as before."""
    w, h, nfeat, sf, nl = g
    cells, row, table, static = hist_lds(w, h, nfeat, sf, nl)
    assert row == sum((hook(w, h, nfeat, sf, nl, l)[0][4] + 1) & ~1 for l in range(nl)) and row % 2 == 0
    assert static >= 1024 + 16 * 4 + 16 * 16                      # part[256], sLevCell[16], sLev[16] of the kernel
    fits = (cells + 1) * 4 + 2 * row + static <= 64 * 1024
    assert table == (2 * row if fits else 0)
    assert (cells + 1) * 4 + table + static <= 64 * 1024 or table == 0


def test_compact_lds_known_geometries():
    assert hist_lds(640, 480, 1000, 1.2, 8)[2] == 4096             # eight levels of 256 cells, 16 bits each
    cells, row, table, _ = hist_lds(2560, 1440, 5000, 1.2, 8)
    assert ((cells + 1) * 4, 2 * row, table) == (34336, 32768, 0)
    assert hist_lds(2560, 1440, 4000, 1.2, 8)[2] == 0 and hist_lds(3000, 1500, 4000, 1.2, 8)[2] == 0
    assert hist_lds(2560, 1440, 1000, 1.2, 8)[2] > 0
