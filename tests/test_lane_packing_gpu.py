"""Batch pyramid and blur with the frames of a launch laid side by side (LanePack, orb_geom.h), bit for bit against the CPU oracle: every level,
un-blurred and blurred, of EVERY frame of batches whose frame count leaves full and partial groups, on an image size whose level widths cover
every w mod 4 and lie on both sides of one wave's 256 pixels.  The frames differ strongly at their edges, so a byte that leaks across a frame
seam, or a lane that reads its neighbour frame, changes a result."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib
from rumi_slam_amd import capi

pytestmark = pytest.mark.gpu

NLEVELS, SCALE, H = 4, 1.2, 240          # level heights 240, 200, 167, 139: k_resize<8> (h >= 200) and k_resize<4>, four 64-row blur walks


def level_widths(w):
    """the project's own level rule, through the geometry hook"""
    Hk = capi.hooks()
    out = []
    for l in range(NLEVELS):
        info, n = np.zeros(8, np.int32), C.c_int32()
        rc = Hk.rumi_hook_lane_packing(w, H, SCALE, NLEVELS, 16, 1, l, 0, capi.ptr(info), None, 0, C.byref(n))
        assert rc in (0, capi.RUMI_E_CAPACITY)
        out.append(int(info[0]))
    return out


@functools.lru_cache(None)
def pick_width():
    for w in range(280, 400):
        ws = level_widths(w)
        if {x % 4 for x in ws} == {0, 1, 2, 3} and min(ws) < 256 < max(ws):
            return w, ws
    raise AssertionError("no candidate width")



def make_frames(n, seed):
    """a seeded texture plus a per-frame offset, the four border columns / rows of every frame inverted: neighbouring frames share no edge bytes"""
    W = pick_width()[0]
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, W), dtype=np.uint8)
    base[40:90, 60:140] = np.kron(rng.integers(0, 2, (10, 16), dtype=np.uint8) * 200 + 20, np.ones((5, 5), np.uint8))     # corners for FAST
    frames = np.empty((n, H, W), np.uint8)
    for f in range(n):
        fr = (base.astype(np.int32) + 37 * f + (f % 3) * np.arange(W)[None, :]).astype(np.uint8)
        edge = np.ones((H, W), bool)
        edge[4:-4, 4:-4] = False
        fr[edge] = 255 - fr[edge] if f % 2 else (fr[edge] // 2 + 11 * f).astype(np.uint8)
        frames[f] = fr
    return frames


def extractor(batch, blur_variant=0):
    from rumi_slam_amd.extractor import ORBextractor
    W = pick_width()[0]
    return ORBextractor(500, SCALE, NLEVELS, 20, 7, max_width=W, max_height=H, max_batch=batch, blur_variant=blur_variant)


def test_widths_cover_every_case():
    WIDTHS = pick_width()[1]
    assert {x % 4 for x in WIDTHS} == {0, 1, 2, 3}, WIDTHS
    assert min(WIDTHS) < 256 < max(WIDTHS), WIDTHS


@pytest.mark.parametrize("blur_variant", [0, 1])
@pytest.mark.parametrize("nframes", [16, 17, 19])
def test_every_level_of_every_frame_bit_exact(nframes, blur_variant):
    """16: the batch blur's threshold (and the packed resize's); 17 and 19 leave a partial last group."""
    import torch
    frames = make_frames(nframes, 100 + nframes)
    g = extractor(nframes, blur_variant)
    o = oracle_lib.OracleExtractor(500, SCALE, NLEVELS, 20, 7, blur_variant=blur_variant)
    g.extract_batch(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    for f in range(nframes):
        o.extract(frames[f], (0, 1000))
        for l in range(NLEVELS):
            a, b = g.pyramid_level(l, frame=f), o.level(l)
            assert a.shape == b.shape and np.array_equal(a, b), f"frame {f} level {l}: {np.count_nonzero(a != b)} pixels differ, first at {np.argwhere(a != b)[:3].tolist()}"
            a, b = g.pyramid_level(l, frame=f, blurred=True), o.level(l, blurred=True)
            assert np.array_equal(a, b), f"frame {f} blurred level {l}: {np.count_nonzero(a != b)} pixels differ, first at {np.argwhere(a != b)[:3].tolist()}"


def test_resident_queue_and_host_batch_match_the_blocking_call():
    """20 frames through the resident queue and through rumi_orb_extract_batch_host: key-points and descriptors of the blocking device call."""
    import torch
    n = 20
    frames = make_frames(n, 77)
    dev = torch.from_numpy(frames).cuda()
    g = extractor(n)
    kp, desc, counts = (t.cpu().numpy() for t in g.extract_batch(dev))
    assert counts[:, 0].min() > 0, "the frames carry key-points"
    cap = kp.shape[1]

    def same(k2, d2, c2, tag):
        assert np.array_equal(c2, counts), f"{tag}: counts"
        for f in range(n):
            m = counts[f, 0]
            assert k2[f, :m].tobytes() == kp[f, :m].tobytes(), f"{tag} frame {f}: key-points"
            assert np.array_equal(d2[f, :m], desc[f, :m]), f"{tag} frame {f}: descriptors"

    (hk, hd, hc) = g.extract_batch_host([frames[f] for f in range(n)])
    torch.cuda.synchronize()
    same(hk.cpu().numpy(), hd.cpu().numpy(), hc.cpu().numpy(), "host batch")

    out = (torch.zeros((n, cap, 7), dtype=torch.float32, device="cuda"), torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda"),
           torch.zeros((n, 2), dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    g.set_resident_queue(True)
    g.extract_batch(dev, wait=False, out=out)
    g.sync()
    torch.cuda.synchronize()
    g.set_resident_queue(False)
    same(out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy(), "resident queue")
