"""k_fast_cells' byte quick test (fast_score_cell_bytes, eight pixels a lane) against the CPU oracle: candidate lists per level,
key-points, descriptors.  Frames made to hit the edges of the byte arithmetic: centres
near 0 and 255 (v +- T saturates), circle contrasts of exactly T and T + 1 (strict inequalities), dense noise, a ramp on which nearly
every pixel passes the quick test in BOTH polarities (a 64-item step then appends more entries than the ring holds: the two-halves
append; tests/test_fast_bytes_cpu.py counts on the CPU that its steps exceed the ring), featureless and saturated frames; thresholds (1, 1), (20, 7),
(254, 1); 640 x 480 (cell widths 26-40, most not multiples of 8; one-frame calls and batches of fewer than 16 frames take the fused
FAST + blur launch k_fast_blur, batches of 16 and more k_fast_cells) and 320 x 240 (tile pitch 68: the run-time-pitch instantiation)."""
import numpy as np
import pytest

import oracle_lib
from rumi_slam_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

THRESHOLDS = [(1, 1), (20, 7), (254, 1)]
KINDS = ["saturating", "contrast_t", "noise", "ramp", "synth", "flat", "white", "black"]
RING_CAP = 640                        # kRingCap of orb_fast.inc: entries the linear ring holds


def make_frame(kind, w=640, h=480, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "saturating":          # centres near 0 and 255 next to every contrast that matters for T = 1, 7, 20
        vals = np.array([0, 1, 2, 3, 7, 8, 9, 20, 21, 22, 233, 234, 235, 246, 247, 248, 252, 253, 254, 255], np.uint8)
        img = vals[rng.integers(0, len(vals), (h // 2 + 1, w // 2 + 1))].repeat(2, 0).repeat(2, 1)[:h, :w]
    elif kind == "contrast_t":        # contrasts of exactly T and T + 1 around a grey centre (T = 1, 7, 20), in 1- and 3-pixel blobs
        vals = np.array([100, 99, 101, 98, 102, 93, 107, 92, 108, 80, 120, 79, 121], np.uint8)
        img = np.full((h, w), 100, np.uint8)
        small = vals[rng.integers(0, len(vals), (h // 3 + 1, w // 3 + 1))].repeat(3, 0).repeat(3, 1)[:h, :w]
        pts = rng.random((h, w)) < 0.3
        img[pts] = vals[rng.integers(0, len(vals), int(pts.sum()))]
        img = np.where(rng.random((h, w)) < 0.5, img, small).astype(np.uint8)
    elif kind == "noise":             # uniform noise: about a third of the pixels pass the quick test at T = 1
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif kind == "ramp":              # 2 x + y (mod 256): at T = 1 the four even circle positions right / below are brighter and the four left /
        y, x = np.mgrid[0:h, 0:w]     # above darker, so a pixel passes in both polarities; bright dots every 9 pixels make real corners
        img = ((2 * x + y) % 256).astype(np.uint8)
        dots = ((y % 9) == 3) & ((x % 9) == 4)
        img[dots] = ((img[dots].astype(np.int32) + 128) % 256).astype(np.uint8)
    elif kind == "synth":
        img = synth_frame(1234 + seed)
        if img.shape != (h, w):
            img = np.ascontiguousarray(img[:h, :w])
    elif kind == "flat":
        img = np.full((h, w), 128, np.uint8)
    elif kind == "white":
        img = np.full((h, w), 255, np.uint8)
    elif kind == "black":
        img = np.zeros((h, w), np.uint8)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(img)


def _extractors(ini, mn, w=640, h=480, batch=1):
    from rumi_slam_amd.extractor import ORBextractor
    return ORBextractor(1000, 1.2, 8, ini, mn, max_width=w, max_height=h, max_batch=batch), oracle_lib.OracleExtractor(1000, 1.2, 8, ini, mn)


def _same(got, ref, tag):
    gm, gk, gd = got
    om, ok, od = ref
    assert len(gk) == len(ok), f"{tag}: key-point count {len(gk)} vs oracle {len(ok)}"
    assert gm == om, f"{tag}: monoIndex {gm} vs {om}"
    assert gk.tobytes() == ok.tobytes(), f"{tag}: key-point records differ"
    assert np.array_equal(gd, od), f"{tag}: descriptors differ"


def _single(ini, mn, kind, w, h):
    g, o = _extractors(ini, mn, w, h)
    img = make_frame(kind, w, h, seed=ini)
    _same(g(img, None, (0, 1000)), o.extract(img, (0, 1000)), f"{kind} {w}x{h} th ({ini}, {mn})")
    for l in range(8):
        gc, oc = g.stage_keypoints(l, 0), o.keypoints(l, False)
        assert gc.tobytes() == oc.tobytes(), f"{kind} {w}x{h} th ({ini}, {mn}): candidate list of level {l} ({len(gc)} vs {len(oc)})"


@pytest.mark.parametrize("ini,mn", THRESHOLDS)
@pytest.mark.parametrize("kind", KINDS)
def test_one_frame_vs_oracle(kind, ini, mn):
    """One-frame calls at 640 x 480: the fused FAST + blur launch (k_fast_blur)."""
    _single(ini, mn, kind, 640, 480)


@pytest.mark.parametrize("ini,mn", THRESHOLDS)
@pytest.mark.parametrize("kind", KINDS)
def test_runtime_pitch_vs_oracle(kind, ini, mn):
    """320 x 240: the largest cell is 57 pixels wide, tile pitch 68, not one of the compile-time pitches."""
    _single(ini, mn, kind, 320, 240)


def _batch_outputs(ini, mn, kinds, w=640, h=480):
    import torch
    g, o = _extractors(ini, mn, w, h, batch=len(kinds))
    frames = np.stack([make_frame(k, w, h, seed=i) for i, k in enumerate(kinds)])
    kp, desc, counts = g.extract_batch(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    kp, desc, counts = kp.cpu().numpy(), desc.cpu().numpy(), counts.cpu().numpy()
    out = []
    for f in range(len(kinds)):
        n = counts[f, 0]
        out.append((int(counts[f, 1]), kp[f, :n].copy().view(oracle_lib.KP_DTYPE).reshape(-1), desc[f, :n].copy()))
    return frames, out, o


BATCH_KINDS = KINDS + KINDS           # 16 frames: the batched launch k_fast_cells<48> (fewer than 16 take the fused FAST + blur launch)


@pytest.mark.parametrize("ini,mn", THRESHOLDS)
def test_batch_vs_oracle(ini, mn):
    """A batch of 16 frames (k_fast_cells<48>), every kind of frame twice."""
    frames, out, o = _batch_outputs(ini, mn, BATCH_KINDS)
    for f, kind in enumerate(BATCH_KINDS):
        _same(out[f], o.extract(frames[f], (0, 1000)), f"batch frame {f} ({kind}) th ({ini}, {mn})")


# ---- the two-halves ring append ------------------------------------------------------------------------------------------------------
EVEN = [(0, 3), (2, 2), (3, 0), (2, -2), (0, -3), (-2, -2), (-3, 0), (-2, 2)]      # (dx, dy) of the even circle positions, circular order


def quick_entries(img, T):
    """ring entries per pixel of the quick test (0, 1 or 2: brighter and darker are separate entries), restated from cv::FAST's strict
    tests: 4 consecutive of the 8 even positions with p > v + T (brighter) / p < v - T (darker)"""
    h, w = img.shape
    v = img.astype(np.int32)
    pad = np.pad(v, 3, mode="edge")
    ring = [pad[3 + dy:3 + dy + h, 3 + dx:3 + dx + w] for dx, dy in EVEN]

    def four(f):
        return np.logical_or.reduce([f[k] & f[(k + 1) % 8] & f[(k + 2) % 8] & f[(k + 3) % 8] for k in range(8)])
    return four([p > v + T for p in ring]).astype(np.int32) + four([p < v - T for p in ring])


def level0_step_entries(img, T):
    """entries each 64-item step of k_fast_cells appends on level 0 (an item = 8 pixels of a row of the cell's detection region, items
    row-major; the cell grid of ORBextractor::ComputeKeyPointsOctTree, W = 35, as the kernel restates it)"""
    e = quick_entries(img, T)
    h, w = img.shape
    minB, maxBX, maxBY = 16, w - 16, h - 16
    nCols, nRows = (maxBX - minB) // 35, (maxBY - minB) // 35
    wCell, hCell = -(-(maxBX - minB) // nCols), -(-(maxBY - minB) // nRows)
    steps = []
    for i in range(nRows):
        iniY = minB + i * hCell
        maxY = min(iniY + hCell + 6, maxBY)
        for j in range(nCols):
            iniX = minB + j * wCell
            maxX = min(iniX + wCell + 6, maxBX)
            if iniY >= maxBY - 3 or iniX >= maxBX - 6 or maxX - iniX < 7 or maxY - iniY < 7:
                continue
            dw, dh = maxX - iniX - 6, maxY - iniY - 6
            ng = -(-dw // 8)
            items = np.zeros((dh, 8 * ng), np.int32)
            items[:, :dw] = e[iniY + 3:iniY + 3 + dh, iniX + 3:iniX + 3 + dw]
            items = items.reshape(dh * ng, 8).sum(1)
            steps += [int(items[s:s + 64].sum()) for s in range(0, len(items), 64)]
    return np.array(steps)


def test_split_append_vs_oracle():
    """GPU: the ramp frame at thresholds (1, 1) through a one-frame call (k_fast_blur) and a 16-frame batch (k_fast_cells): candidate
    lists of every level, key-points and descriptors bit-exact against the oracle; the dots make thousands of level-0 candidates, so an
    entry lost or misplaced by the split append shows."""
    assert (level0_step_entries(make_frame("ramp"), 1) > RING_CAP).any()
    _single(1, 1, "ramp", 640, 480)
    _, o = _extractors(1, 1)
    o.extract(make_frame("ramp"), (0, 1000))
    assert len(o.keypoints(0, False)) > 1000
    frames, out, o = _batch_outputs(1, 1, ["ramp"] * 16)
    for f in range(16):
        _same(out[f], o.extract(frames[f], (0, 1000)), f"ramp batch frame {f}")

