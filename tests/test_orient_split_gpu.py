"""Batches take IC_Angle and the trigonometry in k_disc_angle and rBRIEF in the descriptor-only form of k_orient_desc (csrc/orb_orient_desc.inc;
the rule is orient_desc_split, csrc/orb_device.h: ceil(capSel / 8) * frames > 2048 workgroups).  Every call here is 16 frames of an extractor with
nfeatures = 1000, which is on the batch side of that rule (asserted), and every result is held bit for bit to the CPU oracle built with the same
constructor: records, descriptors, counts, monoIndex.

  * the constructed frames of families C, D and E of extract_cases.py (moments / atan2, the un-blurred level, keys 19 px from the edges, the flat
    field, random texture, several levels, the lapping rule), which with their own nfeatures only ever reach the fused small-call kernel;
  * a ragged batch: an empty frame in the middle, counts that differ and are no multiples of 64 (k_disc_angle's workgroups take 16 key-points,
    the descriptor kernel's 16 as well: all but one count end inside a workgroup), through both output forms and with an output capacity below
    the largest count;
  * level 0 at a pitch and a frame stride of its own;
  * two back-to-back rounds of resident-queue calls on two slots against the blocking calls: a slot's angle array is reused in stream order."""
import numpy as np
import pytest

import extract_cases as EC
import oracle_lib as O

FRAMES, NFEAT = 16, 1000
_orc = {}


def cap_sel(nlevels):
    return NFEAT + 4 * nlevels + 64


def assert_batch_path(nlevels, frames=FRAMES):
    assert -(-cap_sel(nlevels) // 8) * frames > 2048, "the call would take the fused kernel"


def oracle(frame, ctor, lap):
    key = (frame.tobytes(), frame.shape, ctor, lap)
    if key not in _orc:
        _orc[key] = O.OracleExtractor(*ctor).extract(frame, lap)
    return _orc[key]


def extractor(ctor, w, h, batch=FRAMES):
    from rumi_slam_amd.extractor import ORBextractor
    return ORBextractor(*ctor, max_width=w, max_height=h, max_batch=batch)


def hold(tag, kp, desc, counts, frames, ctor, lap, cap=None):
    """kp / desc / counts: numpy copies of a call's outputs.  With cap: slots at and past it are dropped, nothing else moves."""
    for f, frame in enumerate(frames):
        mono, okps, odesc = oracle(frame, ctor, lap)
        n = len(okps)
        assert (int(counts[f, 0]), int(counts[f, 1])) == (n, mono), f"{tag}, frame {f}: counts {counts[f]} against {(n, mono)}"
        m = n if cap is None else min(n, cap)
        got = kp[f, :m].copy().view(O.KP_DTYPE).reshape(-1)
        assert got.tobytes() == okps[:m].tobytes(), f"{tag}, frame {f}: records differ from the oracle"
        assert np.array_equal(desc[f, :m], odesc[:m]), f"{tag}, frame {f}: descriptors differ from the oracle"


def run_batch(ext, frames, lap, cap=None, records=False):
    import torch
    from rumi_slam_amd import rumination
    dev = torch.from_numpy(np.stack(frames)).cuda() if isinstance(frames, list) else frames
    if records:
        c = cap or cap_sel(ext.nlevels)
        kp, desc, counts = rumination.record_views(ext.extract_batch_records(dev, lap, cap=cap), c)
    else:
        kp, desc, counts = ext.extract_batch(dev, lap, cap=cap)
    return kp.cpu().numpy(), desc.cpu().numpy(), counts.cpu().numpy()


# ---- the constructed cases, grouped by frame size and pyramid rule, stacked to 16 with flipped copies ----
CASES = [c for c in EC.all_cases() if c.family in "CDE"]
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault((_c.frame.shape, _c.ctor[1:], _c.lap), []).append(_c)
GROUP_IDS = ["%dx%d-sf%g-l%d-lap%d-%d" % (k[0][1], k[0][0], k[1][0], k[1][1], k[2][0], k[2][1]) for k in GROUPS]


def test_groups_cover_the_named_cases():
    names = {c.name for c in CASES}
    assert {"unblurred", "edge-19", "flat-dot", "blur-random", "half-right", "umax-v15-in", "lap-100-200", "lap-0-0", "texture-3-levels"} <= names


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
def test_constructed_cases_on_the_batch_path(key):
    cases = GROUPS[key]
    (h, w), rest, lap = key
    ctor = (NFEAT,) + rest
    assert_batch_path(ctor[2])
    flips = (lambda f: f, lambda f: f[::-1], lambda f: f[:, ::-1], lambda f: f[::-1, ::-1])
    ext = extractor(ctor, w, h)
    for start in range(0, len(cases), FRAMES):
        chunk = [c.frame for c in cases[start:start + FRAMES]]
        base = list(chunk)
        for i in range(FRAMES - len(chunk)):                                 # fillers: flipped copies, cycling through the chunk's frames
            chunk.append(np.ascontiguousarray(flips[1 + (i // len(base)) % 3](base[i % len(base)])))
        chunk = chunk[1::2] + chunk[0::2]                                    # cases and fillers interleaved
        hold(f"{GROUP_IDS[list(GROUPS).index(key)]} from {start}", *run_batch(ext, chunk, lap), chunk, ctor, lap)


# ---- ragged batch ----
RAGGED_CTOR, RAGGED_LAP, RW, RH = (NFEAT, 1.2, 4, 20, 7), (60, 140), 200, 150


def ragged_frames():
    from rumi_slam_amd.synth import synth_frame
    # different seeds and amounts of texture: counts from a few dozen to several hundred
    frames = [synth_frame(4000 + i, w=RW, h=RH, n_rect=(12, 40, 90, 160)[i % 4] + 3 * i) for i in range(FRAMES)]
    frames[7] = np.full((RH, RW), 90, np.uint8)                              # featureless: count 0
    return frames


@pytest.fixture(scope="module")
def ragged():
    frames = ragged_frames()
    counts = [len(oracle(f, RAGGED_CTOR, RAGGED_LAP)[1]) for f in frames]
    assert counts[7] == 0 and len(set(counts)) >= 12 and all(n % 64 for n in counts if n), counts
    assert max(counts) > 128, counts                                         # many workgroups per frame
    return frames, counts, extractor(RAGGED_CTOR, RW, RH)


@pytest.mark.gpu
@pytest.mark.parametrize("records", [False, True], ids=["three-arrays", "records"])
def test_ragged_batch(ragged, records):
    frames, _, ext = ragged
    assert_batch_path(RAGGED_CTOR[2])
    hold("ragged", *run_batch(ext, frames, RAGGED_LAP, records=records), frames, RAGGED_CTOR, RAGGED_LAP)


@pytest.mark.gpu
def test_ragged_batch_with_a_small_output_capacity(ragged):
    frames, counts, ext = ragged
    cap = 800                                                                # some frames fit, most have slots at and past it
    assert sum(0 < n <= cap for n in counts) >= 3 and sum(n > cap for n in counts) >= 3 and cap % 64
    hold(f"ragged, cap {cap}", *run_batch(ext, frames, RAGGED_LAP, cap=cap), frames, RAGGED_CTOR, RAGGED_LAP, cap=cap)


@pytest.mark.gpu
def test_level0_at_a_pitch_of_its_own(ragged):
    import torch
    frames, _, ext = ragged
    pitch, rows = RW + 24, RH + 3                                            # pitch > width, frame stride (RH + 3) * pitch: not the packed one
    block = torch.full((FRAMES, rows, pitch), 255, dtype=torch.uint8)
    block[:, :RH, :RW] = torch.from_numpy(np.stack(frames))
    view = block.cuda()[:, :RH, :RW]
    assert view.stride(1) == pitch and view.stride(0) == rows * pitch and not view.is_contiguous()
    hold("strided level 0", *run_batch(ext, view, RAGGED_LAP), frames, RAGGED_CTOR, RAGGED_LAP)


@pytest.mark.gpu
def test_resident_queue_reuses_a_slot(ragged):
    """Two different 16-frame calls back to back, twice over, on a resident queue of two slots: calls 3 and 4 reuse the slots (and their angle
    arrays) of calls 1 and 2 in stream order, with no synchronisation in between.  Every call must equal the blocking call's result."""
    import torch
    frames, _, _ = ragged
    other = [np.ascontiguousarray(f[::-1, ::-1]) for f in frames[::-1]]
    ext = extractor(RAGGED_CTOR, RW, RH)
    batches = [torch.from_numpy(np.stack(b)).cuda() for b in (frames, other)]
    ref = [tuple(t.cpu().numpy() for t in ext.extract_batch(b, RAGGED_LAP)) for b in batches]
    hold("blocking call", *ref[0], frames, RAGGED_CTOR, RAGGED_LAP)
    hold("blocking call, second batch", *ref[1], other, RAGGED_CTOR, RAGGED_LAP)
    ext.set_resident_queue(2)
    cap = cap_sel(RAGGED_CTOR[2])
    outs = [(torch.zeros((FRAMES, cap, 7), dtype=torch.float32, device="cuda"), torch.zeros((FRAMES, cap, 32), dtype=torch.uint8, device="cuda"),
             torch.zeros((FRAMES, 2), dtype=torch.int32, device="cuda")) for _ in range(4)]
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        ext.extract_batch(batches[i % 2], RAGGED_LAP, wait=False, out=o)
    ext.sync()
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        kp, desc, counts = (t.cpu().numpy() for t in o)
        rk, rd, rc = ref[i % 2]
        assert np.array_equal(counts, rc), f"resident call {i}: counts"
        for f in range(FRAMES):
            n = rc[f, 0]
            assert kp[f, :n].tobytes() == rk[f, :n].tobytes() and np.array_equal(desc[f, :n], rd[f, :n]), f"resident call {i}, frame {f}"
