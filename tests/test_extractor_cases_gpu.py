"""The extractor kernels against the constructed cases of extract_cases.py (and against the oracle), through the stage taps and the final
records.  Which kernels a call launches depends on the geometry and on the number of frames (csrc/orb_schedule.inc):

  * FAST and blur: geometries whose widest cell is 37..40 px (tile pitch 48, as at 640 x 480) run the fused k_fast_blur in calls of fewer than 16
    frames and k_fast_cells<48> + the blur kernel from 16 frames on.  Families A, C, most of D and the 181 / 183 px wide B cases are on such
    geometries (FUSED below, asserted).  The others (160 x 160, 282 x 132, 320 x 240, 128 x 96, 1118 x 112, family E) run k_fast_cells of their own
    pitch + the blur kernel at every batch size.
  * the final assembly is fused into the descriptor launch in calls of up to 4 frames, a launch of its own from 5 on.
  * the pyramid (family E only: every other case has one level) is one launch up to 4 frames and one launch per level from 5 on.
  * the quadtree keeps its keys in registers in all of these; test_keys_in_memory_quadtree starts a child process in which RUMI_OCT_REGS=0 selects
    the keys-in-memory kernels: 256 threads up to 260 features on level 0, 512 threads above.

Every case runs alone (one-frame call) and inside batches of 3, 5 and 16.  A batch stacks the DIFFERENT cases of one geometry, each held to its own
expectation; where a geometry has fewer cases than the batch has frames, the rest are flipped copies of them held to the oracle, so every batch
mixes different frames and a leak between frames shows."""
import os
import subprocess
import sys

import numpy as np
import pytest

import extract_cases as EC
import oracle_lib as O
from rumi_slam_amd import capi

PRIMS = EC.Prims(O, capi.hooks())
PAT = EC.pattern()
CASES = EC.all_cases() + EC.big_octree_cases(PRIMS.std_sort)
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault(_c.geometry + _c.lap, []).append(_c)
GROUP_IDS = ["%dx%d-n%d-sf%g-l%d-lap%d-%d" % (k[0], k[1], k[2], k[3], k[4], k[7], k[8]) for k in GROUPS]
MAX_BATCH = 16
_ext, _orc = {}, {}


def fused(c):
    """True when the geometry's widest cell gives the tile pitch 48 that k_fast_blur is instantiated for (fast_lds_of, csrc/orb_fast.inc)."""
    h, w = c.frame.shape
    inv = [np.float32(1.0) / s for s in EC.scale_table(c.ctor[1], c.ctor[2])]
    wmax = max(EC.grid(int(np.rint(np.float32(w) * i)), int(np.rint(np.float32(h) * i)))[2] for i in inv)
    return 37 <= wmax <= 40


def extractor(c):
    from rumi_slam_amd.extractor import ORBextractor
    if c.geometry not in _ext:
        h, w = c.frame.shape
        _ext[c.geometry] = ORBextractor(*c.ctor, max_width=w, max_height=h, max_batch=MAX_BATCH)
    return _ext[c.geometry]


def oracle_of(key, frame, ctor, lap):
    if key not in _orc:
        o = O.OracleExtractor(*ctor)
        mono, kps, desc = o.extract(frame, lap)
        _orc[key] = (mono, kps, desc, [o.keypoints(l, False) for l in range(ctor[2])], [o.keypoints(l, True) for l in range(ctor[2])])
    return _orc[key]


def taps(ext, frame):
    return (lambda l: ext.stage_keypoints(l, 0, frame=frame), lambda l: ext.stage_keypoints(l, 1, frame=frame),
            lambda l, blurred=False: ext.pyramid_level(l, frame=frame, blurred=blurred))


def hold_to_oracle(tag, res, orc, nl):
    mono, kps, desc, cand, sel = orc
    assert res.mono == mono and res.kps.tobytes() == kps.tobytes() and np.array_equal(res.desc, desc), f"{tag} differs from the oracle"
    for l in range(nl):
        assert res.cand(l).tobytes() == cand[l].tobytes() and res.sel(l).tobytes() == sel[l].tobytes(), f"{tag}, taps of level {l} differ from the oracle"


def hold(c, res, who):
    EC.check(c, res, who, PRIMS, PAT)
    hold_to_oracle(f"{c.id}: {who}", res, oracle_of(c.id, c.frame, c.ctor, c.lap), c.ctor[2])


def test_fused_geometries():
    """The families whose rules live in the FAST kernel are on geometries that take the fused FAST + blur launch."""
    names = {c.id for c in CASES if fused(c)}
    for c in CASES:
        if c.family in "AC" and c.name != "skip-column" or c.name in ("flat-dot", "edge-19", "blur-random", "half-x", "half-y", "float-root", "nini-1.51"):
            assert c.id in names, c.id
    assert not any(fused(c) for c in CASES if c.family == "E" or c.frame.shape == (160, 160))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_one_frame_call(c):
    ext = extractor(c)
    mono, kps, desc = ext(c.frame, None, c.lap)
    hold(c, EC.Result(mono, kps, desc, *taps(ext, 0)), "one-frame call")


def _fillers(cases, n):
    """n frames that differ from every case of the group and from each other where they can: flips of the cases' frames."""
    flips = (lambda f: f[::-1], lambda f: f[:, ::-1], lambda f: f[::-1, ::-1])
    out = []
    for i in range(n):
        c = cases[(i // 3) % len(cases)]
        out.append((f"{c.id}-flip{i % 3}", np.ascontiguousarray(flips[i % 3](c.frame))))
    return out


def run_batches(cases, B, who):
    import torch
    ext = extractor(cases[0])
    ctor, lap = cases[0].ctor, cases[0].lap
    for start in range(0, len(cases), B):
        chunk = [(c.id, c.frame, c) for c in cases[start:start + B]]
        chunk += [(k, f, None) for k, f in _fillers(cases, B - len(chunk))]
        chunk = chunk[1::2] + chunk[0::2]                                        # cases and fillers interleaved, not in blocks
        kp, desc, counts = ext.extract_batch(torch.from_numpy(np.stack([f for _, f, _ in chunk])).cuda(), lap)
        kp, desc, counts = kp.cpu().numpy(), desc.cpu().numpy(), counts.cpu().numpy()
        for i, (key, frame, c) in enumerate(chunk):
            n = int(counts[i, 0])
            res = EC.Result(int(counts[i, 1]), kp[i, :n].copy().view(O.KP_DTYPE).reshape(-1), desc[i, :n].copy(), *taps(ext, i))
            if c is not None:
                hold(c, res, f"{who}, frame {i}")
            else:
                hold_to_oracle(f"{key}: {who}, frame {i}", res, oracle_of((key,) + ctor + lap, frame, ctor, lap), ctor[2])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 5, MAX_BATCH])
@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
def test_batches_of_stacked_cases(key, B):
    run_batches(GROUPS[key], B, f"batch of {B}")


@pytest.mark.gpu
def test_keys_in_memory_quadtree():
    """The B cases on the keys-in-memory quadtree kernels.  launch_octree reads RUMI_OCT_REGS once per process, so this starts one child process
    with RUMI_OCT_REGS=0 that runs every B geometry in batches of 5: the hand-written cases and the 64-dot lattices at their own N (256 threads), the
    400-dot lattices with N = 280 and 340 (512 threads: more than 260 features on level 0), each held to its expectation and to the oracle."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RUMI_OCT_REGS="0", PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "keys-in-memory ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _child():
    assert os.environ.get("RUMI_OCT_REGS") == "0"
    n256 = n512 = 0
    for key, cases in GROUPS.items():
        bs = [c for c in cases if c.family == "B"]
        if not bs:
            continue
        run_batches(bs, 5, "keys in memory, batch of 5")
        n256 += len(bs) * (key[2] <= 260)
        n512 += len(bs) * (key[2] > 260)
    assert n256 >= 17 and n512 >= 2
    print(f"keys-in-memory ok: {n256} cases at 256 threads, {n512} at 512")


if __name__ == "__main__":
    _child()
