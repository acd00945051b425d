"""The resident queue over the streams its plan drives (orb_geom.h: stream_plan): with four hardware queues a slot has ONE stream, the blur runs
in line behind the pyramid, and a call may put consecutive sub-chunks on one stream.  Whatever the plan, every frame of every call must come
out as the blocking call gives it.

One handle for all cases (320 x 240, eight levels, max_batch 520); frames as bench.py makes them: 32 seeded synthetic images and cyclic
shifts of them on the device.  Call sizes: 1; 15 / 16 / 17 around kPackMinFrames (fused FAST + blur launch below, packed blur from 16 on);
64; 260 = two sub-chunks; 520 = three sub-chunks, so with two or three driven streams one stream carries two sub-chunks of a call back to
back (the in-line arena hazards: blur after the previous k_orient_desc, pyramid after the previous k_disc_angle / k_fast_cells)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, NF, NL, B = 320, 240, 500, 8, 520
CAP = NF + 4 * NL + 64
SIZES = [1, 15, 16, 17, 64, 260, 520]
OFFSETS = [7, 33, 101, 250, 300, 130, 0]          # where each call's frames start in the pool (the 520-frame call is the whole pool)


def _pool(torch):
    from rumi_slam_amd.synth import synth_frame
    base = torch.from_numpy(np.stack([synth_frame(4200 + i, w=W, h=H, n_rect=120) for i in range(32)])).cuda()
    fr = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    for k in range(B):
        fr[k] = torch.roll(base[k % 32], shifts=(7 * (k // 32), 11 * (k // 32)), dims=(0, 1)) if k >= 32 else base[k]
    return fr


def _host(out):
    kp, desc, counts = out
    return kp.cpu().numpy().view(np.uint8).reshape(kp.shape[0], CAP, 28), desc.cpu().numpy(), counts.cpu().numpy()


def _assert_frames_equal(got, ref, what):
    k, d, c = _host(got)
    rk, rd, rc = ref
    assert np.array_equal(c, rc), f"{what}: counts"
    valid = np.arange(CAP)[None, :] < rc[:, 0:1]
    bad = np.nonzero(((k != rk).any(axis=2) | (d != rd).any(axis=2)) & valid)
    assert bad[0].size == 0, f"{what}: frame {bad[0][0]} slot {bad[1][0]} differs"


@pytest.fixture(scope="module")
def rig():
    """The handle, the frame pool and the blocking call's answer for every frame of it (computed once, before the resident queue is ever on)."""
    import torch
    from rumi_slam_amd.extractor import ORBextractor
    g = ORBextractor(NF, 1.2, NL, 20, 7, max_width=W, max_height=H, max_batch=B)
    pool = _pool(torch)
    ref = _host(g.extract_batch(pool, cap=CAP))
    assert ref[2][:, 0].min() > 50 and not np.array_equal(ref[1][0], ref[1][32]), "the frames must be textured and a shifted frame distinct"
    lvl = g.pyramid_level(3, frame=B - 1)
    outs = [(torch.empty((n, CAP, 7), dtype=torch.float32, device="cuda"), torch.empty((n, CAP, 32), dtype=torch.uint8, device="cuda"),
             torch.empty((n, 2), dtype=torch.int32, device="cuda")) for n in SIZES + SIZES]
    torch.cuda.synchronize()
    yield g, pool, ref, lvl, outs
    g.close()


@pytest.mark.parametrize("slots", [2, 3, 4])
def test_back_to_back_calls_equal_the_blocking_call(rig, slots):
    import torch
    g, pool, ref, lvl, outs = rig
    calls = list(zip(SIZES + SIZES, OFFSETS + OFFSETS))
    g.set_resident_queue(slots)

    def check(tag):
        for i, ((n, off), o) in enumerate(zip(calls, outs)):
            _assert_frames_equal(o, tuple(a[off:off + n] for a in ref), f"{slots} slots, {tag}, call {i} ({n} frames)")

    for o in outs:
        for t in o: t.zero_()
    torch.cuda.synchronize()
    for (n, off), o in zip(calls, outs):                 # the seven sizes twice, back to back, one sync at the end
        g.extract_batch(pool[off:off + n], cap=CAP, wait=False, out=o)
    g.sync()
    torch.cuda.synchronize()
    check("first round")
    # second round: every buffer cleared on the caller's stream, the clearing handed to wait_event before each call: it must hold back EVERY
    # stream the call drives (a sub-chunk on a stream that did not wait could land before the clearing and be wiped)
    for o in outs:
        for t in o: t.zero_()
    done = torch.cuda.Event(); done.record()
    for (n, off), o in zip(calls, outs):
        g.wait_event(done)
        g.extract_batch(pool[off:off + n], cap=CAP, wait=False, out=o)
    g.sync()
    torch.cuda.synchronize()
    check("second round")
    # the taps serve the last sub-chunk of the last call (the whole pool: its last frame is the pool's)
    assert np.array_equal(g.pyramid_level(3, frame=B - 1), lvl)


def test_streams_are_made_on_demand_and_freed(rig):
    """A handle that never enables the resident queue, then one that enables it, switches it off and extracts once through the equal
    sub-chunks: every arrangement makes the streams it drives when it first needs them, rumi_orb_destroy frees what exists."""
    from rumi_slam_amd.extractor import ORBextractor
    _, pool, ref, _, _ = rig
    a = ORBextractor(NF, 1.2, NL, 20, 7, max_width=W, max_height=H, max_batch=4)
    a.close()
    b = ORBextractor(NF, 1.2, NL, 20, 7, max_width=W, max_height=H, max_batch=64)
    try:
        b.set_resident_queue(True)
        b.set_resident_queue(False)
        _assert_frames_equal(b.extract_batch(pool[:64], cap=CAP), tuple(x[:64] for x in ref), "64 frames after the resident queue was switched off")
    finally:
        b.close()
