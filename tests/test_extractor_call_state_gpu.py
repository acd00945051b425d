"""No entry of the extractor leaves per-call state behind, not even a refused one: what one call asked of the scheduler beyond its arguments (result
block copied back or written to pinned memory, frame still in the staging buffer, feeder, mirror of a pinned records block) is gone when the next runs.
One handle at 320 x 240, three seeded frames, seven calls in an order that puts every such request in front of an entry it would corrupt.  Every
successful call equals the CPU oracle and the same call on a fresh handle bit for bit; match rows equal oracle_lib.bruteforce_match."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
from test_stream_gpu import _same_features, _same_matches

pytestmark = pytest.mark.gpu

W, H, NF, NL, MAX_BATCH = 320, 240, 1000, 8, 8
CAP = NF + 4 * NL + 64
LAP = (0, 1000)


@functools.lru_cache(maxsize=None)
def _frames():
    from rumi_slam_amd.synth import synth_frame
    return tuple(synth_frame(5200 + i, w=W, h=H, n_rect=150) for i in range(3))


@functools.lru_cache(maxsize=None)
def _reference():
    """(mono, kps, desc) of every frame from the CPU oracle: computed once, shared, never written to."""
    ext = O.OracleExtractor(NF, 1.2, NL, 20, 7)
    out = [ext.extract(img, LAP) for img in _frames()]
    assert all(len(r[1]) > 200 for r in out)
    return tuple(out)


def _extractor():
    from rumi_slam_amd.extractor import ORBextractor
    return ORBextractor(NF, 1.2, NL, 20, 7, max_width=W, max_height=H, max_batch=MAX_BATCH)


def _bit_equal(a, b, tag):
    """Two results of the same call (tuples of ints and arrays, or lists of them), bit for bit."""
    assert len(a) == len(b), tag
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, (tuple, list)):
            _bit_equal(x, y, (tag, k))
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (tag, k)
        else:
            assert x == y, (tag, k)


def _per_frame(kp, desc, counts):
    """(mono, kps, desc) per frame from [B, cap, 7] f32 / [B, cap, 32] u8 / [B, 2] i32 arrays."""
    from rumi_slam_amd.capi import KP_DTYPE
    out = []
    for f in range(len(counts)):
        n, mono = int(counts[f, 0]), int(counts[f, 1])
        assert 0 <= n <= CAP, (f, n)
        out.append((mono, np.frombuffer(np.ascontiguousarray(kp[f, :n]).tobytes(), KP_DTYPE), np.ascontiguousarray(desc[f, :n])))
    return out


def _device_batch(ext, wait):
    """rumi_orb_extract_batch_device (wait) or rumi_orb_extract_batch_device_async + rumi_orb_sync of the three frames, into fresh outputs."""
    import torch
    frames = torch.from_numpy(np.stack(_frames())).cuda()
    out = (torch.zeros((3, CAP, 7), dtype=torch.float32, device="cuda"), torch.zeros((3, CAP, 32), dtype=torch.uint8, device="cuda"),
           torch.zeros((3, 2), dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    ext.extract_batch(frames, LAP, wait=wait, out=out)
    if not wait:
        ext.sync()
    torch.cuda.synchronize()
    return _per_frame(*(t.cpu().numpy() for t in out))


def _host_records(ext):
    """rumi_orb_extract_batch_host_records of the three (pageable) frames with a PINNED h_records: (per-frame results read from the host block,
    the same from the device records, the host block itself)."""
    import torch
    from rumi_slam_amd import capi, rumination
    rb = rumination.record_bytes(CAP)
    imgs = [np.ascontiguousarray(a) for a in _frames()]
    arr = (C.c_void_p * 3)(*[a.ctypes.data for a in imgs])
    d_rec = torch.zeros((3, rb), dtype=torch.uint8, device="cuda")
    h_rec = torch.zeros((3, rb), dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()
    capi.check(ext._lib.rumi_orb_extract_batch_host_records(ext._h, arr, 3, W, H, imgs[0].strides[0], LAP[0], LAP[1], d_rec.data_ptr(), rb, CAP,
                                                            h_rec.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (_per_frame(*(t.numpy() for t in rumination.record_views(h_rec, CAP))),
            _per_frame(*(t.numpy() for t in rumination.record_views(d_rec.cpu(), CAP))), h_rec)


def _small():
    return np.full((64, 64), 90, np.uint8)            # no FAST cell grid at level 0: make_geometry refuses it inside the scheduler


def test_no_entry_leaves_per_call_state_behind():
    from rumi_slam_amd import capi
    from rumi_slam_amd.stream import FrameStream
    ref, imgs = _reference(), _frames()
    ext = _extractor()

    # 1. a refused rumi_orb_extract: the refusal comes from inside the scheduler, after the single-frame options are set
    with pytest.raises(capi.RumiError) as e:
        ext(_small(), None, LAP)
    assert e.value.code == capi.RUMI_E_INVALID

    # 2. asynchronous device batch, then rumi_orb_sync
    got = _device_batch(ext, wait=False)
    for f in range(3):
        _same_features(got[f], ref[f], ("2: async batch", f))
    _bit_equal(got, _device_batch(_extractor(), wait=False), "2: async batch against a fresh handle")

    # 3. host records with a pinned host block: the mirror is live during this call
    host, dev, h_rec = _host_records(ext)
    for f in range(3):
        _same_features(host[f], ref[f], ("3: host records, pinned block", f))
        _same_features(dev[f], ref[f], ("3: host records, device block", f))
    fresh = _host_records(_extractor())
    _bit_equal(host, fresh[0], "3: host records against a fresh handle")
    _bit_equal(dev, fresh[1], "3: device records against a fresh handle")
    snapshot = h_rec.clone()

    # 4. device batch into fresh outputs: a surviving mirror would copy into the block of step 3
    got = _device_batch(ext, wait=True)
    for f in range(3):
        _same_features(got[f], ref[f], ("4: batch", f))
    _bit_equal(got, _device_batch(_extractor(), wait=True), "4: batch against a fresh handle")
    assert h_rec.numpy().tobytes() == snapshot.numpy().tobytes(), "4: the pinned records block of step 3 was written again"

    # 5. a refused push
    fs = FrameStream(ext)
    with pytest.raises(capi.RumiError) as e:
        fs.push(_small())
    assert e.value.code == capi.RUMI_E_INVALID

    # 6. two pushes of real frames
    other = _extractor()
    fresh_fs = FrameStream(other)
    prev = None
    for t in range(2):
        got = fs.push(imgs[t])
        _same_features(got, ref[t], ("6: push", t))
        assert fs.n_prev == (0 if prev is None else len(prev)), t
        _same_matches(got, prev, ("6: push", t))
        _bit_equal(got, fresh_fs.push(imgs[t]), ("6: push against a fresh handle", t))
        prev = got[2]

    # 7. rumi_orb_extract of a real frame
    got = ext(imgs[2], None, LAP)
    _same_features(got, ref[2], "7: extract")
    _bit_equal(got, _extractor()(imgs[2], None, LAP), "7: extract against a fresh handle")
    assert h_rec.numpy().tobytes() == snapshot.numpy().tobytes(), "7: the pinned records block of step 3 was written again"
