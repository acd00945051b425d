"""FrameStream / RumiOrbStream on the device: six synthetic 320 x 240 frames (each the previous one under a small warp), 500 features, 8 levels.
Every push gives the extractor's result for the frame (a second handle's ORBextractor.__call__ and the CPU oracle, bit for bit) and the oracle's
brute-force match of the frame against the previous one; first frame, reset, a frame without key-points, an empty image, an interleaved
rumi_orb_extract, the resident copy and lap = (0, 0)."""
import functools

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

W, H, NF, NL = 320, 240, 500, 8


@functools.lru_cache(maxsize=None)
def _frames():
    from rumi_slam_amd.synth import synth_frame, warp_frame
    imgs = [synth_frame(4100, w=W, h=H, n_rect=150)]
    for i in range(5):
        imgs.append(warp_frame(imgs[-1], 500 + i)[0])
    return tuple(imgs)


@functools.lru_cache(maxsize=None)
def _reference(lap=(0, 1000)):
    """(mono, kps, desc) of every frame from the CPU oracle: computed once, shared, never written to."""
    ext = O.OracleExtractor(NF, 1.2, NL, 20, 7)
    out = [ext.extract(img, lap) for img in _frames()]
    assert all(len(r[1]) > 200 for r in out)
    return tuple(out)


def _extractor():
    from rumi_slam_amd.extractor import ORBextractor
    return ORBextractor(NF, 1.2, NL, 20, 7, max_width=W, max_height=H)


def _stream():
    from rumi_slam_amd.stream import FrameStream
    ext = _extractor()
    return ext, FrameStream(ext)


def _same_features(got, ref, tag):
    mono, kps, desc = got[:3]
    assert mono == ref[0] and len(kps) == len(ref[1]), (tag, mono, ref[0], len(kps), len(ref[1]))
    assert kps.tobytes() == ref[1].tobytes(), (tag, "key-points")
    assert np.array_equal(desc, ref[2]), (tag, "descriptors")


def _same_matches(got, desc_prev, tag):
    desc = got[2]
    if desc_prev is None:
        desc_prev = np.zeros((0, 32), np.uint8)
    for g, r, what in zip(got[3:], O.bruteforce_match(np.ascontiguousarray(desc), np.ascontiguousarray(desc_prev)), ("best index", "best distance", "second distance")):
        assert g.dtype == np.int32 and np.array_equal(g, r), (tag, what)
    if len(desc_prev) == 0:
        assert (got[3] == -1).all() and (got[4] == 256).all() and (got[5] == 256).all(), tag


def test_six_frames_equal_extractor_oracle_and_matcher():
    ref = _reference()
    ext, fs = _stream()
    other = _extractor()
    prev = None
    for t, img in enumerate(_frames()):
        got = fs.push(img)
        _same_features(got, ref[t], t)
        _same_features(other(img, None, (0, 1000)), ref[t], ("second handle", t))
        assert fs.n_prev == (0 if prev is None else len(prev)), t
        _same_matches(got, prev, t)
        if prev is not None:
            assert (got[3] >= 0).sum() == len(got[3]) and (got[4] < 40).sum() > 50, t      # consecutive frames do match
        prev = got[2]


def test_reset_makes_the_next_frame_a_first_frame():
    ref = _reference()
    ext, fs = _stream()
    for t, img in enumerate(_frames()[:5]):
        if t == 3:
            fs.reset()
        got = fs.push(img)
        _same_features(got, ref[t], t)
        assert fs.n_prev == (0 if t in (0, 3) else len(ref[t - 1][1])), t
        _same_matches(got, None if t in (0, 3) else ref[t - 1][2], t)


def test_flat_frame_in_the_middle():
    ref = _reference()
    ext, fs = _stream()
    imgs = _frames()
    fs.push(imgs[0])
    got = fs.push(imgs[1])
    _same_matches(got, ref[0][2], 1)
    flat = fs.push(np.full((H, W), 128, np.uint8))
    assert len(flat[1]) == 0 and flat[2].shape == (0, 32) and all(len(x) == 0 for x in flat[3:]) and fs.n_prev == len(ref[1][1])
    got = fs.push(imgs[2])
    _same_features(got, ref[2], 2)
    assert fs.n_prev == 0
    _same_matches(got, None, "after the flat frame")
    got = fs.push(imgs[3])
    assert fs.n_prev == len(ref[2][1])
    _same_matches(got, ref[2][2], 3)


def test_empty_image_leaves_the_previous_frame():
    from rumi_slam_amd import capi
    ref = _reference()
    ext, fs = _stream()
    imgs = _frames()
    fs.push(imgs[0])
    for empty in (None, np.zeros((0, 0), np.uint8)):
        with pytest.raises(capi.RumiError) as e:
            fs.push(empty)
        assert e.value.code == capi.RUMI_E_EMPTY
    got = fs.push(imgs[1])
    _same_features(got, ref[1], 1)
    assert fs.n_prev == len(ref[0][1])
    _same_matches(got, ref[0][2], "after the empty image")


def test_extract_on_the_same_handle_between_pushes():
    ref = _reference()
    ext, fs = _stream()
    imgs = _frames()
    fs.push(imgs[0])
    _same_features(ext(imgs[4], None, (0, 1000)), ref[4], "interleaved extract")
    got = fs.push(imgs[1])
    _same_features(got, ref[1], 1)
    _same_matches(got, ref[0][2], "after an interleaved extract")
    _same_features(ext(imgs[5], None, (0, 1000)), ref[5], "interleaved extract")
    got = fs.push(imgs[2])
    _same_matches(got, ref[1][2], 2)


def test_resident_copy_equals_the_pinned_one():
    import torch
    ext, fs = _stream()
    imgs = _frames()
    from rumi_slam_amd import capi
    with pytest.raises(capi.RumiError):
        fs.resident()
    for t in range(3):
        mono, kps, desc = fs.push(imgs[t])[:3]
        kp_d, desc_d, counts_d = fs.resident()
        torch.cuda.synchronize()
        n = len(kps)
        assert counts_d.cpu().tolist() == [n, mono]
        assert np.array_equal(desc_d[:n].cpu().numpy(), desc), t
        assert kp_d[:n].cpu().numpy().tobytes() == kps.tobytes(), t


def test_lapping_area_passes_through():
    ref = _reference((0, 0))
    ext, fs = _stream()
    prev = None
    for t, img in enumerate(_frames()[:2]):
        got = fs.push(img, lap=(0, 0))
        _same_features(got, ref[t], ("lap00", t))
        _same_matches(got, prev, ("lap00", t))
        prev = got[2]


def test_profiling_takes_the_copy_path():
    """With profiling on the kernels write device memory and copies bring the block to the host (as rumi_orb_extract does): same results."""
    ref = _reference()
    ext, fs = _stream()
    ext.set_profiling(True)
    prev = None
    for t, img in enumerate(_frames()[:3]):
        got = fs.push(img)
        _same_features(got, ref[t], ("profiled", t))
        assert fs.n_prev == (0 if prev is None else len(prev))
        _same_matches(got, prev, ("profiled", t))
        prev = got[2]
