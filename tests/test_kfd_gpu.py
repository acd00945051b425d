"""The PD frame selector on the device (include/rumi_kfd.h) against its scalar oracle (tests/cpp/kfd_oracle.cc), bit for bit: pyramid and derivative
buffers, tracked points and status bytes for several point counts and for the constructed cases of tests/kfd_scene.py, every field of an 8-frame step
sequence with the extraction of its selected frames, BGR input, and the error paths.  160 x 128 and 131 x 128 frames: the odd width exercises
(w + 1) / 2 and rows that are not dword-aligned."""
import numpy as np
import pytest

import kfd_scene as ks

pytestmark = pytest.mark.gpu
SIZES = [(160, 128), (131, 128)]
ORB = (300, 1.2, 4, 20, 7)


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return ks.build_oracle(tmp_path_factory.mktemp("kfd_oracle"))


@pytest.fixture(scope="module")
def frames():
    return {size: ks.sequence(*size) for size in SIZES}


def _track(prev, cur, pts, **kw):
    from rumi_slam_amd.kfd import KFDSampler
    return KFDSampler.track(prev, cur, pts, **kw)


def _same_track(L, prev, cur, pts, what=""):
    nxt, status = _track(prev, cur, pts)
    onxt, ostatus, diag = ks.oracle_track(L, prev, cur, pts)
    assert status.tobytes() == ostatus.tobytes(), (what, status, ostatus)
    assert nxt.tobytes() == onxt.tobytes(), (what, np.abs(nxt - onxt).max())
    return status, diag


@pytest.mark.parametrize("size", SIZES)
def test_pyramid_and_derivative_buffers(L, frames, size):
    prev, cur = frames[size][0], frames[size][3]
    _, _, levels, derivs = _track(prev, cur, np.zeros((1, 2), np.float32), dumps=True)
    _, _, _, olevels, oderivs = ks.oracle_track(L, prev, cur, np.zeros((1, 2), np.float32), dumps=True)
    for l in range(3):
        assert levels[l].shape == olevels[l].shape
        assert np.array_equal(levels[l], olevels[l]), f"level {l}"
        assert np.array_equal(derivs[l], oderivs[l]), f"derivative of level {l}"
    assert np.array_equal(levels[0], prev)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_track_point_counts(L, frames, size, n):
    w, h = size
    rng = np.random.default_rng(n)
    pts = np.stack([rng.uniform(-20, w + 20, n), rng.uniform(-20, h + 20, n)], 1).astype(np.float32)       # some of them at and beyond the borders
    status, _ = _same_track(L, frames[size][0], frames[size][3], pts, f"n = {n}")
    if n >= 64:
        assert 0 < status.sum() < n


def test_track_without_points(frames):
    nxt, status = _track(frames[SIZES[0]][0], frames[SIZES[0]][1], np.zeros((0, 2), np.float32))
    assert nxt.shape == (0, 2) and status.shape == (0,)


@pytest.mark.parametrize("size", SIZES)
def test_constructed_cases(L, size):
    for c in ks.constructed_cases(*size):
        status, diag = _same_track(L, c.prev, c.cur, c.pts, c.name)
        assert list(status) == c.status, c.name                       # (that the oracle takes the named path: tests/test_kfd_cpu.py)


def _oracle_extractor():
    import oracle_lib
    ex = oracle_lib.OracleExtractor(*ORB)
    return lambda grey: ex.extract(grey, (0, 0))


def _sampler(size):
    from rumi_slam_amd.extractor import ORBextractor
    from rumi_slam_amd.kfd import KFDSampler
    ext = ORBextractor(*ORB, max_width=size[0], max_height=size[1])
    s = KFDSampler(ext)
    s.set_pd(*ks.SEQ_PD)
    return ext, s


def _same_step(got, o, onext, ostatus, oext, k):
    f32 = np.float32
    assert got.selected == bool(o.selected) and got.n_tracked == o.n_tracked and got.n_good == o.n_good, k
    for name in ("moptf", "pd_out", "th"):
        assert f32(getattr(got, name)).tobytes() == f32(getattr(o, name)).tobytes(), (k, name, getattr(got, name), getattr(o, name))
    assert got.next.tobytes() == onext.tobytes() and got.status.tobytes() == ostatus.tobytes(), k
    if o.selected:
        mono, kps, desc = oext
        assert got.mono == mono and got.keypoints.tobytes() == kps.tobytes() and np.array_equal(got.descriptors, desc), k
    else:
        assert len(got.keypoints) == 0 and len(got.descriptors) == 0


@pytest.mark.parametrize("size", SIZES)
def test_step_sequence(L, frames, size):
    ext, s = _sampler(size)
    o = ks.OracleSampler(L, _oracle_extractor(), *ks.SEQ_PD)
    decisions = []
    for k, f in enumerate(frames[size]):
        got = s.step(f, ks.SEQ_TIMES[k])
        so, onext, ostatus, oext = o.step(f, ks.SEQ_TIMES[k])
        _same_step(got, so, onext, ostatus, oext, k)
        decisions.append(got.selected)
        if got.selected:                                               # the extractor alone on the same image gives the same features
            mono, kps, desc = ext(f, None, (0, 0))
            assert mono == got.mono and kps.tobytes() == got.keypoints.tobytes() and np.array_equal(desc, got.descriptors)
    assert decisions == [True, False, False, True, False, False, True, False]
    s.reset()
    o.reset()
    got = s.step(frames[size][2], 11.0)                                # after Reset: a first step, then tracking goes on from its key-points
    _same_step(got, *o.step(frames[size][2], 11.0), "reset")
    assert got.selected and got.n_tracked == 0
    got = s.step(frames[size][3], 11.04)
    _same_step(got, *o.step(frames[size][3], 11.04), "after reset")
    s.close(), ext.close()


def test_bgr_input_is_the_oracles_grey(L, frames):
    size = SIZES[1]
    tex = [ks.Texture(30 + c) for c in range(3)]
    bgr = [np.stack([t.frame(*size, shift) for t in tex], -1) for shift in [(0, 0), (0.6, 0.3), (3.0, 1.0)]]
    grey = [ks.oracle_grey(L, b) for b in bgr]
    assert not np.array_equal(grey[0], bgr[0][..., 1])
    pts = ks.grid_points(*size, margin=20)
    nxt, status, levels, _ = _track(bgr[0], bgr[1], pts, dumps=True)
    assert np.array_equal(levels[0], grey[0])
    onxt, ostatus, _ = ks.oracle_track(L, grey[0], grey[1], pts)
    assert nxt.tobytes() == onxt.tobytes() and status.tobytes() == ostatus.tobytes()
    # the sampler: BGR frames in a padded buffer (a row pitch of its own) step like the oracle on the converted frames
    ext, s = _sampler(size)
    o = ks.OracleSampler(L, _oracle_extractor(), *ks.SEQ_PD)
    for k in range(3):
        padded = np.zeros((size[1], size[0] + 5, 3), np.uint8)
        padded[:, :size[0]] = bgr[k]
        got = s.step(padded[:, :size[0]], 1.0 + 0.04 * k)
        _same_step(got, *o.step(grey[k], 1.0 + 0.04 * k), k)
    s.close(), ext.close()


def test_error_paths_leave_the_state_intact(L, frames):
    from rumi_slam_amd import capi
    size = SIZES[0]
    ext, s = _sampler(size)
    o = ks.OracleSampler(L, _oracle_extractor(), *ks.SEQ_PD)
    fs = frames[size]
    for k in range(2):
        _same_step(s.step(fs[k], ks.SEQ_TIMES[k]), *o.step(fs[k], ks.SEQ_TIMES[k]), k)
    bad = [(np.zeros((0, 0), np.uint8), capi.RUMI_E_EMPTY), (np.full((100, 100), 9, np.uint8), capi.RUMI_E_INVALID),
           (np.zeros((128, 160, 2), np.uint8), capi.RUMI_E_INVALID), (np.zeros((128, 161), np.uint8), capi.RUMI_E_INVALID)]
    for img, code in bad:
        with pytest.raises(capi.RumiError) as e:
            s.step(img, 99.0)
        assert e.value.code == code, (img.shape, e.value)
    for k in range(2, 5):                                              # the sequence goes on as if nothing had been refused (a selecting step among them)
        _same_step(s.step(fs[k], ks.SEQ_TIMES[k]), *o.step(fs[k], ks.SEQ_TIMES[k]), k)
    with pytest.raises(capi.RumiError) as e:
        _track(np.zeros((100, 100), np.uint8), np.zeros((100, 100), np.uint8), np.zeros((1, 2), np.float32))
    assert e.value.code == capi.RUMI_E_INVALID
    s.close(), ext.close()
