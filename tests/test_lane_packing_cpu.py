"""Lane packing of the batch launches of k_resize and k_blur (orb_geom.h: LanePack / lane_slot), checked on the CPU through
rumi_hook_lane_packing: the hook evaluates the launch code's choice of frames per group and the kernels' own (wave, lane) -> (frame, dword
column) function, so what is counted here is what the launches issue.

k_resize: a group's row is G x ceil(w / 4) lanes, waves take 64 consecutive ones; G = 1 is the mapping of a launch per frame.
k_blur (batches): a frame's row has ceil(w / 4) producing columns plus the mirrored halo dword; a wave advances by 62 lanes and its lanes 0
and 63 only carry their neighbours' halo, so no shuffled dword may cross a frame seam into a producing lane and none has to come from memory.
The strip mapping it replaces (256 / 240 / .. pixel strips, halo loads in lanes 0 / 63) has no G: with G = 1 the packed blur is still the
62-lane walk, which the test checks for coverage like every other G."""
import ctypes as C

import numpy as np
import pytest

from rumi_slam_amd import capi

GEOMS = [(640, 480, 1.2, 8), (752, 480, 1.2, 8), (200, 150, 1.2, 4)]
FRAMES = [16, 17, 64, 256]
RESIZE, BLUR = 0, 1


def mapping(w, h, scale, nlevels, nframes, kernel, level, force_g=0):
    H = capi.hooks()
    info = np.zeros(8, np.int32)
    n = C.c_int32()
    rc = H.rumi_hook_lane_packing(w, h, scale, nlevels, nframes, kernel, level, force_g, capi.ptr(info), None, 0, C.byref(n))
    assert rc in (0, capi.RUMI_E_CAPACITY), rc
    slots = np.zeros((n.value, 3), np.int32)
    assert H.rumi_hook_lane_packing(w, h, scale, nlevels, nframes, kernel, level, force_g, capi.ptr(info), capi.ptr(slots), n.value, C.byref(n)) == 0
    keys = ("w", "lpr", "G", "waves", "groups", "step", "halo", "h")
    return dict(zip(keys, (int(v) for v in info))), slots.reshape(-1, 64, 3)


def check_mapping(I, S, nframes, kernel):
    w, lpr, nd = I["w"], I["lpr"], (I["w"] + 3) // 4
    assert lpr == nd + I["halo"] and I["halo"] == (1 if kernel == BLUR else 0)
    assert S.shape[0] == I["groups"] * I["waves"] and 1 <= I["G"] <= 8 and I["groups"] == -(-nframes // I["G"])
    frame, col, flags = S[..., 0], S[..., 1], S[..., 2]
    produce, first, last = (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0
    mapped = frame >= 0
    # no lane maps outside its frame's row (plus the blur's one halo dword); a producing lane holds a pixel of the row
    assert (frame < nframes).all() and ((col >= 0) & (col < lpr))[mapped].all()
    assert mapped[produce].all() and (col[produce] < nd).all() and (4 * col[produce] < w).all()
    # every (frame, row dword) is owned by exactly one producing lane
    owners = np.bincount((frame[produce].astype(np.int64) * nd + col[produce]), minlength=nframes * nd)
    assert len(owners) == nframes * nd and (owners == 1).all(), f"owners per dword: min {owners.min()} max {owners.max()}"
    # a lane's frames lie in its wave's group
    group = np.arange(S.shape[0])[:, None] // I["waves"]
    assert (frame[mapped] // I["G"] == np.broadcast_to(group, frame.shape)[mapped]).all()
    # seam and edge flags agree with the column
    assert (first == (col == 0))[mapped].all() and (last == (col == lpr - 1))[mapped].all()
    if kernel == BLUR:
        lane = np.broadcast_to(np.arange(64), frame.shape)
        assert ((lane >= 1) & (lane <= 62))[produce].all(), "lanes 0 and 63 of a blur wave only carry halo dwords"
        fl, cl, fr, cr = frame[:, :-2], col[:, :-2], frame[:, 2:], col[:, 2:]       # neighbours of lanes 1 .. 62
        p, f, c = produce[:, 1:-1], frame[:, 1:-1], col[:, 1:-1]
        # the right neighbour of a producing lane is the next dword of the same frame (the halo column for the last one); so is the left one,
        # but for a frame's first dword, which mirrors its own bytes
        assert ((fr == f) & (cr == c + 1))[p].all(), "a producing lane's right neighbour crosses a seam"
        assert ((fl == f) & (cl == c - 1))[p & (c > 0)].all(), "a producing lane's left neighbour crosses a seam"
        # right-edge rebuild: a dword that reaches column w or beyond is rebuilt from the one (the halo column: two) dwords to its left, which
        # must sit in the same wave and frame whenever a producing lane uses the rebuilt dword (itself or as its right halo)
        for i in range(1, 64):
            used = (produce[:, i] | produce[:, i - 1]) & (4 * col[:, i] + 3 >= w) & mapped[:, i]
            assert ((frame[:, i - 1] == frame[:, i]) & (col[:, i - 1] == col[:, i] - 1))[used].all(), f"rebuild at lane {i}: left dword"
            halo = used & (col[:, i] == nd)
            if halo.any():
                assert i >= 2 and ((frame[:, i - 2] == frame[:, i]) & (col[:, i - 2] == col[:, i] - 2))[halo].all(), f"rebuild at lane {i}: second dword"
    return int(produce.sum()), int(S.shape[0] * 64)


def occupancy(w, h, scale, nlevels, nframes, kernel, force_g=0):
    """producing lanes / issued lane slots per level, weighted by the level's pixels"""
    num = den = 0.0
    for level in range(1 if kernel == RESIZE else 0, nlevels):
        I, S = mapping(w, h, scale, nlevels, nframes, kernel, level, force_g)
        produced, issued = check_mapping(I, S, nframes, kernel)
        num += I["w"] * I["h"] * produced / issued
        den += I["w"] * I["h"]
    return num / den


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("nframes", FRAMES)
@pytest.mark.parametrize("kernel", [RESIZE, BLUR], ids=["resize", "blur"])
def test_every_dword_has_one_owner_and_no_lane_leaves_its_row(geom, nframes, kernel):
    occ = occupancy(*geom, nframes, kernel)
    print(f"{'blur' if kernel else 'resize'} {geom[0]}x{geom[1]} {nframes} frames: producing / issued lanes = {occ:.4f}")
    assert 0 < occ <= 1


@pytest.mark.parametrize("kernel", [RESIZE, BLUR], ids=["resize", "blur"])
def test_occupancy_of_the_flagship_batch(kernel):
    """640 x 480, 256 frames: producing lanes / issued lane slots, pixel-weighted over the levels, >= 0.90 for each kernel (a condition derived
    from the design, not a measurement; a launch per frame gives ~0.71 for the resize, the strip blur gave ~0.75)."""
    occ = occupancy(640, 480, 1.2, 8, 256, kernel)
    one = occupancy(640, 480, 1.2, 8, 256, kernel, force_g=1)
    print(f"{'blur' if kernel else 'resize'} 640x480 256 frames: producing / issued lanes = {occ:.4f} (one frame per group: {one:.4f})")
    assert occ >= 0.90


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_one_frame_per_group_is_the_launch_per_frame(geom):
    """G = 1 for the resize: ceil(w / 256) waves along the row, lane j of wave k owns dword 64 k + j of frame = group; launches of fewer than
    16 frames pick it.  The packed blur with G = 1 still covers every dword once (checked by check_mapping)."""
    w, h, scale, nlevels = geom
    for level in range(1, nlevels):
        I, S = mapping(w, h, scale, nlevels, 5, RESIZE, level)
        assert I["G"] == 1, "fewer than 16 frames: a launch per frame"
        I, S = mapping(w, h, scale, nlevels, 19, RESIZE, level, force_g=1)
        assert I["waves"] == (I["w"] + 255) // 256 and I["groups"] == 19 and S.shape[0] == 19 * I["waves"]
        dword = (np.arange(S.shape[0])[:, None] % I["waves"]) * 64 + np.arange(64)[None, :]
        inside = 4 * dword < I["w"]
        assert (S[..., 1][inside] == dword[inside]).all()
        assert (S[..., 0] == np.where(inside, np.arange(S.shape[0])[:, None] // I["waves"], -1)).all()
        assert ((S[..., 2] & 1) == inside).all()
    for level in range(nlevels):
        check_mapping(*mapping(w, h, scale, nlevels, 19, BLUR, level, force_g=1), 19, BLUR)
