"""The C++ facade rumi_facade::MatchSubmapKeyPoints (rumi_slam_amd/facade/CloudMergingStep.h) over the mock key-frames of
tests/cpp/mock_model_submap.h, against the oracle (tests/cpp/submap_oracle.cc).  The two sub-maps go to the test binary in a file; the binary
runs the member once and prints the four maps it leaves and its return value.  All of it must equal what the oracle's loop gives."""
import os
import struct
import subprocess

import numpy as np
import pytest

from submap_scene import build_oracle, run_oracle, seeded_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_submap_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


def split_maps(s):
    """Key-frames 1 and 2 as two GetAllKeyFrames() vectors (each frame once) and mKfMatch12 over their indices; the scene's pairs re-ordered as
    std::map walks them (ascending index in map 1)."""
    map1 = sorted({a for a, _ in s.pairs}, reverse=True)            # any order will do: the pairs are found through the indices
    map2 = sorted({b for _, b in s.pairs})
    match = sorted((map1.index(a), map2.index(b)) for a, b in s.pairs)
    return map1, map2, match


def write_maps(path, s, map1, map2, match, nleft=-1, cols=-1):
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", len(s.frames), len(map1), len(map2), len(match), nleft, cols))
        for fr in s.frames:
            assert float(fr.min_x) == int(fr.min_x) and float(fr.min_y) == int(fr.min_y)
            f.write(struct.pack("<3i2f", fr.n, int(fr.min_x), int(fr.min_y), float(fr.w_inv), float(fr.h_inv)))
            f.write(fr.keys.astype("<f4").tobytes() + fr.un.astype("<f4").tobytes() + fr.mp.astype(np.uint8).tobytes())
        f.write(np.array(map1, "<i4").tobytes() + np.array(map2, "<i4").tobytes() + np.array(match, "<i4").tobytes())


def run_facade(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l.split() for l in r.stdout.splitlines()]
    return lines, r.stderr


def test_submap_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_submap_facade"))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 2])
def test_submap_facade_fills_the_oracles_maps(tmp_path, seed):
    from submap_scene import Scene
    exe = str(tmp_path / "test_submap_facade")
    build_facade_test(exe)
    s = seeded_scene(seed)
    map1, map2, match = split_maps(s)
    ordered = Scene(s.frames, [(map1[a], map2[b]) for a, b in match])
    path = str(tmp_path / "maps.bin")
    write_maps(path, s, map1, map2, match)
    lines, _ = run_facade(exe, path)
    best2, pair_start, matches = run_oracle(build_oracle(tmp_path), ordered)
    R = next(l for l in lines if l[0] == "R")
    assert [int(x) for x in R[1:]] == [int(pair_start[-1]), 0] + [len(match)] * 4
    q = ordered.q_start()
    rows = {k: [l for l in lines if l[0] == k] for k in "NPKV"}
    assert all(len(v) == len(match) for v in rows.values())
    for p, (a, b) in enumerate(ordered.pairs):
        want = matches[pair_start[p]:pair_start[p + 1]]
        assert [int(x) for x in rows["N"][p][1:]] == [a, len(want)]
        b2 = best2[q[p]:q[p + 1]]
        assert [int(x) for x in rows["P"][p][1:]] == [a] + [b * 100000 + int(i2) if i2 >= 0 else -1 for i2 in b2]     # sized to key-frame 1's slots
        assert [int(x) for x in rows["K"][p][1:]] == [a] + want.ravel().tolist()
        assert rows["V"][p][1:] == rows["K"][p][1:]
    assert int(pair_start[-1]) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("defect", ["NLeft", "grid"])
def test_submap_facade_refuses_what_is_not_built(tmp_path, defect):
    """A key-frame with NLeft != -1, a grid of 32 columns: 0 matches, the four maps empty, a report on stderr."""
    from rumi_slam_amd import capi
    exe = str(tmp_path / "test_submap_facade")
    build_facade_test(exe)
    s = seeded_scene(0)
    map1, map2, match = split_maps(s)
    path = str(tmp_path / "maps.bin")
    bad = s.pairs[3][1 if defect == "NLeft" else 0]
    write_maps(path, s, map1, map2, match, nleft=bad if defect == "NLeft" else -1, cols=bad if defect == "grid" else -1)
    lines, err = run_facade(exe, path)
    R = next(l for l in lines if l[0] == "R")
    assert [int(x) for x in R[1:]] == [0, capi.RUMI_E_INVALID, 0, 0, 0, 0] and "[rumi]" in err
    assert len(lines) == 1
