"""The C++ facade rumi_facade::CommonRegionsBoWStage (rumi_slam_amd/facade/LoopClosingStep.h) over the mock key-frames of
tests/cpp/mock_model_loopclosing.h.  The scene goes to the test binary in a file; the binary runs the stage once and prints what it leaves per
candidate.  All of it must equal LoopClosing.cc:576-651 read literally: the skips and the abort here in Python, every SearchByBoW by the oracle,
the fold by common_regions_scene.union."""
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from common_regions_scene import most_matches, oracle_pair, seeded_scene, union

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COVISIBLES = 10


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_common_regions_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


def facade_scene():
    """Key-frame numbers of the file: 0 = the current key-frame, k + 1 = table entry k of the seeded scene.  Returns (scene, candidates, covisibles,
    connected of the current key-frame, bad key-frames)."""
    s = seeded_scene(21, n=150)
    g0, g1, g2 = ([k + 1 for k in g] for g in s.groups)
    cov = {k: [] for k in range(len(s.kfs) + 1)}
    cov[g0[0]] = g0[1:] + g1[1:3]                # twelve covisibles: GetBestCovisibilityKeyFrames(10) cuts the list
    cov[g1[0]] = g1[1:8]                         # g1[2] is bad: a member left out, its vvpMatchedMPs stays empty
    cov[g2[0]] = g2[1:6]                         # g2[4] is connected to the current key-frame: the candidate is aborted
    cov[g2[1]] = []                              # an empty covisible list: the candidate alone (:584-586)
    cov[g0[5]] = [g0[6]]                         # one covisible: it is displaced to the end
    cands = [g0[0], -1, g1[0], g2[0], g2[1], g1[2], g0[5]]          # a NULL candidate and a bad one (g1[2]) are skipped
    return s, cands, cov, [g2[4], g2[7]], {g1[2]}


def write_scene(path, s, cands, cov, connected, bad_kfs, nleft=None):
    with open(path, "wb") as f:
        # one point more than the scene's numbering: the good point every good feature of the current key-frame holds
        f.write(struct.pack("<4ifi", len(s.kfs) + 1, len(s.mp_bad) + 1, len(cands), N_COVISIBLES, s.nnratio, int(s.ori)))
        f.write(s.mp_bad.astype(np.uint8).tobytes() + bytes([0]))
        for k, K in enumerate([s.cur] + s.kfs):
            nodes, off, idx = K.fv
            mp = np.where(s.cur_good != 0, len(s.mp_bad), -1).astype(np.int32) if k == 0 else K.mp
            conn = connected if k == 0 else []
            f.write(struct.pack("<6i", K.n, int(k in bad_kfs), 0 if k == nleft else -1, len(nodes), len(cov[k]), len(conn)))
            f.write(K.keys["angle"].astype("<f4").tobytes() + K.desc.tobytes() + mp.astype("<i4").tobytes())
            for a, nd in enumerate(nodes):
                f.write(struct.pack("<2i", int(nd), int(off[a + 1] - off[a])) + idx[off[a]:off[a + 1]].astype("<i4").tobytes())
            f.write(np.array(cov[k], "<i4").tobytes() + np.array(conn, "<i4").tobytes())
        f.write(np.array(cands, "<i4").tobytes())


def literal(s, cands, cov, connected, bad_kfs):
    """LoopClosing.cc:576-651 per candidate: {candidate: (vpCovKFi, vvpMatchedMPs, vpMatchedPoints, vpKeyFrameMatchedMP, num, index, most)}."""
    out = {}
    n = s.cur.n
    for c in cands:
        if c < 0 or c in bad_kfs:
            continue
        v = cov[c][:N_COVISIBLES]
        v = [c] if not v else [c] + v[1:] + [v[0]]
        if any(k in connected for k in v):
            continue
        vv, nums = [], []
        for k in v:
            if k in bad_kfs:
                vv.append(None); nums.append(0); continue
            num, m12 = oracle_pair(O, s, k - 1)
            vv.append(np.where(m12 >= 0, s.kfs[k - 1].mp[np.maximum(m12, 0)], -1)); nums.append(num)
        pt, mem, count = union(n, [[] if x is None else x for x in vv])
        at, most = most_matches(nums)
        out[c] = (v, vv, pt, np.array([v[j] if j >= 0 else -1 for j in mem]), count, at, most)
    return out


def run_facade(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return [l.split() for l in r.stdout.splitlines()], r.stderr


def test_the_scene_holds_what_it_is_for():
    s, cands, cov, connected, bad_kfs = facade_scene()
    want = literal(s, cands, cov, connected, bad_kfs)
    g0, g1, g2 = ([k + 1 for k in g] for g in s.groups)
    assert list(want) == [g0[0], g1[0], g2[1], g0[5]]                                  # NULL, aborted and bad candidates are gone
    assert len(want[g0[0]][0]) == 11 and want[g0[0]][0][-1] == g0[1] and g1[2] not in want[g0[0]][0]        # cut at ten, the first displaced
    assert any(x is None for x in want[g1[0]][1]) and want[g2[1]][0] == [g2[1]] and want[g0[5]][0] == [g0[5], g0[6]]
    assert want[g0[0]][4] >= 20 and want[g2[1]][4] < 20


@pytest.mark.gpu
def test_facade_fills_what_the_literal_loop_gives(tmp_path):
    exe = str(tmp_path / "test_common_regions_facade")
    build_facade_test(exe)
    s, cands, cov, connected, bad_kfs = facade_scene()
    path = str(tmp_path / "scene.bin")
    write_scene(path, s, cands, cov, connected, bad_kfs)
    lines, _ = run_facade(exe, path)
    want = literal(s, cands, cov, connected, bad_kfs)
    assert [int(x) for x in lines[0][1:]] == [len(want), 0, len(want)]
    rows = {}
    for l in lines[1:]:
        rows.setdefault((l[0], int(l[1])), []).append(l[2:])
    assert [c for (t, c) in rows if t == "C"] == list(want)
    for c, (v, vv, pt, kf, count, at, most) in want.items():
        assert [int(x) for x in rows["C", c][0]] == [count, at, most], c
        assert [int(x) for x in rows["V", c][0]] == v
        assert len(rows["M", c]) == len(v)
        for j, r in enumerate(rows["M", c]):
            assert int(r[0]) == j
            if vv[j] is None:
                assert r[1:] == ["empty"], (c, j)
            else:
                assert [int(x) for x in r[1:]] == vv[j].tolist(), (c, j)
        assert [int(x) for x in rows["P", c][0]] == pt.tolist() and [int(x) for x in rows["K", c][0]] == kf.tolist(), c


@pytest.mark.gpu
@pytest.mark.parametrize("who", ["current", "member"])
def test_facade_refuses_two_camera_keyframes(tmp_path, who):
    """A key-frame with NLeft != -1: -1 returned, nothing handed back, a report on stderr."""
    from rumi_slam_amd import capi
    exe = str(tmp_path / "test_common_regions_facade")
    build_facade_test(exe)
    s, cands, cov, connected, bad_kfs = facade_scene()
    path = str(tmp_path / "scene.bin")
    write_scene(path, s, cands, cov, connected, bad_kfs, nleft=0 if who == "current" else s.groups[0][4] + 1)
    lines, err = run_facade(exe, path)
    assert [int(x) for x in lines[0][1:]] == [-1, capi.RUMI_E_INVALID, 0] and len(lines) == 1 and "[rumi]" in err and "NLeft" in err
