"""The C++ facade LocalMappingStep::KeyFrameCullingResident / CloudKeyFrameCullingResident over a CovisibilityGraph
(rumi_slam_amd/facade/) and the mock data model of tests/cpp/mock_model_culling_resident.h.  The binary (tests/cpp/test_culling_resident_facade.cc)
builds the map twice, runs the resident member on one copy and the block member on the other, for two consecutive current key-frames, and
prints both maps: they must be the same map, and each call must cull what the oracle culls on the evolving map."""
import os
import struct
import subprocess

import numpy as np
import pytest

import culling_resident_scene as rs
from culling_scene import build_oracle, run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# sequences (as culling_resident_scene.SEQUENCES) whose first two calls both cull, in both variants, and turn points bad
FACADE_SEQUENCES = [rs.SEQUENCES[0], (5, 52, [(0, 18), (14, 18), (6, 40)])]


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_culling_resident_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("culling_resident_facade") / "test_culling_resident_facade")
    build_facade_test(out)
    return out


def write_map(path, s, cands, cloud, inertial=False, monocular=True, stereo_kf=-1, unseen=-1):
    with open(path, "wb") as f:
        f.write(struct.pack("<10i", s.n_kf, len(s.points), len(cands[0]), len(cands[1]), int(cloud), 0, int(inertial), int(monocular), stereo_kf, unseen))
        for k in range(s.n_kf):
            f.write(struct.pack("<5i", int(s.n[k]), int(s.kf_bad[k]), int(s.kf_init[k]), int(s.not_erase[k]), int(s.cloud[k])))
            f.write(s.octave[k].astype("<i4").tobytes())
        for bad, n, obs in s.points:
            f.write(struct.pack("<3i", int(bad), n, len(obs)))
            f.write(np.array(obs, np.int32).reshape(-1, 2).astype("<i4").tobytes())
        for c in cands:
            f.write(np.array(c, "<i4").tobytes())


def run_facade(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return [l.split() for l in r.stdout.splitlines()], r.stderr


def two_lists(oracle, sc, lists, cloud):
    """The first two candidate lists of a sequence, the second without what the first call culls (KeyFrame::SetBadFlag takes a culled
    key-frame out of every covisible list), and what the oracle culls in each call on the evolving map."""
    from rumi_slam_amd.mapping import CULL_CLOUD, trim
    m = rs.MapMirror.from_scene(sc)
    flags = CULL_CLOUD if cloud else 0
    b = m.batch(lists[0])
    res = trim(b, run_oracle(oracle, b, flags))
    m.apply(lists[0], res)
    second = [k for k in lists[1] if not (m.kf_bad[k] and not sc.kf_bad[k])]
    b2 = m.batch(second)
    res2 = trim(b2, run_oracle(oracle, b2, flags))
    m.apply(second, res2)
    return [lists[0], second], [len(res["culled"]), len(res2["culled"])], m


def test_culling_resident_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_culling_resident_facade"))


@pytest.mark.gpu
@pytest.mark.parametrize("seq", FACADE_SEQUENCES, ids=lambda s: f"seed{s[0]}")
@pytest.mark.parametrize("cloud", [False, True], ids=["plain", "cloud"])
def test_resident_member_leaves_the_block_members_map(tmp_path, exe, seq, cloud):
    oracle = build_oracle(tmp_path)
    sc, lists = rs.sequence(*seq)
    cands, want, m = two_lists(oracle, sc, lists, cloud)
    path = str(tmp_path / "map.bin")
    write_map(path, sc, cands, cloud)
    lines, err = run_facade(exe, path)
    R = {(l[1], int(l[2])): (int(l[3]), int(l[4])) for l in lines if l[0] == "R"}
    for call in (0, 1):
        assert R[("A", call)] == R[("B", call)] == (want[call], 0), (call, R, err[-2000:])
    assert sum(want) >= 2 and want[1] >= 1, "the second call culls too, on the edits the first one staged"
    A = [[l[0]] + l[2:] for l in lines if l[0] in "KMP" and l[1] == "A"]
    B = [[l[0]] + l[2:] for l in lines if l[0] in "KMP" and l[1] == "B"]
    assert len(A) == 2 * sc.n_kf + len(sc.points) and A == B, "bad key-frames, mbToBeErased, slots, observation maps, nObs, bad points"
    K = [l for l in A if l[0] == "K"]
    assert [int(l[2]) for l in K] == [int(x) for x in m.kf_bad] and [int(l[3]) for l in K] == [int(x) for x in m.to_be_erased]
    assert all(int(l[4]) == 2 for l in K)                                               # UpdateBestCovisibles, once per call (:959)
    P = [l for l in A if l[0] == "P"]
    assert [int(l[2]) for l in P] == [int(x) for x in m.pt_bad] and sum(m.pt_bad) > sum(bool(p[0]) for p in sc.points)
    U = [l for l in lines if l[0] == "U"]
    assert all(int(l[2]) == sc.n_kf and int(l[3]) == len(sc.points) for l in U), "the graph holds the map and nothing else"


@pytest.mark.gpu
@pytest.mark.parametrize("inertial,monocular,stereo,unseen", [(True, True, False, False), (False, False, False, False), (False, True, True, False),
                                                              (False, True, False, True)], ids=["inertial", "stereo-sensor", "NLeft", "unseen"])
def test_resident_member_refuses(tmp_path, exe, inertial, monocular, stereo, unseen):
    """Refused with a report and the refusal status; both maps are left as they were, and the graph learns of no key-frame."""
    from rumi_slam_amd import capi
    sc, lists = rs.sequence(*rs.SEQUENCES[0])
    first = list(lists[0])
    if unseen:
        assert sc.empty_kf not in first and not any(k == sc.empty_kf for p in sc.points for k, f in p[2])
        first.append(sc.empty_kf)
    path = str(tmp_path / "map.bin")
    write_map(path, sc, [first, []], False, inertial, monocular, first[3] if stereo else -1, sc.empty_kf if unseen else -1)
    lines, err = run_facade(exe, path)
    R = {(l[1], int(l[2])): (int(l[3]), int(l[4])) for l in lines if l[0] == "R"}
    assert R[("A", 0)] == (-1, capi.RUMI_E_INVALID) and "[rumi]" in err and "KeyFrameCullingResident" in err
    if unseen:
        assert "never seen" in err and R[("B", 0)][1] == 0
        assert [int(l[2]) for l in lines if l[0] == "U"] == [sc.n_kf - 1, sc.n_kf - 1], "nothing is staged behind the caller's back"
    else:
        assert R[("B", 0)] == (-1, capi.RUMI_E_INVALID)
    assert R[("A", 1)] == ((0, 0) if monocular and not inertial else (-1, capi.RUMI_E_INVALID)), "an empty covisible list is no error"
    K = [l for l in lines if l[0] == "K" and l[1] == "A"]
    assert [int(l[3]) for l in K] == sc.kf_bad.astype(int).tolist() and all(int(l[4]) == 0 for l in K)
    for l, p in zip([l for l in lines if l[0] == "P" and l[1] == "A"], sc.points):
        assert int(l[3]) == int(p[0]) and int(l[4]) == p[1] and int(l[5]) == len(p[2])
