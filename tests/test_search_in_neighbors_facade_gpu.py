"""The C++ facade rumi::LocalMappingStep::SearchInNeighborsResident (rumi_slam_amd/facade/LocalMappingStep.h) over a CovisibilityGraph and the
mock data model of tests/cpp/mock_model_search_in_neighbors.h, against the reference's member text over the merged per-target
rumi_facade::ORBmatcher::Fuse on a copy of the same map (tests/cpp/test_search_in_neighbors_facade.cc).  Equal afterwards: every key-frame's
row, every point's observation map, bad flag, mpReplaced and descriptor, the nFused totals, the covisibility vectors after UpdateConnections;
then KeyFrameCulling by slot on the first map against the block member on the second, which passes its on-device consistency check only
if the replay kept the store current."""
import os
import struct
import subprocess

import numpy as np
import pytest

import search_in_neighbors_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_search_in_neighbors_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sin_facade") / "test_search_in_neighbors_facade")
    build_facade_test(out)
    return out


def write_map(path, m, abort=0, inertial=0, nleft=-1, unsynced=-1):
    """Key-frame 0 lists the targets as its covisibles, key-frame 1 lists key-frame 0 and the rest: the second neighbours of :662-677."""
    nk = len(m.kfs)
    with open(path, "wb") as f:
        f.write(struct.pack("<8i", nk, m.n_points, abort, inertial, nleft, unsynced, 0, 0))
        for k, kf in enumerate(m.kfs):
            cov = list(range(1, 1 + m.n_targets)) if k == 0 else ([0] + list(range(1 + m.n_targets, nk)) if k == 1 else [])
            f.write(struct.pack("<i", kf.n) + np.float32(kf.Tcw7).tobytes() + kf.keys.tobytes() + kf.desc.tobytes() + np.int32(kf.row).tobytes())
            f.write(struct.pack("<i", len(cov)) + np.int32(cov).tobytes())
        for p in range(m.n_points):
            f.write(m.pos[p].tobytes() + m.normal[p].tobytes() + struct.pack("<2f", m.min_dist[p], m.max_dist[p]) + m.desc[p].tobytes()
                    + struct.pack("<i", int(m.bad[p])))


def run(exe, tmp_path, m, **kw):
    path = str(tmp_path / "map.bin")
    write_map(path, m, **kw)
    r = subprocess.run([exe, path], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l.split() for l in r.stdout.splitlines()]
    state = {tag: [" ".join(l[:1] + l[2:]) for l in lines if l[0] in "KVP" and l[1] == tag] for tag in "AB"}
    head = {(l[0], l[1]): [int(x) for x in l[2:]] for l in lines if l[0] in "FTC"}
    return state, head, r.stderr


def test_search_in_neighbors_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_search_in_neighbors_facade"))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,nt", S.CONSTRUCTED[:2])
def test_member_leaves_the_map_of_the_member_text(exe, tmp_path, seed, nt):
    m = S.seeded_map(seed, nt)
    state, head, err = run(exe, tmp_path, m)
    assert head["T", "A"] == head["T", "B"] == [len(m.kfs) - 1], "the covisibles and the second neighbours"
    ret, status, again, contra = head["F", "A"]
    assert status == 0 and contra == 0 and ret > 100 and head["F", "B"][:2] == [ret, 0], (head, err[-2000:])
    assert again > 0, "survivors whose descriptor changed were searched again"
    assert len(state["A"]) == 2 * len(m.kfs) + m.n_points and state["A"] == state["B"]
    assert any(l.startswith("P") and l.split()[3] != "-1" for l in state["A"]), "a point was replaced"
    assert head["C", "A"] == head["C", "B"] and head["C", "A"][1] == 0, "the store was current: the culling's consistency check passed"


@pytest.mark.gpu
def test_a_second_search_changes_an_outcome(exe, tmp_path):
    """The map of test_search_in_neighbors_cpu.py::test_a_changed_descriptor_changes_a_later_search: point 0 reaches target 2 only on the
    descriptor the Replace in target 1 left it with."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    b = S.flip_bits(a, 60)
    pts = [S.point_at(200.0, 200.0, 2, a), S.point_at(200.0, 200.0, 2, S.flip_bits(a, 4))]
    feat = lambda d: ([[200.5, 200.0]], [2], [d])
    m = S.tiny_map(pts, [feat(S.flip_bits(a, 4)), feat(S.flip_bits(b, 2))], extra_rows=[[1], None])
    m.kfs[0].row[1] = -1
    m.kfs[0].desc[0] = b
    assert S.expected_call(m)[0][1][0] == -1, "the call-time answer for (target 2, point 0)"
    state, head, err = run(exe, tmp_path, m)
    assert head["F", "A"] == [2, 0, 1, 0] and head["F", "B"][:2] == [2, 0], (head, err[-2000:])
    assert state["A"] == state["B"]
    p0 = next(l for l in state["A"] if l.startswith("P 0 ")).split()
    assert p0[4] == "3" and p0[5:11] == ["0", "0", "1", "0", "2", "0"], "point 0 is observed by the current key-frame and both targets"


@pytest.mark.gpu
def test_abort_after_the_forward_pass(exe, tmp_path):
    m = S.seeded_map(S.CONSTRUCTED[0][0], S.CONSTRUCTED[0][1])
    full, _, _ = run(exe, tmp_path, m)
    state, head, err = run(exe, tmp_path, m, abort=1)
    assert head["F", "A"][1] == 0 and head["F", "A"][0] == head["F", "B"][0] > 20 and head["T", "A"] == head["T", "B"]
    assert state["A"] == state["B"] and state["A"] != full["A"], "no reverse pass, no UpdateConnections"
    assert head["C", "A"] == head["C", "B"] and head["C", "A"][1] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kw,text", [(dict(inertial=1), "mbInertial"), (dict(nleft=2), "NLeft != -1"), (dict(unsynced=2), "never seen or without resident features")])
def test_refusals_leave_the_map_untouched(exe, tmp_path, kw, text):
    m = S.seeded_map(S.CONSTRUCTED[0][0], S.CONSTRUCTED[0][1])
    state, head, err = run(exe, tmp_path, m, **kw)
    assert head["F", "A"][:2] == [-1, E_INVALID] and text in err and ("F", "B") not in head
    assert head["T", "A"] == [0], "no key-frame was stamped"
    assert state["A"] == state["B"], "map B was never touched"
