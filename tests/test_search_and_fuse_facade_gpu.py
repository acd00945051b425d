"""The C++ facade rumi::LoopClosingStep::SearchAndFuseResident (rumi_slam_amd/facade/LoopClosingStep.h) over a CovisibilityGraph and the mock
data model of tests/cpp/mock_model_search_and_fuse.h, against the reference's member text (LoopClosing.cc:1996-2065) over the merged
per-key-frame rumi_facade::ORBmatcher::Fuse(pKF, Scw, ...) on a copy of the same map (tests/cpp/test_search_and_fuse_facade.cc).  Equal
afterwards: every key-frame's row, every point's observation map, bad flag, mpReplaced and descriptor, and the nFused totals; a second pass
over the fused map, which the resident member answers from the store its first pass staged, is equal too."""
import os
import struct
import subprocess

import numpy as np
import pytest

import search_and_fuse_scene as F
import search_in_neighbors_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_search_and_fuse_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("saf_facade") / "test_search_and_fuse_facade")
    build_facade_test(out)
    return out


def write_map(path, m, mode=0, nleft=-1, unsynced=-1, unseen=-1):
    """mode 0: the corrected key-frames with their Sim3; mode 1: the key-frame vector overload, each key-frame stored under the pose it is
    searched with; mode 2: the Sim3 list repeated past RUMI_FUSE_MAX_TARGETS.  The reference's list holds no NULL: the -1 entries are dropped."""
    ids = [p for p in m.ids if p >= 0]
    with open(path, "wb") as f:
        f.write(struct.pack("<8i", len(m.kfs), m.n_points, len(m.corrected), len(ids), nleft, unsynced, unseen, mode))
        for k, kf in enumerate(m.kfs):
            T7 = m.poses[k][0] if mode == 1 and k in m.poses else kf.Tcw7
            f.write(struct.pack("<i", kf.n) + np.float32(T7).tobytes() + kf.keys.tobytes() + kf.desc.tobytes() + np.int32(kf.row).tobytes())
        for k in m.corrected:
            q, t, s = m.sim3[k]
            f.write(struct.pack("<i", k) + np.float32(q).tobytes() + np.float32(t).tobytes() + struct.pack("<f", float(s)))
        f.write(np.int32(ids).tobytes())
        for p in range(m.n_points):
            f.write(m.pos[p].tobytes() + m.normal[p].tobytes() + struct.pack("<2f", m.min_dist[p], m.max_dist[p]) + m.desc[p].tobytes()
                    + struct.pack("<i", int(m.bad[p])))


def run(exe, tmp_path, m, **kw):
    path = str(tmp_path / "map.bin")
    write_map(path, m, **kw)
    r = subprocess.run([exe, path], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l.split() for l in r.stdout.splitlines()]
    state = {tag: [" ".join(l[:1] + l[2:]) for l in lines if l[0] in "KP" and l[1] == tag] for tag in "AB"}
    head = {(l[0], l[1]): [int(x) for x in l[2:]] for l in lines if l[0] in "FG"}
    return state, head, r.stderr


def test_search_and_fuse_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_search_and_fuse_facade"))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_member_leaves_the_map_of_the_member_text(exe, tmp_path, mode):
    """Both overloads on the first constructed seed: the Sim3 range, and the key-frame vector searched under GetPose() with scale 1."""
    m = F.seeded_map(F.CONSTRUCTED[0])
    state, head, err = run(exe, tmp_path, m, mode=mode)
    ret, status, again = head["F", "A"]
    assert status == 0 and ret > 60 and head["F", "B"][:2] == [ret, 0], (head, err[-2000:])
    assert again > 0, "loop points whose descriptor a Replace changed were searched again"
    assert len(state["A"]) == len(m.kfs) + m.n_points and state["A"] == state["B"]
    assert any(l.startswith("P") and l.split()[3] != "-1" for l in state["A"]), "a point was replaced"
    assert head["G", "A"][:2] == head["G", "B"][:2] and head["G", "A"][1] == 0, "the second pass, answered from the store the first one staged"


@pytest.mark.gpu
def test_a_second_search_changes_an_outcome(exe, tmp_path):
    """The map of test_search_and_fuse_cpu.py::test_a_changed_descriptor_changes_a_later_search: loop point 0 reaches the second corrected
    key-frame only on the descriptor the Replace after the first left it with."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    b = S.flip_bits(a, 60)
    pts = [S.point_at(200.0, 200.0, 2, a), S.point_at(200.0, 200.0, 2, S.flip_bits(a, 4))]
    feat = lambda xy, d: ([xy], [2], [d])
    m = F.tiny_map(pts, [feat([610.0, 20.0], b), feat([200.5, 200.0], S.flip_bits(a, 4)), feat([200.5, 200.0], S.flip_bits(b, 2))],
                   rows=[[0], [1], None], ids=[0])
    m.corrected = [1, 2]
    m.sim3 = {k: (np.float32([0, 0, 0, 1]), np.zeros(3, np.float32), np.float32(1.0)) for k in m.corrected}
    assert F.expected_call(m)[1].tolist() == [1, 0], "the call-time answers: nothing for the second key-frame"
    state, head, err = run(exe, tmp_path, m)
    assert head["F", "A"] == [2, 0, 1] and head["F", "B"][:2] == [2, 0], (head, err[-2000:])
    assert state["A"] == state["B"]
    p0 = next(l for l in state["A"] if l.startswith("P 0 ")).split()
    assert p0[4] == "3" and p0[5:11] == ["0", "0", "1", "0", "2", "0"], "point 0 is observed by the loop side and both corrected key-frames"


def with_orphan(m):
    """One more loop point, a copy of point 0 that no key-frame holds: a graph that is given the key-frames only never sees it."""
    m.pos, m.normal, m.desc = np.vstack([m.pos, m.pos[:1]]), np.vstack([m.normal, m.normal[:1]]), np.vstack([m.desc, m.desc[:1]])
    m.min_dist, m.max_dist = np.append(m.min_dist, m.min_dist[0]), np.append(m.max_dist, m.max_dist[0])
    m.bad, m.has_attr = np.append(m.bad, False), np.append(m.has_attr, True)
    m.ids.append(m.n_points - 1)
    return m.n_points - 1


@pytest.mark.gpu
@pytest.mark.parametrize("kw,text", [(dict(nleft=3), "NLeft != -1"), (dict(unsynced=3), "never seen or without resident features"),
                                     (dict(unseen="orphan"), "a loop point the graph has never seen"),
                                     (dict(unseen="held"), "1 searched list entries whose map point has no attributes"),
                                     (dict(mode=2), "RUMI_FUSE_MAX_TARGETS")])
def test_refusals_leave_the_map_untouched(exe, tmp_path, kw, text):
    """A key-frame's Sync stages the points of its row, so a held loop point that was never given to the graph is known but has no
    attributes: the device call refuses it.  A loop point no key-frame holds is refused before anything is uploaded."""
    m = F.seeded_map(F.CONSTRUCTED[0])
    if kw.get("unseen") == "held":
        kw = dict(unseen=next(p for p in m.ids if p >= 0 and not m.bad[p]))
    elif kw.get("unseen") == "orphan":
        kw = dict(unseen=with_orphan(m))
    state, head, err = run(exe, tmp_path, m, **kw)
    assert head["F", "A"][:2] == [-1, E_INVALID] and text in err and ("F", "B") not in head
    assert state["A"] == state["B"], "map B was never touched"
