"""The C++ facade members rumi::LoopClosingStep::SearchByProjectionResident and CovisibleCheckResident (rumi_slam_amd/facade/LoopClosingStep.h)
over a CovisibilityGraph and the mock data model of tests/cpp/mock_model_sim3_projection.h, against the reference's text of
LoopClosing.cc:711-738 and :773-795 over the per-call rumi_facade::ORBmatcher::SearchByProjection on a copy of the same map
(tests/cpp/test_sim3_projection_facade.cc).  Equal afterwards: vpMatchedMP, vpMatchedKF and both counts of every candidate, nNumKFs, the
covisibles visited and the final vpMapPoints; the map itself is untouched on both sides."""
import os
import struct
import subprocess

import numpy as np
import pytest

import sim3_projection_scene as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_CAPACITY = -1, -3
CUR, CANDIDATES = 2, [0, 1]
COVISIBLES = [3, 4, 5, 6, 7, 8]       # of the current key-frame, in covisibility order
OFF_POSE = [4, 8]                     # covisibles stored a metre and a half from where their features were seen: too few matches to be valid


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_sim3_projection_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("s3p_facade") / "test_sim3_projection_facade")
    build_facade_test(out)
    return out


def rot(q):
    x, y, z, w = np.float64(q)
    return np.float64([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def stored_poses(m):
    """GetPose() of every key-frame.  The current key-frame's is (R, t / s) of its Sim3.  A covisible j's is chosen so that
    (Tj * Tc^-1) * Scw (:779-781) searches it under (nearly) the pose its features were generated with; those of OFF_POSE are moved away."""
    q, t, s = m.sim3[CUR]
    Rc, tc = rot(q), np.float64(t) / float(s)
    out = {k: np.float32(kf.Tcw7) for k, kf in enumerate(m.kfs)}
    out[CUR] = np.concatenate([np.float32(q), np.float32(tc)])
    for j in COVISIBLES:
        T7 = np.float64(m.poses[j][0])
        Rjc = rot(T7[:4]) @ Rc.T
        tj = float(s) * (T7[4:] - Rjc @ tc) + Rjc @ tc
        if j in OFF_POSE:
            tj = tj + np.float64([1.5, 0.0, 0.0])
        out[j] = np.concatenate([np.float32(T7[:4]), np.float32(tj)])
    return out


def write_map(path, m, mode=0, nleft=-1, unsynced=-1, unseen=-1):
    poses = stored_poses(m)
    cov = {0: [1], 1: [0], CUR: COVISIBLES}
    with open(path, "wb") as f:
        f.write(struct.pack("<8i", len(m.kfs), m.n_points, nleft, unsynced, unseen, mode, CUR, len(CANDIDATES)))
        for k, kf in enumerate(m.kfs):
            f.write(struct.pack("<i", kf.n) + poses[k].tobytes() + kf.keys.tobytes() + kf.desc.tobytes() + np.int32(kf.row).tobytes())
            c = cov.get(k, [])
            f.write(struct.pack("<i", len(c)) + np.int32(c).tobytes())
        q, t, s = m.sim3[CUR]
        f.write(np.float32(q).tobytes() + np.float32(t).tobytes() + struct.pack("<f", float(s)) + np.int32(CANDIDATES).tobytes())
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
    out = {tag: [" ".join(l[:1] + l[2:]) for l in lines if l[0] in "SC" and l[1] == tag] for tag in "AB"}
    return state, out, lines, r.stderr


def test_sim3_projection_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_sim3_projection_facade"))


@pytest.mark.gpu
def test_members_equal_the_member_text(exe, tmp_path):
    m = P.seeded_map(P.SEEDS[0])
    state, out, lines, err = run(exe, tmp_path, m)
    assert len(out["A"]) == len(CANDIDATES) + 1 and out["A"] == out["B"], (out["A"][-1][:200], out["B"][-1][:200], err[-2000:])
    for l in (x for x in lines if x[0] == "S" and x[1] == "A"):
        assert int(l[3]) > 20 and int(l[4]) > 10, l[:5]
        bar = [i for i, x in enumerate(l) if x == "|"]
        assert len(bar) == 3 and bar[1] - bar[0] - 1 == m.kfs[CUR].n, "vpMatchedMP has the current key-frame's size"
        assert any(x != "-1" for x in l[bar[1] + 1:bar[2]]), "vpMatchedKF is filled"
    # the covisible check: the third valid covisible is the fourth of six, so two were searched speculatively and must not show
    counts = next(l for l in lines if l[0] == "N")
    searched = [int(x) for x in counts[2:counts.index("of")]]
    assert counts[-1] == "6" and len(searched) == 4 and [c >= 30 for c in searched] == [True, False, True, True], counts
    c = next(l for l in lines if l[0] == "C" and l[1] == "A")
    assert c[2:4] == ["4", "3"] and len(c) > 100
    assert state["A"] == state["B"] and len(state["A"]) == len(m.kfs) + m.n_points, "neither side changes the map"


def with_orphan(m):
    """One more point, a copy of point 0 that no key-frame holds: a graph that is given the key-frames only never sees it."""
    m.pos, m.normal, m.desc = np.vstack([m.pos, m.pos[:1]]), np.vstack([m.normal, m.normal[:1]]), np.vstack([m.desc, m.desc[:1]])
    m.min_dist, m.max_dist = np.append(m.min_dist, m.min_dist[0]), np.append(m.max_dist, m.max_dist[0])
    m.bad, m.has_attr = np.append(m.bad, False), np.append(m.has_attr, True)
    return m.n_points - 1


@pytest.mark.gpu
@pytest.mark.parametrize("kw,text,status", [(dict(nleft=CUR), "NLeft != -1", E_INVALID),
                                            (dict(unsynced=CUR), "never seen or without resident features", E_INVALID),
                                            (dict(unseen="orphan"), "a point the graph has never seen", E_INVALID),
                                            (dict(unseen="held"), "searched list entries whose map point has no attributes", E_INVALID),
                                            (dict(mode=2), "RUMI_FUSE_MAX_TARGETS", E_CAPACITY)])
def test_refusals_leave_the_map_and_the_outputs_untouched(exe, tmp_path, kw, text, status):
    """A key-frame's Sync stages the points of its row, so a held point that was never given to the graph is known but has no attributes: the
    device call refuses it.  A point no key-frame holds is refused before anything is uploaded.  641 jobs: the device call fails."""
    m = P.seeded_map(P.SEEDS[0])
    if kw.get("unseen") == "held":
        kw = dict(unseen=next(p for p in m.kfs[0].row if p >= 0 and not m.bad[p]))
    elif kw.get("unseen") == "orphan":
        kw = dict(unseen=with_orphan(m))
    state, out, lines, err = run(exe, tmp_path, m, **kw)
    r = next(l for l in lines if l[0] == "R")
    assert int(r[2]) == -1 and int(r[3]) == status and text in err, (r, err[-1500:])
    assert r[-1] == "untouched" and not out["A"] and not out["B"]
    assert state["A"] == state["B"], "map B was never touched"
