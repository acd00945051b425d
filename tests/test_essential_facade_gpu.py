"""Optimizer::OptimizeEssentialGraph, both overloads, through facade/shells/Optimizer_essential.cc (compiled against the declarations of
tests/cpp/ref_decls_essential/) over the mock map of tests/cpp/mock_model_essential.h.  The test binary builds a ten-key-frame map that
exercises every gate of the gathering and prints the gathered graph and the map it leaves.  The edge list is compared, in order and count,
with an expectation written by hand from Optimizer.cc:1425-1547 / :1757-1859; poses and points with the oracle (tests/cpp/essential_oracle.cc)
driven by the same gathered graph."""
import os
import subprocess

import numpy as np
import pytest

import essential_scene as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# current = 9, loop = 1, key-frame 4 bad, 8 and 9 corrected.  Loop connections first (std::map order: 8, then 9): (8,1) has weight 60 and is
# dropped, (9,1) has weight 50 but is the (current, loop) pair and stays (:1436), (9,2) has 150.  Then per key-frame: parent, earlier loop
# edges with a smaller id, covisibles of weight >= 100, heaviest first, that are neither parent nor child nor bad, have a smaller id and are
# not in sInsertedEdges.  (7,2) appears twice: once as a loop edge, once as a covisibility edge (the sLoopEdges test is commented out, :1523).
LOOP_EDGES = [(9, 1), (9, 2),
              (1, 0), (2, 1), (3, 2), (3, 1), (5, 7), (5, 2), (6, 3), (6, 2), (7, 6), (7, 2), (7, 2), (8, 7), (8, 6), (9, 8), (9, 7)]
# fixed 0 1 2 (good pose), fixed-corrected 3 4 (good and bad), free 4 (listed again: visited twice) 5 7 8 9 (bad pose), 6 bad, 10 outside.
# (9,1) as a loop edge has no relation (bad-only with good-only); (8,3) is a loop edge and therefore no covisibility edge (:1822).
MERGE_EDGES = [(1, 0), (2, 1), (2, 0), (3, 2), (4, 3), (4, 3), (5, 4), (5, 3), (7, 5), (8, 7), (8, 3), (9, 8), (9, 7)]


def build(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DRUMI_HAVE_SOPHUS=1", "-I", os.path.join(ROOT, "tests", "cpp", "ref_decls_essential"),
           "-I", os.path.join(ROOT, "tests", "cpp"), "-I", os.path.join(ROOT, "include"), "-I", fac,
           os.path.join(ROOT, "tests", "cpp", "test_essential_facade.cc"), os.path.join(fac, "shells", "Optimizer_essential.cc"),
           "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip", "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


def run(exe, which):
    r = subprocess.run([exe, which], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rows = {}
    for l in r.stdout.splitlines():
        t = l.split()
        rows.setdefault(t[0], []).append([float(x) for x in t[1:]])
    return rows, r.stderr


def test_essential_facade_and_shell_compile(tmp_path):
    build(str(tmp_path / "test_essential_facade"))


def gathered(rows):
    V = np.array(rows["V"]); M = np.array(rows["M"])
    ids = V[:, 0].astype(int).tolist()
    E = [(int(a), int(b)) for a, b in rows["E"]]
    sc = es.Scene(V[:, 3:11], V[:, 1], V[:, 2], [ids.index(a) for a, _ in E], [ids.index(b) for _, b in E], M[:, 1:9], None)
    return ids, E, sc


def pose_of(S):
    """g2o::Sim3 [sR t; 0 1] -> SE(3) [R t/s; 0 1] as (q, t)."""
    return np.concatenate([S[:4], S[4:7] / S[7]])


def same_pose(a, b, tol=1e-4):
    q = a[:4] if np.dot(a[:4], b[:4]) >= 0 else -a[:4]
    return np.abs(q - b[:4]).max() < tol and np.abs(a[4:7] - b[4:7]).max() < tol * max(1.0, np.abs(b[4:7]).max())


@pytest.mark.gpu
def test_loop_overload(tmp_path):
    exe = str(tmp_path / "test_essential_facade")
    build(exe)
    rows, _ = run(exe, "loop")
    ids, E, sc = gathered(rows)
    assert E == LOOP_EDGES
    assert ids == [0, 1, 2, 3, 5, 6, 7, 8, 9]                                           # the bad key-frame has no vertex
    assert sc.fixed.tolist() == [1] + [0] * 8 and not sc.fix_scale.any()
    assert abs(sc.S[ids.index(9), 7] - 0.93) < 1e-12 and sc.S[ids.index(3), 7] == 1.0    # CorrectedSim3 where present, else Sim3(R, t, 1)
    ref = es.run_oracle(sc, 20)
    assert rows["T"][0][2] == ref["stats"][2] == 8 and rows["R"][0][0] == 0 and rows["C"][0][0] == 1
    K = {int(r[0]): np.array(r[1:8]) for r in rows["K"]}; O = {int(r[0]): np.array(r[1:8]) for r in rows["O"]}
    for v, i in enumerate(ids):
        assert same_pose(K[i], pose_of(ref["S"][v])), i
    assert np.array_equal(K[4], O[4]) and not same_pose(K[5], O[5], 1e-3)               # the bad one keeps its pose, the others moved
    # points: 0 by its reference key-frame 3, 1 by mnCorrectedReference 8 (corrected by the current key-frame), 2 bad, 3 without a reference, 4 by 9, 5 by 0
    X = np.array(rows["X"])[:, 1:4]; P = np.array(rows["P"])
    refv = np.array([ids.index(3), ids.index(8), -1, -1, ids.index(9), ids.index(0)], np.int32)
    want = es.oracle_correct_points(0, X, refv, sc.S, np.array([es.sinv(S) for S in ref["S"]]))
    assert np.abs(P[:, 1:4] - want).max() <= 1e-4 * np.abs(want).max()
    assert P[:, 4].astype(int).tolist() == [1, 1, 0, 0, 1, 1]                            # UpdateNormalAndDepth once per corrected point
    assert np.array_equal(P[[2, 3], 1:4].astype(np.float32), X[[2, 3]].astype(np.float32))


@pytest.mark.gpu
def test_merge_overload(tmp_path):
    exe = str(tmp_path / "test_essential_facade")
    build(exe)
    rows, err = run(exe, "merge")
    ids, E, sc = gathered(rows)
    assert E == MERGE_EDGES
    assert ids == [0, 1, 2, 3, 4, 5, 7, 8, 9]                                           # 4 once, the bad 6 not at all
    assert sc.fixed.tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0] and sc.fix_scale.tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0]
    ref = es.run_oracle(sc, 20)
    assert rows["T"][0][2] == ref["stats"][2] == 4 and rows["R"][0][0] == 0 and rows["C"][0][0] == 0
    K = {int(r[0]): np.array(r[1:]) for r in rows["K"]}; O = {int(r[0]): np.array(r[1:8]) for r in rows["O"]}
    inv7 = lambda T: es.sinv(np.concatenate([T, [1.0]]))[:7]
    for v, i in enumerate(ids):
        assert same_pose(K[i][:7], pose_of(ref["S"][v])), i
    for i in (4, 5, 7, 8, 9):                                                            # mTwcBefMerge = the inverse of the pose before the call
        assert same_pose(K[i][7:14], inv7(O[i]), 1e-5), i
    assert np.array_equal(K[6][:7], O[6])
    # points: 0 by key-frame 5, 2 by 8, 4 by 4 (bad pose: corrected); 1 by the fixed 1 and 5 by the outsider 10 are left alone; 3 is bad
    X = np.array(rows["X"])[:, 1:4]; P = np.array(rows["P"])
    want = X.copy()
    for p, i in ((0, 5), (2, 8), (4, 4)):
        T = es.smul(np.concatenate([inv7(K[i][:7]), [1.0]]), es.sinv(np.concatenate([K[i][7:14], [1.0]])))
        want[p] = es.smap(T, X[p])
    assert np.abs(P[:, 1:4] - want).max() <= 1e-4 * np.abs(want).max()
    assert P[:, 4].astype(int).tolist() == [1, 0, 1, 0, 1, 0] and "left alone" in err
    assert np.abs(P[0, 1:4] - X[0]).max() > 1e-3
