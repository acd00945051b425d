"""The C++ facade rumi::LocalMappingStep::CreateNewMapPointsResident (rumi_slam_amd/facade/LocalMappingStep.h) with the key-frames staged through
CovisibilityGraph::Sync / SyncFeatures / SyncAttributes (facade/CovisibilityGraph.h), over the mock data model of
tests/cpp/mock_model_newpoints_resident.h, against the oracle on the same scene.  The scene file, the K / P / Q lines and the comparison are
those of tests/test_newpoints_facade_gpu.py; R is the call made while one neighbour's features had not been synced, U the feature bytes a
second call on the same graph uploaded."""
import os
import subprocess

import numpy as np
import pytest

from newpoints_scene import K_TUM3, SF, TH_FAR, H, W, NewPointsScene, build_oracle, params, run_oracle
from test_newpoints_facade_gpu import _floats, write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_newpoints_resident_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


def test_newpoints_resident_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_newpoints_resident_facade"))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,nn,nf,coarse,ori,far,stop", [(50, 30, 1000, 0, 0, 0, 4), (51, 7, 1000, 1, 1, 1, 2)])
def test_newpoints_resident_facade_against_oracle(tmp_path, seed, nn, nf, coarse, ori, far, stop):
    from rumi_slam_amd import capi
    from rumi_slam_amd.mapping import KeyFrameView
    from rumi_slam_amd.matcher import FeatureVector, FrameView
    exe = str(tmp_path / "test_newpoints_resident_facade")
    build_facade_test(exe)
    s = NewPointsScene(seed, nn, nf)
    scene = str(tmp_path / "scene.bin")
    write_scene(scene, s, coarse, ori, far)
    r = subprocess.run([exe, scene, str(stop)], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=300)
    assert r.returncode == 0, "\n".join(l for l in r.stdout.splitlines() if not l.startswith(("K ", "P "))) + r.stderr[-3000:]
    lines = [l.split() for l in r.stdout.splitlines()]
    poses = {int(l[1]): _floats(l[2:]) for l in lines if l[0] == "K"}
    assert len(poses) == nn + 1
    views = []
    for k, v in enumerate(s.views):
        p = poses[k]
        views.append(KeyFrameView(FrameView(v["keys"], v["desc"], W, H, SF), FeatureVector.from_csr(*v["fv"]), v["kf_mp"], K_TUM3, p[:12], p[12:15],
                                  v["mp_pos"] if k else None, p[15:24], p[24:26]))
    want = run_oracle(build_oracle(tmp_path), views[0], views[1:], params(coarse, ori, far, TH_FAR))
    got = [l for l in lines if l[0] == "P"]
    assert len(got) == len(want["points"]) > 100
    for g, w in zip(got, want["points"]):
        assert [int(x) for x in g[1:4]] == [int(w["neigh"]), int(w["idx1"]), int(w["idx2"])]
        assert _floats(g[4:7]).tobytes() == w["x3D"].tobytes()
    q = [l for l in lines if l[0] == "Q"]
    assert len(q) == 1 and int(q[0][1]) == stop and int(q[0][2]) == int(want["per_neigh"][:stop].sum()) > 0
    refused = [l for l in lines if l[0] == "R"]
    assert len(refused) == 1 and int(refused[0][1]) == capi.RUMI_E_INVALID and int(refused[0][2]) == 0
    assert "without resident features" in r.stderr
    u = [l for l in lines if l[0] == "U"]
    assert len(u) == 1 and int(u[0][1]) == 0
