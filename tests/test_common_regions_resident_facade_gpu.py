"""The C++ facade rumi_facade::CommonRegionsBoWStageResident (rumi_slam_amd/facade/LoopClosingStep.h) through
tests/cpp/test_common_regions_resident_facade.cc: over the mock key-frames of tests/cpp/mock_model_loopclosing.h in a synced graph it must fill
BowStageResult field by field as CommonRegionsBoWStage does by host pointers, with and without member matches, and as LoopClosing.cc:576-651
read literally gives (test_common_regions_facade_gpu.literal); it refuses a member without SyncFeatures; and with one member left unsynced
LoopClosingStep::DetectCommonRegionsFromBoWResident returns the same outputs through the host-pointer stage."""
import os
import subprocess

import pytest

import sim3_projection_scene as P
from test_common_regions_facade_gpu import facade_scene, literal, write_scene
from test_place_recognition_facade_gpu import CUR, REACH, THRESHOLDS, write_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_common_regions_resident_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("crr_facade") / "test_common_regions_resident_facade")
    build_facade_test(out)
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return [l.split() for l in r.stdout.splitlines()], r.stderr


@pytest.mark.gpu
def test_by_slot_stage_equals_the_host_pointer_stage_and_the_literal_loop(exe, tmp_path):
    s, cands, cov, connected, bad_kfs = facade_scene()
    path = str(tmp_path / "scene.bin")
    write_scene(path, s, cands, cov, connected, bad_kfs)
    lines, err = run(exe, "lc", path, -1)
    assert lines[0] == ["E", "with", "equal"] and lines[1] == ["E", "without", "equal"], (lines[:2], err[-1500:])
    want = literal(s, cands, cov, connected, bad_kfs)
    assert [int(x) for x in lines[2][1:]] == [len(want), 0, len(want)]
    rows = {}
    for l in lines[3:]:
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
def test_by_slot_stage_refuses_a_keyframe_without_features(exe, tmp_path, who):
    """-1 returned, nothing handed back, a report on stderr; a member of the first candidate's group, or the current key-frame."""
    s, cands, cov, connected, bad_kfs = facade_scene()
    path = str(tmp_path / "scene.bin")
    write_scene(path, s, cands, cov, connected, bad_kfs)
    lines, err = run(exe, "lc", path, 0 if who == "current" else s.groups[0][4] + 1)
    assert lines == [["R", "-1", str(E_INVALID), "0"]] and "[rumi]" in err and "SyncFeatures" in err, (lines, err[-1500:])


@pytest.mark.gpu
def test_by_slot_stage_refuses_two_camera_keyframes(exe, tmp_path):
    s, cands, cov, connected, bad_kfs = facade_scene()
    path = str(tmp_path / "scene.bin")
    write_scene(path, s, cands, cov, connected, bad_kfs, nleft=s.groups[0][4] + 1)
    lines, err = run(exe, "lc", path, 99)                    # (any unsynced >= 0 prints the by-slot stage's return alone)
    assert lines == [["R", "-1", str(E_INVALID), "0"]] and "NLeft" in err


@pytest.mark.gpu
def test_detect_common_regions_with_one_member_unsynced_takes_the_host_pointer_stage(exe, tmp_path):
    """Graph B lacks the features of candidate 1 (a member of candidate 0's group as well): its call makes no by-slot call and returns what
    graph A's call, which does, returns."""
    path = str(tmp_path / "map.bin")
    m = P.seeded_map(P.SEEDS[0], n_feat=320, n_world=230)
    write_map(path, m, alone=True)
    lines, err = run(exe, "pr", path, *[THRESHOLDS[k] for k in ("nBoWMatches", "nBoWInliers", "nSim3Inliers", "nProjMatches", "nProjOptMatches")], REACH[1])
    stage = {l[1]: int(l[2]) for l in lines if l[0] == "S"}
    assert stage == {"B": E_INVALID, "A": 0}, (stage, err[-1500:])
    d = {l[1]: l[2:] for l in lines if l[0] == "D"}
    assert d["A"] == d["B"], (d["A"][:24], d["B"][:24], err[-2000:])
    assert int(d["A"][0]) >= 0 and d["A"][1] in [str(c) for c in REACH] and d["A"][4] == str(CUR), d["A"][:8]
    # the by-slot stage over the real CovisibilityGraph, with and without member matches, against the host-pointer stage
    e = [l for l in lines if l[0] == "E"]
    assert e == [["E", "with", "equal"], ["E", "without", "equal"]], (e, err[-1500:])
    ret, n_results, matched, dirty = (int(x) for x in next(l for l in lines if l[0] == "N")[1:])
    assert ret == n_results == 3 and matched >= 2 * THRESHOLDS["nBoWMatches"] and dirty == 0, (ret, n_results, matched, dirty)
