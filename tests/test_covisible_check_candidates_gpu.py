"""rumi::LoopClosingStep::CovisibleCheckResident over several candidates (rumi_slam_amd/facade/LoopClosingStep.h: the covisible check
LoopClosing.cc:773-795 of every candidate that reached it, all (candidate, covisible) searches in one device call) against one call of the
single-candidate member per candidate, which test_sim3_projection_facade_gpu.py holds against the reference's text
(tests/cpp/test_covisible_check_candidates.cc).  Equal per candidate: the covisibles visited, nNumKFs and vpMapPoints; a candidate that
arrives with nNumKFs = 3 visits nothing and keeps its vpMapPoints; a refusal leaves every candidate untouched."""
import os
import subprocess

import pytest

import sim3_projection_scene as P
from test_sim3_projection_facade_gpu import COVISIBLES, E_INVALID, write_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_covisible_check_candidates.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("covis_cands") / "test_covisible_check_candidates")
    build_test(out)
    return out


def run(exe, tmp_path, **kw):
    path = str(tmp_path / "map.bin")
    write_map(path, P.seeded_map(P.SEEDS[0]), **kw)
    r = subprocess.run([exe, path], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return [l.split() for l in r.stdout.splitlines()], r.stderr


def test_covisible_check_candidates_compiles(tmp_path):
    build_test(str(tmp_path / "test_covisible_check_candidates"))


@pytest.mark.gpu
def test_several_candidates_equal_one_call_each(exe, tmp_path):
    lines, err = run(exe, tmp_path)
    side = {tag: [l[2:] for l in lines if l[0] == "C" and l[1] == tag] for tag in "AB"}
    assert len(side["A"]) == 3 and side["A"] == side["B"], (side["A"], side["B"], err[-2000:])
    assert next(l for l in lines if l[0] == "J")[1:] == ["3", "6"]
    first, second, last = side["A"]
    assert first[1:3] == ["4", "3"] and len(first) > 100, "the first candidate: the third valid covisible is the fourth of six"
    assert int(second[1]) >= 3 and len(second) > 100 and second[4:] != first[4:], "the second candidate has its own list"
    assert last[1:3] == ["0", "3"] and last[4:] == ["0", "0", "0"], "nNumKFs = 3 on arrival: nothing visited, vpMapPoints kept"


@pytest.mark.gpu
def test_a_refusal_leaves_every_candidate_untouched(exe, tmp_path):
    lines, err = run(exe, tmp_path, nleft=COVISIBLES[0])
    r = next(l for l in lines if l[0] == "R")
    assert r[2:] == ["-1", str(E_INVALID), "untouched"] and "NLeft != -1" in err, (r, err[-1500:])
    assert not [l for l in lines if l[0] == "C"]
