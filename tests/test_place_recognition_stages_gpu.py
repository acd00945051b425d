"""The C++ facade stages rumi_facade::Sim3RansacStage and OptimizeSim3Stage (rumi_slam_amd/facade/PlaceRecognitionStages.h: every candidate of
DetectCommonRegionsFromBoW in one device call each) against the reference's text of LoopClosing.cc:655-676 and :728 over the per-candidate members
(the Sim3Solver shell on rumi_sim3_ransac, Optimizer::OptimizeSim3 on rumi_optimize_sim3), on a second copy of the same scene
(tests/cpp/test_place_recognition_stages.cc).  Equal afterwards: bConverge, the inliers, the estimated R, t, s and g2oS12 byte for byte, the matches
OptimizeSim3 removes, and the next rand()."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_stage_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "cpp", "ref_decls"), "-I", fac, "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_place_recognition_stages.cc"),
           "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip", "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


def test_place_recognition_stages_compile(tmp_path):
    build_stage_test(str(tmp_path / "test_place_recognition_stages"))


@pytest.mark.gpu
def test_stages_equal_the_per_candidate_text(tmp_path):
    exe = str(tmp_path / "test_place_recognition_stages")
    build_stage_test(exe)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failure(s)" in r.stdout
