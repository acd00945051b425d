"""rumi_facade::TrackLocalMapResident (rumi_slam_amd/facade/TrackingStep.h) and the attribute members of CovisibilityGraph
(facade/CovisibilityGraph.h) on the mock model of tests/cpp/mock_model_localmap.h: the test binary (tests/cpp/test_localmap_facade.cc)
compares the member state the resident call leaves with that of UpdateLocalMap() + the existing TrackLocalMap step, and the bytes uploaded
after a SetWorldPos on one point."""
import os
import subprocess

import pytest

from rumi_slam_amd.synth import synth_frame, warp_homography
from test_tracking_loop_gpu import _homography, _pose_gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_localmap_facade.cc"), os.path.join(fac, "ORBextractor.cc"),
                           "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip", "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out])


def test_localmap_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_localmap_facade"))


@pytest.mark.gpu
def test_resident_call_leaves_the_two_step_state(tmp_path):
    exe = str(tmp_path / "test_localmap_facade")
    build_facade_test(exe)
    img0 = synth_frame(4242)
    frames = []
    for k, img in enumerate((img0, warp_homography(img0, _homography(*_pose_gt(2))))):
        frames.append(str(tmp_path / f"frame{k}.bin"))
        img.tofile(frames[-1])
    r = subprocess.run([exe] + frames, capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "FAIL" not in r.stdout and "localmap facade OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[rumi]" not in r.stderr, r.stderr[-2000:]
