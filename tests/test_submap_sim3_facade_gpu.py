"""The C++ facade member rumi_facade::ComputeSubmapSim3 (rumi_slam_amd/facade/CloudMergingStep.h, with RUMI_HAVE_SOPHUS) over the mock maps of
tests/cpp/mock_model_submap_sim3.h, against the same function composed in tests/cpp/test_submap_sim3_facade.cc from the per-call path (the shell's
Sim3Solver in blocks of 20, rumi_facade::ComputeInliersNum, Optimizer::OptimizeCloudSim3) with the same order, srand and Umeyama stub."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "cpp", "ref_decls"), "-I", fac, "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "test_submap_sim3_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"),
           "-lrumi_hip", "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


def test_submap_sim3_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_submap_sim3_facade"))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("submap_sim3_facade") / "test_submap_sim3_facade")
    build_facade_test(out)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["converge", "noconverge", "nleft"])
def test_submap_sim3_facade_equals_the_per_call_path(exe, scene):
    r = subprocess.run([exe, scene], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and f"submap sim3 facade ({scene}): 0 failure(s)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    if scene == "nleft":
        assert "[rumi]" in r.stderr and "NLeft" in r.stderr
