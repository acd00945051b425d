"""CovisibilityGraph::SyncPoses / SyncPointMaps (rumi_slam_amd/facade/CovisibilityGraph.h) over the mock data model of
tests/cpp/mock_model_lba_resident.h: the two members stage on the host, so the C++ program reads back what they left in the store's mirror
and needs no device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sync_poses_and_point_maps(tmp_path):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    exe = str(tmp_path / "test_lba_resident_sync_facade")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_lba_resident_sync_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("done 0"), r.stdout + r.stderr[-2000:]
