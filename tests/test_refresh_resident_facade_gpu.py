"""The C++ facade rumi_facade::RefreshMapPointsResident and the resident forms of the two LocalMapping loops
(rumi_slam_amd/facade/MapPointRefresh.h) over a CovisibilityGraph and the mock data model of tests/cpp/mock_model_refresh_resident.h.  The test
binary loads one map twice, refreshes one copy through the graph and the other through rumi_facade::RefreshMapPoints (whose members
tests/test_refresh_facade_gpu.py checks against the oracle), and compares the members it reads back from the mock points in process, bit for
bit; it also reads the store's attribute records back and compares them with those members."""
import os
import subprocess

import pytest

from refresh_scene import RefreshScene
from test_refresh_facade_gpu import write_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_refresh_resident_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


def test_refresh_resident_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_refresh_resident_facade"))


@pytest.mark.gpu
def test_refresh_resident_facade_equals_block_facade(tmp_path):
    exe = str(tmp_path / "test_refresh_resident_facade")
    build_facade_test(exe)
    s = RefreshScene(20, 340, 120, 150)
    path = str(tmp_path / "map.bin")
    write_map(path, s)
    r = subprocess.run([exe, path], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    equal = {l.split()[1]: int(l.split()[2]) for l in r.stdout.splitlines() if l.startswith("E ")}
    assert equal == {"all": len(s.points), "associate": len(s.points), "keyframe": len(s.points)}, r.stdout[-2000:]
    assert "FAIL" not in r.stdout


def test_refresh_header_compiles_on_its_own(tmp_path):
    """facade/MapPointRefresh.h names every standard header it uses: a translation unit that includes nothing else before it compiles."""
    src = tmp_path / "alone.cc"
    src.write_text('#define RUMI_HAVE_SOPHUS 1\n#include "mock_sophus.h"\n#include "MapPointRefresh.h"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "rumi_slam_amd", "facade"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), str(src)])
