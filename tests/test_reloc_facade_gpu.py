"""rumi_facade::Relocalization (rumi_slam_amd/facade/TrackingStep.h) over the mock data model and the scripted solver of
tests/cpp/test_reloc_facade.cc, against a per-hypothesis replay of the single-entry facade members in the control flow of Tracking.cc:3226-3348:
return value, mvpMapPoints, mvbOutlier with its layers, pose and the solver's step counts, with speculateRound on and off."""
import subprocess

import pytest

from rumi_slam_amd.synth import synth_frame
from test_facade_gpu import build_facade_test


def test_reloc_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_reloc_facade"), "test_reloc_facade.cc")


@pytest.mark.gpu
def test_reloc_facade(tmp_path):
    exe = str(tmp_path / "test_reloc_facade")
    build_facade_test(exe, "test_reloc_facade.cc")
    img = tmp_path / "frame.bin"
    synth_frame(7).tofile(str(img))
    r = subprocess.run([exe, str(img)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "reloc facade ok" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
