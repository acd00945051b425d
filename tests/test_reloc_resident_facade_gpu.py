"""rumi_facade::ComputeBoWResident and rumi_facade::RelocalizationResident (rumi_slam_amd/facade/TrackingStep.h) over the mock data model, a
CovisibilityGraph and the scripted solver of tests/cpp/test_reloc_resident_facade.cc, against rumi_facade::Relocalization on a copy of the same
frame: return value, mvpMapPoints, mvbOutlier, pose, the solver's step counts and TrackStep's counters, with speculateRound on and off; the -1
paths leave the frame untouched."""
import subprocess

import pytest

import voc_scene
from rumi_slam_amd.synth import synth_frame
from test_facade_gpu import build_facade_test


def test_reloc_resident_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_reloc_resident_facade"), "test_reloc_resident_facade.cc")


@pytest.mark.gpu
def test_reloc_resident_facade(tmp_path):
    exe = str(tmp_path / "test_reloc_resident_facade")
    build_facade_test(exe, "test_reloc_resident_facade.cc")
    img = tmp_path / "frame.bin"
    synth_frame(7).tofile(str(img))
    voc = tmp_path / "voc.txt"
    voc_scene.write_text(str(voc), voc_scene.synthetic_vocabulary(3, 10, 3), 10, 3)
    r = subprocess.run([exe, str(img), str(voc)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "reloc resident facade ok" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
