"""Builds tests/cpp/test_stream_facade.cc (rumi_facade::FrameStream over the mock cv types) against librumi_hip.so and runs it on the GPU: Push
on three frames against the C entries."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", fac, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_stream_facade.cc"), os.path.join(fac, "ORBextractor.cc"),
                           "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip", "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out])


def test_stream_facade_compiles(tmp_path):
    _build(str(tmp_path / "test_stream_facade"))                # CPU: FrameStream.h compiles and links against the mock cv types


@pytest.mark.gpu
def test_stream_facade_against_c_entry(tmp_path):
    from rumi_slam_amd.synth import synth_frame, warp_frame
    exe = str(tmp_path / "test_stream_facade")
    _build(exe)
    img = synth_frame(4300, w=320, h=240, n_rect=150)
    names = []
    for k in range(3):
        names.append(str(tmp_path / f"f{k}.bin"))
        img.tofile(names[-1])
        img = warp_frame(img, 40 + k)[0]
    r = subprocess.run([exe] + names, capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
