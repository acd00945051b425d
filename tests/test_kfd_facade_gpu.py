"""Builds tests/cpp/test_kfd_facade.cc (the facade KFDSample over the mock cv types) against librumi_hip.so and runs it on the GPU: the 8-frame
sequence of tests/kfd_scene.py, decisions and GetAllKF().size() against the oracle's."""
import os
import subprocess

import pytest

import kfd_scene as ks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", fac, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_kfd_facade.cc"), os.path.join(fac, "ORBextractor.cc"),
                           "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip", "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out])


def test_kfd_facade_compiles(tmp_path):
    _build(str(tmp_path / "test_kfd_facade"))                   # CPU: KFDSample.h compiles and links against the mock cv types


@pytest.mark.gpu
def test_kfd_facade_against_oracle(tmp_path):
    import oracle_lib
    exe = str(tmp_path / "test_kfd_facade")
    _build(exe)
    w, h = 160, 128
    frames = ks.sequence(w, h)
    ex = oracle_lib.OracleExtractor(300, 1.2, 4, 20, 7)
    o = ks.OracleSampler(ks.build_oracle(tmp_path), lambda grey: ex.extract(grey, (0, 0)), *ks.SEQ_PD)
    decisions, args = "", []
    for k, f in enumerate(frames):
        decisions += "1" if o.step(f, ks.SEQ_TIMES[k])[0].selected else "0"
        name = str(tmp_path / f"f{k}.bin")
        f.tofile(name)
        args += [name, repr(ks.SEQ_TIMES[k])]
    assert "1" in decisions[1:] and "0" in decisions
    r = subprocess.run([exe, str(w), str(h), decisions] + args, capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
