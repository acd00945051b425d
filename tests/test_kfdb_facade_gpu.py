"""The C++ facade rumi_facade::KeyFrameDatabaseT (rumi_slam_amd/facade/KeyFrameDatabase.h) over the mock data model of
tests/cpp/test_kfdb_facade.cc, against the oracle (tests/cpp/kfdb_oracle.cc) on the same call sequence: adds, queries, covisibility changes
between queries, a map merge, a bad map, erases and a clearMap."""
import os
import subprocess

import pytest

from kfdb_scene import build_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_kfdb_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_kfdb_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


def strip_scored(line):
    """oracle line without its scored (id:si) section: "R qid | cand" / "N qid | loop | merge" """
    f = line.split("|")
    return "|".join([f[0]] + f[2:])


def test_kfdb_facade_compiles(tmp_path):
    build_kfdb_facade_test(str(tmp_path / "test_kfdb_facade"))


@pytest.mark.gpu
def test_kfdb_facade_against_oracle(tmp_path):
    exe = str(tmp_path / "test_kfdb_facade")
    build_kfdb_facade_test(exe)
    script = str(tmp_path / "script.txt")
    env = dict(os.environ, RUMI_NO_TORCH="1")
    r = subprocess.run([exe, script], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.splitlines()
    oracle = build_oracle(tmp_path)
    with open(script) as f:
        o = subprocess.run([oracle], stdin=f, capture_output=True, text=True, timeout=300)
    assert o.returncode == 0, o.stderr
    want = [strip_scored(l) for l in o.stdout.splitlines()]
    assert len(got) == len(want) > 100
    assert sum(1 for l in want if l.split("|")[1].split()) > 30           # the queries do find candidates
    for g, w in zip(got, want):
        assert g.split() == w.split()
