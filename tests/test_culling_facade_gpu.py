"""The C++ facade LocalMappingStep::KeyFrameCulling / CloudKeyFrameCulling (rumi_slam_amd/facade/LocalMappingStep.h) over the mock data
model of tests/cpp/mock_model_culling.h, against the oracle (tests/cpp/culling_oracle.cc).  The map goes to the test binary in a file; the
binary runs the member once on mock objects whose SetBadFlag / EraseObservation are written as the reference's, and prints the map that is
left: bad key-frames, mbToBeErased, every key-frame's slots, every point's observation map, nObs and bad flag.  All of it must equal the map
the oracle's loop leaves."""
import os
import struct
import subprocess

import numpy as np
import pytest

from culling_scene import SCENES, CullScene, build_oracle, run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_culling_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out]
    subprocess.check_call(cmd)


def write_map(path, s, cloud, inertial=False, monocular=True, stereo_kf=-1):
    with open(path, "wb") as f:
        f.write(struct.pack("<8i", s.n_kf, len(s.points), len(s.cand), int(cloud), int(s.abort_ba), int(inertial), int(monocular), stereo_kf))
        for k in range(s.n_kf):
            f.write(struct.pack("<5i", int(s.n[k]), int(s.kf_bad[k]), int(s.kf_init[k]), int(s.not_erase[k]), int(s.cloud[k])))
            f.write(s.octave[k].astype("<i4").tobytes())
        for bad, n, obs in s.points:
            f.write(struct.pack("<3i", int(bad), n, len(obs)))
            f.write(np.array(obs, np.int32).reshape(-1, 2).astype("<i4").tobytes())
        f.write(np.array(s.cand, "<i4").tobytes())


def run_facade(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l.split() for l in r.stdout.splitlines()]
    ret = next(l for l in lines if l[0] == "R")
    return int(ret[1]), int(ret[2]), lines, r.stderr


def test_culling_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_culling_facade"))


@pytest.mark.gpu
@pytest.mark.parametrize("scene", [s for s in SCENES if s[1] > 0], ids=lambda s: f"scene{s[0]}-{s[1]}")
@pytest.mark.parametrize("cloud", [False, True], ids=["plain", "cloud"])
def test_culling_facade_leaves_the_oracles_map(tmp_path, scene, cloud):
    exe = str(tmp_path / "test_culling_facade")
    build_facade_test(exe)
    s = CullScene(*scene)
    path = str(tmp_path / "map.bin")
    write_map(path, s, cloud)
    ret, status, lines, _ = run_facade(exe, path)
    out, st = run_oracle(build_oracle(tmp_path), s.batch(), s.flags(cloud), state=True)
    assert ret == int(out["n_culled"][0]) and status == 0
    K = [l for l in lines if l[0] == "K"]
    M = [l for l in lines if l[0] == "M"]
    P = [l for l in lines if l[0] == "P"]
    assert len(K) == s.n_kf and len(P) == len(s.points)
    assert [int(l[2]) for l in K] == st["kf_bad"][:s.n_kf].tolist()                    # the set of bad key-frames
    assert [int(l[3]) for l in K] == st["kf_to_be_erased"][:s.n_kf].tolist()           # mbToBeErased
    assert all(int(l[4]) == 1 for l in K)                                                # UpdateBestCovisibles, once (:959)
    for k, l in enumerate(M):
        assert [int(x) for x in l[2:]] == st["mp_after"][k].tolist(), k
    b = s.batch()
    for i, l in enumerate(P):
        assert int(l[2]) == st["pt_bad"][i] and int(l[3]) == st["pt_nobs"][i], i
        n = int(l[4])
        got = {(int(l[5 + 2 * j]), int(l[6 + 2 * j])) for j in range(n)}
        o0 = int(b.pts["obs_begin"][i])
        assert got == {o for j, o in enumerate(s.points[i][2]) if st["obs_in_map"][o0 + j]}, i
    if cloud:                                                                            # the cloud variant leaves cloud key-frames alone
        for k in range(s.n_kf):
            if s.cloud[k]:
                assert int(K[k][2]) == int(s.kf_bad[k]) and int(K[k][3]) == 0
    assert st["kf_bad"][:s.n_kf].sum() > s.kf_bad.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("inertial,monocular,stereo_kf", [(True, True, -1), (False, False, -1), (False, True, 3)],
                         ids=["inertial", "stereo-sensor", "NLeft"])
def test_culling_facade_refuses_what_is_not_built(tmp_path, inertial, monocular, stereo_kf):
    """Refused with a report and the refusal status; the map is left as it was."""
    from rumi_slam_amd import capi
    exe = str(tmp_path / "test_culling_facade")
    build_facade_test(exe)
    s = CullScene(*SCENES[0])
    if stereo_kf >= 0:
        stereo_kf = s.cand[stereo_kf]
    path = str(tmp_path / "map.bin")
    write_map(path, s, False, inertial, monocular, stereo_kf)
    ret, status, lines, err = run_facade(exe, path)
    assert ret == -1 and status == capi.RUMI_E_INVALID and "[rumi]" in err
    assert [int(l[2]) for l in lines if l[0] == "K"] == s.kf_bad.astype(int).tolist()
    assert all(int(l[3]) == 0 for l in lines if l[0] == "K")
    for l, p in zip([l for l in lines if l[0] == "P"], s.points):
        assert int(l[2]) == int(p[0]) and int(l[3]) == p[1] and int(l[4]) == len(p[2])
