"""The C++ facade CovisibilityGraph (rumi_slam_amd/facade/CovisibilityGraph.h) over the mock data model of tests/cpp/mock_model_covis.h,
against the oracle (tests/cpp/covis_oracle.cc).  The map goes to the test binary in a file; the binary syncs it into a store, runs
UpdateConnections on a list and UpdateLocalMap on frames, and prints what is left on the mock objects: the connection maps of every
key-frame (the listed ones and the ones they connected to), the ordered vectors, parents and children, mvpLocalKeyFrames,
mvpLocalMapPoints, mpReferenceKF, the frame's NULLed points and the stamps.  All of it must equal what the oracle's lists give when the
reference's host side (AddConnection, UpdateBestCovisibles, the member writes, the parent choice) is replayed on them in Python."""
import os
import subprocess

import numpy as np
import pytest

from covis_scene import build_oracle, lm_scenes, oracle_connections, oracle_local_map, random_world
from rumi_slam_amd.covis import EMPTY, NBEST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_facade_test(out):
    fac = os.path.join(ROOT, "rumi_slam_amd", "facade")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", fac, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_covis_facade.cc"), "-L", os.path.join(ROOT, "rumi_slam_amd"), "-lrumi_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "rumi_slam_amd"), "-lpthread", "-o", out])


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("covis_facade")
    exe = str(d / "test_covis_facade")
    build_facade_test(exe)
    return exe, build_oracle(d), d


def timestamps(w):
    return {s: float((s * 37) % 101) for s in w.kf}


def write_map(path, w, batch, frames, cloud=False, refuse=0):
    ts = timestamps(w)
    with open(path, "w") as f:
        f.write(f"{w.max_kf} {w.max_points} {len(w.kf)} {len(w.pt)}\n")
        for s in sorted(w.kf):
            d = w.kf[s]
            row = lambda v: f"{len(v)} " + " ".join(str(x) for x in v)
            f.write(f"{s} {d['key']} {d['map']} {int(d['bad'])} {ts[s]} {int(d['parent'] < 0)} {row(d['mp'])} {row(d['best'])} {d['parent']} {row(d['children'])}\n")
        for p in sorted(w.pt):
            d = w.pt[p]
            f.write(f"{p} {int(d['bad'])} {len(d['obs'])} " + " ".join(str(k) for k in d["obs"]) + "\n")
        f.write(f"{int(cloud)} {len(batch)} " + " ".join(str(s) for s in batch) + f"\n{refuse} {len(frames)}\n")
        for fr in frames:
            f.write(f"{len(fr)} " + " ".join(str(p) for p in fr) + "\n")


def run_facade(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True, env=dict(os.environ, RUMI_NO_TORCH="1"), timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return [[x for x in l.split()] for l in r.stdout.splitlines()], r.stderr


def replay(L, w, batch, cloud):
    """The state the reference's host side leaves, from the oracle's lists: (connection maps, ordered vectors, parent, children, world after)."""
    o = oracle_connections(L, w, batch)
    key, bad, ts = {s: d["key"] for s, d in w.kf.items()}, {s: d["bad"] for s, d in w.kf.items()}, timestamps(w)
    conn = {s: {b: 1000 - j for j, b in enumerate(d["best"])} for s, d in w.kf.items()}
    ordered = {s: [(b, 1000 - j) for j, b in enumerate(d["best"])] for s, d in w.kf.items()}
    parent, children = {s: d["parent"] for s, d in w.kf.items()}, {s: set(d["children"]) for s, d in w.kf.items()}
    first = {s: d["parent"] < 0 for s, d in w.kf.items()}
    init = sorted(w.kf)[0]
    for b, s in enumerate(batch):
        if o["status"][b] == EMPTY:
            continue
        ordl = list(zip(o["ord_slot"][o["ord_off"][b]:o["ord_off"][b + 1]].tolist(), o["ord_weight"][o["ord_off"][b]:o["ord_off"][b + 1]].tolist()))
        for k, wt in ordl:                                             # AddConnection + UpdateBestCovisibles on the other key-frame
            if conn[k].get(s) != wt:
                conn[k][s] = wt
                ordered[k] = [(k2, w2) for w2, _, k2 in sorted(((w2, key[k2], k2) for k2, w2 in conn[k].items()), reverse=True) if not bad[k2]]
        conn[s] = dict(zip(o["conn_slot"][o["conn_off"][b]:o["conn_off"][b + 1]].tolist(), o["conn_count"][o["conn_off"][b]:o["conn_off"][b + 1]].tolist()))
        ordered[s] = ordl
        if first[s] and s != init:
            cands = [k for k, _ in ordl if not cloud or ts[k] < ts[s]]
            if cands:
                parent[s] = cands[0]; children[cands[0]].add(s); first[s] = False
    w2 = w.copy()
    for s, d in w2.kf.items():
        d["best"], d["parent"], d["children"] = [k for k, _ in ordered[s][:NBEST]], parent[s], sorted(children[s])
    return conn, ordered, parent, children, w2


def check(tools, tmp_path, w, batch, frames, cloud):
    exe, L, _ = tools
    path = str(tmp_path / "map.txt")
    write_map(path, w, batch, frames, cloud)
    lines, err = run_facade(exe, path)
    assert [l for l in lines if l[0] in "SU"] == [["S", "0"], ["U", "0"]] and "[rumi]" not in err
    conn, ordered, parent, children, w2 = replay(L, w, batch, cloud)
    key = {s: d["key"] for s, d in w.kf.items()}
    pairs = lambda l: [(int(l[3 + 2 * i]), int(l[4 + 2 * i])) for i in range(int(l[2]))]
    for l in lines:
        s = int(l[1]) if len(l) > 1 else -1
        if l[0] == "K":
            assert int(l[2]) == parent[s] and {int(x) for x in l[5:]} == children[s] and int(l[4]) == len(children[s]), s
        elif l[0] == "C":
            assert pairs(l) == sorted(conn[s].items(), key=lambda kv: key[kv[0]]), s          # std::map order: by address = by key
        elif l[0] == "O":
            assert pairs(l) == ordered[s], s
    assert sum(l[0] == "C" for l in lines) == len(w.kf)
    flat = w2.flat()
    for f, fr in enumerate(frames):
        want = oracle_local_map(L, w2, fr, flat)
        F, Lk, P, N, T = [next(l for l in lines if l[0] == c and int(l[1]) == f) for c in "FLPNT"]
        assert int(F[2]) == 0
        assert [int(x) for x in Lk[2:]] == want["local_kf"].tolist() and [int(x) for x in P[2:]] == want["local_points"].tolist()
        if want["ref_kf"] >= 0:
            assert int(F[3]) == want["ref_kf"] and int(F[4]) == want["ref_kf"]
        assert [int(x) for x in N[2:]] == [-1 if (p < 0 or b) else p for p, b in zip(fr, want["frame_point_bad"])]
        cut = T.index("-2")
        assert sorted(int(x) for x in T[2:cut]) == sorted(want["local_kf"].tolist())
        assert sorted(int(x) for x in T[cut + 1:]) == sorted(want["local_points"].tolist())
    return lines


def test_covis_facade_compiles(tmp_path):
    build_facade_test(str(tmp_path / "test_covis_facade"))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("cloud", [False, True], ids=["plain", "cloud"])
def test_facade_leaves_the_oracles_state(tools, tmp_path, seed, cloud):
    w, frames = random_world(600 + seed, 40, nfeat=(60, 90), n_frames=2)
    rng = np.random.default_rng(seed)
    batch = [int(s) for s in rng.permutation(sorted(w.kf))[:25]] + [int(rng.integers(0, 40))]
    lines = check(tools, tmp_path, w, batch, frames, cloud)
    got_parent = {int(l[1]): int(l[2]) for l in lines if l[0] == "K"}
    assert sum(got_parent[s] != w.kf[s]["parent"] for s in w.kf) >= 1                      # a first connection chose a parent


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["neighbours_and_children", "parent_ends_the_loop", "shared_point_and_own_points"])
def test_facade_on_local_map_scenes(tools, tmp_path, name):
    _, w, frames, expect = next(s for s in lm_scenes() if s[0] == name)
    lines = check(tools, tmp_path, w, [], frames, False)
    assert [int(x) for x in next(l for l in lines if l[0] == "L")[2:]] == expect


@pytest.mark.gpu
@pytest.mark.parametrize("refuse", [1, 2], ids=["vote-from-last-frame", "inertial-sensor"])
def test_facade_refuses_the_inertial_branches(tools, tmp_path, refuse):
    from rumi_slam_amd import capi
    exe, L, _ = tools
    w, frames = random_world(600, 20, nfeat=(30, 40), n_frames=1)
    path = str(tmp_path / "map.txt")
    write_map(path, w, [], frames, False, refuse)
    lines, err = run_facade(exe, path)
    F, Lk, P, N = [next(l for l in lines if l[0] == c) for c in "FLPN"]
    assert int(F[2]) == capi.RUMI_E_INVALID and "[rumi]" in err
    assert Lk[2:] == [] and P[2:] == [] and [int(x) for x in N[2:]] == frames[0] and int(F[3]) == -1
