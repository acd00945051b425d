"""The batch quadtree pipeline (csrc/orb_octree_kernel.hip: k_compact's cell histogram -> k_octree_narrow -> k_octree_redo -> k_oct_select), which
batched calls of more than 256 trees take, and with RUMI_OCT_REGS=0 every batched call.  launch_octree reads RUMI_OCT_REGS and RUMI_OCT_NARROW once
per process, so every test starts child processes (this file, run as a script) as test_keys_in_memory_quadtree does:

  * RUMI_OCT_REGS=0 RUMI_OCT_NARROW=0: the one-launch keys-in-memory kernels stay covered -- every family-B geometry in batches of 5, each case held
    to its expectation and to the oracle (with the default, test_keys_in_memory_quadtree now runs the pipeline);
  * RUMI_OCT_REGS=0: the same batches, and per call the number of trees k_octree_redo took over (rumi_orb_octree_stats) against a prediction made
    here on the CPU: a walk like extract_cases.py's py_octree that reports whether a node of table depth D with more than one key is created in a
    round that is not the last -- the point at which the count tables end and k_octree_narrow hands the tree on.  Two constructed 320 x 240 cases
    with N = 40 (dots spread one to a depth-3 cell: stays in the tables; a lattice of dots 8 px apart among singles: outgrows them) run in one batch that
    interleaves both kinds (issue case infeasible -- 40 dots in one depth-4 cell with N = 30 -- see the note at NC below);
  * handle reuse: two calls with different frames and a shorter third one on ONE handle against fresh handles (stale histogram or list state);
  * no environment: 33 frames of 640 x 480 with 8 levels = 264 trees, just over the 256 that select the batch kernels, byte for byte against a
    second child under RUMI_OCT_NARROW=0, and no tree redone (the performance case rests on that)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import extract_cases as EC
import oracle_lib as O
from rumi_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD_SORT = EC.Prims(O, capi.hooks()).std_sort      # libstdc++'s order of equal (size, UL.x) keys in the fine rounds


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU prediction
# ---------------------------------------------------------------------------------------------------------------------------------
def tab_depth(n_ini, N):
    """oct_tab_depth (csrc/orb_octree.h)."""
    D = 4 if N <= 256 else 5 if N <= 1024 else 6 if N <= 1152 else 5
    while D > 1 and (n_ini << (2 * D)) > 4096:
        D -= 1
    return D


def outgrows_tables(kp, W, H, N, std_sort):
    """DistributeOctTree as py_octree walks it, with the depth of every node: True when a round that is not the last one creates a node of depth
    D = tab_depth with more than one key (its quadrant counts are not in the count tables, and a later round may divide it)."""
    f = np.float32
    nini = EC.c_round(f(W) / f(H))
    D = tab_depth(nini, N)
    hx = f(W) / f(nini)
    roots = [EC._Node(int(hx * f(i)), int(hx * f(i + 1)), 0, H) for i in range(nini)]
    for k, p in enumerate(kp):
        roots[min(int(f(p[0]) / hx), nini - 1)].keys.append(k)
    nodes = [n for n in roots if n.keys]
    for n in nodes:
        n.no_more, n.depth = len(n.keys) == 1, 0

    def children(n):
        out = [q for q in EC._divide(n, kp) if q.keys]
        for q in out:
            q.depth = n.depth + 1
        return out

    fine, open_ = False, []
    while True:
        prev, deep = len(nodes), False
        if not fine:
            open_, front, rest = [], [], []
            for n in nodes:
                if n.no_more:
                    rest.append(n)
                    continue
                for q in children(n):
                    front.insert(0, q)
                    if len(q.keys) > 1:
                        open_.append(q)
                        deep |= q.depth >= D
            nodes = front + rest
            done = len(nodes) >= N or len(nodes) == prev
            fine = not done and len(nodes) + 3 * len(open_) > N
        else:
            keys = [len(n.keys) * 65536 + n.x0 for n in open_]
            order = sorted(range(len(keys)), key=lambda i: keys[i]) if len(set(keys)) == len(keys) else std_sort(keys)
            prev_open, open_ = [open_[i] for i in order], []
            for n in reversed(prev_open):
                for q in children(n):
                    nodes.insert(0, q)
                    if len(q.keys) > 1:
                        open_.append(q)
                        deep |= q.depth >= D
                nodes.remove(n)
                if len(nodes) >= N:
                    break
            done = len(nodes) >= N or len(nodes) == prev
        if done:
            return False
        if deep:
            return True


def frame_outgrows(frame, N, std_sort):
    """A one-level dot frame of family B (flat background EC.B0, single-pixel dots, all detected)."""
    h, w = frame.shape
    ys, xs = np.nonzero(frame != EC.B0)
    pts = EC.cell_major(w, h, [(int(x), int(y), int(frame[y, x]) - EC.B0) for x, y in zip(xs, ys)])
    return outgrows_tables([(p[0] - 16, p[1] - 16, p[2] - 1) for p in pts], w - 32, h - 32, N, std_sort)


# The two constructed cases: 320 x 240, one level, N = 40.  The box is 288 x 208, a cell of depth 3 is 36 x 26, one of depth 4 18 x 13.
# ISSUE CASE INFEASIBLE: the issue describes a cluster of about 40 dots inside ONE depth-4 cell with N = 30.  That cannot be built:
# single-pixel dots must lie 8 px apart to survive the non-maximum suppression, so no 40 of them fit one depth-4 cell; and a cluster alone ends
# the loop at once -- a round that yields one child per node leaves the list as long as it was.  Hence a lattice with singles around it, and N = 40.
NC = 40


def spread_frame():
    """42 dots 41 x 34 px apart: at most one per cell of depth 3, so the list reaches 42 >= N before any node of depth 4 exists."""
    return EC.dots(320, 240, [(22 + 41 * i, 22 + 34 * j, 30 + 3 * ((i + 2 * j) % 7)) for j in range(6) for i in range(7)])


def lattice_frame():
    """42 dots 8 px apart (7 x 6) in the middle and 12 singles around them: the singles keep the list growing while the lattice sits two and
    three to a depth-4 cell, short of N."""
    pts = [(120 + 8 * i, 90 + 8 * j, 30 + 3 * ((2 * i + j) % 7)) for j in range(6) for i in range(7)]
    pts += [(30 + 60 * i, 30, 40 + i) for i in range(5)] + [(30 + 60 * i, 200, 50 + i) for i in range(5)] + [(30, 115, 45), (280, 115, 46)]
    return EC.dots(320, 240, pts)


def test_prediction_on_constructed_cases():
    """The CPU walk itself, without a GPU: the constructed cases are one of each kind."""
    assert not frame_outgrows(spread_frame(), NC, STD_SORT)
    assert frame_outgrows(lattice_frame(), NC, STD_SORT)
    # a single key per root / per child never outgrows anything; a pair inside one depth-4 cell with N far away does not either (the round that
    # would have to divide it changes nothing and is the last)
    assert not outgrows_tables([(10, 10, 30)], 288, 208, 30, STD_SORT)
    assert not outgrows_tables([(10, 10, 30), (14, 10, 30)], 288, 208, 30, STD_SORT)
    # flips keep the kind (the interleaved batch and the handle-reuse calls use them)
    for f in (spread_frame(), lattice_frame()):
        assert len({frame_outgrows(np.ascontiguousarray(g), NC, STD_SORT) for g in (f, f[::-1], f[:, ::-1], f[::-1, ::-1])}) == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# parents
# ---------------------------------------------------------------------------------------------------------------------------------
def child(mode, env_extra, *args, timeout=300):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    for k in ("RUMI_OCT_REGS", "RUMI_OCT_NARROW"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, *args], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"{mode} ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
def test_one_launch_kernels_stay_covered():
    out = child("old", {"RUMI_OCT_REGS": "0", "RUMI_OCT_NARROW": "0"})
    print(out[-400:])


@pytest.mark.gpu
def test_redo_count_against_cpu_prediction():
    out = child("redo", {"RUMI_OCT_REGS": "0"})
    print(out[-800:])


@pytest.mark.gpu
def test_handle_reuse():
    out = child("reuse", {"RUMI_OCT_REGS": "0"})
    print(out[-400:])


@pytest.mark.gpu
def test_natural_route_equals_one_launch_kernel():
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "narrow.npz"), os.path.join(d, "old.npz")
        sa = json.loads(child("natural", {}, a).splitlines()[-2])
        sb = json.loads(child("natural", {"RUMI_OCT_NARROW": "0"}, b).splitlines()[-2])
        print(sa, sb)
        assert sa == {"narrow": 264, "redone": 0} and sb == {"narrow": 0, "redone": 0}
        A, B = np.load(a), np.load(b)
        for k in ("kp", "desc", "counts"):
            assert A[k].tobytes() == B[k].tobytes(), k
        assert int(A["counts"][:, 0].min()) > 500          # real frames, not empty results


# ---------------------------------------------------------------------------------------------------------------------------------
# children
# ---------------------------------------------------------------------------------------------------------------------------------
def _b_groups(T):
    return [(key, [c for c in cases if c.family == "B"]) for key, cases in T.GROUPS.items() if any(c.family == "B" for c in cases)]


def _child_old():
    import test_extractor_cases_gpu as T
    assert os.environ.get("RUMI_OCT_REGS") == "0" and os.environ.get("RUMI_OCT_NARROW") == "0"
    n256 = n512 = 0
    for key, bs in _b_groups(T):
        ext = T.extractor(bs[0])
        T.run_batches(bs, 5, "one-launch keys in memory, batch of 5")
        assert ext.octree_stats() == (0, 0)
        n256 += len(bs) * (key[2] <= 260)
        n512 += len(bs) * (key[2] > 260)
    assert n256 >= 17 and n512 >= 2
    print(f"{n256} cases at 256 threads, {n512} at 512\nold ok")


def _run_frames(T, ext, frames, ctor, lap, who):
    """One batched call of `frames` [(key, frame)], every frame held to the oracle; returns the call's (narrow, redone) and its raw results."""
    import torch
    kp, desc, counts = ext.extract_batch(torch.from_numpy(np.stack([f for _, f in frames])).cuda(), lap)
    stats = ext.octree_stats()
    kp, desc, counts = kp.cpu().numpy(), desc.cpu().numpy(), counts.cpu().numpy()
    raw = []
    for i, (key, frame) in enumerate(frames):
        n = int(counts[i, 0])
        res = EC.Result(int(counts[i, 1]), kp[i, :n].copy().view(T.O.KP_DTYPE).reshape(-1), desc[i, :n].copy(), *T.taps(ext, i))
        T.hold_to_oracle(f"{key}: {who}, frame {i}", res, T.oracle_of((key,) + ctor + lap, frame, ctor, lap), ctor[2])
        raw.append((int(counts[i, 1]), res.kps.tobytes(), res.desc.tobytes()))
    return stats, raw


def _child_redo():
    import test_extractor_cases_gpu as T
    assert os.environ.get("RUMI_OCT_REGS") == "0" and "RUMI_OCT_NARROW" not in os.environ
    std_sort = STD_SORT
    kinds = [0, 0]
    for key, bs in _b_groups(T):
        ext = T.extractor(bs[0])
        calls, orig = [], ext.extract_batch

        def recording(*a, _orig=orig, _ext=ext, _calls=calls, **k):
            r = _orig(*a, **k)
            _calls.append(_ext.octree_stats())
            return r
        ext.extract_batch = recording
        T.run_batches(bs, 5, "pipeline, batch of 5")
        ext.extract_batch = orig
        # run_batches' chunks: five cases each, the last one filled up with flips
        want = []
        for start in range(0, len(bs), 5):
            frames = [c.frame for c in bs[start:start + 5]]
            frames += [f for _, f in T._fillers(bs, 5 - len(frames))]
            want.append(sum(frame_outgrows(f, key[2], std_sort) for f in frames))
        assert len(calls) == len(want)
        for got, w in zip(calls, want):
            assert got == (5 - w, w), (key, calls, want)
            kinds[0] += 5 - w
            kinds[1] += w
    print(f"family B: {kinds[0]} trees from the tables, {kinds[1]} redone")
    # the constructed pair, interleaved: redone trees between finished ones, in one call
    spread, lattice = spread_frame(), lattice_frame()
    ctor, lap = (NC, 1.2, 1, EC.INI, EC.MIN), (0, 1000)
    from rumi_slam_amd.extractor import ORBextractor
    ext = ORBextractor(*ctor, max_width=320, max_height=240, max_batch=16)
    mix = [("spread", spread), ("lattice", lattice), ("spread-flip", np.ascontiguousarray(spread[::-1])), ("lattice-flip", np.ascontiguousarray(lattice[:, ::-1])),
           ("spread", spread), ("lattice", lattice), ("spread", spread)]
    want = sum(frame_outgrows(f, NC, std_sort) for _, f in mix)
    assert [frame_outgrows(f, NC, std_sort) for _, f in mix[:2]] == [False, True] and 2 <= want <= 4
    stats, _ = _run_frames(T, ext, mix, ctor, lap, "interleaved")
    assert stats == (len(mix) - want, want), (stats, want)
    kinds[0] += stats[0]
    kinds[1] += stats[1]
    assert kinds[0] >= 10 and kinds[1] >= 4, kinds       # both kinds occur
    print(f"interleaved: {stats}\nredo ok")


def _child_reuse():
    import test_extractor_cases_gpu as T
    from rumi_slam_amd.extractor import ORBextractor
    assert os.environ.get("RUMI_OCT_REGS") == "0"
    spread, lattice = spread_frame(), lattice_frame()
    ctor, lap = (NC, 1.2, 1, EC.INI, EC.MIN), (0, 1000)
    flip = lambda f: np.ascontiguousarray(f[::-1, ::-1])
    calls = [[("lattice", lattice), ("spread", spread), ("lattice", lattice), ("spread-flip", flip(spread)), ("lattice-flip", flip(lattice)), ("spread", spread)],
             [("spread", spread), ("lattice-flip", flip(lattice)), ("spread-flip", flip(spread)), ("spread", spread), ("lattice", lattice), ("lattice", lattice)],
             [("spread-flip", flip(spread)), ("lattice", lattice), ("spread", spread)]]
    new = lambda: ORBextractor(*ctor, max_width=320, max_height=240, max_batch=16)
    one = new()
    for i, frames in enumerate(calls):
        got = _run_frames(T, one, frames, ctor, lap, f"reused handle, call {i}")
        fresh = _run_frames(T, new(), frames, ctor, lap, f"fresh handle, call {i}")
        assert got == fresh, (i, got[0], fresh[0])
        assert got[0][1] >= 1 and sum(got[0]) == len(frames)
    print("reuse ok")


def _child_natural(path):
    import torch
    from rumi_slam_amd.extractor import ORBextractor
    from rumi_slam_amd.synth import synth_frame
    assert "RUMI_OCT_REGS" not in os.environ
    frames = np.stack([synth_frame(1234 + i) for i in range(33)])
    assert frames.shape == (33, 480, 640)
    ext = ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=33)
    kp, desc, counts = ext.extract_batch(torch.from_numpy(frames).cuda())
    narrow, redone = ext.octree_stats()
    counts = counts.cpu().numpy()
    kp, desc = kp.cpu().numpy(), desc.cpu().numpy()
    for i in range(33):                                   # beyond a frame's count the buffers hold whatever torch.empty left
        kp[i, counts[i, 0]:] = 0
        desc[i, counts[i, 0]:] = 0
    np.savez(path, kp=kp, desc=desc, counts=counts)
    print(json.dumps({"narrow": narrow, "redone": redone}))
    print("natural ok")


if __name__ == "__main__":
    {"old": _child_old, "redo": _child_redo, "reuse": _child_reuse, "natural": _child_natural}[sys.argv[1]](*sys.argv[2:])
