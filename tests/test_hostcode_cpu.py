"""CPU tests of product host code (no GPU needed): the C-ABI library loads and exports every declared
symbol; the host compilation of code shared with the kernels (sort replay, array quadtree, scalar math)
agrees with the oracle / libm / libstdc++."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from rumi_slam_amd import capi
from rumi_slam_amd.extractor import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    L = capi.lib()
    declared = set()
    for hdr in ("rumi_orb.h", "rumi_testhooks.h", "rumi_match.h", "rumi_opt.h", "rumi_voc.h", "rumi_track.h", "rumi_queue.h", "rumi_dist.h"):
        p = os.path.join(ROOT, "include", hdr)
        if not os.path.exists(p):
            continue
        txt = re.sub(r"/\*.*?\*/", "", open(p).read(), flags=re.S)
        declared |= set(re.findall(r"\b(rumi_[a-z0-9_]+)\s*\(", txt))
    assert declared, "no declarations parsed"
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, f"declared in include/*.h but not exported: {missing}"
    assert set(capi.ORB_SYMBOLS) <= declared


def test_create_without_gpu_fails_loudly():
    L = capi.lib()
    if L.rumi_device_count() > 0:
        pytest.skip("GPU present")
    cfg = capi.RumiOrbConfig(1000, 1.2, 8, 20, 7, 640, 480, 1, -1, 0, 0)
    h = C.c_void_p()
    assert L.rumi_orb_create(C.byref(cfg), C.byref(h)) == capi.RUMI_E_NO_DEVICE
    assert b"no CPU fallback" in L.rumi_last_error()

    # every other handle that allocates when it is created refuses the same way.  (rumi_kfdb_create takes a vocabulary handle, which cannot
    # exist without a device: its check is out of reach here.)
    from rumi_slam_amd.matcher import ORBmatcher
    from rumi_slam_amd.optimizer import Optimizer
    from rumi_slam_amd.queue import RuminationQueue
    from rumi_slam_amd.vocabulary import ORBVocabulary
    from voc_scene import synthetic_vocabulary
    eager = {"matcher": lambda: ORBmatcher(max_features=64, max_queries=64), "optimizer": lambda: Optimizer(64, 4, 4, 64, 64),
             "vocabulary": lambda: ORBVocabulary(*synthetic_vocabulary(0, k=2, L=1)), "queue": lambda: RuminationQueue(1000, 1.2, 8, 20, 7, [0], 1)}
    for name, create in eager.items():
        with pytest.raises(capi.RumiError) as e:
            create()
        assert e.value.code == capi.RUMI_E_NO_DEVICE and "no CPU fallback" in str(e.value), name

    # a handle that binds its device at the first call is created fine, refuses its first well-formed call and the next one alike, and is
    # destroyed without having touched a device
    from covis_scene import World
    from culling_scene import small_batch
    from refresh_scene import capacity_batch
    from rumi_slam_amd.mapping import REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH, KeyFrameCuller, MapPointRefresher
    cull, cb = KeyFrameCuller(), small_batch()
    refresh, rb = MapPointRefresher(), capacity_batch(6)
    w = World(8, 16)
    for s in range(4):
        w.add_kf(s, 10 + s, mp=[s, s + 1, -1], best=[(s + 1) % 4], parent=(s + 3) % 4, children=[(s + 1) % 4])
    for p in range(6):
        w.add_pt(p, [p % 4, (p + 1) % 4])
    store = w.handle()                                               # the edits only write the host mirror
    lazy = {"culler": lambda: cull.status(cb, 0, cb.outputs()),
            "refresher": lambda: refresh.status(rb, REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH, rb.outputs()),
            "covis update_connections": lambda: store.update_connections_into([0, 1], store.connection_outputs(2, 16, 16), 16, 16),
            "covis local_map": lambda: store.local_map_into([0, 1, -1], store.local_map_outputs(3, 8, 16), 8, 16)}
    for name, call in lazy.items():
        for attempt in range(2):
            assert call() == capi.RUMI_E_NO_DEVICE, (name, attempt)
            assert b"no CPU fallback" in L.rumi_last_error(), (name, attempt)
    cull.close(); refresh.close(); store.close()


def test_invalid_config_rejected():
    L = capi.lib()
    h = C.c_void_p()
    for bad in (capi.RumiOrbConfig(0, 1.2, 8, 20, 7, 640, 480, 1, -1, 0, 0), capi.RumiOrbConfig(1000, 1.0, 8, 20, 7, 640, 480, 1, -1, 0, 0),
                capi.RumiOrbConfig(1000, 1.2, 0, 20, 7, 640, 480, 1, -1, 0, 0), capi.RumiOrbConfig(1000, 1.2, 17, 20, 7, 640, 480, 1, -1, 0, 0)):
        assert L.rumi_orb_create(C.byref(bad), C.byref(h)) == capi.RUMI_E_INVALID


@pytest.mark.parametrize("cfg", [(1000, 1.2, 8), (2000, 1.2, 8), (5000, 1.2, 8), (1500, 1.1, 12), (300, 1.5, 4)])
def test_tables_match_oracle(cfg):
    nf, sf, nl = cfg
    a, b = tables(nf, sf, nl), O.OracleExtractor(nf, sf, nl, 20, 7).tables()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_sort_replay_equals_libstdcxx():
    """Ties in (size, UL.x) are ordered by std::sort's algorithm; the oracle calls the real std::sort inside
    its quadtree, the product replays it.  Compare on the quadtree level below and here directly through a
    stable-vs-unstable fingerprint: sorted keys must be ascending and ids a permutation."""
    H = capi.hooks()
    rng = np.random.default_rng(0)
    for n in [0, 1, 2, 15, 16, 17, 18, 33, 100, 257, 1000]:
        for rng_hi in (2, 5, 1000):
            keys = rng.integers(0, rng_hi, n).astype(np.uint32)
            ids = np.arange(n, dtype=np.uint16)
            k2, i2 = keys.copy(), ids.copy()
            assert H.rumi_hook_sort_like_std(capi.ptr(k2), capi.ptr(i2), n) == 0
            assert (np.diff(k2.astype(np.int64)) >= 0).all()
            assert sorted(i2.tolist()) == list(range(n))
            assert np.array_equal(keys[i2], k2)
            k3, i3 = keys.copy(), ids.copy()                     # the real std::sort of the libstdc++ in this image
            assert H.rumi_hook_std_sort(capi.ptr(k3), capi.ptr(i3), n) == 0
            assert np.array_equal(i2, i3), f"tie order differs from std::sort at n={n}"


def _pack(x, y, s):
    return (x.astype(np.uint32) | (y.astype(np.uint32) << 12) | (s.astype(np.uint32) << 24)).astype(np.uint32)


@pytest.mark.parametrize("trial", range(40))
def test_array_quadtree_equals_oracle_list_quadtree(trial):
    """Product quadtree (arrays + replayed sort) vs oracle (std::list + real std::sort): same key-points in the
    same order — including sizes > 16 nodes with many (size, UL.x) ties, where std::sort's tie order matters."""
    H = capi.hooks()
    rng = np.random.default_rng(100 + trial)
    W, Hh = int(rng.integers(60, 700)), int(rng.integers(60, 500))
    if W < Hh // 2:
        W = Hh
    n = int(rng.integers(0, 7000))
    N = int(rng.integers(0, 1200)) if trial % 4 else int(rng.integers(0, 40))
    n = min(n, W * Hh // 2)
    pos = np.sort(rng.choice(W * Hh, n, replace=False)) if n else np.zeros(0, np.int64)
    x, y = (pos % W).astype(np.int64), (pos // W).astype(np.int64)
    s = rng.integers(7, 10 if trial % 5 == 0 else 255, n)
    cand = np.zeros(n, O.KP_DTYPE)
    cand["x"], cand["y"], cand["response"] = x, y, s
    ref = O.octree(cand, 16, 16 + W, 16, 16 + Hh, N)
    packed = _pack(x, y, s)
    out = np.zeros(n + 8, np.int32)
    m = C.c_int32()
    assert H.rumi_hook_quadtree(capi.ptr(packed), n, 16, 16 + W, 16, 16 + Hh, N, capi.ptr(out), len(out), C.byref(m)) == 0
    assert m.value == len(ref)
    sel = out[:m.value]
    assert np.array_equal(x[sel], ref["x"].astype(np.int64)) and np.array_equal(y[sel], ref["y"].astype(np.int64))
    assert np.array_equal(s[sel], ref["response"].astype(np.int64))


def test_restated_sinf_cosf_equal_libm():
    H = capi.hooks()
    libm = C.CDLL("libm.so.6")
    libm.sinf.restype = libm.cosf.restype = C.c_float
    libm.sinf.argtypes = libm.cosf.argtypes = [C.c_float]
    k = np.float32(np.pi / 180.0)
    rng = np.random.default_rng(0)
    degs = np.concatenate([np.arange(0, 360, 0.25, dtype=np.float32), rng.uniform(0, 360, 20000).astype(np.float32),
                           np.float32([0, 1e-5, 45, 90, 180, 270, 359.99997])])
    for d in degs:
        a = float(np.float32(d) * k)
        assert H.rumi_hook_sinf(a) == libm.sinf(a), d
        assert H.rumi_hook_cosf(a) == libm.cosf(a), d


def test_atan2_and_round_equal_oracle():
    H, L = capi.hooks(), O.lib()
    rng = np.random.default_rng(1)
    for _ in range(20000):
        y, x = (float(v) for v in rng.integers(-400000, 400000, 2))
        assert H.rumi_hook_fast_atan2(y, x) == L.orc_fast_atan2(y, x)
    for v in (0.5, 1.5, 2.5, -0.5, -2.5, 7.49999, 1e6 + 0.5):
        assert H.rumi_hook_cv_round(v) == L.orc_cv_round(float(np.float32(v)))


def test_pattern_tables_identical():
    a = open(os.path.join(ROOT, "oracle", "orb_pattern.inc")).read()
    b = open(os.path.join(ROOT, "rumi_slam_amd", "csrc", "orb_pattern.inc")).read()
    assert a == b
    nums = [int(v) for v in re.findall(r"-?\d+", re.sub(r"//.*", "", a))]
    assert len(nums) == 1024 and max(map(abs, nums)) <= 13
    assert nums[:8] == [8, -3, 9, 5, 4, 2, 7, -12]          # first two test pairs of the ORB pattern


def test_divide_free_indexing_is_exact():
    """The FAST cell kernel replaces idx / d by a multiply-shift.  Its index always satisfies idx < 98 * d (an index
    into a tile of at most 98 rows of d elements): exhaustive over that domain."""
    H = capi.hooks()
    for d in range(1, 99):
        for idx in range(0, 98 * d + d):
            assert H.rumi_hook_magic_div(idx, d) == idx // d, (idx, d)


def test_sim3solver_decl_is_minimal():
    """tests/cpp/ref_decls/Sim3Solver.h is a test stand-in, not upstream's header: it may declare only names that
    facade/shells/Sim3Solver.cc defines or touches (no reference text under tests/)."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    decl = open(os.path.join(root, "tests", "cpp", "ref_decls", "Sim3Solver.h")).read()
    shell = open(os.path.join(root, "rumi_slam_amd", "facade", "shells", "Sim3Solver.cc")).read()
    body = decl[decl.index("protected:"):]
    body = re.sub(r"//[^\n]*", "", body)
    members = set(re.findall(r"\b(m[A-Z][A-Za-z0-9]*|mv[A-Za-z0-9]+|mn[A-Za-z0-9]+|mp[A-Za-z0-9]+|ms12i|mt12i|mbFixScale|pCamera[12]|N)\b", body))
    assert len(members) >= 30
    missing = [m for m in sorted(members) if not re.search(r"\b" + re.escape(m) + r"\b", shell)]
    assert not missing, f"declared but never used by the shell: {missing}"
    for helper in ("ComputeCentroid", "ComputeSim3", "CheckInliers", "FromCameraToImage", "mT21i", "mSigma2", "mTh"):
        assert helper not in body


def test_series_form_of_the_se3_exponential(tmp_path):
    """opt_math.h's se3_exp_series (PoseOptimization's oplus: no rotation matrix, no square root, no sin / cos call) against the closed form
    in long double over 200 k random twists, and its hand-over to the general form outside 1e-5 <= theta <= 0.5 (tests/cpp/opt_math_check.cc)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "opt_math_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(root, "rumi_slam_amd", "csrc"),
                    os.path.join(root, "tests", "cpp", "opt_math_check.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
