"""rumi_track_reloc_begin / rumi_track_reloc_refine (include/rumi_track.h): Tracking::Relocalization's refine chain (R/lib_src/Tracking.cc:3287-3345)
of every pose hypothesis of a round in one call, on the constructed cases of reloc_cases.py.

  byte equality   each case alone (H = 1) equals the chain of single entries through the mirrors -- rumi_pose_optimization and
                  rumi_search_by_projection_reloc -- in frame_mp, outlier_last, every field of RumiRelocResult, Tcw bit for bit
  oracle parity   against reloc_cases.chain_oracle: masks, counts, frame_mp and flags identical, Tcw within 1e-4 relative
  batching        all cases as hypotheses of one call equal each alone, also in reversed order
and session reuse, the size boundaries, the candidate-list arena and the refusals."""
import numpy as np
import pytest

import reloc_cases as R
from rumi_slam_amd import capi
from rumi_slam_amd import tracker as TR
from scene import K_TUM3

pytestmark = pytest.mark.gpu

CASES, PTS = R.scene()
NAMES = list(CASES)
INDEX = {n: k for k, n in enumerate(NAMES)}


def _cand(case, n):
    return dict(kf_keys=case["kf_keys"], kf_mp=case["kf_mp"], matches=case["matches"][:n])


class Rig:
    def __init__(self):
        from rumi_slam_amd.matcher import FrameView, ORBmatcher
        from rumi_slam_amd.optimizer import Optimizer
        F = R.frame()
        self.t = TR.Tracker(R.NFEATURES, 1.2, R.NLEVELS, 20, 7, R.W, R.H, max_points=8192)
        _, keys, desc = self.t.extract(F["img"])
        assert keys.tobytes() == F["keys"].tobytes() and np.array_equal(desc, F["desc"]), "the resident frame is the cases' frame"
        self.n = len(keys)
        self.opt = Optimizer()
        self.match = {ori: ORBmatcher(0.9, bool(ori), max_features=2048, max_queries=8192) for ori in (0, 1)}
        self.cur = FrameView(F["keys"], F["desc"], R.W, R.H, F["sf"])
        self.begin_all()
        self._single, self._chain = {}, {}

    def begin_all(self):
        self.t.reloc_begin(K_TUM3, [_cand(CASES[n], self.n) for n in NAMES], PTS)

    def params(self, case):
        p = self.t.reloc_default_params()
        for k, v in case["params"].items():
            setattr(p, k, v)
        return p

    def hyp(self, name, cand=None):
        c = CASES[name]
        return (INDEX[name] if cand is None else cand, c["Tcw7"], c["inliers"][:self.n])

    def single(self, name):
        """The case alone, H = 1 (computed once, read-only)."""
        if name not in self._single:
            mp, ol, res = self.t.reloc_refine([self.hyp(name)], self.params(CASES[name]))
            self._single[name] = (mp[0], ol[0], res[0], self.t.reloc_attempts())
        return self._single[name]

    def chain(self, name):
        """The chain of single C entries through the mirrors, with their uploads and downloads."""
        if name not in self._chain:
            from rumi_slam_amd.matcher import SearchByProjection_Reloc
            case = CASES[name]
            m = self.match[int(case["params"]["check_orientation"])]

            def search(T, Ow, skip, cur, th, dist):
                return SearchByProjection_Reloc(m, self.cur, R.LOG_SF, T, Ow, K_TUM3, case["kf_keys"], case["kf_mp"], dict(PTS, skip=skip), cur, th, dist)
            self._chain[name] = R.run_chain(case, PTS, self.opt.PoseOptimization, search)
        return self._chain[name]


@pytest.fixture(scope="module")
def rig():
    return Rig()


def _same(got, want, what):
    mp, ol, res = got[:3]
    wmp, wol, wres = want[:3]
    assert np.array_equal(mp, wmp), (what, "frame_mp", int((mp != wmp).sum()))
    assert np.array_equal(ol, wol), (what, "outlier_last", int((ol != wol).sum()))
    assert res.tobytes() == wres.tobytes(), (what, res, wres)


@pytest.mark.parametrize("name", NAMES)
def test_alone_equals_the_chain_of_single_entries(rig, name):
    mp, ol, res, _ = rig.single(name)
    ref = rig.chain(name)
    assert int(res["ran"]) == ref["ran"] and res["ngood"].tolist() == ref["ngood"] and res["nadditional"].tolist() == ref["nadditional"]
    assert int(res["ngood_final"]) == ref["ngood_final"]
    assert np.array_equal(mp, ref["frame_mp"]), int((mp != ref["frame_mp"]).sum())
    assert np.array_equal(ol, ref["outlier_last"]), int((ol != ref["outlier_last"]).sum())
    assert res["Tcw"].tobytes() == np.asarray(ref["Tcw"], np.float32).tobytes(), (res["Tcw"], ref["Tcw"])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_parity(rig, name):
    mp, ol, res, _ = rig.single(name)
    ref = R.oracle_result(name)
    assert int(res["ran"]) == ref["ran"] and res["ngood"].tolist() == ref["ngood"] and res["nadditional"].tolist() == ref["nadditional"]
    assert int(res["ngood_final"]) == ref["ngood_final"]
    assert np.array_equal(mp, ref["frame_mp"]) and np.array_equal(ol, ref["outlier_last"])
    assert np.abs(res["Tcw"] - ref["Tcw"]).max() <= 1e-4 * max(1.0, float(np.abs(ref["Tcw"]).max())), (res["Tcw"], ref["Tcw"])
    if CASES[name]["constructed"]:
        e = R.expected(CASES[name])
        assert int(res["ran"]) == e["ran"] and res["ngood"].tolist() == e["ngood"] and res["nadditional"].tolist() == e["nadditional"]


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_batching_invariance(rig, order):
    """A hypothesis' result depends neither on its neighbours nor on its place in the call."""
    names = R.standard_names()
    assert len(names) >= 18
    if order == "reversed":
        names = names[::-1]
    mp, ol, res = rig.t.reloc_refine([rig.hyp(n) for n in names])
    assert rig.t.reloc_attempts() == 1
    for h, n in enumerate(names):
        _same((mp[h], ol[h], res[h]), rig.single(n), (order, n))


def test_hypotheses_may_share_a_candidate(rig):
    """Two rounds' worth of hypotheses on one candidate: the winning pose and a pose that leaves it fewer than three correspondences."""
    c = CASES["s2_50"]
    none = np.zeros(rig.n, np.uint8)
    mp, ol, res = rig.t.reloc_refine([rig.hyp("s2_50"), (INDEX["s2_50"], c["Tcw7"], none), rig.hyp("s2_50")])
    for h in (0, 2):
        _same((mp[h], ol[h], res[h]), rig.single("s2_50"), h)
    assert int(res[1]["ran"]) == 1 and int(res[1]["ngood_final"]) == -1 and (mp[1] == -1).all() and (ol[1] == 255).all()
    assert res[1]["Tcw"].tobytes() == c["Tcw7"].tobytes()


def test_session_reuse(rig):
    """Two begin sessions on one tracker with different K and table sizes: the second is unaffected by the first."""
    sub = ["s2_50", "p2_31", "p1_9"]
    top = max(int(max(CASES[n]["kf_mp"].max(initial=-1), CASES[n]["matches"].max(initial=-1))) for n in sub) + 1
    small = {k: v[:top] for k, v in PTS.items()}
    assert top < len(PTS["bad"])
    want = {n: rig.single(n) for n in sub}
    try:
        rig.t.reloc_begin(K_TUM3, [_cand(CASES[n], rig.n) for n in sub], small)
        mp, ol, res = rig.t.reloc_refine([(k, CASES[n]["Tcw7"], CASES[n]["inliers"]) for k, n in enumerate(sub)])
    finally:
        rig.begin_all()
    for h, n in enumerate(sub):
        _same((mp[h], ol[h], res[h]), want[n], n)
    for n in sub:                                            # and the first session's results again after the second
        mp1, ol1, res1 = rig.t.reloc_refine([rig.hyp(n)])
        _same((mp1[0], ol1[0], res1[0]), rig.single(n), n)


def _outputs(rig, H, fill=0x5A):
    return (np.full((max(H, 1), rig.t.cap), fill | (fill << 8) | (fill << 16) | (fill << 24), np.int32), np.full((max(H, 1), rig.t.cap), fill, np.uint8),
            np.frombuffer(bytes([fill]) * (max(H, 1) * TR.RELOC_RESULT_DTYPE.itemsize), TR.RELOC_RESULT_DTYPE).copy())


def _untouched(out, fill=0x5A):
    return all((np.frombuffer(a.tobytes(), np.uint8) == fill).all() for a in out)


def test_hypothesis_count_boundaries(rig):
    """H = 0, 1, 2, the capacity RELOC_MAX_HYPOTHESES (RUMI_RELOC_MAX_HYPOTHESES) and one above it, which is refused."""
    out = _outputs(rig, 1)
    assert rig.t.reloc_refine_into([], None, *out) == capi.RUMI_OK and _untouched(out)
    mp, ol, res = rig.t.reloc_refine([rig.hyp("p2_49"), rig.hyp("p1_two")])
    _same((mp[0], ol[0], res[0]), rig.single("p2_49"), "H=2/0")
    _same((mp[1], ol[1], res[1]), rig.single("p1_two"), "H=2/1")
    assert (mp[0] != mp[1]).any()
    # rows behind the frame's n features are not written
    out = _outputs(rig, 2)
    assert rig.t.reloc_refine_into([rig.hyp("p2_49"), rig.hyp("p1_two")], None, *out) == capi.RUMI_OK
    assert (out[1][:, rig.n:] == 0x5A).all() and np.array_equal(out[0][:, :rig.n], mp)
    H = TR.RELOC_MAX_HYPOTHESES
    names = [["p1_9", "p1_10", "s1_50"][h % 3] for h in range(H)]
    mp, ol, res = rig.t.reloc_refine([rig.hyp(n) for n in names])
    for h in (0, 1, 2, H - 3, H - 2, H - 1):
        _same((mp[h], ol[h], res[h]), rig.single(names[h]), h)
    assert all(res[h].tobytes() == rig.single(names[h])[2].tobytes() for h in range(H))
    out = _outputs(rig, H + 1)
    assert rig.t.reloc_refine_into([rig.hyp("p1_9")] * (H + 1), None, *out) == capi.RUMI_E_CAPACITY and _untouched(out)
    mp, ol, res = rig.t.reloc_refine([rig.hyp("p1_10")])
    _same((mp[0], ol[0], res[0]), rig.single("p1_10"), "after the refusal")


def test_pose_instantiations(rig):
    """P1 with 1152 and with 1153 correspondences: the LDS and the global-memory instantiation of k_pose_opt."""
    for name, cnt in (("big_1152", 1152), ("big_1153", 1153)):
        mp, ol, res, _ = rig.single(name)
        assert int((CASES[name]["inliers"] != 0).sum()) == cnt == int(res["ngood"][0]) and int(res["ran"]) == 3
        assert (ol != 255).sum() == cnt and (ol[ol != 255] == 0).all()


def test_dense_windows_outgrow_the_list_arena(rig):
    """The lists are sized exactly (count / allocate / fill); the arena starts at four candidates a (hypothesis, key-frame feature) pair, the dense
    case needs many times that: the chain runs again with a larger arena, inside the call, and the result is the single entries'."""
    case = CASES["dense"]
    assert case["dense_window"] > 8
    rig.single("dense")
    mp, ol, res = rig.t.reloc_refine([rig.hyp("dense")], rig.params(case))
    _same((mp[0], ol[0], res[0]), rig.single("dense"), "dense again")
    assert rig.t.reloc_attempts() == 1, "the arena a tracker has grown is kept"
    ref = rig.chain("dense")
    assert np.array_equal(mp[0], ref["frame_mp"]) and res[0]["nadditional"].tolist() == ref["nadditional"] and ref["nadditional"][0] > 4


def test_dense_first_call_grows_the_arena():
    """On a fresh tracker the dense case is the first refine: its lists cannot fit four a pair."""
    t = TR.Tracker(R.NFEATURES, 1.2, R.NLEVELS, 20, 7, R.W, R.H, max_points=8192)
    t.extract(R.frame()["img"])
    t.reloc_begin(K_TUM3, [_cand(CASES[n], len(R.frame()["keys"])) for n in NAMES], PTS)
    case = CASES["dense"]
    p = t.reloc_default_params()
    for k, v in case["params"].items():
        setattr(p, k, v)
    mp, ol, res = t.reloc_refine([(INDEX["dense"], case["Tcw7"], case["inliers"])], p)
    assert t.reloc_attempts() >= 2
    ref = R.oracle_result("dense")
    assert np.array_equal(mp[0], ref["frame_mp"]) and res[0]["nadditional"].tolist() == ref["nadditional"]


def test_refusals(rig):
    """Each before any device work, outputs untouched, the handle usable afterwards."""
    F = R.frame()
    t = TR.Tracker(R.NFEATURES, 1.2, R.NLEVELS, 20, 7, R.W, R.H, max_points=len(PTS["bad"]))
    hyp = rig.hyp("p1_10")
    cands = [_cand(CASES[n], rig.n) for n in NAMES]

    def refused(code, hyps):
        out = _outputs(rig, len(hyps))
        assert t.reloc_refine_into(hyps, None, *out) == code and _untouched(out)

    assert t.reloc_begin_status(K_TUM3, cands, PTS) == capi.RUMI_E_INVALID, "no frame is resident"
    t.extract(F["img"])
    refused(capi.RUMI_E_INVALID, [hyp])                                          # refine before begin
    t.reloc_begin(K_TUM3, cands, PTS)
    good = t.reloc_refine([hyp])
    _same((good[0][0], good[1][0], good[2][0]), rig.single("p1_10"), "another tracker")
    refused(capi.RUMI_E_INVALID, [(len(NAMES), hyp[1], hyp[2])])                 # cand outside [0, K)
    refused(capi.RUMI_E_INVALID, [(-1, hyp[1], hyp[2])])
    refused(capi.RUMI_E_INVALID, [hyp, (hyp[0], hyp[1], None)])                  # NULL inliers
    # a refused begin leaves the session as it was
    more = {k: np.concatenate([v, v[:1]]) for k, v in PTS.items()}
    assert t.reloc_begin_status(K_TUM3, cands, more) == capi.RUMI_E_CAPACITY     # a point table above max_points
    badc = [dict(c) for c in cands]
    badc[3] = dict(badc[3], kf_mp=np.where(np.arange(len(badc[3]["kf_mp"])) == 2, len(PTS["bad"]), badc[3]["kf_mp"]).astype(np.int32))
    assert t.reloc_begin_status(K_TUM3, badc, PTS) == capi.RUMI_E_INVALID        # an id outside the table
    badc[3] = dict(cands[3], matches=np.where(np.arange(rig.n) == 5, -2, cands[3]["matches"]).astype(np.int32))
    assert t.reloc_begin_status(K_TUM3, badc, PTS) == capi.RUMI_E_INVALID
    again = t.reloc_refine([hyp])
    _same((again[0][0], again[1][0], again[2][0]), rig.single("p1_10"), "after the refused begins")
    # a new rumi_track_extract ends the session
    t.extract(F["img"])
    refused(capi.RUMI_E_INVALID, [hyp])
    t.reloc_begin(K_TUM3, cands, PTS)
    again = t.reloc_refine([hyp])
    _same((again[0][0], again[1][0], again[2][0]), rig.single("p1_10"), "a new session")


def test_empty_frame_and_empty_session():
    """A frame with n = 0: the chain ends at :3307 with nothing to optimise; a session without candidates refuses every hypothesis."""
    t = TR.Tracker(R.NFEATURES, 1.2, R.NLEVELS, 20, 7, R.W, R.H, max_points=8192)
    _, keys, _ = t.extract(R.frame(True)["img"])
    assert len(keys) == 0
    c = CASES["p1_10"]
    t.reloc_begin(K_TUM3, [dict(kf_keys=c["kf_keys"], kf_mp=c["kf_mp"], matches=np.zeros(0, np.int32))], PTS)
    mp, ol, res = t.reloc_refine([(0, c["Tcw7"], np.zeros(1, np.uint8))])
    assert mp.shape == (1, 0) and int(res[0]["ran"]) == 1 and int(res[0]["ngood_final"]) == -1 and res[0]["ngood"].tolist() == [0, 0, 0]
    assert res[0]["Tcw"].tobytes() == c["Tcw7"].tobytes()
    t.reloc_begin(K_TUM3, [], PTS)
    out = (np.zeros((1, t.cap), np.int32), np.zeros((1, t.cap), np.uint8), np.zeros(1, TR.RELOC_RESULT_DTYPE))
    assert t.reloc_refine_into([(0, c["Tcw7"], np.zeros(1, np.uint8))], None, *out) == capi.RUMI_E_INVALID
