"""rumi_track_compute_bow / rumi_track_reloc_bow / rumi_track_reloc_begin_resident (include/rumi_track.h): Tracking::Relocalization by slot.

  compute_bow      the bytes rumi_track_reference_keyframe writes for the same frame and vocabulary, and the CPU vocabulary's
  reloc_bow        per candidate rumi_search_by_bow on the same key-frame by host pointers, the matcher oracle, and the hand-stated rows of
                   reloc_resident_scene.py, in both vocabulary settings (nodes of 2 .. 62 features; one node of 1400)
  begin_resident   + refine against begin + refine with the same data by host pointers: every case of reloc_cases.py, through table_ids
and candidate order, K = 1 against K = 6, the FeatureVector under other matcher calls, session reuse, a new extract, refusals, empty inputs."""
import numpy as np
import pytest

import oracle_lib as O
import reloc_cases as R
import reloc_resident_scene as S
import voc_scene
from rumi_slam_amd import capi
from rumi_slam_amd import matcher as M
from rumi_slam_amd import tracker as TR
from rumi_slam_amd.covis import Covisibility
from rumi_slam_amd.vocabulary import ORBVocabulary
from scene import K_TUM3

pytestmark = pytest.mark.gpu

SETTINGS = list(S.SETTINGS)
FILL = 0x5A
# slots of the scene's store that exist for the refusals
SLOT_UNUSED, SLOT_NO_FEATURES, SLOT_SHORT_ROW, SLOT_NO_ATTRIBUTES = 0, 12, 13, 14


def _tracker(max_points=8192):
    return TR.Tracker(R.NFEATURES, 1.2, R.NLEVELS, 20, 7, R.W, R.H, max_points=max_points)


def _scene_store(scene):
    """The scene in a store, plus three slots that are wrong in one way each and one point without attributes."""
    F = R.frame()
    npt = len(scene["points"]["bad"])
    cov = Covisibility(16, npt + 8)
    keep = S.fill_store(cov, scene, K_TUM3)
    kf = scene["kfs"][S.EDGES]
    cov.set_points([npt], [0], [[]])                                                     # a point that never gets attributes
    rows = [[-1] * 5, kf["mp"][:-1], np.where(np.arange(len(kf["mp"])) == 0, npt, kf["mp"])]
    cov.set_keyframes([SLOT_NO_FEATURES, SLOT_SHORT_ROW, SLOT_NO_ATTRIBUTES], [901, 902, 903], [0] * 3, [0] * 3, rows, [[]] * 3, [-1] * 3, [[]] * 3)
    fr = M.FrameView(kf["keys"], kf["desc"], R.W, R.H, F["sf"])
    fv = M.FeatureVector.from_csr(*kf["fv"])
    cov.set_keyframe_features(SLOT_SHORT_ROW, fr, fv, K_TUM3)
    cov.set_keyframe_features(SLOT_NO_ATTRIBUTES, fr, fv, K_TUM3)
    return cov, keep + [fr, fv]


class Rig:
    def __init__(self):
        F = R.frame()
        self.F = F
        self.t = _tracker()
        _, keys, desc = self.t.extract(F["img"])
        assert keys.tobytes() == F["keys"].tobytes() and np.array_equal(desc, F["desc"]), "the resident frame is the scene's frame"
        self.n = len(keys)
        self.voc = ORBVocabulary(*S.voc_table())
        self.ovoc = O.OracleVocabulary(*S.voc_table())
        self.cur = M.FrameView(F["keys"], F["desc"], R.W, R.H, F["sf"])
        self.scene = {s: S.build(s) for s in SETTINGS}
        self.store, self._keep = {}, []
        for s in SETTINGS:
            self.store[s], keep = _scene_store(self.scene[s])
            self._keep += keep
        self.single = {}
        self._bow, self._walk = {}, {}

    def bow(self, setting):
        """compute_bow under a setting: the frame's FeatureVector is then the tracker's (computed again whenever the setting changes)."""
        out = self.t.compute_bow(self.voc, S.SETTINGS[setting])
        self._bow.setdefault(setting, out)
        return out

    def walk(self, setting, nnratio=S.NNRATIO, ori=True):
        """reloc_bow over the scene's six slots (first result kept, read-only)."""
        key = (setting, nnratio, ori)
        self.bow(setting)
        got = self.t.reloc_bow(self.store[setting], S.SLOTS, nnratio, ori)
        self._walk.setdefault(key, got)
        return got

    def by_host_pointers(self, setting, k, nnratio=S.NNRATIO, ori=True):
        """rumi_search_by_bow given candidate k by host pointers, the frame's FeatureVector as compute_bow's transform assembles it."""
        key = (setting, k, nnratio, ori)
        if key not in self.single:
            b = self._bow[setting] if setting in self._bow else self.bow(setting)
            f_fv = M.FeatureVector.from_csr(*self.voc.assemble(b["word_id"], b["word_weight"], b["node_id"])[1])
            kf = self.scene[setting]["kfs"][k]
            m = M.ORBmatcher(nnratio, ori, max_features=2048, max_queries=8192)
            self.single[key] = m.SearchByBoW(M.FrameView(kf["keys"], kf["desc"], R.W, R.H, self.F["sf"]), M.FeatureVector.from_csr(*kf["fv"]), kf["mp"],
                                             np.concatenate([self.scene[setting]["points"]["bad"], np.zeros(8, np.uint8)]), self.cur, f_fv)
            m.close()
        return self.single[key]


@pytest.fixture(scope="module")
def rig():
    return Rig()


# ---- compute_bow -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS)
def test_compute_bow_bytes(rig, setting):
    sc = rig.scene[setting]
    got = rig.bow(setting)
    kf = sc["kfs"][S.EDGES]
    pts = dict(sc["points"], obs=np.ones(len(sc["points"]["bad"]), np.int32))
    ref = rig.t.reference_keyframe(rig.voc, K_TUM3, R.T_TRUE, M.FrameView(kf["keys"], kf["desc"], R.W, R.H, rig.F["sf"]), M.FeatureVector.from_csr(*kf["fv"]),
                                   kf["mp"], pts, levelsup=S.SETTINGS[setting])
    for f in ("word_id", "word_weight", "node_id"):
        assert got[f].tobytes() == ref[f].tobytes(), f
    word, w, node = rig.ovoc.transform_features(rig.F["desc"], S.SETTINGS[setting])
    assert np.array_equal(got["word_id"], word) and np.array_equal(got["node_id"], node) and got["word_weight"].tobytes() == w.tobytes()
    fv = rig.voc.assemble(got["word_id"], got["word_weight"], got["node_id"])[1]
    assert all(np.array_equal(a, b) for a, b in zip(fv, sc["fv"])), "the frame's FeatureVector is the scene's"


# ---- reloc_bow ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("nnratio,ori", [(S.NNRATIO, True), (S.NNRATIO, False), (S.NNRATIO_TIES, True)])
def test_reloc_bow_equals_host_pointers_oracle_and_hand(rig, setting, nnratio, ori):
    sc = rig.scene[setting]
    nm, rows = rig.walk(setting, nnratio, ori)
    assert rows.shape == (S.K, rig.n)
    print(f"{setting}: node sizes met {sc['sizes']}; counts {nm.tolist()}")
    for k in range(S.K):
        if sc["bad_slot"][k]:
            assert nm[k] == -1 and (rows[k] == -1).all()
            continue
        n1, row1 = rig.by_host_pointers(setting, k, nnratio, ori)
        assert np.array_equal(rows[k], row1) and nm[k] == n1, (k, np.nonzero(rows[k] != row1)[0])
        kf = sc["kfs"][k]
        n2, row2 = O.search_by_bow(kf["keys"], kf["desc"], kf["mp"], sc["points"]["bad"], kf["fv"], rig.F["keys"], rig.F["desc"], sc["fv"], nnratio, ori)
        assert np.array_equal(rows[k], row2) and nm[k] == n2, (k, np.nonzero(rows[k] != row2)[0])
        if nnratio == S.NNRATIO and ori:
            assert np.array_equal(rows[k], sc["expect"][k]) and nm[k] == sc["counts"][k]
        if nnratio == S.NNRATIO_TIES:
            for f, p in list(sc["expect_ties"][k].items()) + list(sc["expect_ties_lane"][k].items()):
                assert rows[k][f] == p, "of two frame features at one distance the earlier position wins"
    if not ori:
        assert nm[S.ROTATION] == sum(c for _, c in S.ROT_BINS)


@pytest.mark.parametrize("setting", SETTINGS)
def test_candidate_order_and_count_do_not_matter(rig, setting):
    nm, rows = rig.walk(setting)
    rig.bow(setting)
    order = [4, 0, 5, 3, 1, 2]
    nm2, rows2 = rig.t.reloc_bow(rig.store[setting], [S.SLOTS[k] for k in order])
    assert np.array_equal(nm2, nm[order]) and np.array_equal(rows2, rows[order])
    for k in range(S.K):
        nm1, rows1 = rig.t.reloc_bow(rig.store[setting], [S.SLOTS[k]])
        assert nm1[0] == nm[k] and np.array_equal(rows1[0], rows[k]), k


def test_feature_vector_survives_other_matcher_calls(rig):
    """Between compute_bow and reloc_bow: a reference_keyframe under the OTHER levelsup (it builds another FeatureVector of the same frame in the
    matcher's staging buffers and the transform block) and a SearchByProjection of the refine chain."""
    nm, rows = rig.walk("small")
    rig.bow("small")
    sc = rig.scene["small"]
    kf = sc["kfs"][S.SIZES]
    pts = dict(sc["points"], obs=np.ones(len(sc["points"]["bad"]), np.int32))
    rig.t.reference_keyframe(rig.voc, K_TUM3, R.T_TRUE, M.FrameView(kf["keys"], kf["desc"], R.W, R.H, rig.F["sf"]), M.FeatureVector.from_csr(*kf["fv"]), kf["mp"],
                             pts, levelsup=S.SETTINGS["root"])
    nm2, rows2 = rig.t.reloc_bow(rig.store["small"], S.SLOTS)
    assert np.array_equal(nm2, nm) and np.array_equal(rows2, rows)
    ids = rig.t.reloc_begin_resident(rig.store["small"], K_TUM3, [S.EDGES])
    rig.t.reloc_refine([(0, R.T_NEAR, (rows[S.EDGES] >= 0).astype(np.uint8))])
    nm3, rows3 = rig.t.reloc_bow(rig.store["small"], S.SLOTS)
    assert np.array_equal(nm3, nm) and np.array_equal(rows3, rows) and len(ids) > 0


# ---- begin_resident + refine -------------------------------------------------------------------------------------------------------------
def _first_appearance(rows):
    seen, out = set(), []
    for r in rows:
        for p in np.asarray(r).tolist():
            if p >= 0 and p not in seen:
                seen.add(p); out.append(p)
    return np.array(out, np.int32)


def _same(got, want, what):
    for a, b, f in zip(got, want, ("frame_mp", "outlier_last", "result")):
        assert a.tobytes() == b.tobytes(), (what, f)


@pytest.mark.parametrize("setting", SETTINGS)
def test_scene_session_equals_host_pointers(rig, setting):
    """The scene's candidates that keep 15 matches: table order, one row for a point two candidates share, and a refine of every candidate."""
    sc = rig.scene[setting]
    nm, rows = rig.walk(setting)
    keep = [k for k in range(S.K) if nm[k] >= 15]
    assert S.EDGES in keep and S.SHARED in keep and S.BAD not in keep
    ids = rig.t.reloc_begin_resident(rig.store[setting], K_TUM3, keep)
    assert np.array_equal(ids, _first_appearance([sc["kfs"][k]["mp"] for k in keep])) and len(set(ids.tolist())) == len(ids)
    shared = set(sc["kfs"][S.EDGES]["mp"].tolist()) & set(sc["kfs"][S.SHARED]["mp"].tolist()) - {-1}
    assert len(shared) >= 10 and all((ids == p).sum() == 1 for p in shared)
    hyps = [(j, R.T_NEAR, (rows[k] >= 0).astype(np.uint8)) for j, k in enumerate(keep)]
    mp, ol, res = rig.t.reloc_refine(hyps)
    mp2, ol2, res2 = rig.t.reloc_refine(hyps[::-1])                                       # the session again, second round
    _same((mp2[::-1], ol2[::-1], res2[::-1]), (mp, ol, res), "second round")
    pts = sc["points"]
    rig.t.reloc_begin(K_TUM3, [dict(kf_keys=sc["kfs"][k]["keys"], kf_mp=sc["kfs"][k]["mp"], matches=rows[k]) for k in keep], pts)
    mph, olh, resh = rig.t.reloc_refine(hyps)
    _same((np.stack([TR.rows_to_ids(r, ids) for r in mp]), ol, res), (mph, olh, resh), "host pointers")
    assert all(int(r["ngood"][0]) >= 15 for r in res), "the chains ran on the matches"


def _cases_store():
    """Every case of reloc_cases.scene() as a slot: its key-points and row as they are (store point id = row of the cases' table), descriptors
    and mFeatVec such that the BoW walk finds the case's matches -- a key-frame feature whose point the case matches to frame feature f carries
    f's descriptor and lies in the one node of a vocabulary without stopped words, the others in no node."""
    cases, pts = R.scene()
    F = R.frame()
    voc = voc_scene.synthetic_vocabulary(5, 4, 1, stop_frac=0.0)
    npt = len(pts["bad"])
    cov = Covisibility(len(cases) + 1, npt)
    names = list(cases)
    cov.set_keyframes(list(range(len(names))), [7000 + k for k in range(len(names))], [0] * len(names), [0] * len(names), [cases[n]["kf_mp"] for n in names],
                      [[]] * len(names), [-1] * len(names), [[]] * len(names))
    cov.set_points(list(range(npt)), pts["bad"], [[]] * npt)
    cov.set_point_attributes(list(range(npt)), pts["pos"], np.zeros((npt, 3), np.float32), pts["min_dist"], pts["max_dist"], pts["desc"])
    root = int(O.OracleVocabulary(*voc).transform(F["desc"][:1], 1)[1][0][0])
    keep = []
    for k, name in enumerate(names):
        c = cases[name]
        at = {int(p): f for f, p in enumerate(c["matches"]) if p >= 0}
        desc = np.zeros((len(c["kf_mp"]), 32), np.uint8)
        inside = [i for i, p in enumerate(c["kf_mp"].tolist()) if p in at]
        for i in inside:
            desc[i] = F["desc"][at[int(c["kf_mp"][i])]]
        fr = M.FrameView(c["kf_keys"], desc, R.W, R.H, F["sf"])
        fv = M.FeatureVector({root: inside} if inside else {})
        cov.set_keyframe_features(k, fr, fv, K_TUM3)
        keep += [fr, fv]
    return cov, keep, ORBVocabulary(*voc)


def test_every_reloc_case_through_the_store():
    cases, pts = R.scene()
    names = list(cases)
    F = R.frame()
    t = _tracker()
    t.extract(F["img"])
    n = len(F["keys"])
    cov, keep, voc = _cases_store()
    t.compute_bow(voc, 1)
    nm, rows = t.reloc_bow(cov, list(range(len(names))), 0.75, True)
    _, first, counts = np.unique(F["desc"], axis=0, return_index=True, return_counts=True)
    unique = np.zeros(n, bool)
    unique[first[counts == 1]] = True
    exact = 0
    for k, name in enumerate(names):
        c = cases[name]
        want = np.where(np.isin(c["matches"][:n], c["kf_mp"]) & unique, c["matches"][:n], -1)
        if c["spec"]["twin"] == 0 and name != "dense":
            assert np.array_equal(rows[k], want), name
            exact += 1
    assert exact >= 15
    ids = t.reloc_begin_resident(cov, K_TUM3, list(range(len(names))))
    assert np.array_equal(ids, _first_appearance([cases[nm_]["kf_mp"] for nm_ in names]))

    def params(c):
        p = t.reloc_default_params()
        for key, v in c["params"].items():
            setattr(p, key, v)
        return p

    got = {}
    for k, name in enumerate(names):
        mp, ol, res = t.reloc_refine([(k, cases[name]["Tcw7"], cases[name]["inliers"][:n])], params(cases[name]))
        got[name] = (TR.rows_to_ids(mp[0], ids), ol[0], res[0])
    t.reloc_begin(K_TUM3, [dict(kf_keys=cases[nm_]["kf_keys"], kf_mp=cases[nm_]["kf_mp"], matches=rows[k]) for k, nm_ in enumerate(names)], pts)
    ran = set()
    for k, name in enumerate(names):
        mp, ol, res = t.reloc_refine([(k, cases[name]["Tcw7"], cases[name]["inliers"][:n])], params(cases[name]))
        _same(got[name], (mp[0], ol[0], res[0]), name)                                       # Tcw and every count bit for bit
        ran.add(int(res[0]["ran"]))
    assert {1, 3, 7, 15, 31, 63} <= ran, "the cases still reach every stage of the chain"


def test_relocalize_resident_equals_relocalize(rig):
    sc = rig.scene["small"]
    nm, rows = rig.walk("small")
    inl = {k: (rows[k] >= 0).astype(np.uint8) for k in range(S.K)}
    made = {}
    for spec in (True, False):
        rig.bow("small")
        st = TR.relocalize_resident(rig.t, rig.store["small"], S.SLOTS, lambda k: (True, True, inl[k], R.T_NEAR), K_TUM3, make=lambda k, m: made.setdefault(k, m.copy()),
                                    speculate_round=spec)
        assert sorted(made) == [k for k in range(S.K) if nm[k] >= 15] and all(np.array_equal(made[k], rows[k]) for k in made)
        cands = [dict(kf_keys=sc["kfs"][k]["keys"], kf_mp=sc["kfs"][k]["mp"], matches=rows[k]) if nm[k] >= 15 else None for k in range(S.K)]
        ref = TR.relocalize(rig.t, cands, sc["points"], lambda k: (True, True, inl[k], R.T_NEAR), speculate_round=spec, K4=K_TUM3)
        assert st["matched"] == ref["matched"] and st["winner"] == ref["winner"] and st["steps"] == ref["steps"]
        assert np.array_equal(st["frame_mp"], ref["frame_mp"]) and np.array_equal(st["outlier"], ref["outlier"]) and st["Tcw"].tobytes() == ref["Tcw"].tobytes()


# ---- states and refusals -----------------------------------------------------------------------------------------------------------------
def _bow_out(t, K):
    return np.full((K, max(getattr(t, "_n", 0), 1)), FILL | FILL << 8 | FILL << 16 | FILL << 24, np.int32), np.full(max(K, 1), FILL | FILL << 8 | FILL << 16 | FILL << 24, np.int32)


def _untouched(*arrays):
    return all((np.frombuffer(a.tobytes(), np.uint8) == FILL).all() for a in arrays)


def test_refusals_and_a_new_extract(rig):
    """Each refusal before any device work, pre-filled outputs untouched, the handle usable afterwards."""
    F = R.frame()
    sc, cov = rig.scene["small"], rig.store["small"]
    want_nm, want_rows = rig.walk("small")
    t = _tracker()
    word, wgt, node = (np.full(t.cap, 0x5A5A5A5A, np.uint32), np.frombuffer(bytes([FILL]) * (8 * t.cap), np.float64).copy(), np.full(t.cap, 0x5A5A5A5A, np.uint32))

    def bow_refused(slots, code=capi.RUMI_E_INVALID):
        out = _bow_out(t, max(len(slots), 1))
        assert t.reloc_bow_into(cov, slots, 0.75, 1, *out) == code and _untouched(*out), slots

    def begin_refused(cand, code=capi.RUMI_E_INVALID, table_cap=4096, tr=None):
        ids, nt = np.full(4096, 0x5A5A5A5A, np.int32), np.full(1, 0x5A5A5A5A, np.int32)
        assert (tr or t).reloc_begin_resident_into(cov, K_TUM3, cand, ids, table_cap, nt) == code and _untouched(ids, nt), cand

    # no frame resident
    assert t.compute_bow_into(rig.voc, 1, word, wgt, node) == capi.RUMI_E_INVALID and _untouched(word, wgt, node)
    t._n = 0
    bow_refused(S.SLOTS)
    begin_refused([0])
    t.extract(F["img"])
    # a NULL argument; no compute_bow on this frame
    assert t.compute_bow_into(None, 1, word, wgt, node) == capi.RUMI_E_INVALID and t.compute_bow_into(rig.voc, 1, None, wgt, node) == capi.RUMI_E_INVALID
    assert t.compute_bow_into(rig.voc, 1, word, None, node) == capi.RUMI_E_INVALID and t.compute_bow_into(rig.voc, 1, word, wgt, None) == capi.RUMI_E_INVALID
    assert _untouched(word, wgt, node)
    bow_refused(S.SLOTS)
    t.compute_bow(rig.voc, S.SETTINGS["small"])
    begin_refused([0])                                                                    # no reloc_bow on this frame
    # the slots
    bow_refused([])                                                                       # K < 1
    for wrong in (-1, 16, SLOT_UNUSED, SLOT_NO_FEATURES, SLOT_SHORT_ROW):
        bow_refused(S.SLOTS[:2] + [wrong] + S.SLOTS[2:])
    bow_refused(S.SLOTS + S.SLOTS[:1])                                                    # named twice
    begin_refused([0])                                                                    # the refused walks opened nothing
    nm, rows = t.reloc_bow(cov, S.SLOTS + [SLOT_NO_ATTRIBUTES])
    assert np.array_equal(nm[:S.K], want_nm) and np.array_equal(rows[:S.K], want_rows), "usable after the refusals"
    # the candidates
    begin_refused([-1]); begin_refused([S.K + 1]); begin_refused([S.EDGES, S.BAD]); begin_refused([S.EDGES, S.EDGES])
    begin_refused([S.EDGES, S.K])                                                         # a row point without attributes
    assert "1 row point(s) without attributes" in capi.lib().rumi_last_error().decode(), "counted on the device"
    n_rows = len(_first_appearance([sc["kfs"][S.EDGES]["mp"], sc["kfs"][S.SHARED]["mp"]]))
    begin_refused([S.EDGES, S.SHARED], capi.RUMI_E_CAPACITY, table_cap=n_rows - 1)        # table_cap
    ids = np.full(4096, -1, np.int32); nt = np.zeros(1, np.int32)
    assert t.reloc_begin_resident_into(cov, K_TUM3, [S.EDGES, S.SHARED], ids, n_rows, nt) == capi.RUMI_OK and nt[0] == n_rows
    hyp = [(0, R.T_NEAR, (rows[S.EDGES] >= 0).astype(np.uint8))]
    good = t.reloc_refine(hyp)
    small = _tracker(max_points=n_rows - 1)                                               # the tracker's max_points
    small.extract(F["img"]); small.compute_bow(rig.voc, S.SETTINGS["small"]); small.reloc_bow(cov, S.SLOTS)
    begin_refused([S.EDGES, S.SHARED], capi.RUMI_E_CAPACITY, tr=small)
    # a new extract ends the FeatureVector, the walk and the session
    t.extract(F["img"])
    bow_refused(S.SLOTS)
    begin_refused([S.EDGES])
    out = (np.zeros((1, t.cap), np.int32), np.zeros((1, t.cap), np.uint8), np.zeros(1, TR.RELOC_RESULT_DTYPE))
    assert t.reloc_refine_into(hyp, None, *out) == capi.RUMI_E_INVALID
    t.compute_bow(rig.voc, S.SETTINGS["small"])
    begin_refused([S.EDGES])
    nm, rows = t.reloc_bow(cov, S.SLOTS)
    t.reloc_begin_resident(cov, K_TUM3, [S.EDGES, S.SHARED])
    _same(t.reloc_refine(hyp), good, "a new session")


def test_empty_frame_and_no_candidates(rig):
    t = _tracker()
    _, keys, _ = t.extract(R.frame(True)["img"])
    assert len(keys) == 0
    word, wgt, node = np.full(t.cap, 0x5A5A5A5A, np.uint32), np.frombuffer(bytes([FILL]) * (8 * t.cap), np.float64).copy(), np.full(t.cap, 0x5A5A5A5A, np.uint32)
    assert t.compute_bow_into(rig.voc, 1, word, wgt, node) == capi.RUMI_OK and _untouched(word, wgt, node)
    cov = rig.store["small"]
    nm, rows = t.reloc_bow(cov, S.SLOTS)
    assert rows.shape == (S.K, 0) and nm.tolist() == [0 if k != S.BAD else -1 for k in range(S.K)]
    ids = t.reloc_begin_resident(cov, K_TUM3, [S.EDGES])
    assert np.array_equal(ids, _first_appearance([rig.scene["small"]["kfs"][S.EDGES]["mp"]]))
    mp, ol, res = t.reloc_refine([(0, R.T_TRUE, np.zeros(1, np.uint8))])
    assert mp.shape == (1, 0) and int(res[0]["ran"]) == 1 and int(res[0]["ngood_final"]) == -1 and res[0]["Tcw"].tobytes() == R.T_TRUE.tobytes()
    # Kc = 0 on the scene's frame: an empty table, a session that refuses every hypothesis
    rig.walk("small")
    ids = rig.t.reloc_begin_resident(rig.store["small"], K_TUM3, [])
    assert len(ids) == 0
    out = (np.zeros((1, rig.t.cap), np.int32), np.zeros((1, rig.t.cap), np.uint8), np.zeros(1, TR.RELOC_RESULT_DTYPE))
    assert rig.t.reloc_refine_into([(0, R.T_TRUE, np.zeros(rig.n, np.uint8))], None, *out) == capi.RUMI_E_INVALID
