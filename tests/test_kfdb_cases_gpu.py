"""The constructed key-frame database cases (tests/kfdb_cases.py) on the device: every output line equals the line spelled in the case, bit for bit,
on a fresh database (batched and single calls), on one long-lived database whose slots are reused, and across a tile split; and the device
BowVector assembly (k_bow_assemble) on hand-filled per-feature rows."""
import numpy as np
import pytest

import kfdb_cases as KC
from kfdb_scene import run_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voc():
    from voc_scene import synthetic_vocabulary_fast
    from rumi_slam_amd.vocabulary import ORBVocabulary, TF_IDF
    v = ORBVocabulary(*synthetic_vocabulary_fast(5, 10, 5), weighting=TF_IDF)       # TF_IDF: a repeated word sums its weights (addWeight)
    assert v.size() == KC.NW
    return v


def new_db(voc, max_kf=512, max_entries=100_000):
    from rumi_slam_amd.kfdb import KeyFrameDatabase
    return KeyFrameDatabase(voc, max_kf, max_entries)


@pytest.mark.parametrize("batch", [True, False], ids=["batched", "single"])
@pytest.mark.parametrize("case", KC.CASES, ids=repr)
def test_case_on_a_fresh_database(voc, case, batch):
    db = new_db(voc)
    got = run_gpu(db, case.script, batch=batch)
    db.close()
    assert got == case.expect


def test_cases_on_one_long_lived_database(voc):
    """clear() between the cases: slots are reused and sequences are late.  A key-frame keeps its query state by id across erase and re-add, so
    each case runs with ids of its own (kfdb_cases.shifted)."""
    db = new_db(voc)
    wrong = []
    for n, case in enumerate(KC.CASES):
        script, want = KC.shifted(case, 10_000 * (n + 1), 100_000 * (n + 1))
        if run_gpu(db, script) != want:
            wrong.append(case.name)
        db.clear()
        assert db.size() == 0
    assert db.next_seq() == sum(1 for c in KC.CASES for x in c.script if x[0] == "A")
    db.close()
    assert wrong == []


def test_tile_split(voc):
    """max_kf = 2^21 leaves room for 4 queries a tile (about half a gigabyte of device memory, of which only the slots in use are touched): the
    eight consecutive queries of the T case are split by the wrapper and give the same lines."""
    case = KC.BY_NAME["T_eight_queries"]
    db = new_db(voc, max_kf=1 << 21)
    assert db.max_batch() == 4
    got = run_gpu(db, case.script, batch=True)
    db.close()
    assert got == case.expect
    small = new_db(voc)
    assert small.max_batch() >= 8                    # ... and there the same eight went in one call (test_case_on_a_fresh_database)
    small.close()


# ---- BowVector assembly ----
def _rows(cases, cap):
    import torch
    word = np.zeros((len(cases), cap), np.uint32)
    weight = np.zeros((len(cases), cap), np.float64)
    counts = np.zeros((len(cases), 2), np.int32)
    for f, (w, x, n) in enumerate(cases):
        word[f, :len(w)] = w
        weight[f, :len(x)] = x
        counts[f, 0] = n
    return word, weight, (torch.from_numpy(word.view(np.int32)).cuda(), torch.from_numpy(weight).cuda(), torch.from_numpy(counts).cuda())


def _check_assembly(voc, db, kid, words, weights, n, want_w, want_v, name):
    gw, gv = db.bow(kid)
    assert np.array_equal(gw, np.asarray(want_w, np.uint32)), name
    assert gv.tobytes() == np.asarray(want_v, np.float64).tobytes(), name          # the values spelled in the case
    (bi, bv), _ = voc.assemble(words[:n], weights[:n], np.zeros(n, np.uint32))
    assert np.array_equal(gw, bi) and gv.tobytes() == bv.tobytes(), name           # ... and the host assembly of the same rows


def test_bow_assembly_cases(voc):
    import torch
    db = new_db(voc)
    cap = KC.ASSEMBLY_CAP
    word, weight, dev = _rows([(w, x, n) for _, w, x, n, _, _, _ in KC.ASSEMBLY], cap)
    ids = np.arange(1, len(KC.ASSEMBLY) + 1, dtype=np.uint64)
    db.add_batch_device(ids, np.ones(len(ids), np.int32), *dev)
    torch.cuda.synchronize()
    for f, (name, _, _, n, want_w, want_v, _) in enumerate(KC.ASSEMBLY):
        _check_assembly(voc, db, ids[f], word[f], weight[f], n, want_w, want_v, name)
    # the frame whose every weight is 0 has no posting: a query of its words does not meet it (nor the frame of no feature)
    names = [a[0] for a in KC.ASSEMBLY]
    hidden = {int(ids[names.index("all_zero")]), int(ids[names.index("count_0")])}
    cands, scored = db.detect_relocalization_candidates([900], [1], [KC.vec([5, 6, 7], 0.25)], with_scored=True)
    assert len(scored[0][0]) > 0 and not hidden & set(int(x) for x in scored[0][0])
    db.close()


def test_bow_assembly_counts_above_cap(voc):
    name, cap, w, x, n, want_w, want_v, _ = KC.ASSEMBLY_CLAMP
    db = new_db(voc)
    word, weight, dev = _rows([(w, x, n)], cap)
    assert n > cap
    db.add_batch_device(np.array([1], np.uint64), np.ones(1, np.int32), *dev)
    _check_assembly(voc, db, 1, word[0], weight[0], cap, want_w, want_v, name)
    db.close()
