"""What tests/test_sim3_projection_batch_gpu.py relies on, checked on the CPU with the oracle alone: the scenes of
tests/sim3_projection_scene.py make the ORDER of a job's list matter, so that bytes equal to the oracle's mean the device reproduces the
member's sequential loop (R/lib_src/ORBmatcher.cc:372-471, `vpMatched[bestIdx] = pMP` at :465) and not just independent searches.  These tests
look at the scenes, not at rumi_search_by_projection_sim3_resident."""
import numpy as np
import pytest

import sim3_projection_scene as P


@pytest.fixture(scope="module", params=P.SEEDS)
def seeded(request):
    m = P.seeded_map(request.param)
    return P.scenes(m, request.param)


def test_seeded_lists_have_entries_whose_answer_depends_on_the_order(seeded):
    """An entry whose answer in its list differs from its answer alone lost a feature to an earlier entry (and took its next choice, or none).
    Every whole-list stage-A job of a seeded scene has at least MIN_ORDER_DEPENDENT of them."""
    jobs = seeded["one"].jobs + seeded["same_slot"].jobs[:1]
    counts = [P.order_dependent(seeded["one"], j) for j in jobs]
    print("order-dependent entries per job:", counts)
    assert min(counts) >= P.MIN_ORDER_DEPENDENT, counts


def test_seeded_scenes_cover_the_gates_and_both_projections(seeded):
    sc = seeded["mixed"]
    ids = sc.ids
    assert (ids < 0).any() and sc.m.bad[ids[ids >= 0]].any() and len(set(ids.tolist())) < len(ids)
    assert {j.variant for j in sc.jobs} == {0, 1} and {(j.th, j.ratio) for j in sc.jobs} == {P.STAGE_A, P.STAGE_B, P.COVISIBLE}
    n = [P.oracle_job(sc, j)[0] for j in sc.jobs]
    assert min(n) > 20, n


def test_cascade_runs_its_full_length_and_depends_on_the_order():
    sc = P.cascade(0)
    j = sc.jobs[0]
    n, row = P.oracle_job(sc, j)
    assert n == P.CASCADE and P.taken(row, j.count).tolist() == list(range(P.CASCADE)), "entry i holds feature i"
    assert P.alone(sc, j).tolist() == [0] + list(range(P.CASCADE - 1)), "alone, entry i prefers feature i - 1"
    rev = P.Scene(sc.m, sc.ids[::-1].copy(), sc.jobs)
    n2, row2 = P.oracle_job(rev, j)
    took = P.taken(row2, j.count)[::-1]                       # per point again
    assert n2 == P.CASCADE - 1 and took.tolist() == [-1] + list(range(P.CASCADE - 1)), "reversed, nobody loses a first choice but entry 0"


@pytest.mark.parametrize("d0,cascades", [(75, True), (76, False)])
def test_a_non_match_does_not_block(d0, cascades):
    sc = P.cascade(d0)
    j = sc.jobs[0]
    n, row = P.oracle_job(sc, j)
    want = list(range(P.CASCADE)) if cascades else [-1] + list(range(P.CASCADE - 1))
    assert P.taken(row, j.count).tolist() == want and n == P.CASCADE - (not cascades)


def test_crowd_is_contended_throughout():
    sc = P.crowd()
    j = sc.jobs[0]
    n, row = P.oracle_job(sc, j)
    assert n == j.count == 150 and (row[:150] >= 0).all(), "every entry finds a feature, every feature is taken"
    assert (P.taken(row, j.count) != P.alone(sc, j)).sum() > 100


# ---- the call sites: the member text over the oracle against the job composition the facade members use ----
def find_matches_list(m, matched, cov):
    """The list of FindMatchesByProjection (LoopClosing.cc:871-905): the points of the matched key-frame's covisibles, of itself and of the
    covisibles' covisibles, first occurrence, not bad.  (spCheckKFs and spCurrentCovisbles reach nothing that leaves the function.)"""
    n = 10
    vp = list(cov.get(matched, []))[:n]
    n0 = len(vp)
    vp.append(matched)
    if n0 < n:
        for i in range(n0):
            vp += list(cov.get(vp[i], []))[:n]
    seen, out = set(), []
    for k in vp:
        for p in m.kfs[k].row:
            if p >= 0 and not m.bad[p] and p not in seen:
                seen.add(p)
                out.append(p)
    return out


def test_covisible_check_is_one_list_and_a_replay_over_the_counts():
    """:773-795 as written -- the list rebuilt and one search per covisible until three are valid -- against: the list once, every covisible
    a job on the same range, the while loop replayed over the counts.  The third valid covisible is the fourth of six: the two after it are
    searched by the composition and passed over."""
    m = P.seeded_map(P.SEEDS[0])
    c = m.corrected
    cov = {0: [1], 1: [0]}
    covisibles = c[1:7]
    pose = {k: (P.shifted(m.poses[k], [1.5, 0.0, 0.0]) if k in (covisibles[1], covisibles[5]) else m.poses[k]) for k in covisibles}
    # the member text
    n_text, j, lists, counts = 0, 0, [], []
    while n_text < 3 and j < len(covisibles):
        vp = find_matches_list(m, 0, cov)
        k = covisibles[j]
        num, _ = P.oracle_list(m, k, pose[k], vp, *P.COVISIBLE, 0)
        lists.append(vp); counts.append(num)
        n_text += num >= 30
        j += 1
    assert all(l == lists[0] for l in lists), "the list depends on the matched key-frame alone"
    assert [x >= 30 for x in counts] == [True, False, True, True] and j == 4 and n_text == 3, counts
    # the composition
    vp = find_matches_list(m, 0, cov)
    sc = P.Scene(m, vp, [P.Job(k, pose[k], 0, len(vp), P.COVISIBLE, 0) for k in covisibles])
    num = [P.oracle_job(sc, job)[0] for job in sc.jobs]
    n_comp, jj = 0, 0
    while n_comp < 3 and jj < len(covisibles):
        n_comp += num[jj] >= 30
        jj += 1
    assert (jj, n_comp, num[:jj], vp) == (j, n_text, counts, lists[-1]) and len(num) == 6 and num[4] >= 30, "the speculative answers do not leak"


def test_stage_jobs_are_the_two_searches_of_every_candidate():
    """:711-738 as written -- per candidate a fresh vector and the overload with key-frames (th 8, ratio 1.5), then a fresh vector and the
    overload without (th 5, ratio 1.0) -- against two jobs a candidate on the candidate's range of one id array."""
    m = P.seeded_map(P.SEEDS[0])
    cur = m.corrected[0]
    cands = {0: find_matches_list(m, 0, {0: [1]}), 1: find_matches_list(m, 1, {})}
    scw = {0: m.poses[cur], 1: P.shifted(m.poses[cur], [0.01, -0.005, 0.0])}
    text = []
    for k, vp in cands.items():
        text.append(P.oracle_list(m, cur, scw[k], vp, *P.STAGE_A, 1))
        text.append(P.oracle_list(m, cur, scw[k], vp, *P.STAGE_B, 0))
    ids, jobs = [], []
    for k, vp in cands.items():
        jobs += [P.Job(cur, scw[k], len(ids), len(vp), P.STAGE_A, 1), P.Job(cur, scw[k], len(ids), len(vp), P.STAGE_B, 0)]
        ids += vp
    sc = P.Scene(m, ids, jobs)
    for (n, row), job in zip(text, sc.jobs):
        n2, row2 = P.oracle_job(sc, job)
        assert n2 == n and row2.tobytes() == row.tobytes() and n > 10
