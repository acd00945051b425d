"""The constructed scenes of reloc_resident_scene.py without a device: every condition holds (build() asserts them from the Hamming distances),
and the matcher oracle's SearchByBoW returns the hand-stated matches for them."""
import numpy as np
import pytest

import oracle_lib as O
import reloc_cases as R
import reloc_resident_scene as S


def _oracle(scene, k, nnratio=S.NNRATIO, check_ori=True):
    F = R.frame()
    kf = scene["kfs"][k]
    return O.search_by_bow(kf["keys"], kf["desc"], kf["mp"], scene["points"]["bad"], kf["fv"], F["keys"], F["desc"], scene["fv"], nnratio, check_ori)


@pytest.mark.parametrize("setting", list(S.SETTINGS))
def test_conditions_hold_and_sizes(setting):
    scene = S.build(setting)                                 # asserts every constructed condition
    names = {g[0] for g in scene["gadgets"]}
    assert {"th50", "th51", "ratio30_40", "ratio29_39", "tie", "contend_runner_up", "contend_nothing", "null", "bad_point", "absent_node"} <= names
    assert all(len(kf["mp"]) <= 400 for kf in scene["kfs"]) and len(scene["kfs"]) <= 6
    print(f"{setting}: levelsup {scene['levelsup']}, {len(scene['fv'][0])} frame node(s), node sizes met by the key-frames: {scene['sizes']}")
    if setting == "root":
        assert len(scene["fv"][0]) == 1 and scene["sizes"][0] > 512, "the whole frame in one node, above the old batch kernel's limit"
    else:
        assert min(scene["sizes"]) < 16 < max(scene["sizes"]) and max(scene["sizes"]) <= 512


@pytest.mark.parametrize("setting", list(S.SETTINGS))
def test_oracle_returns_the_hand_stated_matches(setting):
    scene = S.build(setting)
    for k in range(S.K):
        if scene["bad_slot"][k]:
            continue
        n, row = _oracle(scene, k)
        assert np.array_equal(row, scene["expect"][k]), (k, np.nonzero(row != scene["expect"][k])[0])
        assert n == scene["counts"][k]


@pytest.mark.parametrize("setting", list(S.SETTINGS))
def test_oracle_ties_and_rotation(setting):
    scene = S.build(setting)
    n, row = _oracle(scene, S.ORDER, S.NNRATIO_TIES)
    ties = scene["expect_ties"][S.ORDER]
    assert len(ties) == 2 and sorted(ties.values())[0] == -1 and sorted(ties.values())[1] >= 0
    lane = scene["expect_ties_lane"][S.ORDER]
    assert len(lane) == 2 and sorted(lane.values())[0] == -1 and sorted(lane.values())[1] >= 0
    for f, p in list(ties.items()) + list(lane.items()):
        assert row[f] == p, (f, p, row[f])
    n_on, row_on = _oracle(scene, S.ORDER)
    n_off, row_off = _oracle(scene, S.ORDER, check_ori=False)
    assert n_off == sum(c for _, c in S.CUT_BINS) and n_on == n_off - S.CUT_BINS[-1][1], "the second and third bin stand ON the 0.1f cut and stay"
    n_off, row_off = _oracle(scene, S.ROTATION, check_ori=False)
    n_on, row_on = _oracle(scene, S.ROTATION)
    assert n_off == sum(c for _, c in S.ROT_BINS) and n_on == n_off - S.ROT_BINS[-1][1]
    assert int(((row_off >= 0) & (row_on < 0)).sum()) == S.ROT_BINS[-1][1]
