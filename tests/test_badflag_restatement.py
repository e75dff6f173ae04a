"""The restatement of orbl_set_bad_keyframes (tests/npbadflag.py: the literal sequential loop of src/KeyFrame.cc:460-553) against the
hand-worked cases of tests/badflagcases.py, and the two conditions that keep the GPU comparison (tests/test_gpu_badflag.py) from passing
vacuously: every path of the loop is taken by the hand cases and by the seeded maps, and an implementation blind to the order of the
targets answers differently.  No GPU."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import badflagcases as bc  # noqa: E402
from tests import npbadflag as npb  # noqa: E402

HAND = bc.hand_cases()
_SEEDED = None


def _seeded():
    global _SEEDED
    if _SEEDED is None:
        _SEEDED = {name: (pr, npb.set_bad_keyframes(pr)) for name, pr in bc.seeded().items()}
    return _SEEDED


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in b)


@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_gives_the_hand_worked_outputs(name):
    pr, exp = HAND[name]
    got = npb.set_bad_keyframes(pr, points="kf_slot_off" in pr)
    for k, v in exp.items():
        assert got[k].dtype == v.dtype or k == "tgt_Tcp", k
        assert np.array_equal(got[k], v), (k, got[k], v)


def test_every_path_is_taken_by_the_hand_cases_and_by_the_seeded_maps():
    hand, seeded = Counter(), Counter()
    for pr, _ in HAND.values():
        hand.update(npb.set_bad_keyframes(pr, points="kf_slot_off" in pr)["paths"])
    for _, exp in _seeded().values():
        seeded.update(exp["paths"])
    assert set(hand) <= set(npb.PATHS) and set(seeded) <= set(npb.PATHS)
    assert [p for p in npb.PATHS if hand[p] == 0] == []
    assert [p for p in npb.PATHS if seeded[p] == 0] == []


def test_seeded_maps_are_what_the_gpu_tests_need():
    sizes = sorted({pr["nkf"] for pr, _ in _seeded().values()})
    assert sizes == [12, 40, 300]
    pr = _seeded()["n300"][0]
    assert np.diff(pr["conn_off"]).max() >= 280                       # a sort over more than one 256-entry tile
    for pr, _ in _seeded().values():
        assert len(pr["tgt_kf"]) <= 6 and 20 <= np.diff(pr["kf_slot_off"]).mean() <= 40


def test_an_order_blind_variant_answers_differently():
    n = 0
    for name, (pr, exp) in _seeded().items():
        if int(exp["counts"][0]) < 2:
            continue
        n += 1
        blind = npb.order_blind(pr)
        assert not _same(exp, blind), name
        blind = npb.order_blind(pr, points=False)
        assert not _same(npb.set_bad_keyframes(pr, points=False), blind), name
    assert n >= 5
