"""The restatement of KeyFrame::UpdateConnections over a keyframe list (tests/npconnections.py) against the hand-worked cases of
tests/connectioncases.py, and the conditions the problems must meet so that the GPU comparison (tests/test_gpu_connections.py) cannot
pass vacuously: every path of the loop is taken, and an order-blind implementation (every list = its keyframe's own entries >= th)
answers differently."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import connectioncases as cc  # noqa: E402
from tests import npconnections as npc  # noqa: E402

KEYS = ("tgt_status", "tgt_parent", "counts", "aff_kf", "conn_off", "conn_kf", "conn_w", "ord_off", "ord_kf", "ord_w", "link_off", "link_kf")
HAND = cc.hand_cases()
SEEDED = cc.seeded()


def _same(got, exp, what):
    for k in KEYS:
        if exp[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k] is not None and got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k, got[k], exp[k])


@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_gives_the_hand_worked_outputs(name):
    pr, exp = HAND[name]
    _same(npc.connections(pr), exp, name)


def test_hand_cases_cover_a_to_g():
    assert sorted(n[0] for n in HAND) == list("abcdefg")


def test_every_path_is_taken_by_the_hand_cases_and_by_the_seeded_maps():
    for what, problems in (("hand", [pr for pr, _ in HAND.values()]), ("seeded", [pr for _, pr in SEEDED])):
        total = dict.fromkeys(npc.PATHS, 0)
        for pr in problems:
            for k, v in npc.connections(pr)["paths"].items():
                total[k] += v
        print(what, total)
        assert all(total[k] >= 1 for k in npc.PATHS), (what, total)


def test_sparse_keyframes_give_the_empty_counter_and_the_fallback_in_every_seeded_map():
    for name, pr in SEEDED:
        p = npc.connections(pr)["paths"]
        assert p["empty"] >= 1 and p["fallback"] >= 1, name


def test_order_blind_answers_differ_on_the_seeded_maps():
    differ = 0
    for name, pr in SEEDED:
        a, b = npc.connections(pr), npc.connections(pr, order_blind=True)
        differ += not (np.array_equal(a["ord_off"], b["ord_off"]) and np.array_equal(a["ord_kf"], b["ord_kf"]))
    assert differ == len(SEEDED)
    pr, exp = HAND["d_resort_brings_in_below_th"]
    assert not np.array_equal(npc.connections(pr, order_blind=True)["ord_kf"], exp["ord_kf"])


def test_generator_is_reproducible_and_its_maps_are_consistent():
    a, b = cc.make(3, nkf=30), cc.make(3, nkf=30)
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]
    # a target holds p in a slot iff p's observations contain the target
    for t, k in enumerate(a["tgt_kf"]):
        sl = sorted(int(p) for p in a["slot_pt"][a["slot_off"][t]:a["slot_off"][t + 1]] if p >= 0)
        ob = sorted(p for p in range(a["npts"]) if k in a["obs_kf"][a["obs_off"][p]:a["obs_off"][p + 1]])
        assert sl == ob
    # the tables at entry: no row names itself or a keyframe twice
    for k in range(a["nkf"]):
        row = a["conn_kf"][a["conn_off"][k]:a["conn_off"][k + 1]].tolist()
        assert k not in row and len(set(row)) == len(row)
