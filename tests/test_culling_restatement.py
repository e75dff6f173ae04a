"""The restatement of LocalMapping::KeyFrameCulling (tests/npculling.py) against the hand-worked cases of tests/cullingcases.py, and
the conditions the seeded problems must meet so that the GPU comparison (tests/test_gpu_culling.py) cannot pass vacuously: enough
keyframes culled, enough points turned bad, and enough decisions that an order-blind implementation (every candidate scored against
the initial state) gets wrong."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import cullingcases as cc  # noqa: E402
from tests import npculling as npc  # noqa: E402

KEYS = ("culled", "n_redundant", "n_map_points", "pt_bad", "pt_nobs", "obs_erased")
HAND = cc.hand_cases()


@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_gives_the_hand_worked_outputs(name):
    pr, exp = HAND[name]
    got = npc.culling(pr)
    for k in KEYS:
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (name, k, got[k], exp[k])


def test_hand_cases_cover_a_to_i():
    assert sorted(set(n[0] for n in HAND)) == list("abcdefghi")


def test_order_blind_answers_differ_on_the_order_cases():
    for name in ("e_order_AB", "e_order_BA", "f_cascade"):
        pr, exp = HAND[name]
        assert not np.array_equal(npc.culling(pr, sequential=False)["culled"], exp["culled"]), name


def test_generator_is_consistent_and_reproducible():
    a, b = cc.make(3, **cc.CONFIGS["small"][0]), cc.make(3, **cc.CONFIGS["small"][0])
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]
    # keyframe k holds p in a slot iff p's observations contain k, at the same level
    for c, k in enumerate(a["cand_kf"]):
        sl = sorted((int(a["slot_pt"][s]), int(a["slot_level"][s])) for s in range(a["slot_off"][c], a["slot_off"][c + 1]))
        ob = sorted((p, int(a["obs_level"][e])) for p in range(a["npts"]) for e in range(a["obs_off"][p], a["obs_off"][p + 1]) if a["obs_kf"][e] == k)
        assert sl == ob


@pytest.mark.parametrize("name,pr", cc.seeded(), ids=[n for n, _ in cc.seeded()])
def test_seeded_problems_discriminate(name, pr):
    seq = npc.culling(pr)
    par = npc.culling(pr, sequential=False)
    n_culled = int(seq["culled"].sum()); n_differ = int((seq["culled"] != par["culled"]).sum()); n_bad = int(seq["pt_bad"].sum())
    print(name, "culled", n_culled, "differ", n_differ, "bad", n_bad, "do_not_erase culled", int((seq["culled"] & (pr["cand_flags"] >> 1)).sum()))
    if name.startswith("tiny"):
        assert n_differ >= 2
    else:
        assert n_culled >= 10 and n_differ >= 5 and n_bad >= 50
    if name in ("wide-0", "wide-1", "wide-3"):
        assert int((seq["culled"] & (pr["cand_flags"] >> 1)).sum()) >= 1
    if name.startswith("wide"):                                     # two points seen by every keyframe: lists longer than a wave
        assert (np.diff(pr["obs_off"])[:2] == 140).all()
