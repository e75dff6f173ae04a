"""CPU checks of the restatement tests/npmapedit.py (the literal sequential replay of MapPoint::AddObservation / Replace / SetBadFlag over an
edit list) and of the problems tests/mapeditcases.py makes for the GPU tests: the restatement gives the hand-worked outputs, the hand
cases and the seeded maps each take every path, the seeded maps have the sizes the kernels need, and an implementation blind to the
order of the edits answers differently on every seeded map."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import mapeditcases as mc  # noqa: E402
from tests import npmapedit as npm  # noqa: E402

HAND = mc.hand_cases()
KEYS = ("op_status", "op_found", "pt_touched", "kf_slot_pt", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced", "oobs_off", "oobs_kf", "oobs_slot", "oobs_src",
        "oobs_level", "oobs_uv", "counts")


@pytest.fixture(scope="module")
def seeded():
    return {name: (pr, npm.apply_map_edits(pr)) for name, pr in mc.seeded().items()}


@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_gives_the_hand_worked_outputs(name):
    pr, exp = HAND[name]
    got = npm.apply_map_edits(pr)
    assert got["status"] == 0
    for k in KEYS:
        if exp[k] is None:
            assert got[k] is None, (name, k)
        else:
            assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (name, k, got[k], exp[k])


def test_hand_cases_take_every_path():
    paths = Counter()
    for pr, _ in HAND.values():
        paths += npm.apply_map_edits(pr)["paths"]
    assert sorted(paths) == sorted(npm.PATHS), set(npm.PATHS) ^ set(paths)


def test_seeded_maps_take_every_path(seeded):
    paths = Counter()
    for _, exp in seeded.values():
        paths += exp["paths"]
    assert sorted(paths) == sorted(npm.PATHS), set(npm.PATHS) ^ set(paths)
    dead, exp = seeded["big-5-dead"]
    assert exp["paths"]["obs_dead"] > 0 and len(dead["op_kind"]) > 1024
    lo, hi = dead["obs_off"][:-1], dead["obs_off"][1:]
    holes = np.add.reduceat(np.append(dead["obs_dead"], 0).astype(np.int64), lo) * (hi > lo)
    assert ((hi - lo > 64) & (holes > 0)).any()                          # a row longer than a wave with dead entries in it
    assert npm.apply_map_edits(mc.with_dead(seeded["small-1"][0]))["paths"]["obs_dead"] > 0      # (the pure rebuild)
    statuses = set()
    for _, exp in seeded.values():
        statuses |= set(int(v) for v in exp["op_status"])
        assert exp["status"] == 0 and exp["counts"][6] > 0               # (in range throughout; a late add)
    assert statuses == set(range(10))


def test_seeded_maps_have_the_sizes_the_kernels_need(seeded):
    small, big = seeded["small-1"][0], seeded["big-4"][0]
    assert (small["nkf"], small["npts"]) == (8, 60) and 40 <= len(small["op_kind"]) <= 80
    assert (big["nkf"], big["npts"]) == (80, 2000) and len(big["op_kind"]) > 1024
    assert np.diff(big["obs_off"]).max() > 64                            # a list longer than a wave ...
    exp = seeded["big-4"][1]
    assert np.diff(exp["oobs_off"]).max() > 64 and exp["pt_bad"][0] == 1  # ... that merges into another one
    assert mc.long_chain(big) >= 40
    for pr, _ in seeded.values():
        assert sorted(pr["kf_rank"]) == list(range(pr["nkf"])) and list(pr["kf_rank"]) != list(range(pr["nkf"]))
        lists = [list(pr["obs_kf"][pr["obs_off"][p]:pr["obs_off"][p + 1]]) for p in range(pr["npts"])]
        assert all(len(set(r)) == len(r) for r in lists)
        rank = pr["kf_rank"]
        assert any([rank[k] for k in r] != sorted(rank[k] for k in r) for r in lists)       # the input lists are not in rank order
        for p, r in enumerate(lists):                                    # every observation's slot holds its point
            for e in range(pr["obs_off"][p], pr["obs_off"][p + 1]):
                if pr["obs_dead"] is not None and pr["obs_dead"][e]:
                    continue
                assert pr["kf_slot_pt"][pr["kf_slot_off"][pr["obs_kf"][e]] + pr["obs_slot"][e]] == p


def test_an_order_blind_implementation_answers_differently_on_every_seeded_map(seeded):
    for name, (pr, exp) in seeded.items():
        rev = npm.apply_map_edits(mc.reversed_ops(pr))
        assert not np.array_equal(rev["kf_slot_pt"], exp["kf_slot_pt"]), name
        assert not np.array_equal(rev["pt_bad"], exp["pt_bad"]) or not np.array_equal(rev["oobs_kf"], exp["oobs_kf"]), name


def test_out_of_range_ops_are_absent_in_the_restatement():
    pr, exp = HAND["c_replace"]
    ops = mc.ops_of(pr)
    bad = mc.with_ops(pr, ops[:1] + [(mc.ADD, 99, 0, 0, 0), (mc.FUSE, 1, 0, 7, 0), (mc.FIND_OR_ADD, 1, 0, 0, 4), (mc.REPLACE_FOUND, 1, 0, 0, 0), (7, 0, 0, 0, 0)] + ops[1:])
    got = npm.apply_map_edits(bad)
    assert list(got["op_status"]) == [8, 10, 10, 10, 10, 10, 1, 8] and got["status"] == npm.ST_PT | npm.ST_KF | npm.ST_SLOT
    for k in ("kf_slot_pt", "pt_bad", "pt_nobs", "oobs_off", "oobs_kf", "oobs_slot", "oobs_src", "pt_found", "pt_replaced"):
        assert np.array_equal(got[k], exp[k]), k
