"""CPU checks of the yardstick of the UpdateLocalMap tests: the hand-worked cases of tests/localmapcases.py equal the restatement
tests/nplocalmap.py key by key, the seeded problems reproduce the table recorded beside them, every path of the keyframe walk (the
parent-break, the > 80 stop, the no-vote return) is taken by at least one seed, and the problems tell the reference's quirks from the
plausible alternatives (index order instead of rank order, a walk that goes on after a parent, a bad parent left out)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import localmapcases as lc  # noqa: E402
from tests import nplocalmap as nlm  # noqa: E402


def test_hand_worked_cases_equal_the_restatement():
    H = lc.hand_cases()
    assert len(H) == 15
    for name, (pr, exp) in H.items():
        r = nlm.update_local_map(pr)
        for k, v in exp.items():
            assert np.array_equal(np.asarray(r[k]).reshape(-1), np.asarray(v).reshape(-1)), (name, k, r[k], v)
        assert r["n_local_kf"] == len(exp["local_kf"]) and r["n_local_pt"] == len(exp["local_pt"])


def test_seeded_problems_reproduce_their_table_and_take_every_path():
    taken = dict(parent_break=0, stop80=0, no_votes=0)
    names = []
    for name, pr in lc.seeded():
        r = nlm.update_local_map(pr)
        paths = tuple(k for k in ("no_votes", "stop80", "parent_break") if r["paths"][k])
        assert (r["n_local_kf"], r["n_local_pt"], paths) == lc.TABLE[name], name
        for k in paths:
            taken[k] += 1
        names.append(name)
        # the marks are exactly the lists
        assert sorted(np.nonzero(r["pt_mark"])[0]) == sorted(r["local_pt"])
        if r["status"] == nlm.OK:
            assert sorted(np.nonzero(r["kf_mark"])[0]) == sorted(r["local_kf"])
    assert sorted(names) == sorted(lc.TABLE)
    assert taken == dict(parent_break=4, stop80=2, no_votes=1)


def test_the_cases_tell_the_quirks_from_their_alternatives():
    H = lc.hand_cases()
    # rank order, not index order: with the identity rank the tie goes to keyframe 0
    pr, exp = H["b_tie_by_rank"]
    q = dict(pr); q["kf_rank"] = None
    assert nlm.update_local_map(q)["ref_kf"] == 0 and exp["ref_kf"] == 2
    # a walk that went on after the parent would reach keyframe 3
    pr, exp = H["e_parent_ends_walk"]
    q = dict(pr); q["kf_parent"] = np.full(4, -1, np.int32)
    assert list(nlm.update_local_map(q)["local_kf"]) == [0, 1, 3] and exp["local_kf"] == [0, 1, 2]
    # the bad keyframe 1 of case (d) enters as a parent; as a neighbour it would not
    pr, exp = H["d_bad_parent"]
    q = dict(pr); q["kf_parent"] = np.full(2, -1, np.int32); q["cov_off"] = np.array([0, 1, 1], np.int32); q["cov_kf"] = np.array([1], np.int32)
    assert list(nlm.update_local_map(q)["local_kf"]) == [0] and exp["local_kf"] == [0, 1]
    # 80 voted keyframes allow one iteration, 81 none: the same neighbour lists, another outcome
    assert H["f_voted_80"][1]["local_pt"] == [0, 1] and H["f_voted_81"][1]["local_pt"] == [0]
