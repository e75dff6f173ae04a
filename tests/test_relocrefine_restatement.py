"""CPU checks behind orbt_relocalization_refine's tests.
(1) The early-exit argument on the toy model (tests/nprelocrefine.py: lists of candidate features per point, no geometry): the literal
    `for (ip < N_)` loop of src/Tracking.cc:1096-1104 - one SearchByProjection per ip - and the loop stopped at its first empty pass leave
    the same slots and the same nadditional, over 4000 seeds, both orientation-check values, duplicated point ids.
(2) The same on the real restatement over the oracle for the cases that reach the narrow search.
(3) The case set (tests/relocrefinecases.py) reaches every stage that CAN be reached under the default flag, and the third solve under
    narrow_in_loop = 0.

About (3).  Under the default flag MATCH_THIRD and FAIL_THIRD cannot be reached, by the argument that makes the loop cheap: the third solve
needs nadditional != 0, nadditional is the return value of pass N_ - 1, and that pass assigns something only if every one of the N_
passes did (an empty pass empties all later ones).  Each non-empty pass keeps at least one match in a slot that was free when the loop
began, so N_ non-empty passes need N_ free slots - but the loop is entered with nGood > 30 slots filled.  So pass N_ - 1 is always empty,
nadditional is always 0 and `nGood + nadditional >= 50` fails with nGood < 50: the default flag ends in FAIL_NARROW whenever it enters
the narrow search.  The test asserts exactly that (the seven reachable stages are reached, the two others are not), and a non-empty last
pass - which the issue asks for "if you can construct one" - does not exist."""
import numpy as np
import pytest

from tests import nprelocrefine as R
from tests import relocrefinecases as RC


def test_literal_loop_equals_early_exit_loop_on_toy_lists():
    most = total = nonzero = dups = 0
    for seed in range(4000):
        ori = bool(seed & 1)
        a = R.toy_loop(seed, ori, False)
        b = R.toy_loop(seed, ori, True)
        assert a[0] == b[0] and a[1] == b[1], (seed, a, b)
        N, pid, _, _, _ = R.toy_instance(seed)
        assert a[2] == N and b[2] <= N
        most = max(most, b[2]); total += b[2]; nonzero += a[1] != 0
        dups += len([p for p in pid if p >= 0]) != len(set(p for p in pid if p >= 0))
    print("early-exit form: at most %d passes, %.2f on average; nadditional != 0 in %d instances; %d instances with a duplicated id" % (most, total / 4000, nonzero, dups))
    assert nonzero == 0 and dups > 500 and most >= 5


def test_three_maxima_keeps_the_first_fullest_bin():
    assert R.three_maxima([0] * 30) == (-1, -1, -1)
    assert R.three_maxima([0, 4, 0, 4, 1]) == (1, 3, 4)
    assert R.three_maxima([0, 40, 3, 3]) == (1, -1, -1)
    assert R.three_maxima([0, 40, 4, 3]) == (1, 2, -1)


@pytest.fixture(scope="module")
def results(oracle):
    _, F, _, _ = RC.two_frames(oracle)
    out = {}
    for flag in (True, False):
        paths = {}
        out[flag] = ({name: R.refine(oracle, F, RC.candidate(oracle, **kw), True, flag, paths=paths) for name, kw in RC.CASES.items()}, paths)
    return out


def test_case_set_reaches_every_reachable_stage(results):
    res, paths = results[True]
    for name, r in res.items():
        print("%-22s %-12s nGood %s nadditional %s correspondences %s passes %d" % (name, R.STAGE_NAMES[r["stage"]], r["n_good"], r["n_additional"], r["n_correspondences"], r["narrow_passes"]))
    stages = set(r["stage"] for r in res.values())
    assert stages == {R.NO_POSE, R.FEW_INLIERS, R.MATCH_FIRST, R.MATCH_SECOND, R.FAIL_WIDE, R.FAIL_SECOND, R.FAIL_NARROW}
    assert res["no_pose"]["n_correspondences"] == [-1, -1, -1] and res["two_correspondences"]["stage"] == R.NO_POSE
    assert res["two_correspondences"]["n_correspondences"][0] == 2 and res["three_correspondences"]["n_correspondences"][0] == 3
    assert res["three_correspondences"]["stage"] == R.FEW_INLIERS
    for k in ("no_pose", "few_inliers", "wide_search", "second_solve", "narrow_search", "matched"):
        assert paths.get(k, 0) > 0, k
    assert "third_solve" not in paths and "narrow_added" not in paths        # (the module's docstring: it cannot be otherwise)
    narrow = [r for r in res.values() if r["n_additional"][1] >= 0]
    assert len(narrow) >= 2 and all(r["narrow_passes"] == len(r["slot_kf"]) and r["n_additional"][1] == 0 and r["stage"] == R.FAIL_NARROW for r in narrow)
    # the passes are not idle: the narrow loop leaves more slots filled than the second solve saw
    assert any((r["slot_kf"] >= 0).sum() > r["n_correspondences"][1] for r in narrow)
    # quirks: outlier slots are cleared behind the first solve, and stay behind the second
    r = res["narrow"]
    assert (r["outlier"] & (r["slot_kf"] >= 0)).any()
    r = res["fail_wide"]
    assert not (r["outlier"] & (r["slot_kf"] >= 0)).any() and r["outlier"].any()


def test_case_set_reaches_the_third_solve_behind_the_loop(results):
    res, paths = results[False]
    assert res["narrow"]["stage"] == R.MATCH_THIRD and res["narrow_third_fails"]["stage"] == R.FAIL_THIRD
    assert paths["third_solve"] == 2 and paths["narrow_added"] >= 2
    for name in ("narrow", "narrow_third_fails"):
        r = res[name]
        assert r["narrow_passes"] == 1 and r["n_additional"][1] > 0 and r["n_good"][2] >= 0 and not (r["outlier"] & (r["slot_kf"] >= 0)).any()
    for name, r in res.items():                                                 # everything in front of the narrow search does not see the flag
        d = results[True][0][name]
        assert r["n_good"][:2] == d["n_good"][:2] and r["n_additional"][0] == d["n_additional"][0]


def test_restatement_early_exit_equals_literal_loop(oracle, results):
    _, F, _, _ = RC.two_frames(oracle)
    for name in ("narrow", "narrow_third_fails", "match_second"):
        for ori in (True, False):
            c = RC.candidate(oracle, **RC.CASES[name])
            a = R.refine(oracle, F, c, ori, True) if not ori else results[True][0][name]
            b = R.refine(oracle, F, c, ori, True, early_exit=True)
            for k in a:
                if k != "narrow_passes":
                    assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (name, ori, k)
            assert b["narrow_passes"] <= a["narrow_passes"]
            if name != "match_second":
                assert 2 <= b["narrow_passes"] < 20 and a["narrow_passes"] == len(F["kps4"])


def test_duplicate_ids_share_one_set_element(oracle):
    """A point held at two keyframe features: once it sits in a slot, `found` keeps BOTH features out of the search."""
    _, F, _, _ = RC.two_frames(oracle)
    c = RC.candidate(oracle, **RC.CASES["match_second"])
    ids, cnt = np.unique(c["pt"][c["pt"] >= 0], return_counts=True)
    twice = ids[cnt == 2]
    assert len(twice) == 3
    r = R.refine(oracle, F, c, True, True)
    held = c["pt"][r["slot_kf"][r["slot_kf"] >= 0]]
    # unique ids instead: the second feature of each pair becomes a point of its own and is matched as well
    u = dict(c, pt=c["pt"].copy())
    for i in twice:
        k = np.nonzero(c["pt"] == i)[0][1]
        u["pt"][k] = 10 ** 6 + k
    r2 = R.refine(oracle, F, u, True, True)
    print("slots filled with duplicated ids %d, with unique ids %d" % ((r["slot_kf"] >= 0).sum(), (r2["slot_kf"] >= 0).sum()))
    assert len(held) >= 200 and r["stage"] == r2["stage"] == R.MATCH_SECOND
