"""CPU evidence for the restatement that the GPU tests of orbl_loop_sim3_candidates compare with (tests/nploopsim3.py): its search equals
the C++ oracle's SearchByBoW(KeyFrame*, KeyFrame*) per candidate, the hand-worked cases come out as worked, and the cases provably take
every path - a count per path is asserted, so an implementation that ignores list order, the rotation check's vbMatched2 or the
observation tables answers differently on these inputs.

Two of the constructor's four skip reasons cannot follow a SearchByBoW on unchanged tables: the search only matches slots that hold a point
which is not bad, so `!map_point_1` and `isBad()` (src/Sim3Solver.cc:78-80) are reached only with a match vector from elsewhere.  The
constructor's loop is therefore also run on match vectors written by hand (test_constructor_skips_for_each_reason)."""
import numpy as np
import pytest

from tests import loopsim3cases as lc
from tests import nploopsim3 as NL


@pytest.fixture(scope="module")
def seeded():
    return [lc.make(s) for s in lc.SEEDS]


def _oracle_search(oracle, tab, k1, k2, check_ori=True):
    d1, v1, a1 = NL.search_inputs(tab, k1)
    d2, v2, a2 = NL.search_inputs(tab, k2)
    return oracle.search_by_bow(d1, v1, a1, d2, v2, a2, NL.feature_vector(tab, k1), NL.feature_vector(tab, k2), ratio=0.75, th=50, strict=True, check_ori=check_ori)


def _pairs(seeded):
    out = [(tab, cur, int(k)) for _, tab, cur, cand, _ in lc.hand_cases() for k in cand]
    tab, cur, cand, _ = lc.gate_case()
    out += [(tab, cur, int(k)) for k in cand]
    for m in seeded[:4]:
        out += [(m["tab"], m["cur_kf"], int(k)) for k in m["cand_kf"]]
    m = lc.seam_case()
    out += [(m["tab"], m["cur_kf"], int(k)) for k in m["cand_kf"][[0, -1]]]
    return out


def test_search_equals_the_oracle(oracle, seeded):
    n = 0
    for tab, cur, k2 in _pairs(seeded):
        for check_ori in (True, False):
            nm, m12 = NL.search_by_bow(tab, cur, k2, 0.75, check_ori)
            onm, om12 = _oracle_search(oracle, tab, cur, k2, check_ori)
            assert nm == onm and np.array_equal(m12, om12), (cur, k2, check_ori)
            n += nm
    assert n > 2000


def test_hand_cases_come_out_as_worked():
    for name, tab, cur, cand, want in lc.hand_cases():
        r = NL.sim3_candidates(tab, cur, cand, **want["args"])
        for k, v in want.items():
            if k != "args":
                assert np.array_equal(np.asarray(r[k], np.float64), np.asarray(v, np.float64)), (name, k, r[k])
        assert r["counts"].tolist() == [want["off"][-1], sum(s == 0 for s in want["cand_status"])], name


def test_the_gate_case():
    tab, cur, cand, want = lc.gate_case()
    r = NL.sim3_candidates(tab, cur, cand)
    assert r["nmatches"].tolist() == want["nmatches"] and r["cand_status"].tolist() == want["cand_status"] and r["off"].tolist() == want["off"]
    # one candidate with 19 matches and one with 20; one kept with >= 20 matches and fewer than 20 rows; a bad keyframe
    assert 19 in r["nmatches"] and 20 in r["nmatches"] and 1 in r["cand_status"]
    assert any(r["cand_status"][c] == 0 and r["nmatches"][c] >= 20 and r["off"][c + 1] - r["off"][c] < 20 for c in range(len(cand)))


def test_constructor_skips_for_each_reason():
    """slot 0: a row; slot 1: no match; slot 2: holds no point; slot 3: its own point is bad; slot 4: the matched point is bad; slot 5: no
    observation of the current keyframe; slot 6: the matched point has none of the candidate"""
    B = lc.Builder()
    k0, k1 = B.keyframe(), B.keyframe()
    D = np.zeros(32, np.uint8)
    p = [B.point((i, 0, 2), bad=i in (3, 11)) for i in range(14)]
    for i in range(7):
        B.slot(k0, -1 if i == 2 else p[i], D, 0.0, i)
        B.slot(k1, p[7 + i], D, 0.0, 7 - i)
    B.observe(p[5], k0, None); B.observe(p[13], k1, None)
    tab = B.tables()
    skipped = {}
    rows = NL.constructor_rows(tab, k0, k1, [0, -1, 2, 3, 4, 5, 6], skipped)
    assert [r["i1"] for r in rows] == [0] and (rows[0]["pt1"], rows[0]["pt2"]) == (p[0], p[7])
    assert skipped == {NL.SKIP_NO_MATCH: 1, NL.SKIP_NO_POINT1: 1, NL.SKIP_BAD_POINT: 2, NL.SKIP_NO_INDEX: 2}


def test_the_seeded_maps_take_every_path(seeded):
    for m in seeded:
        tab, cur, cand = m["tab"], m["cur_kf"], m["cand_kf"]
        skipped = {}
        r = NL.sim3_candidates(tab, cur, cand, min_matches=8, skipped=skipped)
        assert 1 in r["cand_status"] and 0 in r["cand_status"], "a bad candidate keyframe and a kept one"
        assert skipped.get(NL.SKIP_NO_MATCH, 0) > 0 and skipped.get(NL.SKIP_NO_INDEX, 0) > 0
        assert r["counts"][0] > 20
        lo1 = int(tab["kf_slot_off"][cur])
        # a point whose observation of the keyframe names another slot, with another octave, than the slot it sits in - among the ROWS
        moved = sum(1 for q in r["_rows"] if q["x1"] != q["i1"] and tab["kf_slot_level"][lo1 + q["x1"]] != tab["kf_slot_level"][lo1 + q["i1"]])
        assert moved > 0
        # a point with no observation of the keyframe, among the matched slots
        none = sum(1 for c in range(len(cand)) if r["cand_status"][c] == 0 for i1 in np.nonzero(r["match12"][c] >= 0)[0]
                   if NL.index_in_keyframe(tab, int(tab["kf_slot_pt"][lo1 + i1]), cur) < 0)
        assert none > 0
        tot = dict(one_sided_nodes=0, tied_best=0, tied_runner_up=0, rotation_rejected=0, blocked=0)
        for c, k2 in enumerate(int(k) for k in cand):
            if r["cand_status"][c] == 1:
                continue
            m12, cnt = NL.search_paths(tab, cur, k2, 0.75, True)
            assert np.array_equal(m12, r["match12"][c]), "the counted walk is the checked search"
            for k in tot:
                tot[k] += cnt[k]
        assert all(v > 0 for v in tot.values()), tot


def test_the_seam_case_reaches_the_far_end_of_long_lists():
    m = lc.seam_case()
    tab, cur = m["tab"], m["cur_kf"]
    r = NL.sim3_candidates(tab, cur, m["cand_kf"][[0, -1]], min_matches=1)
    # a match beyond position 256 of a candidate's node list: the kernel's tail from memory
    n2, i2, e2 = NL.feature_vector(tab, int(m["cand_kf"][0]))
    deep = {int(s) for q in range(len(n2)) for s in e2[i2[q] + 256:i2[q + 1]]}
    assert len(deep) > 0 and len(deep & set(r["match12"][0].tolist())) > 0
    assert r["cand_status"].tolist() == [0, 2] and r["nmatches"][1] == 0, "a candidate without feature-vector nodes matches nothing"
