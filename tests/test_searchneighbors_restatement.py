"""CPU checks of the SearchInNeighbors restatement (tests/npsearchneighbors.py): it reproduces every hand-worked case of
tests/searchneighborscases.py, the seeded maps take the paths the GPU tests rely on - the chain cases among them -, and the generator
ends for every committed seed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import npsearchneighbors as ns  # noqa: E402
from tests import searchneighborscases as sc  # noqa: E402

_RUNS = {}


def _run(seed):
    if seed not in _RUNS:
        m = sc.make(seed)
        _RUNS[seed] = (m, ns.search_in_neighbors(m["tab"], m["cur_kf"], m["cur_id"]))
    return _RUNS[seed]


@pytest.mark.parametrize("name", sorted(sc.target_cases()))
def test_target_cases(name):
    c = sc.target_cases()[name]
    r = ns.fuse_targets(c["tab"], c["cur_kf"], c["cur_id"], c["nn"], c["nn2"])
    assert r["tgt_kf"].tolist() == c["tgt_kf"] and r["counts"].tolist() == c["counts"] and r["kf_fuse_target"].tolist() == c["kf_fuse_target"]


def test_target_cases_take_every_branch():
    P = sum((ns.fuse_targets(c["tab"], c["cur_kf"], c["cur_id"], c["nn"], c["nn2"])["paths"] for c in sc.target_cases().values()), ns.Counter())
    for k in ("tgt_bad", "tgt_stamped", "tgt_second_bad", "tgt_second_stamped", "tgt_second_is_cur", "tgt_listed_twice", "tgt_cut_first", "tgt_cut_second"):
        assert P[k] > 0, k


def test_row_case():
    c = sc.row_case()
    P = ns.Counter()
    for K, want in c["expect"].items():
        r = ns.fuse_rows(c["tab"], K, c["pts"])
        for k, w in want.items():
            assert r[k].tolist() == w, (K, k)
        assert r["op_kf"].tolist() == [K] * len(c["pts"]) and r["op_arg"].tolist() == [0] * len(c["pts"]) and r["status"] == 0
        P += r["paths"]
    # the projections the case states
    uv = ns.fuse_rows(c["tab"], 0, c["pts"])["q_uv"]
    assert uv[1].tolist() == [0.0, 240.0] and uv[7].tolist() == [576.0, 240.0] and uv[13].tolist() == [325.0, 176.0] and uv[14].tolist() == [638.0, 176.0]
    for k in ("null", "neg_depth", "out_of_image", "too_near", "too_far", "viewing", "level_clamp_high", "no_candidate", "level_window", "chi2", "tie_first_wins",
              "over_th_low", "kp_outside_grid"):
        assert P[k] > 0, k


def test_row_case_tie_tells_cell_order_from_index_order():
    """an index-order tie-break picks the other keypoint of point 13"""
    c = sc.row_case()
    M = ns.Map(c["tab"])
    p = int(c["pts"][13])
    bi, bd, u, v, lvl = M.search(0, p, 3.0)
    cand = M.grid(0).features_in_area(u, v, ns.F32(ns.F32(3.0) * M.sf[lvl]))
    by_index = min(cand, key=lambda i: (int(ns._POP[M.kdesc[0][i] ^ M.desc[p]].sum()), i))
    assert by_index != bi and bi == c["expect"][0]["best_idx"][13] and cand[0] == bi and cand[0] > cand[1]


def test_level_clamp_at_the_bottom_is_counted():
    """PredictScale's lower clamp: reachable through the gates only at dist == 1.2 max, so the restatement is asked directly"""
    c = sc.row_case()
    M = ns.Map(c["tab"])
    assert M.predict_scale(0, ns.F32(M.max_dist[0] * ns.F32(1.5))) == 0 and M.paths["level_clamp_low"] == 1


def test_log_scale_factor_is_the_float_the_reference_holds():
    from ceres_mono_orb_slam2_amd import localmapping
    assert float(ns.LOG_SCALE) == localmapping.LOG_SCALE_FACTOR == float.fromhex("0x1.756506p-3")


def test_candidate_case():
    c = sc.candidate_case()
    r = ns.fuse_candidates(c["tab"], c["tgt_kf"], c["cur_id"])
    assert r["cand_pt"].tolist() == c["cand_pt"] and r["counts"].tolist() == c["counts"] and r["pt_fuse_cand"].tolist() == c["pt_fuse_cand"]
    for k in ("cand_null", "cand_bad", "cand_stamped", "cand_again"):
        assert r["paths"][k] > 0, k
    # with a capacity the points beyond it stay unstamped
    r = ns.fuse_candidates(c["tab"], c["tgt_kf"], c["cur_id"], cap=2)
    assert r["status"] == ns.ST_CAP and r["counts"].tolist() == c["counts"] and r["pt_fuse_cand"].tolist() == [9, 0, 9, 9, 8, 0, 0]


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_generator_ends_and_keeps_the_shapes(seed):
    m, _ = _run(seed)
    t = m["tab"]
    n = np.diff(t["kf_slot_off"])
    assert 10 <= len(n) <= 14 and n.min() >= 40 and n.max() <= 150 and 200 <= len(t["pt_bad"]) <= 400
    M = ns.Map(t)
    for p in range(M.npts):                                                  # no PredictScale quotient near an integer, in any keyframe
        for k in range(M.nkf):
            q = float(ns.log_ratio(M.max_dist[p], ns.F32(np.linalg.norm(M.X[p] - M.center[k]))))
            assert abs(q - round(q)) > sc.NEAR_INTEGER, (p, k, q)
    # the tables are what orbl_apply_map_edits requires: a slot holds the point that observes it, the lists are in rank order
    for p in range(M.npts):
        lst = [(int(t["obs_kf"][e]), int(t["obs_slot"][e])) for e in range(t["obs_off"][p], t["obs_off"][p + 1])]
        assert lst == M.sorted_obs(p) and all(M.mp[k][s] == p for k, s in lst) and t["pt_nobs"][p] == len(lst)


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_seeded_maps_take_the_chain_paths(seed):
    m, r = _run(seed)
    P = r["paths"]
    for k in ("stale_differs", "inherited_skip", "cur_point_bad_skip", "cur_slot_changed", "replace_p", "replace_q", "add", "skip_bad", "skip_in_keyframe", "tgt_listed_twice",
              "tgt_stamped", "tgt_bad", "tgt_cut_second", "cand_null", "cand_bad", "cand_stamped", "cand_again", "chi2", "level_window", "over_th_low", "out_of_image", "q_bad", "viewing"):
        assert P[k] > 0, k
    assert len(r["tgt_kf"]) > len(set(r["tgt_kf"])) and len(r["n_fused"]) == len(r["tgt_kf"]) + 1 and r["n_fused"][-1] > 0
    # the injected point survived its Replace with another descriptor, and holds a keypoint of a later target
    A = m["injected"]
    assert not r["tab"]["pt_bad"][A] and r["tab"]["pt_bad"][A + 1] and r["tab"]["pt_replaced"][A + 1] == A
    assert r["tab"]["pt_nobs"][A] >= 4 and not np.array_equal(r["tab"]["pt_desc"][A], m["tab"]["pt_desc"][A])


def test_in_loop_descriptor_matters():
    """the same map with the descriptors frozen at entry ends elsewhere: the chain cases are not decoration"""
    m, _ = _run(sc.SEEDS[0])

    def first_loop(frozen):
        M = ns.Map(m["tab"])
        if frozen:
            M.compute_distinctive_descriptors = lambda p: None
        tg = ns.fuse_targets(m["tab"], m["cur_kf"], m["cur_id"], M=M)
        snapshot = list(M.mp[m["cur_kf"]])
        for k in tg["tgt_kf"]:
            M.fuse(int(k), snapshot)
        return M.tables()["kf_slot_pt"]
    assert not np.array_equal(first_loop(False), first_loop(True))
