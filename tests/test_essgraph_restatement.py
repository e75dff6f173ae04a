"""CPU checks of the test infrastructure of orbl_essential_graph_assemble / orbl_essential_graph_apply: the restatement tests/npessgraph.py
gives the edge list worked out by hand for the map of tests/essgraphcases.hand_map, names the same edges in the same order as
tests/dropin_checker.optimize_essential_graph on that map's state, and no seeded map is vacuous.  These call nothing of the library
(tests/test_essgraph_abi.py and tests/test_gpu_essgraph*.py are the ones that need the feature)."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import essgraphcases as ec  # noqa: E402
from tests import npessgraph as npe  # noqa: E402

_SEEDED = []
SEEDED_SHAPES = ((41, 300, 3000), (42, 700, 2500))                  # nkf crosses one and two scan units of 256


def seeded():
    """every seeded map with its restated outputs (assembled, a stand-in solver result, applied), computed once and shared"""
    if not _SEEDED:
        for seed, nkf, npts in SEEDED_SHAPES:
            m = ec.seeded_map(seed, nkf, npts)
            asm = npe.assemble(m)
            opt = ec.solver_result(900 + seed, asm["lie7"])
            _SEEDED.append(("nkf %d" % nkf, m, asm, opt, npe.apply(m, asm["vtx_kf"], asm["lie7"], opt)))
    return _SEEDED


def test_restatement_reproduces_the_hand_worked_map():
    m, hand = ec.hand_map()
    got = npe.assemble(m)
    for k in ("vtx_kf", "kf_vtx", "vtx_fixed", "counts"):
        assert got[k].tolist() == hand[k], k
    assert got["edges"] == hand["edges"]
    assert got["edge_kind"].tolist() == [k for _, _, k in hand["edges"]]
    assert got["edge_j"].tolist() == [hand["kf_vtx"][j] for j, _, _ in hand["edges"]] and got["edge_i"].tolist() == [hand["kf_vtx"][i] for _, i, _ in hand["edges"]]
    # keyframe 0 is at the identity pose: its block is the zero tangent, and its parent edge to keyframe 1 is keyframe 1's pose inverted
    assert got["lie7"][hand["kf_vtx"][0]].tolist() == [0.0] * 7
    # the group's blocks are the logarithms of the corrected Sim3s (scale 1.1), the others have scale 1
    for v, k in enumerate(hand["vtx_kf"]):
        assert abs(got["lie7"][v][6] - (np.log(1.1) if k in (4, 5, 6) else 0.0)) < 1e-12, k
    # a loop connection is exp(block j) * exp(block i)^-1 - the CORRECTED Sim3 of keyframe 6 - and a parent edge inside the group uses the non-corrected ones
    from oracle import pyoracle as po
    assert np.abs(got["edge_Sji"][0] - po.sim3_inverse(m["corrected"][2])).max() < 1e-12
    assert np.abs(got["edge_Sji"][7] - po.sim3_mul(m["non_corrected"][1], po.sim3_inverse(m["non_corrected"][2]))).max() < 1e-12
    lie_opt = ec.solver_result(5, got["lie7"])
    out = npe.apply(m, got["vtx_kf"], got["lie7"], lie_opt, normal=np.full((6, 3), ec.POISON), min_max=np.full((6, 2), ec.POISON, np.float32))
    assert out["pt_moved"].tolist() == hand["pt_moved"] and out["nd_written"].tolist() == hand["nd_written"] and out["counts"].tolist() == hand["apply_counts"]
    assert np.array_equal(out["kf_Tcw"][3], m["kf_Tcw"][3]) and not np.array_equal(out["kf_Tcw"][0], m["kf_Tcw"][0])      # (the bad keyframe keeps its pose)
    stay = [p for p in range(6) if not hand["pt_moved"][p]]
    assert np.array_equal(out["X"][stay], m["X"][stay]) and np.all(out["normal"][[1, 3, 4, 5]] == ec.POISON)
    # lie_opt = lie_orig: every point stays where it is, to rounding
    same = npe.apply(m, got["vtx_kf"], got["lie7"], got["lie7"])
    assert np.abs(same["X"] - m["X"]).max() < 1e-12


class _Recorder:
    """the oracle handed to dropin_checker: the Sim3 arithmetic is the CPU oracle's, the solve records its edge list and moves nothing"""

    def __init__(self):
        from oracle import pyoracle as po
        self.po = po
        self.problem = None

    def __getattr__(self, name):
        return getattr(self.po, name)

    def optimize_essential_graph(self, lie, fixed, ej, ei, es, max_iters=100):
        self.problem = (np.array(lie), np.array(fixed), np.array(ej), np.array(ei), np.array(es))
        return np.array(lie), {}

    def essential_graph_correct(self, lie, lie_opt, ref, pts):
        return np.zeros((len(lie), 12)), np.array(pts, np.float64).reshape(-1, 3)


def _scene(m):
    """the state of tests/dropin_checker.Scene that optimize_essential_graph reads, from the tables"""
    rank = npe._ranks(m)
    kfs = []
    for k in range(m["nkf"]):
        T = np.eye(4); T[:3, :] = m["kf_Tcw"][k].reshape(3, 4)
        row = lambda off, arr: [int(v) for v in m[arr][m[off][k]:m[off][k + 1]]]
        kf = types.SimpleNamespace(id=int(m["kf_id"][k]), bad=bool(m["kf_bad"][k]), T=T, parent=int(m["kf_parent"][k]), children=set(row("child_off", "child_kf")),
                                   loop_edges=sorted(row("loop_off", "loop_kf"), key=lambda v: rank[v]), conn=row("ord_off", "ord_kf"), conn_w=row("ord_off", "ord_w"),
                                   weights=dict(zip(row("conn_off", "conn_kf"), row("conn_off", "conn_w"))))
        kf.set_pose = lambda T, kf=kf: setattr(kf, "T", np.array(T))
        kfs.append(kf)
    n = m["npts"]
    return types.SimpleNamespace(kfs=kfs, map_kfs=sorted(range(m["nkf"]), key=lambda k: rank[k]), map_mps=list(range(n)), mp_bad=[bool(v) for v in m["pt_bad"]],
                                 corrected_by=[int(m["kf_id"][m["cur"]]) if d else -1 for d in m["pt_done"]],
                                 corrected_ref=[int(m["kf_id"][c]) if c >= 0 else -1 for c in m["pt_corr_ref"]], ref_kf=[int(v) for v in m["pt_ref_kf"]],
                                 pos=np.array(m["X"]), n_update_normal=[0] * n)


def _checker_problem(m):
    """tests/dropin_checker walks its std::map / std::set by keyframe INDEX (its scenes hold the keyframes in pointer order), so the map is
    first renumbered by rank"""
    from tests import dropin_checker as dc
    rank = npe._ranks(m)
    S = _scene(m)
    new = {k: rank[k] for k in range(m["nkf"])}                      # old index -> new index
    S2 = types.SimpleNamespace(**vars(S))
    S2.kfs = [None] * m["nkf"]
    for k, kf in enumerate(S.kfs):
        q = types.SimpleNamespace(**vars(kf))
        q.parent = new[kf.parent] if kf.parent >= 0 else -1; q.children = {new[c] for c in kf.children}; q.loop_edges = sorted(new[c] for c in kf.loop_edges)
        q.conn = [new[c] for c in kf.conn]; q.weights = {new[c]: w for c, w in kf.weights.items()}
        q.set_pose = lambda T, q=q: setattr(q, "T", np.array(T))
        S2.kfs[new[k]] = q
    S2.map_kfs = list(range(m["nkf"]))
    S2.ref_kf = [new[r] if r >= 0 else -1 for r in S.ref_kf]
    non = {new[int(k)]: m["non_corrected"][c] for c, k in enumerate(m["conn_group_kf"])}
    cor = {new[int(k)]: m["corrected"][c] for c, k in enumerate(m["conn_group_kf"])}
    lc = {new[int(t)]: [new[int(v)] for v in m["link_kf"][m["link_off"][c]:m["link_off"][c + 1]]] for c, t in enumerate(m["tgt_kf"])}
    rec = _Recorder()
    n_edges = dc.optimize_essential_graph(S2, rec, new[m["loop"]], new[m["cur"]], non, cor, lc)
    return n_edges, rec.problem


def test_restatement_names_the_edges_of_the_dropin_checker_in_its_order():
    m, hand = ec.hand_map()
    got = npe.assemble(m)
    n_edges, (lie, fixed, ej, ei, es) = _checker_problem(m)
    assert n_edges == len(hand["edges"])
    assert ej.tolist() == got["edge_j"].tolist() and ei.tolist() == got["edge_i"].tolist() and fixed.tolist() == got["vtx_fixed"].tolist()
    assert np.abs(lie - got["lie7"]).max() < 1e-12 and np.abs(es - got["edge_Sji"]).max() < 1e-12
    m2 = ec.seeded_map(7, 40, 50, n_group=6)
    got = npe.assemble(m2)
    n_edges, (lie, fixed, ej, ei, es) = _checker_problem(m2)
    assert n_edges == got["counts"][1] > 20 and ej.tolist() == got["edge_j"].tolist() and ei.tolist() == got["edge_i"].tolist()
    assert np.abs(es - got["edge_Sji"]).max() < 1e-12


def test_no_seeded_map_is_vacuous_and_sizes_cross_the_scan_units():
    sizes = []
    for name, m, asm, opt, out in seeded():
        kinds = np.bincount(asm["edge_kind"], minlength=4)
        assert np.all(kinds >= 3), (name, kinds)
        assert asm["counts"][3] >= 2 and asm["counts"][0] < m["nkf"], name                    # dropped edges, bad keyframes
        assert not np.array_equal(m["kf_rank"], np.arange(m["nkf"])), name
        lens = np.diff(m["ord_off"])
        allpass = [k for k in range(m["nkf"]) if lens[k] and m["ord_w"][m["ord_off"][k + 1] - 1] >= 100]
        straddle = [k for k in range(m["nkf"]) if lens[k] and m["ord_w"][m["ord_off"][k]] >= 100 > m["ord_w"][m["ord_off"][k + 1] - 1]]
        assert len(allpass) >= 5 and len(straddle) >= 20, name
        for k in range(m["nkf"]):                                    # the ordered lists are sorted by weight
            w = m["ord_w"][m["ord_off"][k]:m["ord_off"][k + 1]]
            assert np.all(np.diff(w) <= 0), (name, k)
        ids = m["kf_id"][m["kf_bad"] == 0]
        assert len(set(ids.tolist())) == len(ids), name              # the precondition
        assert 0 < out["pt_moved"].sum() < m["npts"] and 0 < out["nd_written"].sum() < out["pt_moved"].sum(), name
        assert np.any(m["pt_done"][out["pt_moved"] == 1]) and np.any(m["pt_ref_kf"] == -1), name
        sizes.append(m["nkf"])
    assert min(sizes) > 256 and max(sizes) > 512
