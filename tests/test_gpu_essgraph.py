"""orbl_essential_graph_assemble(_device) and orbl_essential_graph_apply(_device) on the MI355X against the restatement tests/npessgraph.py
(the literal loops of src/CeresOptimizer.cc:769-956).  Integer outputs - vertices, edges, kinds, counts, flags, status words - are compared
==.  The floating outputs pass through the device's sin / cos / atan2 / log / exp, which are not the host's, so they are compared with the
project's bound for exactly this arithmetic, _close(..., 1e-12) of tests/test_gpu_essential_graph.py: |a - b| <= 1e-12 * max(1, max|b|).
Normals and depth ranges get no tolerance of their own: orbl_update_map_points on the apply's own X and centres must give the same bits.
Host and device forms, and two runs, give the same bytes.  Rows a call must leave alone are poisoned first."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import essgraphcases as ec  # noqa: E402
from tests import npessgraph as npe  # noqa: E402
from tests.test_essgraph_restatement import seeded  # noqa: E402
from tests.test_gpu_essential_graph import _close as _close_nonempty  # noqa: E402

pytestmark = pytest.mark.gpu

ASM_DT = dict(vtx_kf=(np.int32, 1, 0), lie7=(np.float64, 7, 0), vtx_fixed=(np.uint8, 1, 0), edge_j=(np.int32, 1, 1), edge_i=(np.int32, 1, 1), edge_Sji=(np.float64, 7, 1),
              edge_kind=(np.uint8, 1, 1))
ASM_INT = ("vtx_kf", "kf_vtx", "vtx_fixed", "edge_j", "edge_i", "edge_kind", "counts")
ASM_FLT = ("lie7", "edge_Sji")
ASM_KEYS = ASM_INT + ASM_FLT
AP_INT = ("pt_moved", "nd_written", "counts")
AP_FLT = ("kf_Tcw", "kf_center", "X")
AP_KEYS = AP_INT + AP_FLT + ("normal", "min_max")
TABLES = ("kf_id", "kf_bad", "kf_rank", "kf_Tcw", "kf_parent", "child_off", "child_kf", "loop_off", "loop_kf", "conn_off", "conn_kf", "conn_w", "ord_off", "ord_kf", "ord_w",
          "conn_group_kf", "corrected", "non_corrected", "tgt_kf", "link_off", "link_kf", "kf_center", "X", "pt_bad", "pt_done", "pt_corr_ref", "pt_ref_kf", "obs_off", "obs_kf",
          "ref_level", "scale_factors")
HAND_MAP, HAND = ec.hand_map()
SMALL = ec.small_cases()


def _close(a, b, rtol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and (a.size == 0 or bool(_close_nonempty(a, b, rtol)))           # (an empty table has nothing to compare)


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _t(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).cuda()              # (a copy: the shared maps are read-only)


def _tab(m, conv=lambda v: v):
    return {k: conv(m.get(k)) for k in TABLES}


def _caps(m):
    return m["nkf"], len(m["link_kf"]) + m["nkf"] + len(m["loop_kf"]) + len(m["ord_kf"])


def _poison(m, cap):
    return {k: np.full(w * cap[c], 99 if dt == np.uint8 else ec.POISON, dt) for k, (dt, w, c) in ASM_DT.items()}


def _asm_host(m, caps=None, check=True):
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    cap = _caps(m) if caps is None else caps
    pres = _poison(m, cap)
    r = lc.essential_graph_assemble(m["loop"], m["cur"], _tab(m), min_weight=m["min_weight"], caps=cap, out=pres, check=check)
    if r["rc"] == 0:
        n = (int(r["counts"][0]), int(r["counts"][1]))
        for k, (dt, w, c) in ASM_DT.items():                        # what lies behind the lists is not touched
            assert np.all(pres[k][w * n[c]:] == (99 if dt == np.uint8 else dt(ec.POISON))), k
    else:
        for k, (dt, w, c) in ASM_DT.items():                        # ORBHIP_ECAP: only counts[] is written
            assert np.all(pres[k] == (99 if dt == np.uint8 else dt(ec.POISON))), k
    return r


def _asm_device(m, caps=None, tab=None):
    import torch
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    cap = _caps(m) if caps is None else caps
    pres = {k: _t(v) for k, v in _poison(m, cap).items()}
    r = lc.essential_graph_assemble(m["loop"], m["cur"], _tab(m, _t) if tab is None else tab, min_weight=m["min_weight"], caps=cap, out=pres, device=True)
    torch.cuda.synchronize()
    o = {k: r[k].cpu().numpy() for k in ASM_KEYS}
    o["status"] = int(r["status"].item()) & 0xFFFFFFFF
    n = (int(o["counts"][0]), int(o["counts"][1]))
    for k, (dt, w, c) in ASM_DT.items():                            # the guard words beyond the count - and beyond the capacity - are intact
        m_ = min(n[c], cap[c])
        assert np.all(o[k][w * m_:] == (99 if dt == np.uint8 else dt(ec.POISON))), k
        o[k] = o[k][:w * m_].reshape((-1, 7) if w == 7 else (-1,))
    return o


def _same_asm(got, exp, what):
    for k in ASM_INT:
        assert np.asarray(got[k]).tolist() == np.asarray(exp[k]).tolist(), (what, k)
    for k in ASM_FLT:
        g, e = np.asarray(got[k], np.float64).reshape(-1, 7), np.asarray(exp[k], np.float64).reshape(-1, 7)
        assert g.shape == e.shape, (what, k)
        assert g.size == 0 or _close(g, e, 1e-12), (what, k, np.abs(g - e).max())


def _same_bytes(a, b, keys, what):
    for k in keys:
        if a.get(k) is None or b.get(k) is None:
            assert a.get(k) is None and b.get(k) is None, (what, k)
            continue
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _asm_both(m, what, exp=None):
    exp = npe.assemble(m) if exp is None else exp
    h = _asm_host(m)
    _same_asm(h, exp, what + " host")
    d = _asm_device(m)
    _same_asm(d, exp, what + " device")
    assert d["status"] == 0, what
    _same_bytes(h, d, ASM_KEYS, what + " host / device")
    return exp, h, d


def _poison_nd(m):
    n = m["npts"]
    return dict(normal=np.full((n, 3), ec.POISON), min_max=np.full((n, 2), ec.POISON, np.float32), nd_written=np.full(n, 77, np.uint8))


def _ap_host(m, vtx_kf, lie, opt, normals=True):
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    r = lc.essential_graph_apply(vtx_kf, lie, opt, _tab(m), normals=normals, out=_poison_nd(m) if normals else None)
    for k, s in (("kf_Tcw", (-1, 12)), ("kf_center", (-1, 3)), ("X", (-1, 3))):
        r[k] = None if r[k] is None else r[k].reshape(s)
    return r


def _ap_device(m, vtx_kf, lie, opt, normals=True, tab=None):
    import torch
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    out = {k: _t(v) for k, v in _poison_nd(m).items()} if normals else None
    r = lc.essential_graph_apply(_t(vtx_kf), _t(lie), _t(opt), _tab(m, _t) if tab is None else tab, normals=normals, out=out, device=True)
    torch.cuda.synchronize()
    o = {k: (None if r.get(k) is None else r[k].cpu().numpy()) for k in AP_KEYS}
    o["status"] = int(r["status"].item()) & 0xFFFFFFFF
    for k, s in (("kf_Tcw", (-1, 12)), ("kf_center", (-1, 3)), ("X", (-1, 3)), ("normal", (-1, 3)), ("min_max", (-1, 2))):
        o[k] = None if o[k] is None else o[k].reshape(s)
    return o


def _check_apply(m, got, exp, what, normals=True):
    from ceres_mono_orb_slam2_amd import localmapping as lm
    for k in AP_INT:
        if exp[k] is None:
            assert got.get(k) is None, (what, k)
        else:
            assert np.asarray(got[k]).tolist() == np.asarray(exp[k]).tolist(), (what, k)
    for k in AP_FLT:
        assert _close(got[k], exp[k], 1e-12), (what, k, np.abs(np.asarray(got[k]) - exp[k]).max())
    moved = np.asarray(got["pt_moved"]) != 0
    stay = ~moved
    assert np.array_equal(_bits(got["X"][stay]), _bits(np.asarray(m["X"])[stay])), what       # a point that stays keeps its bits
    if not normals or m["npts"] == 0:
        return
    # normals and depth ranges: the parent commit's orbl_update_map_points on the apply's own X and centres, bit for bit
    good = (moved & (np.asarray(m["pt_ref_kf"]) >= 0)).astype(np.uint8)
    ref = lm.update_map_points(m["obs_off"], X=got["X"], ref_kf=m["pt_ref_kf"], ref_level=m["ref_level"], obs_kf=m["obs_kf"], kf_center=got["kf_center"],
                               scale_factors=m["scale_factors"], pt_good=good, what=lm.MP_NORMAL_DEPTH, out=_poison_nd(m))
    w = np.asarray(got["nd_written"]) != 0
    assert np.array_equal(w, (ref["nd_written"] == 1) & moved), what
    assert np.array_equal(_bits(got["normal"][w]), _bits(ref["normal"][w])) and np.array_equal(_bits(got["min_max"][w]), _bits(ref["min_max"][w])), what
    assert np.all(got["normal"][~w] == ec.POISON) and np.all(got["min_max"][~w] == np.float32(ec.POISON)), what      # rows of other points are untouched


def _ap_both(m, asm, opt, what, exp=None, normals=True):
    exp = npe.apply(m, asm["vtx_kf"], asm["lie7"], opt, normals=normals) if exp is None else exp
    h = _ap_host(m, asm["vtx_kf"], asm["lie7"], opt, normals)
    _check_apply(m, h, exp, what + " host", normals)
    d = _ap_device(m, asm["vtx_kf"], asm["lie7"], opt, normals)
    _check_apply(m, d, exp, what + " device", normals)
    assert d["status"] == 0, what
    _same_bytes(h, d, AP_KEYS, what + " host / device")
    return h, d


def test_hand_worked_map():
    exp, h, d = _asm_both(HAND_MAP, "hand")
    for k in ("vtx_kf", "kf_vtx", "vtx_fixed", "counts"):
        assert h[k].tolist() == HAND[k], k
    assert [(int(h["vtx_kf"][j]), int(h["vtx_kf"][i]), int(k)) for j, i, k in zip(h["edge_j"], h["edge_i"], h["edge_kind"])] == HAND["edges"]
    # the restated problem (host arithmetic) as the apply's input: both forms read the same bytes
    opt = ec.solver_result(5, exp["lie7"])
    ha, _ = _ap_both(HAND_MAP, exp, opt, "hand")
    assert ha["pt_moved"].tolist() == HAND["pt_moved"] and ha["nd_written"].tolist() == HAND["nd_written"] and ha["counts"].tolist() == HAND["apply_counts"]
    assert np.array_equal(_bits(ha["kf_Tcw"][3]), _bits(HAND_MAP["kf_Tcw"][3]))                 # the bad keyframe keeps its pose
    _ap_both(HAND_MAP, exp, opt, "hand without normals", normals=False)
    plain = ec.without(HAND_MAP, pt_done=None, pt_corr_ref=None)      # no loop-closing stamps: every point goes through its reference keyframe
    hp, _ = _ap_both(plain, exp, opt, "hand without pt_done")
    assert hp["pt_moved"].tolist() == [1, 0, 0, 0, 0, 1]


@pytest.mark.parametrize("name", sorted(SMALL))
def test_empty_and_one_vertex_cases(name):
    m = SMALL[name]
    exp, h, _ = _asm_both(m, name)
    assert exp["counts"][1] == 0                                    # no edges at all
    assert exp["counts"][0] == (0 if name == "one bad keyframe" else m["nkf"])
    opt = ec.solver_result(6, exp["lie7"])
    _ap_both(m, exp, opt, name)


@pytest.mark.parametrize("which", [0, 1])
def test_seeded_maps(which):
    name, m, exp, opt, exp_ap = seeded()[which]
    _, h, d = _asm_both(m, name, exp)
    d2 = _asm_device(m)                                             # determinism: the same bytes again
    _same_bytes(d, d2, ASM_KEYS, name + " second run")
    ha, da = _ap_both(m, exp, opt, name, exp_ap)
    da2 = _ap_device(m, exp["vtx_kf"], exp["lie7"], opt)
    _same_bytes(da, da2, AP_KEYS, name + " second apply")
    # index order instead of kf_rank names other vertices: the rank is read
    blind = npe.assemble(ec.without(m, kf_rank=None))
    assert blind["vtx_kf"].tolist() != exp["vtx_kf"].tolist()


def test_capacities():
    name, m, exp, _, _ = seeded()[0]
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    nv, ne = int(exp["counts"][0]), int(exp["counts"][1])
    for cap, bit in (((nv, ne - 1), lc.EG_CAP_EDGES), ((nv - 1, ne), lc.EG_CAP_VTX), ((nv - 1, ne - 1), lc.EG_CAP_VTX | lc.EG_CAP_EDGES)):
        r = _asm_host(m, caps=cap, check=False)
        assert r["rc"] == lc.ECAP and r["counts"].tolist() == exp["counts"].tolist(), cap
        with pytest.raises(Exception, match="wanted %d vertices, %d edges" % (nv, ne)):
            _asm_host(m, caps=cap)
        d = _asm_device(m, caps=cap)                                # (checks the guard words beyond the capacity)
        assert d["status"] == bit and d["counts"].tolist() == exp["counts"].tolist(), cap
        assert d["edge_j"].tolist() == exp["edge_j"][:cap[1]].tolist() and d["vtx_kf"].tolist() == exp["vtx_kf"][:cap[0]].tolist(), cap
        assert d["kf_vtx"].tolist() == exp["kf_vtx"].tolist(), cap
    r = _asm_host(m, caps=(nv, ne))                                 # an exact fit
    _same_asm(r, exp, "exact fit")


def _without_entries(m, off, arrs, positions):
    """the map with some entries of a CSR table taken out"""
    keep = np.ones(len(m[arrs[0]]), bool); keep[list(positions)] = False
    row = np.searchsorted(m[off], np.arange(len(keep)), side="right") - 1
    new_off = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=len(m[off]) - 1))]).astype(np.int32)
    ch = {off: new_off}
    ch.update({a: np.array(m[a])[keep] for a in arrs})
    return ch


def test_out_of_range_entries_in_the_device_form_are_absent():
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    name, m, _, _, _ = seeded()[0]
    nkf = m["nkf"]
    rng = np.random.default_rng(77)
    bad, ref = {}, {}
    for off, arrs in (("child_off", ("child_kf",)), ("loop_off", ("loop_kf",)), ("conn_off", ("conn_kf", "conn_w")), ("link_off", ("link_kf",))):
        pos = rng.choice(len(m[arrs[0]]), 4, replace=False)
        a = np.array(m[arrs[0]]); a[pos] = [nkf, -1, nkf + 5, -7]
        bad[arrs[0]] = a
        ref.update(_without_entries(m, off, arrs, pos))
    # an ordered list: an entry of the prefix of a list that straddles min_weight (taking it out leaves the prefix rule as it was)
    lens = np.diff(m["ord_off"])
    k = next(k for k in range(nkf) if lens[k] >= 3 and m["ord_w"][m["ord_off"][k] + 1] >= 100 > m["ord_w"][m["ord_off"][k + 1] - 1] and not m["kf_bad"][k])
    a = np.array(m["ord_kf"]); a[m["ord_off"][k]] = nkf
    bad["ord_kf"] = a
    ref.update(_without_entries(m, "ord_off", ("ord_kf", "ord_w"), [m["ord_off"][k]]))
    par = np.array(m["kf_parent"]); kids = np.nonzero(par >= 0)[0][:2]; par[kids] = [nkf, -2]
    bad["kf_parent"] = par
    rp = np.array(m["kf_parent"]); rp[kids] = -1
    ref["kf_parent"] = rp
    # a target and a group member that are not there: their rows go with them
    tg = np.array(m["tgt_kf"]); tg[1] = nkf
    bad["tgt_kf"] = tg
    rows = [ref["link_kf"][ref["link_off"][c]:ref["link_off"][c + 1]].tolist() for c in range(len(tg))]
    del rows[1]
    ref["tgt_kf"] = np.delete(m["tgt_kf"], 1)
    ref["link_off"], ref["link_kf"] = ec.csr(rows)
    gk = np.array(m["conn_group_kf"]); gk[0] = -3
    bad["conn_group_kf"] = gk
    ref.update(conn_group_kf=m["conn_group_kf"][1:], corrected=m["corrected"][1:], non_corrected=m["non_corrected"][1:])
    mb, mr = ec.without(m, **bad), ec.without(m, **ref)
    exp = npe.assemble(mr)
    d = _asm_device(mb, caps=_caps(m))
    assert d["status"] == lc.EG_KF
    _same_asm(d, exp, "out of range")
    # a Sim3 of the group that is not finite: its keyframe counts as outside the group
    cor = np.array(m["corrected"]); cor[2, 5] = np.nan
    d = _asm_device(ec.without(m, corrected=cor))
    sel = np.arange(len(m["conn_group_kf"])) != 2
    exp = npe.assemble(ec.without(m, conn_group_kf=m["conn_group_kf"][sel], corrected=m["corrected"][sel], non_corrected=m["non_corrected"][sel]))
    assert d["status"] == lc.EG_SIM3
    _same_asm(d, exp, "NaN Sim3")
    # a rank that is no permutation is flagged, and nothing is written out of bounds (the guards are checked)
    rk = np.array(m["kf_rank"]); rk[5] = rk[6]
    d = _asm_device(ec.without(m, kf_rank=rk))
    assert d["status"] & lc.EG_RANK
    off = np.array(m["ord_off"]); off[3] = off[-1] + 9
    d = _asm_device(ec.without(m, ord_off=off))
    assert d["status"] & lc.EG_OFFSETS
    # apply: a vertex whose keyframe is out of range writes no pose, a point whose reference keyframe is out of range stays
    asm = npe.assemble(m)
    opt = ec.solver_result(3, asm["lie7"])
    vk = np.array(asm["vtx_kf"]); vk[4] = nkf
    prf = np.array(m["pt_ref_kf"])
    p = next(i for i in range(m["npts"]) if not m["pt_bad"][i] and not m["pt_done"][i] and prf[i] >= 0 and asm["kf_vtx"][prf[i]] >= 0 and asm["kf_vtx"][prf[i]] != 4)
    prf[p] = nkf + 1
    got = _ap_device(ec.without(m, pt_ref_kf=prf), vk, asm["lie7"], opt)
    sel = np.arange(len(vk)) != 4
    rprf = np.array(m["pt_ref_kf"]); rprf[p] = -1
    mr = ec.without(m, pt_ref_kf=rprf)
    exp = npe.apply(mr, asm["vtx_kf"][sel], asm["lie7"][sel], opt[sel])
    assert got["status"] == lc.EG_KF
    _check_apply(mr, got, exp, "apply out of range")


@pytest.mark.parametrize("device", [False, True])
def test_end_to_end_against_the_oracle(oracle, device):
    """optimize_essential_graph_on_tables against restatement-assemble, oracle.optimize_essential_graph, restatement-apply: the same iteration
    count and termination; poses and points within the tolerance of tests/test_gpu_essential_graph.py for the solve (tangents to 1e-7)."""
    import torch
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    m = ec.loop_map(11)
    asm = npe.assemble(m)
    assert asm["counts"][2] == 1 and asm["counts"][1] > m["nkf"]
    ox, os_ = oracle.optimize_essential_graph(asm["lie7"], asm["vtx_fixed"], asm["edge_j"], asm["edge_i"], asm["edge_Sji"])
    exp = npe.apply(m, asm["vtx_kf"], asm["lie7"], ox)
    assert os_["final_cost"] < 0.2 * os_["initial_cost"] and np.abs(exp["kf_Tcw"] - m["kf_Tcw"]).max() > 0.05      # the loop closes: the map moves
    r = lc.optimize_essential_graph_on_tables(m["loop"], m["cur"], _tab(m, _t) if device else _tab(m), device=device)
    s = r["summary"]
    assert (s["iterations"], s["successful_steps"], s["termination"]) == (os_["iterations"], os_["successful_steps"], os_["termination"])
    assert _close(r["lie_opt"], ox, 1e-7)
    a = r["applied"]
    if device:
        torch.cuda.synchronize()
        assert int(a["status"].item()) == 0
        a = {k: a[k].cpu().numpy() for k in ("kf_Tcw", "kf_center", "X", "pt_moved", "nd_written", "counts")}
    assert np.asarray(a["pt_moved"]).tolist() == exp["pt_moved"].tolist() and np.asarray(a["nd_written"]).tolist() == exp["nd_written"].tolist()
    assert np.asarray(a["counts"]).tolist() == exp["counts"].tolist()
    for k, s in (("kf_Tcw", (-1, 12)), ("kf_center", (-1, 3)), ("X", (-1, 3))):
        assert _close(np.asarray(a[k]).reshape(s), exp[k], 1e-7), k
