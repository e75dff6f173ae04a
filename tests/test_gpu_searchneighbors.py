"""orbl_fuse_targets, orbl_fuse_rows, orbl_fuse_candidates, orbl_update_map_points_on_tables (host and device forms) and
localmapping.search_in_neighbors_on_tables on the MI355X against the restatement tests/npsearchneighbors.py, the literal sequential
LocalMapping::SearchInNeighbors.  EVERYTHING here is compared byte for byte - normals and depth ranges included: their summation order is
fixed by csrc/orb_maptable.h - so there is no tolerance anywhere in this file.  tests/test_searchneighbors_restatement.py shows that the
cases and the seeded maps take the paths these comparisons rely on."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import npmappoint  # noqa: E402
from tests import npsearchneighbors as ns  # noqa: E402
from tests import searchneighborscases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = ("op_kind", "op_pt", "op_arg", "op_kf", "op_slot", "best_idx", "best_dist", "q_uv", "q_level")
CHAIN_TABLES = ("kf_slot_pt", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced", "obs_off", "obs_kf", "obs_slot", "pt_desc", "pt_normal", "pt_min_dist",
                "pt_max_dist", "kf_fuse_target", "pt_fuse_cand")
UPDATED = ("pt_desc", "pt_normal", "pt_min_dist", "pt_max_dist")
_MAPS = {}


def _map(seed):
    """a seeded map, its literal replay and the state after the first loop's targets, computed once, shared and read-only"""
    if seed not in _MAPS:
        m = sc.make(seed)
        for v in m["tab"].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _MAPS[seed] = (m, ns.search_in_neighbors(m["tab"], m["cur_kf"], m["cur_id"]))
    return _MAPS[seed]


def _lm():
    from ceres_mono_orb_slam2_amd import localmapping
    return localmapping


def _dev(tab):
    import torch
    dt = dict(_lm()._SN_TAB)
    return {k: (None if v is None else torch.as_tensor(np.array(v, dt[k])).cuda()) for k, v in tab.items()}


def _np(t):
    return None if t is None else t.cpu().numpy()


def _status(t):
    return int(t.cpu()[0]) & 0xFFFFFFFF


def _same(got, exp, what):
    g, e = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert g.dtype == e.dtype and g.shape == e.shape and g.tobytes() == e.tobytes(), (what, got, exp)


def _same_rows(got, exp, what):
    for k in ROWS:
        _same(np.asarray(got[k]).reshape(np.asarray(exp[k]).shape), exp[k], (what, k))


def _word(k):
    import torch
    return torch.tensor([k], dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------------------ targets
def _targets_both(tab, cur_kf, cur_id, nn=20, nn2=5):
    import torch
    lm = _lm()
    h = lm.fuse_targets(cur_kf, cur_id, tab, nn, nn2)
    d_tab = _dev({k: tab.get(k) for k in ("kf_bad", "ord_off", "ord_kf", "kf_fuse_target")})
    d = lm.fuse_targets(cur_kf, cur_id, d_tab, nn, nn2, device=True)
    torch.cuda.synchronize()
    n = int(_np(d["counts"])[0])
    dd = dict(tgt_kf=_np(d["tgt_kf"])[:n], counts=_np(d["counts"]), kf_fuse_target=_np(d_tab["kf_fuse_target"]))
    assert _status(d["status"]) == 0
    return h, dd


@pytest.mark.parametrize("name", sorted(sc.target_cases()))
def test_target_cases_host_and_device(name):
    c = sc.target_cases()[name]
    for r, form in zip(_targets_both(c["tab"], c["cur_kf"], c["cur_id"], c["nn"], c["nn2"]), ("host", "device")):
        _same(r["tgt_kf"], np.array(c["tgt_kf"], np.int32), (name, form))
        _same(r["counts"], np.array(c["counts"], np.int32), (name, form))
        _same(r["kf_fuse_target"], np.array(c["kf_fuse_target"], np.int32), (name, form))


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_targets_of_the_seeded_maps(seed):
    m, _ = _map(seed)
    exp = ns.fuse_targets(m["tab"], m["cur_kf"], m["cur_id"])
    for r, form in zip(_targets_both(m["tab"], m["cur_kf"], m["cur_id"]), ("host", "device")):
        for k in ("tgt_kf", "counts", "kf_fuse_target"):
            _same(r[k], exp[k], (seed, form, k))


def test_targets_capacity_and_bounds_on_the_device():
    import torch
    lm = _lm()
    c = sc.target_cases()["mixed"]
    d_tab = _dev(c["tab"])
    out = dict(tgt_kf=torch.full((4,), -7, dtype=torch.int32, device="cuda")[:3])
    guard = out["tgt_kf"]._base if out["tgt_kf"]._base is not None else None
    d = lm.fuse_targets(0, 7, d_tab, cap_tgt=3, device=True, out=out)
    torch.cuda.synchronize()
    assert _status(d["status"]) == lm.SN_CAP and _np(d["counts"]).tolist() == [6, 2] and _np(d["tgt_kf"]).tolist() == [1, 4, 5]
    assert guard is None or int(guard[3]) == -7                              # nothing beyond the capacity
    bad = dict(c["tab"], ord_kf=np.where(np.arange(len(c["tab"]["ord_kf"])) == 1, 99, c["tab"]["ord_kf"]).astype(np.int32))          # the bad neighbour 2 -> no keyframe
    d = lm.fuse_targets(0, 7, _dev(bad), device=True)
    torch.cuda.synchronize()
    assert _status(d["status"]) == lm.SN_KF and _np(d["tgt_kf"])[:6].tolist() == c["tgt_kf"]


# ------------------------------------------------------------------------------------------------------------------ rows
def _rows_both(tab, K, pts):
    import torch
    lm = _lm()
    h = lm.fuse_rows(K, pts, tab)
    d_tab = _dev({k: tab[k] for k in lm._SN_ROW_KF + lm._SN_ROW_SLOT + lm._SN_ROW_PT})
    d = lm.fuse_rows(_word(K), torch.as_tensor(np.array(pts, np.int32)).cuda(), d_tab, device=True)
    torch.cuda.synchronize()
    assert _status(d["status"]) == 0
    return h, {k: _np(d[k]) for k in ROWS}


def _fuse_batch_of(tab, K, exp):
    """orbl_fuse_batch fed with the restatement's projection of the same points into the same keyframe"""
    lm = _lm()
    lo, hi = int(tab["kf_slot_off"][K]), int(tab["kf_slot_off"][K + 1])
    kps = np.zeros((hi - lo, 4), np.float32)
    kps[:, :2] = np.asarray(tab["kf_slot_uv"], np.float32).reshape(-1, 2)[lo:hi]; kps[:, 2] = tab["kf_slot_level"][lo:hi]
    kf = dict(kps=kps, desc=np.asarray(tab["kf_slot_desc"]).reshape(-1, 32)[lo:hi], bounds=np.asarray(tab["kf_bounds"]).reshape(-1, 4)[K])
    lvl = exp["q_level"]
    radius = (np.float32(3.0) * np.asarray(tab["scale_factors"], np.float32)[np.maximum(lvl, 0)]).astype(np.float32)
    desc = np.asarray(tab["pt_desc"]).reshape(-1, 32)[np.maximum(exp["op_pt"], 0)]
    return lm.fuse_batch([kf], exp["q_uv"][None], radius[None], lvl[None], desc, tab["inv_level_sigma2"])


def test_row_case_host_and_device():
    c = sc.row_case()
    for K, want in c["expect"].items():
        exp = ns.fuse_rows(c["tab"], K, c["pts"])
        for r, form in zip(_rows_both(c["tab"], K, c["pts"]), ("host", "device")):
            for k, w in want.items():                                        # the expectations worked by hand
                assert np.asarray(r[k]).tolist() == w, (K, form, k)
            _same_rows(r, exp, (K, form))
    bi, bd = _fuse_batch_of(c["tab"], 0, ns.fuse_rows(c["tab"], 0, c["pts"]))
    assert bi[0].tolist() == c["expect"][0]["best_idx"] and bd[0].tolist() == c["expect"][0]["best_dist"]


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_rows_of_the_seeded_maps(seed):
    m, rep = _map(seed)
    tab, cur = m["tab"], m["cur_kf"]
    lo, hi = tab["kf_slot_off"][cur], tab["kf_slot_off"][cur + 1]
    snapshot = tab["kf_slot_pt"][lo:hi]
    cases = [(k, snapshot) for k in sorted(set(rep["tgt_kf"]))[:4]] + [(cur, rep["cand_pt"])]
    n_fuse = 0
    for K, pts in cases:
        exp = ns.fuse_rows(tab, K, pts)
        h, d = _rows_both(tab, K, pts)
        _same_rows(h, exp, (seed, K, "host"))
        _same_rows(d, exp, (seed, K, "device"))
        bi, bd = _fuse_batch_of(tab, K, exp)
        _same(bi[0], exp["best_idx"], (seed, K, "orbl_fuse_batch best_idx")); _same(bd[0], exp["best_dist"], (seed, K, "orbl_fuse_batch best_dist"))
        n_fuse += int((exp["op_kind"] == ns.FUSE).sum())
    assert n_fuse > 20


def test_rows_bounds_on_the_device():
    import torch
    lm = _lm()
    c = sc.row_case()
    d_tab = _dev({k: c["tab"][k] for k in lm._SN_ROW_KF + lm._SN_ROW_SLOT + lm._SN_ROW_PT})
    npts = len(c["tab"]["pt_bad"])
    pts = torch.as_tensor(np.array([5, npts, -2, 5], np.int32)).cuda()
    d = lm.fuse_rows(_word(0), pts, d_tab, device=True)
    torch.cuda.synchronize()
    assert _status(d["status"]) == lm.SN_PT and _np(d["op_kind"]).tolist() == [4, 0, 0, 4] and _np(d["op_pt"]).tolist() == [5, -1, -1, 5]
    d = lm.fuse_rows(_word(2), pts[:1], d_tab, device=True)                  # no such keyframe: every row a NOP
    torch.cuda.synchronize()
    assert _status(d["status"]) == lm.SN_KF and _np(d["op_kind"]).tolist() == [0] and _np(d["best_idx"]).tolist() == [-1]


# ------------------------------------------------------------------------------------------------------------------ candidates
def _cands_both(tab, tgt, cur_id, **kw):
    import torch
    lm = _lm()
    h = lm.fuse_candidates(tgt, cur_id, tab)
    d_tab = _dev({k: tab[k] for k in ("kf_slot_off", "kf_slot_pt", "pt_bad", "pt_fuse_cand")})
    d = lm.fuse_candidates(torch.as_tensor(np.array(tgt, np.int32)).cuda(), cur_id, d_tab, device=True, **kw)
    torch.cuda.synchronize()
    n = int(_np(d["counts"])[0])
    return h, dict(cand_pt=_np(d["cand_pt"])[:n], counts=_np(d["counts"]), pt_fuse_cand=_np(d_tab["pt_fuse_cand"]), status=_status(d["status"]))


def test_candidate_case_host_and_device():
    c = sc.candidate_case()
    for r, form in zip(_cands_both(c["tab"], c["tgt_kf"], c["cur_id"]), ("host", "device")):
        _same(r["cand_pt"], np.array(c["cand_pt"], np.int32), form); _same(r["counts"], np.array(c["counts"], np.int32), form)
        _same(r["pt_fuse_cand"], np.array(c["pt_fuse_cand"], np.int32), form)
    exp = ns.fuse_candidates(c["tab"], c["tgt_kf"], c["cur_id"], cap=2)       # the capacity: the wanted count, nothing beyond, those points unstamped
    _, d = _cands_both(c["tab"], c["tgt_kf"], c["cur_id"], cap_cand=2)
    assert d["status"] == _lm().SN_CAP and d["counts"].tolist() == c["counts"] and d["cand_pt"][:2].tolist() == c["cand_pt"][:2]
    _same(d["pt_fuse_cand"], exp["pt_fuse_cand"], "capacity")


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_candidates_of_the_seeded_maps(seed):
    m, rep = _map(seed)
    exp = ns.fuse_candidates(m["tab"], rep["tgt_kf"], m["cur_id"])
    assert len(exp["cand_pt"]) > 100 and len(set(rep["tgt_kf"])) < len(rep["tgt_kf"])
    for r, form in zip(_cands_both(m["tab"], rep["tgt_kf"], m["cur_id"]), ("host", "device")):
        for k in ("cand_pt", "counts", "pt_fuse_cand"):
            _same(r[k], exp[k], (seed, form, k))
    assert _cands_both(m["tab"], rep["tgt_kf"], m["cur_id"])[1]["status"] == 0


def test_candidates_bounds_on_the_device():
    c = sc.candidate_case()
    _, d = _cands_both(c["tab"], c["tgt_kf"], c["cur_id"])
    import torch
    lm = _lm()
    d_tab = _dev(c["tab"])
    r = lm.fuse_candidates(torch.as_tensor(np.array([1, 7, 2, 1], np.int32)).cuda(), c["cur_id"], d_tab, device=True)          # 7: no keyframe, skipped
    torch.cuda.synchronize()
    assert _status(r["status"]) == lm.SN_KF and _np(r["cand_pt"])[:4].tolist() == c["cand_pt"] and _np(r["counts"]).tolist() == [4, 4]


# ------------------------------------------------------------------------------------------------------------------ the point update
def _gathered(tab, pt_good):
    """the lists of orbl_update_map_points, gathered from the tables on the host"""
    off = np.asarray(tab["obs_off"])
    so, sd, sl = np.asarray(tab["kf_slot_off"]), np.asarray(tab["kf_slot_desc"]).reshape(-1, 32), np.asarray(tab["kf_slot_level"])
    at = so[tab["obs_kf"]] + tab["obs_slot"]
    ref = np.asarray(tab["pt_ref_kf"])
    lvl = np.zeros(len(ref), np.int32)
    for p in range(len(ref)):
        e = [e for e in range(off[p], off[p + 1]) if tab["obs_kf"][e] == ref[p]]
        lvl[p] = sl[at[e[0]]] if e else sl[so[ref[p]]]
    return dict(obs_off=off, obs_desc=sd[at], obs_kf_good=(1 - np.asarray(tab["kf_bad"])[tab["obs_kf"]]).astype(np.uint8), X=tab["X"], ref_kf=ref, ref_level=lvl,
                obs_kf=tab["obs_kf"], kf_center=tab["kf_center"], scale_factors=tab["scale_factors"], pt_good=pt_good.astype(np.uint8))


@pytest.mark.parametrize("what", (1, 2, 3))
@pytest.mark.parametrize("form", ("mask", "keyframe", "both"))
def test_update_on_tables_equals_the_restatement_and_the_list_entry(what, form):
    import torch
    lm = _lm()
    m, _ = _map(sc.SEEDS[0])
    tab, cur = m["tab"], m["cur_kf"]
    npts = len(tab["pt_bad"])
    rng = np.random.default_rng(what)
    mask = (rng.random(npts) < 0.4).astype(np.uint8) if form != "keyframe" else None
    mask_kf = cur if form != "mask" else -1
    exp = ns.update_map_points_on_tables(tab, what, mask, mask_kf)
    h = lm.update_map_points_on_tables(what, tab, pt_mask=mask, mask_kf=mask_kf)
    d_tab = _dev({k: tab[k] for k in lm._SN_UPD_IN + lm._SN_UPD_INOUT})
    d = lm.update_map_points_on_tables(what, d_tab, pt_mask=None if mask is None else torch.as_tensor(mask).cuda(), mask_kf=mask_kf, device=True)
    torch.cuda.synchronize()
    assert _status(d["status"]) == 0
    # the same points through orbl_update_map_points on gathered lists
    sel = np.zeros(npts, bool) if mask is None else mask.astype(bool)
    if mask_kf >= 0:
        row = tab["kf_slot_pt"][tab["kf_slot_off"][cur]:tab["kf_slot_off"][cur + 1]]
        sel[row[row >= 0]] = True
    good = sel & ~np.asarray(tab["pt_bad"]).astype(bool)
    out = dict(best_obs=np.full(npts, -1, np.int32), desc=np.array(tab["pt_desc"]).reshape(-1, 32), normal=np.array(tab["pt_normal"]).reshape(-1, 3),
               min_max=np.stack([tab["pt_min_dist"], tab["pt_max_dist"]], 1).astype(np.float32), nd_written=np.zeros(npts, np.uint8))
    lst = lm.update_map_points(what=what, out=out, **_gathered(tab, good))
    changed = 0
    for k in UPDATED:
        want = exp[k].reshape(np.asarray(tab[k]).shape)
        _same(np.asarray(h[k]).reshape(want.shape), want, (what, form, "host", k))
        _same(_np(d_tab[k]).reshape(want.shape), want, (what, form, "device", k))
        changed += int((want != np.asarray(tab[k])).sum())
    _same(lst["desc"], exp["pt_desc"].reshape(-1, 32), "orbl_update_map_points desc"); _same(lst["normal"], exp["pt_normal"].reshape(-1, 3), "orbl_update_map_points normal")
    _same(lst["min_max"][:, 0], exp["pt_min_dist"], "orbl_update_map_points min"); _same(lst["min_max"][:, 1], exp["pt_max_dist"], "orbl_update_map_points max")
    if what & 1:
        _same(h["best_obs"], lst["best_obs"], "best_obs host"); _same(_np(d["best_obs"]), lst["best_obs"], "best_obs device")
    if what & 2:
        _same(h["nd_written"], lst["nd_written"], "nd_written host"); _same(_np(d["nd_written"]), lst["nd_written"], "nd_written device")
        assert lst["nd_written"].sum() == good.sum() - sum(1 for p in np.nonzero(good)[0] if tab["obs_off"][p] == tab["obs_off"][p + 1])
    assert changed > 0


def test_reference_keyframe_not_in_the_list_reads_keypoint_0():
    lm = _lm()
    m, _ = _map(sc.SEEDS[0])
    tab = dict(m["tab"])
    p = next(p for p in range(len(tab["pt_bad"])) if not tab["pt_bad"][p] and tab["obs_off"][p + 1] - tab["obs_off"][p] == 1)
    seen = int(tab["obs_kf"][tab["obs_off"][p]])
    ref = next(k for k in range(len(tab["kf_bad"])) if k != seen and tab["kf_slot_level"][tab["kf_slot_off"][k]] != tab["kf_slot_level"][tab["kf_slot_off"][seen] + tab["obs_slot"][tab["obs_off"][p]]])
    tab["pt_ref_kf"] = np.array(tab["pt_ref_kf"]); tab["pt_ref_kf"][p] = ref
    mask = np.zeros(len(tab["pt_bad"]), np.uint8); mask[p] = 1
    exp = ns.update_map_points_on_tables(tab, 2, mask)
    h = lm.update_map_points_on_tables(2, tab, pt_mask=mask)
    for k in UPDATED[1:]:
        _same(np.asarray(h[k]).reshape(exp[k].shape), exp[k], k)
    lvl = int(tab["kf_slot_level"][tab["kf_slot_off"][ref]])
    n, mn, mx = npmappoint.normal_and_depth(tab["X"][p], tab["kf_center"][[seen]], tab["kf_center"][ref], lvl, tab["scale_factors"])
    assert h["pt_max_dist"][p] == mx and h["pt_min_dist"][p] == mn and h["nd_written"].tolist() == mask.tolist()


# ------------------------------------------------------------------------------------------------------------------ the whole function
def _chain(seed, device):
    import torch
    lm = _lm()
    m, _ = _map(seed)
    tab = _dev(m["tab"]) if device else {k: (None if v is None else np.array(v)) for k, v in m["tab"].items()}
    r = lm.search_in_neighbors_on_tables(m["cur_kf"], m["cur_id"], tab, device=device)
    torch.cuda.synchronize()
    out = {k: (_np(r["tab"][k]) if device else r["tab"][k]) for k in CHAIN_TABLES}
    conn = {k: (_np(v) if device and hasattr(v, "cpu") else v) for k, v in r["connections"].items() if k != "_workspace"}
    return r, out, conn


def _same_chain(r, out, conn, rep, what):
    assert r["status"] == 0 and r["tgt_kf"] == rep["tgt_kf"] and r["n_fused"] == rep["n_fused"], what
    _same(r["cand_pt"], rep["cand_pt"], (what, "cand_pt"))
    for k in CHAIN_TABLES:
        want = rep["tab"][k]
        _same(np.asarray(out[k]).reshape(want.shape), want, (what, k))
    ec = rep["connections"]
    n_aff, n_conn, n_ord, _ = (int(v) for v in ec["counts"])
    _same(conn["counts"], ec["counts"], (what, "connection counts"))
    assert int(np.asarray(conn["status"]).reshape(-1)[0]) == 0
    for k, n in (("tgt_status", 1), ("tgt_parent", 1), ("aff_kf", n_aff), ("conn_off", n_aff + 1), ("conn_kf", n_conn), ("conn_w", n_conn), ("ord_off", n_aff + 1),
                 ("ord_kf", n_ord), ("ord_w", n_ord)):
        _same(np.asarray(conn[k])[:n], np.asarray(ec[k], np.int32)[:n], (what, "connections", k))


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_search_in_neighbors_on_tables_equals_the_literal_replay(seed):
    _, rep = _map(seed)
    assert sum(rep["n_fused"]) > 50 and rep["connections"]["counts"][0] > 0
    r, out, conn = _chain(seed, True)
    _same_chain(r, out, conn, rep, (seed, "resident"))


def test_search_in_neighbors_from_host_tables_and_twice():
    seed = sc.SEEDS[1]
    _, rep = _map(seed)
    r, out, conn = _chain(seed, False)
    _same_chain(r, out, conn, rep, (seed, "host tables"))
    r2, out2, conn2 = _chain(seed, True)                                     # a second run: the same bytes
    for k in CHAIN_TABLES:
        _same(np.asarray(out2[k]).reshape(-1), np.asarray(out[k]).reshape(-1), ("second run", k))
    assert r2["n_fused"] == r["n_fused"] and r2["tgt_kf"] == r["tgt_kf"]


def test_entries_twice_give_identical_bytes():
    m, rep = _map(sc.SEEDS[0])
    tab, cur = m["tab"], m["cur_kf"]
    snapshot = tab["kf_slot_pt"][tab["kf_slot_off"][cur]:tab["kf_slot_off"][cur + 1]]
    a, b = _rows_both(tab, rep["tgt_kf"][0], snapshot)[1], _rows_both(tab, rep["tgt_kf"][0], snapshot)[1]
    _same_rows(a, b, "rows twice")
    a, b = _cands_both(tab, rep["tgt_kf"], m["cur_id"])[1], _cands_both(tab, rep["tgt_kf"], m["cur_id"])[1]
    for k in ("cand_pt", "counts", "pt_fuse_cand"):
        _same(a[k], b[k], ("candidates twice", k))
