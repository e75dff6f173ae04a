"""LoopClosing's two map-moving steps on the GPU (include/orbslam_hip.h: orbl_correct_loop*, orbl_propagate_global_ba*): the pose and
point correction of CorrectLoop (src/LoopClosing.cc:437-523) and the write-back of the global bundle adjustment (:681-739).
There is no CPU fallback: without the library or a GPU the calls raise."""
import numpy as np

from . import _lib
from ._lib import carray as _c, flat as _flat, ptr as _p, ptr_nonempty as _pn

ML_OFFSETS, ML_KF, ML_PT, ML_RANK, ML_LEVEL, ML_SCW = 1, 2, 4, 8, 16, 32        # *d_status bits of orbl_correct_loop_device
GB_KF, GB_CYCLE, GB_STALE = 1, 2, 4                                             # *d_status bits of orbl_propagate_global_ba_device


def _copy(a, dt, shape):
    return np.array(a, dtype=dt, order="C").reshape(shape)          # (always a copy: the in/out tables are returned, the caller's stay)


def correct_loop(kf_Tcw, conn_kf, Scw, slot_off, slot_pt, X, kf_center=None, conn_rank=None, pt_bad=None, pt_done=None, obs_off=None, obs_kf=None,
                 ref_kf=None, ref_level=None, scale_factors=None, normal=None, min_max=None, nd_written=None, device=False, **kw):
    """CorrectLoop's Sim3 maps, point correction, normals and SetPose in one call (orbl_correct_loop; include/orbslam_hip.h states the
    inputs and the semantics).  kf_Tcw [nkf, 12] (or [nkf, 3, 4]), X [npts, 3]; kf_center, conn_rank, pt_bad, pt_done may be None; the
    normals are computed when obs_off, obs_kf, ref_kf, ref_level, scale_factors are all given (then kf_center is needed); normal,
    min_max, nd_written: optional preset arrays, of which only the rows of moved points are rewritten.  Returns a dict: kf_Tcw, kf_center,
    X (new copies), corrected, non_corrected [nconn, 7], pt_owner, counts = {n_moved, n_contested}, and normal / min_max / nd_written.
    device=True: correct_loop_device on torch CUDA tensors, in place."""
    if device:
        return correct_loop_device(kf_Tcw, conn_kf, Scw, slot_off, slot_pt, X, kf_center=kf_center, conn_rank=conn_rank, pt_bad=pt_bad, pt_done=pt_done,
                                   obs_off=obs_off, obs_kf=obs_kf, ref_kf=ref_kf, ref_level=ref_level, scale_factors=scale_factors, normal=normal,
                                   min_max=min_max, nd_written=nd_written, **kw)
    L = _lib.load()
    T = _copy(kf_Tcw, np.float64, (-1, 12)); nkf = len(T)
    Cn = None if kf_center is None else _copy(kf_center, np.float64, (-1, 3))
    ck = _c(conn_kf, np.int32).reshape(-1); nconn = len(ck)
    cr = _flat(conn_rank, np.int32)
    S = _c(Scw, np.float64).reshape(-1)
    so = _c(slot_off, np.int32).reshape(-1); sp = _c(slot_pt, np.int32).reshape(-1)
    Xn = _copy(X, np.float64, (-1, 3)); npts = len(Xn)
    pb = _flat(pt_bad, np.uint8); pd = _flat(pt_done, np.uint8)
    oo = _flat(obs_off, np.int32); ok_ = _flat(obs_kf, np.int32); rk = _flat(ref_kf, np.int32); rl = _flat(ref_level, np.int32); sf = _flat(scale_factors, np.float32)
    nd = all(v is not None for v in (oo, ok_, rk, rl, sf))
    assert nd or all(v is None for v in (oo, ok_, rk, rl, sf)), "the normal / depth inputs are given as a set"
    assert len(S) == 7 and len(so) == nconn + 1 and len(sp) >= so[-1] and (Cn is None or len(Cn) == nkf) and (cr is None or len(cr) == nconn)
    assert (pb is None or len(pb) == npts) and (pd is None or len(pd) == npts)
    if ok_ is not None and ok_.size == 0:
        ok_ = np.zeros(1, np.int32)
    o = dict(corrected=np.zeros((nconn, 7)), non_corrected=np.zeros((nconn, 7)), pt_owner=np.zeros(npts, np.int32), counts=np.zeros(2, np.int32),
             normal=None, min_max=None, nd_written=None)
    if nd:
        assert len(oo) == npts + 1 and len(ok_) >= oo[-1] and len(rk) == npts and len(rl) == npts
        o["normal"] = np.zeros((npts, 3)) if normal is None else normal
        o["min_max"] = np.zeros((npts, 2), np.float32) if min_max is None else min_max
        o["nd_written"] = np.zeros(npts, np.uint8) if nd_written is None else nd_written
        for k, dt, n in (("normal", np.float64, 3 * npts), ("min_max", np.float32, 2 * npts), ("nd_written", np.uint8, npts)):
            assert o[k].dtype == dt and o[k].flags.c_contiguous and o[k].size == n, k
    _lib.check(L.orbl_correct_loop(nkf, _p(T), _p(Cn), nconn, _p(ck), _p(cr), _p(S), _p(so), _p(sp), npts, _p(Xn), _p(pb), _p(pd),
                                   _p(oo), _p(ok_) if nd else None, _p(rk), _p(rl), _p(sf), len(sf) if nd else 0, _p(o["corrected"]),
                                   _p(o["non_corrected"]), _p(o["pt_owner"]), _p(o["normal"]), _p(o["min_max"]), _p(o["nd_written"]),
                                   _p(o["counts"])), "orbl_correct_loop")
    o.update(kf_Tcw=T, kf_center=Cn, X=Xn)
    return o


def correct_loop_device(kf_Tcw, conn_kf, Scw, slot_off, slot_pt, X, kf_center=None, conn_rank=None, pt_bad=None, pt_done=None, obs_off=None, obs_kf=None,
                        ref_kf=None, ref_level=None, scale_factors=None, normal=None, min_max=None, nd_written=None, out=None, workspace=None):
    """orbl_correct_loop_device on torch CUDA tensors (float64 / int32 / uint8 / float32 as in correct_loop; None where a pointer may be
    NULL), enqueued on the current stream, nothing synchronised.  kf_Tcw, kf_center and X change IN PLACE.  out: optional dict of preset
    output tensors; workspace: optional uint8 tensor to reuse.  Returns a dict of device tensors: the three tables, corrected,
    non_corrected, pt_owner, counts[2], status (the ML_* bits), normal / min_max / nd_written, and the workspace under "_workspace"."""
    import torch
    L = _lib.load()
    dev = kf_Tcw.device
    nkf, nconn, nslots, npts = kf_Tcw.numel() // 12, conn_kf.numel(), slot_pt.numel(), X.numel() // 3
    nd = obs_off is not None
    nobs = obs_kf.numel() if obs_kf is not None else 0
    ws = _lib.workspace("orbl_correct_loop_workspace", nkf, nconn, npts, device=dev, min_bytes=16, reuse=workspace)
    o = {} if out is None else dict(out)
    o.update({k: v for k, v in (("normal", normal), ("min_max", min_max), ("nd_written", nd_written)) if v is not None})
    sizes = [("corrected", torch.float64, 7 * nconn), ("non_corrected", torch.float64, 7 * nconn), ("pt_owner", torch.int32, npts), ("counts", torch.int32, 2),
             ("status", torch.int32, 1)]
    if nd:
        sizes += [("normal", torch.float64, 3 * npts), ("min_max", torch.float32, 2 * npts), ("nd_written", torch.uint8, npts)]
    for k, dt, n in sizes:
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 1), dtype=dt, device=dev)[:n]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == n, k
    for t in (kf_Tcw, kf_center, X):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float64)
    _lib.check(L.orbl_correct_loop_device(nkf, _p(kf_Tcw), _p(kf_center), nconn, _p(conn_kf), _p(conn_rank), _p(Scw), nslots, _p(slot_off), _p(slot_pt), npts, _p(X),
                                          _p(pt_bad), _p(pt_done), nobs, _p(obs_off), _p(obs_kf), _p(ref_kf), _p(ref_level), _p(scale_factors),
                                          scale_factors.numel() if scale_factors is not None else 0, _p(o["corrected"]), _p(o["non_corrected"]), _p(o["pt_owner"]),
                                          _p(o.get("normal")), _p(o.get("min_max")), _p(o.get("nd_written")), _p(o["counts"]), _p(o["status"]), _p(ws),
                                          _lib.stream()), "orbl_correct_loop_device")
    r = dict(o)
    for k in ("normal", "min_max", "nd_written"):
        r.setdefault(k, None)
    r.update(kf_Tcw=kf_Tcw, kf_center=kf_center, X=X, _workspace=ws)                 # (the workspace is kept alive until the caller synchronises)
    return r


def propagate_global_ba(kf_Tcw, kf_gba_Tcw, kf_in_gba, kf_parent, origin_kf, X, pt_ref_kf, kf_center=None, pt_bad=None, pt_in_gba=None, pt_gba_X=None,
                        kf_bef_Tcw=None, device=False, **kw):
    """The global-BA write-back in one call (orbl_propagate_global_ba; include/orbslam_hip.h states the inputs and the semantics).
    kf_bef_Tcw: optional preset [nkf, 12] array, of which only the rows of reached keyframes are rewritten.  Returns a dict: kf_Tcw,
    kf_gba_Tcw, kf_in_gba, kf_center, X (new copies), kf_bef_Tcw, kf_reached, pt_moved, counts = {n_reached, n_propagated, n_points_moved,
    n_stale}.  device=True: propagate_global_ba_device on torch CUDA tensors, in place."""
    if device:
        return propagate_global_ba_device(kf_Tcw, kf_gba_Tcw, kf_in_gba, kf_parent, origin_kf, X, pt_ref_kf, kf_center=kf_center, pt_bad=pt_bad,
                                          pt_in_gba=pt_in_gba, pt_gba_X=pt_gba_X, kf_bef_Tcw=kf_bef_Tcw, **kw)
    L = _lib.load()
    T = _copy(kf_Tcw, np.float64, (-1, 12)); nkf = len(T)
    G = _copy(kf_gba_Tcw, np.float64, (-1, 12)); F = _copy(kf_in_gba, np.uint8, (-1,))
    par = _c(kf_parent, np.int32).reshape(-1); org = _c(origin_kf, np.int32).reshape(-1)
    Cn = None if kf_center is None else _copy(kf_center, np.float64, (-1, 3))
    Xn = _copy(X, np.float64, (-1, 3)); npts = len(Xn)
    pb = _flat(pt_bad, np.uint8); pin = _flat(pt_in_gba, np.uint8)
    pgx = None if pt_gba_X is None else _c(pt_gba_X, np.float64).reshape(-1, 3)
    ref = _c(pt_ref_kf, np.int32).reshape(-1)
    assert len(G) == nkf and len(F) == nkf and len(par) == nkf and (Cn is None or len(Cn) == nkf) and len(ref) == npts
    assert (pb is None or len(pb) == npts) and (pin is None or len(pin) == npts) and (pgx is None or len(pgx) == npts)
    bef = np.zeros((nkf, 12)) if kf_bef_Tcw is None else kf_bef_Tcw
    assert bef.dtype == np.float64 and bef.flags.c_contiguous and bef.size == 12 * nkf
    o = dict(kf_bef_Tcw=bef, kf_reached=np.zeros(nkf, np.uint8), pt_moved=np.zeros(npts, np.uint8), counts=np.zeros(4, np.int32))
    _lib.check(L.orbl_propagate_global_ba(nkf, _p(T), _p(G), _p(F), _p(par), len(org), _p(org), _p(Cn), npts, _p(Xn), _p(pb), _p(pin),
                                          _p(pgx), _p(ref), _p(bef), _p(o["kf_reached"]), _p(o["pt_moved"]), _p(o["counts"])),
               "orbl_propagate_global_ba")
    o.update(kf_Tcw=T, kf_gba_Tcw=G, kf_in_gba=F, kf_center=Cn, X=Xn)
    return o


def propagate_global_ba_device(kf_Tcw, kf_gba_Tcw, kf_in_gba, kf_parent, origin_kf, X, pt_ref_kf, kf_center=None, pt_bad=None, pt_in_gba=None, pt_gba_X=None,
                               kf_bef_Tcw=None, out=None, workspace=None):
    """orbl_propagate_global_ba_device on torch CUDA tensors, enqueued on the current stream, nothing synchronised.  kf_Tcw, kf_gba_Tcw,
    kf_in_gba, kf_center and X change IN PLACE.  Returns a dict of device tensors: those five, kf_bef_Tcw, kf_reached, pt_moved,
    counts[4], status (the GB_* bits), and the workspace under "_workspace"."""
    import torch
    L = _lib.load()
    dev = kf_Tcw.device
    nkf, npts, n_origin = kf_Tcw.numel() // 12, X.numel() // 3, origin_kf.numel()
    ws = _lib.workspace("orbl_propagate_global_ba_workspace", nkf, npts, device=dev, reuse=workspace)
    o = {} if out is None else dict(out)
    if kf_bef_Tcw is not None:
        o["kf_bef_Tcw"] = kf_bef_Tcw
    for k, dt, n in (("kf_bef_Tcw", torch.float64, 12 * nkf), ("kf_reached", torch.uint8, nkf), ("pt_moved", torch.uint8, npts), ("counts", torch.int32, 4),
                     ("status", torch.int32, 1)):
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 1), dtype=dt, device=dev)[:n]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == n, k
    for t in (kf_Tcw, kf_gba_Tcw, kf_center, X):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float64)
    _lib.check(L.orbl_propagate_global_ba_device(nkf, _p(kf_Tcw), _p(kf_gba_Tcw), _p(kf_in_gba), _p(kf_parent), n_origin, _p(origin_kf), _p(kf_center), npts, _p(X),
                                                 _p(pt_bad), _p(pt_in_gba), _p(pt_gba_X), _p(pt_ref_kf), _p(o["kf_bef_Tcw"]), _p(o["kf_reached"]), _p(o["pt_moved"]),
                                                 _p(o["counts"]), _p(o["status"]), _p(ws), _lib.stream()),
               "orbl_propagate_global_ba_device")
    r = dict(o)
    r.update(kf_Tcw=kf_Tcw, kf_gba_Tcw=kf_gba_Tcw, kf_in_gba=kf_in_gba, kf_center=kf_center, X=X, _workspace=ws)
    return r


# ---------------------------------------------------------------------------------------------- OptimizeEssentialGraph on the tables
EG_OFFSETS, EG_KF, EG_RANK, EG_LEVEL, EG_CAP_VTX, EG_CAP_EDGES, EG_SIM3 = 1, 2, 8, 16, 32, 64, 512     # *d_status bits of orbl_essential_graph_*_device
ECAP = -4                            # ORBHIP_ECAP
_EG_KF = (("kf_id", np.int32), ("kf_bad", np.uint8), ("kf_rank", np.int32), ("kf_Tcw", np.float64), ("kf_parent", np.int32))
_EG_CSR = (("child_off", "child_kf"), ("loop_off", "loop_kf"), ("conn_off", "conn_kf", "conn_w"), ("ord_off", "ord_kf", "ord_w"))
_EG_OUT = (("vtx_kf", np.int32, 1, 0), ("lie7", np.float64, 7, 0), ("vtx_fixed", np.uint8, 1, 0), ("edge_j", np.int32, 1, 1), ("edge_i", np.int32, 1, 1),
           ("edge_Sji", np.float64, 7, 1), ("edge_kind", np.uint8, 1, 1))                                # (name, dtype, width, which capacity)
_EG_ORDER = ("vtx_kf", "kf_vtx", "lie7", "vtx_fixed", "edge_j", "edge_i", "edge_Sji", "edge_kind")        # (the order of the C arguments)
_EA_ND = ("obs_off", "obs_kf", "ref_level", "scale_factors")


def _eg_caps(t, nkf, caps):
    """(cap_vtx, cap_edges): by default bounds no call exceeds - every keyframe, and every link, parent, loop edge and ordered entry"""
    if caps is not None:
        return tuple(int(c) for c in caps)
    n = lambda k: 0 if t.get(k) is None else (t[k].numel() if hasattr(t[k], "numel") else np.asarray(t[k]).size)
    return nkf, n("link_kf") + nkf + n("loop_kf") + n("ord_kf")


def essential_graph_assemble(loop_kf, cur_kf, tab, min_weight=100, caps=None, out=None, check=True, device=False, **kw):
    """The problem of CeresOptimizer::OptimizeEssentialGraph from the map tables (orbl_essential_graph_assemble; include/orbslam_hip.h
    states the inputs and the semantics).  loop_kf, cur_kf: keyframe indices.  tab: dict of the tables kf_id, kf_bad, kf_rank, kf_Tcw
    [nkf, 12], kf_parent, child_off / child_kf, loop_off / loop_kf, conn_off / conn_kf / conn_w, ord_off / ord_kf / ord_w, the two Sim3 maps
    conn_group_kf, corrected [nconn, 7], non_corrected [nconn, 7], and loop_connections tgt_kf, link_off / link_kf (kf_bad, kf_rank may be
    None or missing; so may the group and the targets, as empty).  caps = (cap_vtx, cap_edges), by default bounds no call exceeds.  out:
    optional dict of preset output arrays of those capacities.  Returns a dict trimmed to the written counts: vtx_kf, kf_vtx [nkf], lie7
    [n_vtx, 7], vtx_fixed, edge_j, edge_i, edge_Sji [n_edges, 7], edge_kind, counts = {n_vtx, n_edges, n_loop_connection_edges, n_dropped}
    and rc; check=False returns rc = ORBHIP_ECAP with only counts filled instead of raising.  device=True: essential_graph_assemble_device
    on torch CUDA tensors."""
    if device:
        return essential_graph_assemble_device(loop_kf, cur_kf, tab, min_weight=min_weight, caps=caps, out=out, **kw)
    L = _lib.load()
    t = {k: _flat(tab.get(k), dt) for k, dt in _EG_KF}
    for row in _EG_CSR + (("link_off", "link_kf"),):
        t.update({k: _flat(tab.get(k), np.int32) for k in row})
    t.update(conn_group_kf=_flat(tab.get("conn_group_kf"), np.int32), tgt_kf=_flat(tab.get("tgt_kf"), np.int32), corrected=_flat(tab.get("corrected"), np.float64),
             non_corrected=_flat(tab.get("non_corrected"), np.float64))
    nkf = len(t["kf_id"])
    nconn = 0 if t["conn_group_kf"] is None else len(t["conn_group_kf"])
    ntgt = 0 if t["tgt_kf"] is None else len(t["tgt_kf"])
    assert len(t["kf_Tcw"]) == 12 * nkf and len(t["kf_parent"]) == nkf and (t["kf_bad"] is None or len(t["kf_bad"]) == nkf) and (t["kf_rank"] is None or len(t["kf_rank"]) == nkf)
    for row in _EG_CSR:
        assert len(t[row[0]]) == nkf + 1 and all(len(t[k]) >= (t[row[0]][-1] if nkf else 0) for k in row[1:]), row     # (the library checks the rest)
    assert nconn == 0 or (len(t["corrected"]) == 7 * nconn and len(t["non_corrected"]) == 7 * nconn)
    assert ntgt == 0 or (len(t["link_off"]) == ntgt + 1 and (t["link_off"][-1] == 0 or len(t["link_kf"]) >= t["link_off"][-1]))
    cap = _eg_caps(t, nkf, caps)
    o = {} if out is None else out
    for k, dt, w, c in _EG_OUT:
        o.setdefault(k, np.zeros(w * cap[c], dt))
        assert o[k].dtype == dt and o[k].flags.c_contiguous and o[k].size == w * cap[c], k
    o.setdefault("kf_vtx", np.zeros(nkf, np.int32)); o.setdefault("counts", np.zeros(4, np.int32))
    rc = L.orbl_essential_graph_assemble(nkf, *[_pn(t[k]) for k, _ in _EG_KF], *[_p(t[k]) if k.endswith("_off") else _pn(t[k]) for row in _EG_CSR for k in row], nconn,
                                         _pn(t["conn_group_kf"]), _pn(t["corrected"]), _pn(t["non_corrected"]), ntgt, _pn(t["tgt_kf"]), _p(t["link_off"]) if ntgt else None,
                                         _pn(t["link_kf"]), int(loop_kf), int(cur_kf), int(min_weight), cap[0], cap[1], _p(o["counts"]), *[_pn(o[k]) for k in _EG_ORDER])
    if rc == ECAP and not check:
        return dict(rc=rc, counts=o["counts"])
    _lib.check(rc, "orbl_essential_graph_assemble")
    n = (int(o["counts"][0]), int(o["counts"][1]))
    r = dict(rc=0, counts=o["counts"], kf_vtx=o["kf_vtx"])
    for k, _, w, c in _EG_OUT:
        r[k] = o[k][:w * n[c]].reshape((-1, 7) if w == 7 else (-1,))
    return r


def essential_graph_assemble_device(loop_kf, cur_kf, tab, min_weight=100, caps=None, out=None, workspace=None):
    """orbl_essential_graph_assemble_device on torch CUDA tensors (dtypes as in essential_graph_assemble; None where a pointer may be NULL),
    enqueued on the current stream, nothing synchronised.  Returns a dict of device tensors of FULL capacity - counts[4] holds the wanted
    sizes, status (uint32 as int32[1]) the EG_* bits - with kf_vtx and the workspace under "_workspace"."""
    import torch
    L = _lib.load()
    g = tab.get
    dev = tab["kf_id"].device
    nkf = tab["kf_id"].numel()
    n = lambda k: 0 if g(k) is None else g(k).numel()
    cap = _eg_caps(tab, nkf, caps)
    ws = _lib.workspace("orbl_essential_graph_assemble_workspace", nkf, device=dev, reuse=workspace)
    o = {} if out is None else dict(out)
    tdt = {np.int32: torch.int32, np.float64: torch.float64, np.uint8: torch.uint8}
    sizes = [(k, tdt[dt], w * cap[c]) for k, dt, w, c in _EG_OUT] + [("kf_vtx", torch.int32, nkf), ("counts", torch.int32, 4), ("status", torch.int32, 1)]
    for k, dt, m in sizes:
        if o.get(k) is None:
            o[k] = torch.empty(max(m, 1), dtype=dt, device=dev)[:m]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == m, k
    csr = []
    for row in _EG_CSR:
        csr += [n(row[1]), _p(tab[row[0]])] + [_pn(g(k)) for k in row[1:]]
    ntgt = n("tgt_kf")
    _lib.check(L.orbl_essential_graph_assemble_device(nkf, *[_pn(g(k)) for k, _ in _EG_KF], *csr, n("conn_group_kf"), _pn(g("conn_group_kf")), _pn(g("corrected")),
                                                      _pn(g("non_corrected")), ntgt, _pn(g("tgt_kf")), n("link_kf"), _p(tab["link_off"]) if ntgt else None, _pn(g("link_kf")), int(loop_kf),
                                                      int(cur_kf), int(min_weight), cap[0], cap[1], _pn(o["counts"]), *[_pn(o[k]) for k in _EG_ORDER], _pn(o["status"]), _pn(ws),
                                                      _lib.stream()), "orbl_essential_graph_assemble_device")
    r = dict(o)
    r["_workspace"] = ws                                         # (kept alive until the caller synchronises)
    return r


def essential_graph_apply(vtx_kf, lie_orig, lie_opt, tab, normals=True, out=None, device=False, **kw):
    """The write-back of CeresOptimizer::OptimizeEssentialGraph on the map tables (orbl_essential_graph_apply; include/orbslam_hip.h states
    the inputs and the semantics).  vtx_kf, lie_orig = lie7 as essential_graph_assemble returned them, lie_opt [n_vtx, 7] from
    optimizer.optimize_essential_graph.  tab: dict of the tables kf_Tcw, kf_center, X, pt_bad, pt_done, pt_corr_ref, pt_ref_kf and, for the
    normals, obs_off, obs_kf, ref_level, scale_factors (pt_bad, pt_done / pt_corr_ref may be None or missing).  normals=False leaves step 3
    out.  out: optional dict of preset normal [npts, 3], min_max [npts, 2], nd_written [npts] arrays, of which only the rows of points with
    a new normal are rewritten (nd_written wholly).  Returns a dict: new copies of kf_Tcw, kf_center, X; pt_moved [npts], normal, min_max,
    nd_written, counts = {n_poses_written, n_points_moved}.  device=True: essential_graph_apply_device on torch CUDA tensors, in place."""
    if device:
        return essential_graph_apply_device(vtx_kf, lie_orig, lie_opt, tab, normals=normals, out=out, **kw)
    L = _lib.load()
    T = _copy(tab["kf_Tcw"], np.float64, (-1, 12)); nkf = len(T)
    Cn = None if tab.get("kf_center") is None else _copy(tab["kf_center"], np.float64, (-1, 3))
    Xn = _copy(tab["X"], np.float64, (-1, 3)); npts = len(Xn)
    vk = _flat(vtx_kf, np.int32); lo = _flat(lie_orig, np.float64); ln = _flat(lie_opt, np.float64); nv = len(vk)
    pb = _flat(tab.get("pt_bad"), np.uint8); pd = _flat(tab.get("pt_done"), np.uint8); pc = _flat(tab.get("pt_corr_ref"), np.int32); pr = _flat(tab.get("pt_ref_kf"), np.int32)
    assert len(lo) == 7 * nv and len(ln) == 7 * nv and len(pr) == npts and (Cn is None or len(Cn) == nkf)
    assert all(v is None or len(v) == npts for v in (pb, pd, pc))
    o = {} if out is None else out
    o["pt_moved"] = np.zeros(npts, np.uint8); o["counts"] = np.zeros(2, np.int32)
    nd = [None] * 4
    n_levels = 0
    if normals:
        nd = [_flat(tab[k], np.float32 if k == "scale_factors" else np.int32) for k in _EA_ND]
        n_levels = len(nd[3])
        assert len(nd[0]) == npts + 1 and len(nd[2]) == npts and len(nd[1]) >= (nd[0][-1] if npts else 0)
        if nd[1].size == 0:
            nd[1] = np.zeros(1, np.int32)
        o.setdefault("normal", np.zeros((npts, 3))); o.setdefault("min_max", np.zeros((npts, 2), np.float32)); o.setdefault("nd_written", np.zeros(npts, np.uint8))
        for k, dt, m in (("normal", np.float64, 3 * npts), ("min_max", np.float32, 2 * npts), ("nd_written", np.uint8, npts)):
            assert o[k].dtype == dt and o[k].flags.c_contiguous and o[k].size == m, k
    else:
        o.update(normal=None, min_max=None, nd_written=None)
    nda = _p if npts else (lambda x: None)      # (no points: the set has no rows and is left out)
    _lib.check(L.orbl_essential_graph_apply(nv, _pn(vk), _pn(lo), _pn(ln), nkf, _pn(T), _pn(Cn), npts, _pn(Xn), _pn(pb), _pn(pd), _pn(pc), _pn(pr), *[nda(v) for v in nd], n_levels,
                                            nda(o["normal"]), nda(o["min_max"]), nda(o["nd_written"]), _pn(o["pt_moved"]), _p(o["counts"])), "orbl_essential_graph_apply")
    r = dict(o)
    r.update(kf_Tcw=T, kf_center=Cn, X=Xn)
    return r


def essential_graph_apply_device(vtx_kf, lie_orig, lie_opt, tab, normals=True, out=None, workspace=None, n_vtx=None):
    """orbl_essential_graph_apply_device on torch CUDA tensors, enqueued on the current stream, nothing synchronised.  kf_Tcw, kf_center and
    X of tab change IN PLACE.  n_vtx: the number of vertices when vtx_kf / lie_orig are the full-capacity tensors of
    essential_graph_assemble_device.  Returns a dict of device tensors: the three tables, pt_moved, normal / min_max / nd_written,
    counts[2], status (the EG_* bits), and the workspace under "_workspace"."""
    import torch
    L = _lib.load()
    g = tab.get
    dev = tab["kf_Tcw"].device
    nkf, npts = tab["kf_Tcw"].numel() // 12, tab["X"].numel() // 3
    nv = vtx_kf.numel() if n_vtx is None else int(n_vtx)
    assert vtx_kf.numel() >= nv and lie_orig.numel() >= 7 * nv and lie_opt.numel() >= 7 * nv
    nobs = g("obs_kf").numel() if (normals and g("obs_kf") is not None) else 0
    ws = _lib.workspace("orbl_essential_graph_apply_workspace", nkf, nv, device=dev, reuse=workspace)
    o = {} if out is None else dict(out)
    sizes = [("pt_moved", torch.uint8, npts), ("counts", torch.int32, 2), ("status", torch.int32, 1)]
    if normals:
        sizes += [("normal", torch.float64, 3 * npts), ("min_max", torch.float32, 2 * npts), ("nd_written", torch.uint8, npts)]
    for k, dt, m in sizes:
        if o.get(k) is None:
            o[k] = torch.empty(max(m, 1), dtype=dt, device=dev)[:m]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == m, k
    for k in ("kf_Tcw", "kf_center", "X"):
        assert g(k) is None or (g(k).is_contiguous() and g(k).dtype == torch.float64), k
    nd = [_p(g(k)) if (normals and npts) else None for k in _EA_ND]
    sf = g("scale_factors")
    _lib.check(L.orbl_essential_graph_apply_device(nv, _pn(vtx_kf), _pn(lie_orig), _pn(lie_opt), nkf, _pn(g("kf_Tcw")), _pn(g("kf_center")), npts, _pn(g("X")), _pn(g("pt_bad")),
                                                   _pn(g("pt_done")), _pn(g("pt_corr_ref")), _pn(g("pt_ref_kf")), nobs, nd[0], nd[1] if nobs else None, nd[2], nd[3],
                                                   sf.numel() if (normals and sf is not None) else 0,
                                                   *[_p(o.get(k)) if (normals and npts) else None for k in ("normal", "min_max", "nd_written")], _pn(o["pt_moved"]), _pn(o["counts"]),
                                                   _pn(o["status"]), _pn(ws), _lib.stream()), "orbl_essential_graph_apply_device")
    r = dict(o)
    for k in ("normal", "min_max", "nd_written"):
        r.setdefault(k, None)
    r.update(kf_Tcw=g("kf_Tcw"), kf_center=g("kf_center"), X=g("X"), _workspace=ws)
    return r


def optimize_essential_graph_on_tables(loop_kf, cur_kf, tab, min_weight=100, max_iters=100, normals=True, device=False, out=None):
    """CeresOptimizer::OptimizeEssentialGraph on the map tables: essential_graph_assemble, optimizer.optimize_essential_graph on the
    compact problem (its structure pass is host code: 7 doubles per vertex and the edge list cross to the host between the two calls),
    essential_graph_apply.  tab holds the tables of both calls.  Returns dict(assembled, lie_opt [n_vtx, 7], summary, applied)."""
    from . import optimizer
    asm = essential_graph_assemble(loop_kf, cur_kf, tab, min_weight=min_weight, device=device)
    if device:
        c = asm["counts"].cpu().tolist()                         # (waits for the stream: the solver reads the problem on the host)
        st = int(asm["status"].item()) & 0xFFFFFFFF
        if st & (EG_CAP_VTX | EG_CAP_EDGES):
            raise _lib.OrbHipError("essential_graph_assemble_device: a list did not fit (status %d)" % st)
        nv, ne = c[0], c[1]
        h = dict(lie7=asm["lie7"][:7 * nv].cpu().numpy().reshape(-1, 7), vtx_fixed=asm["vtx_fixed"][:nv].cpu().numpy(), edge_j=asm["edge_j"][:ne].cpu().numpy(),
                 edge_i=asm["edge_i"][:ne].cpu().numpy(), edge_Sji=asm["edge_Sji"][:7 * ne].cpu().numpy().reshape(-1, 7))
    else:
        h = asm
        nv = int(asm["counts"][0])
    if nv == 0:                                                  # (:795: nothing to optimise, nothing to write back)
        return dict(assembled=asm, lie_opt=np.zeros((0, 7)), summary=None, applied=None)
    lie_opt, summary = optimizer.optimize_essential_graph(h["lie7"], h["vtx_fixed"], h["edge_j"], h["edge_i"], h["edge_Sji"], max_iters)
    if device:
        import torch
        up = torch.as_tensor(np.ascontiguousarray(lie_opt)).to(tab["kf_Tcw"].device)
        applied = essential_graph_apply_device(asm["vtx_kf"], asm["lie7"], up, tab, normals=normals, out=out, n_vtx=nv)
        applied["_uploads"] = [up]
    else:
        applied = essential_graph_apply(asm["vtx_kf"], asm["lie7"], lie_opt, tab, normals=normals, out=out)
    return dict(assembled=asm, lie_opt=lie_opt, summary=summary, applied=applied)


# ---- CeresOptimizer::GlobalBundleAdjustemnt on the map tables (orbl_global_ba_assemble*, orbl_global_ba_apply*) ------------------------
GA_OFFSETS, GA_KF, GA_PT, GA_LEVEL, GA_CAP_CAM, GA_CAP_PTS, GA_CAP_OBS, GA_REPEAT, GA_POSE = 1, 2, 4, 16, 32, 64, 128, 1024, 2048    # *d_status bits
_GA_KF = (("kf_id", np.int32), ("kf_bad", np.uint8), ("kf_Tcw", np.float64), ("kf_K4", np.float64))
_GA_PT = (("X", np.float64), ("pt_bad", np.uint8), ("obs_off", np.int32), ("obs_kf", np.int32), ("obs_uv", np.float32), ("obs_level", np.int32),
          ("inv_level_sigma2", np.float32))
# (name, dtype, entries per place, which capacity) in the order of the C arguments; kf_cam [nkf] and pt_idx [npts] stand between them
_GA_OUT = (("cam_kf", np.int32, 1, 0), ("kf_cam", np.int32, 1, -1), ("K4", np.float64, 4, 0), ("poses7", np.float64, 7, 0), ("cam_fixed", np.uint8, 1, 0),
           ("gpt_pt", np.int32, 1, 1), ("pt_idx", np.int32, 1, -2), ("pts3", np.float64, 3, 1), ("gobs_cam", np.int32, 1, 2), ("gobs_pt", np.int32, 1, 2),
           ("gobs_uv", np.float64, 2, 2), ("gobs_weight", np.float64, 1, 2), ("gobs_robust", np.uint8, 1, 2), ("gobs_src", np.int32, 1, 2))
_GP_ND = ("pt_ref_kf", "obs_off", "obs_kf", "ref_level", "scale_factors")
_GP_ND_DT = (np.int32, np.int32, np.int32, np.int32, np.float32)


def _numel(a):
    return 0 if a is None else (a.numel() if hasattr(a, "numel") else np.asarray(a).size)


def _ga_sizes(tab, ba_kf, ba_pt, caps):
    nkf, npts, nobs = _numel(tab["kf_id"]), _numel(tab["X"]) // 3, _numel(tab.get("obs_kf"))
    nbk, nbp = (nkf if ba_kf is None else _numel(ba_kf)), (npts if ba_pt is None else _numel(ba_pt))
    # by default bounds no call exceeds: every list entry a camera, every listed point, every observation
    cap = (min(nbk, nkf), min(nbp, npts), nobs) if caps is None else tuple(int(c) for c in caps)
    return nkf, npts, nobs, nbk, nbp, cap


def global_ba_assemble(tab, ba_kf=None, ba_pt=None, is_robust=True, caps=None, out=None, check=True, device=False, **kw):
    """The arguments of ba_solve for CeresOptimizer::GlobalBundleAdjustemnt from the map tables (orbl_global_ba_assemble;
    include/orbslam_hip.h states the inputs and the semantics).  ba_kf, ba_pt: the keyframe and point lists, None = all.  tab: dict of the
    tables kf_id, kf_bad, kf_Tcw [nkf, 12], kf_K4 [nkf, 4], X [npts, 3], pt_bad, obs_off / obs_kf / obs_uv / obs_level, inv_level_sigma2
    (kf_bad, pt_bad may be None or missing).  caps = (cap_cam, cap_pts, cap_obs), by default bounds no call exceeds.  out: optional dict of
    preset output arrays of those capacities.  Returns a dict trimmed to the written counts: cam_kf, kf_cam [nkf], K4, poses7, cam_fixed,
    gpt_pt, pt_idx [npts], pts3, gobs_cam, gobs_pt, gobs_uv, gobs_weight, gobs_robust, gobs_src, counts = {ncam, npts_ba, nobs_ba} and rc;
    check=False returns rc = ORBHIP_ECAP with only counts filled instead of raising.  device=True: global_ba_assemble_device."""
    if device:
        return global_ba_assemble_device(tab, ba_kf=ba_kf, ba_pt=ba_pt, is_robust=is_robust, caps=caps, out=out, **kw)
    L = _lib.load()
    t = {k: _flat(tab.get(k), dt) for k, dt in _GA_KF + _GA_PT}
    bk, bp = _flat(ba_kf, np.int32), _flat(ba_pt, np.int32)
    nkf, npts, nobs, nbk, nbp, cap = _ga_sizes(t, bk, bp, caps)
    assert len(t["kf_Tcw"]) == 12 * nkf and len(t["kf_K4"]) == 4 * nkf and len(t["obs_off"]) == npts + 1
    assert all(t[k] is None or len(t[k]) == n for k, n in (("kf_bad", nkf), ("pt_bad", npts)))
    assert nobs >= (t["obs_off"][-1] if npts else 0) and len(t["obs_uv"]) == 2 * nobs and len(t["obs_level"]) == nobs
    o = {} if out is None else out
    dims = {-1: nkf, -2: npts, 0: cap[0], 1: cap[1], 2: cap[2]}
    for k, dt, w, c in _GA_OUT:
        o.setdefault(k, np.zeros(w * dims[c], dt))
        assert o[k].dtype == dt and o[k].flags.c_contiguous and o[k].size == w * dims[c], k
    o.setdefault("counts", np.zeros(3, np.int32))
    rc = L.orbl_global_ba_assemble(nbk, _pn(bk), nbp, _pn(bp), nkf, *[_pn(t[k]) for k, _ in _GA_KF], npts, *[_pn(t[k]) for k, _ in _GA_PT], len(t["inv_level_sigma2"]),
                                   int(bool(is_robust)), cap[0], cap[1], cap[2], _p(o["counts"]), *[_pn(o[k]) for k, _, _, _ in _GA_OUT])
    if rc == ECAP and not check:
        return dict(rc=rc, counts=o["counts"])
    _lib.check(rc, "orbl_global_ba_assemble")
    n = {-1: nkf, -2: npts, 0: int(o["counts"][0]), 1: int(o["counts"][1]), 2: int(o["counts"][2])}
    r = dict(rc=0, counts=o["counts"])
    for k, _, w, c in _GA_OUT:
        r[k] = o[k][:w * n[c]].reshape((-1, w) if w > 1 else (-1,))
    return r


def global_ba_assemble_device(tab, ba_kf=None, ba_pt=None, is_robust=True, caps=None, out=None, workspace=None):
    """orbl_global_ba_assemble_device on torch CUDA tensors (dtypes as in global_ba_assemble; None where a pointer may be NULL), enqueued on
    the current stream, nothing synchronised.  Returns a dict of device tensors of FULL capacity - counts[3] holds the wanted sizes, status
    (uint32 as int32[1]) the GA_* bits - with kf_cam, pt_idx and the workspace under "_workspace"."""
    import torch
    L = _lib.load()
    g = tab.get
    dev = tab["kf_id"].device
    nkf, npts, nobs, nbk, nbp, cap = _ga_sizes(tab, ba_kf, ba_pt, caps)
    ws = _lib.workspace("orbl_global_ba_assemble_workspace", nkf, npts, nbk, nbp, device=dev, reuse=workspace)
    o = {} if out is None else dict(out)
    tdt = {np.int32: torch.int32, np.float64: torch.float64, np.uint8: torch.uint8}
    dims = {-1: nkf, -2: npts, 0: cap[0], 1: cap[1], 2: cap[2]}
    sizes = [(k, tdt[dt], w * dims[c]) for k, dt, w, c in _GA_OUT] + [("counts", torch.int32, 3), ("status", torch.int32, 1)]
    for k, dt, m in sizes:
        if o.get(k) is None:
            o[k] = torch.empty(max(m, 1), dtype=dt, device=dev)[:m]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == m, k
    _lib.check(L.orbl_global_ba_assemble_device(nbk, _pn(ba_kf), nbp, _pn(ba_pt), nkf, *[_pn(g(k)) for k, _ in _GA_KF], npts, _pn(g("X")), _pn(g("pt_bad")), nobs,
                                                *[_pn(g(k)) for k, _ in _GA_PT[2:]], g("inv_level_sigma2").numel(), int(bool(is_robust)), cap[0], cap[1], cap[2],
                                                _pn(o["counts"]), *[_pn(o[k]) for k, _, _, _ in _GA_OUT], _pn(o["status"]), _pn(ws),
                                                _lib.stream()), "orbl_global_ba_assemble_device")
    r = dict(o)
    r["_workspace"] = ws                                         # (kept alive until the caller synchronises)
    return r


def global_ba_apply(cam_kf, gpt_pt, poses7, pts3, tab, stage=0, normals=True, out=None, device=False, **kw):
    """The write-back of CeresOptimizer::BundleAdjustment on the map tables (orbl_global_ba_apply; include/orbslam_hip.h states the inputs
    and the semantics).  cam_kf, gpt_pt as global_ba_assemble returned them, poses7 [ncam, 7] and pts3 [npts_ba, 3] from
    optimizer.bundle_adjustment.  tab: kf_bad, pt_bad (None or missing allowed) and, stage 0: kf_Tcw, kf_center, X and for the normals
    pt_ref_kf, obs_off, obs_kf, ref_level, scale_factors; stage 1: optional kf_gba_Tcw [nkf, 12], pt_gba_X [npts, 3] whose unwritten rows
    are kept (zeros otherwise; nkf and npts are taken from kf_Tcw and X).  normals=False leaves step 3 out.  out: optional dict of preset
    normal [npts, 3], min_max [npts, 2], nd_written [npts].  Returns a dict of new copies: stage 0 kf_Tcw, kf_center, X, normal, min_max,
    nd_written; stage 1 kf_gba_Tcw, kf_in_gba, pt_gba_X, pt_in_gba; counts = {n_poses_written, n_points_written, n_normals_written}.
    device=True: global_ba_apply_device on torch CUDA tensors, in place."""
    if device:
        return global_ba_apply_device(cam_kf, gpt_pt, poses7, pts3, tab, stage=stage, normals=normals, out=out, **kw)
    L = _lib.load()
    nkf, npts = np.asarray(tab["kf_Tcw"]).size // 12, np.asarray(tab["X"]).size // 3
    ck, gp = _flat(cam_kf, np.int32), _flat(gpt_pt, np.int32)
    p7, p3 = _flat(poses7, np.float64), _flat(pts3, np.float64)
    assert len(p7) == 7 * len(ck) and len(p3) == 3 * len(gp)
    kb, pb = _flat(tab.get("kf_bad"), np.uint8), _flat(tab.get("pt_bad"), np.uint8)
    assert (kb is None or len(kb) == nkf) and (pb is None or len(pb) == npts)
    o = {} if out is None else out
    o["counts"] = np.zeros(3, np.int32)
    T = Cn = Xn = gT = gX = kin = pin = None
    nd, ndo, n_levels = [None] * 5, [None] * 3, 0
    if stage == 0:
        T = _copy(tab["kf_Tcw"], np.float64, (-1, 12)); Xn = _copy(tab["X"], np.float64, (-1, 3))
        Cn = None if tab.get("kf_center") is None else _copy(tab["kf_center"], np.float64, (-1, 3))
        if normals:
            nd = [_flat(tab[k], dt) for k, dt in zip(_GP_ND, _GP_ND_DT)]
            n_levels = len(nd[4])
            assert len(nd[0]) == npts and len(nd[1]) == npts + 1 and len(nd[3]) == npts and len(nd[2]) >= (nd[1][-1] if npts else 0)
            if nd[2].size == 0:
                nd[2] = np.zeros(1, np.int32)
            o.setdefault("normal", np.zeros((npts, 3))); o.setdefault("min_max", np.zeros((npts, 2), np.float32)); o.setdefault("nd_written", np.zeros(npts, np.uint8))
            for k, dt, m in (("normal", np.float64, 3 * npts), ("min_max", np.float32, 2 * npts), ("nd_written", np.uint8, npts)):
                assert o[k].dtype == dt and o[k].flags.c_contiguous and o[k].size == m, k
            ndo = [o["normal"], o["min_max"], o["nd_written"]]
        else:
            o.update(normal=None, min_max=None, nd_written=None)
    else:
        gT = np.zeros((nkf, 12)) if tab.get("kf_gba_Tcw") is None else _copy(tab["kf_gba_Tcw"], np.float64, (-1, 12))
        gX = np.zeros((npts, 3)) if tab.get("pt_gba_X") is None else _copy(tab["pt_gba_X"], np.float64, (-1, 3))
        kin, pin = np.zeros(nkf, np.uint8), np.zeros(npts, np.uint8)
        assert len(gT) == nkf and len(gX) == npts
    nda = _p if npts else (lambda x: None)      # (no points: the set has no rows and is left out)
    _lib.check(L.orbl_global_ba_apply(len(ck), _pn(ck), _pn(p7), len(gp), _pn(gp), _pn(p3), int(stage), nkf, _pn(kb), _pn(T), _pn(Cn), npts, _pn(Xn), _pn(pb), _pn(gT), _pn(kin),
                                      _pn(gX), _pn(pin), *[nda(v) for v in nd], n_levels, *[nda(v) for v in ndo], _p(o["counts"])), "orbl_global_ba_apply")
    r = dict(o)
    if stage == 0:
        r.update(kf_Tcw=T, kf_center=Cn, X=Xn)
    else:
        r.update(kf_gba_Tcw=gT, kf_in_gba=kin, pt_gba_X=gX, pt_in_gba=pin)
    return r


def global_ba_apply_device(cam_kf, gpt_pt, poses7, pts3, tab, stage=0, normals=True, out=None, workspace=None, n=None):
    """orbl_global_ba_apply_device on torch CUDA tensors, enqueued on the current stream, nothing synchronised.  Stage 0: kf_Tcw, kf_center
    and X of tab change IN PLACE; stage 1: kf_gba_Tcw, kf_in_gba, pt_gba_X, pt_in_gba of tab (made when missing) are written.
    n = (ncam, npts_ba) when cam_kf / gpt_pt are the full-capacity tensors of global_ba_assemble_device.  Returns a dict of device
    tensors: the written tables, normal / min_max / nd_written, counts[3], status (the GA_* bits), the workspace under "_workspace"."""
    import torch
    L = _lib.load()
    g = tab.get
    dev = tab["kf_Tcw"].device
    nkf, npts = tab["kf_Tcw"].numel() // 12, tab["X"].numel() // 3
    ncam, npb = (cam_kf.numel(), gpt_pt.numel()) if n is None else (int(n[0]), int(n[1]))
    assert cam_kf.numel() >= ncam and poses7.numel() >= 7 * ncam and gpt_pt.numel() >= npb and pts3.numel() >= 3 * npb
    run_nd = bool(normals) and stage == 0 and npts > 0
    nobs = g("obs_kf").numel() if (run_nd and g("obs_kf") is not None) else 0
    ws = _lib.workspace("orbl_global_ba_apply_workspace", nkf, npts, device=dev, reuse=workspace)
    o = {} if out is None else dict(out)
    sizes = [("counts", torch.int32, 3), ("status", torch.int32, 1)]
    if run_nd:
        sizes += [("normal", torch.float64, 3 * npts), ("min_max", torch.float32, 2 * npts), ("nd_written", torch.uint8, npts)]
    if stage:
        for k in ("kf_gba_Tcw", "kf_in_gba", "pt_gba_X", "pt_in_gba"):
            o.setdefault(k, g(k))
        sizes += [("kf_gba_Tcw", torch.float64, 12 * nkf), ("kf_in_gba", torch.uint8, nkf), ("pt_gba_X", torch.float64, 3 * npts), ("pt_in_gba", torch.uint8, npts)]
    for k, dt, m in sizes:
        if o.get(k) is None:
            o[k] = torch.zeros(max(m, 1), dtype=dt, device=dev)[:m]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == m, k
    for k in ("kf_Tcw", "kf_center", "X"):
        assert g(k) is None or (g(k).is_contiguous() and g(k).dtype == torch.float64), k
    nd = [_p(g(k)) if run_nd else None for k in _GP_ND]
    if not nobs:
        nd[2] = None
    sf = g("scale_factors")
    s0 = stage == 0
    _lib.check(L.orbl_global_ba_apply_device(ncam, _pn(cam_kf), _pn(poses7), npb, _pn(gpt_pt), _pn(pts3), int(stage), nkf, _pn(g("kf_bad")), _pn(g("kf_Tcw")) if s0 else None,
                                             _pn(g("kf_center")) if s0 else None, npts, _pn(g("X")) if s0 else None, _pn(g("pt_bad")),
                                             *[_pn(o.get(k)) if stage else None for k in ("kf_gba_Tcw", "kf_in_gba", "pt_gba_X", "pt_in_gba")], nd[0], nobs, nd[1], nd[2], nd[3], nd[4],
                                             sf.numel() if (run_nd and sf is not None) else 0, *[_p(o.get(k)) if run_nd else None for k in ("normal", "min_max", "nd_written")],
                                             _pn(o["counts"]), _pn(o["status"]), _pn(ws), _lib.stream()), "orbl_global_ba_apply_device")
    r = dict(o)
    for k in ("normal", "min_max", "nd_written"):
        r.setdefault(k, None)
    if s0:
        r.update(kf_Tcw=g("kf_Tcw"), kf_center=g("kf_center"), X=g("X"))
    r["_workspace"] = ws
    return r


def global_bundle_adjustment_on_tables(tab, ba_kf=None, ba_pt=None, n_iterations=200, stop_flag=None, stage=0, is_robust=True, normals=True, device=False, out=None):
    """CeresOptimizer::GlobalBundleAdjustemnt on the map tables: global_ba_assemble, optimizer.bundle_adjustment on the compact problem (its
    structure pass is host code: the problem crosses to the host between the two calls, the map does not), global_ba_apply.  The write-back
    also runs after a raised stop flag: the reference writes back whatever the solve left, and RunGlobalBundleAdjustment decides afterwards
    whether to propagate.  With no camera nothing is solved and nothing written (:67-70).  Returns dict(assembled, poses7, pts3, summary,
    applied)."""
    from . import optimizer
    asm = global_ba_assemble(tab, ba_kf=ba_kf, ba_pt=ba_pt, is_robust=is_robust, device=device)
    keys = ("K4", "poses7", "cam_fixed", "pts3", "gobs_cam", "gobs_pt", "gobs_uv", "gobs_weight", "gobs_robust")
    if device:
        c = asm["counts"].cpu().tolist()                         # (waits for the stream: the solver reads the problem on the host)
        st = int(asm["status"].item()) & 0xFFFFFFFF
        if st & (GA_CAP_CAM | GA_CAP_PTS | GA_CAP_OBS):
            raise _lib.OrbHipError("global_ba_assemble_device: a list did not fit (status %d)" % st)
        per = {k: (w, c[cc]) for k, _, w, cc in _GA_OUT if cc >= 0}
        h = {k: asm[k][:per[k][0] * per[k][1]].cpu().numpy() for k in keys}
    else:
        h = asm
        c = [int(v) for v in asm["counts"]]
    if c[0] == 0:
        return dict(assembled=asm, poses7=np.zeros((0, 7)), pts3=np.zeros((0, 3)), summary=None, applied=None)
    poses7, pts3, summary = optimizer.bundle_adjustment(h["K4"].reshape(-1, 4), h["poses7"].reshape(-1, 7), h["cam_fixed"], h["pts3"].reshape(-1, 3), h["gobs_cam"], h["gobs_pt"],
                                                        h["gobs_uv"].reshape(-1, 2), h["gobs_weight"], h["gobs_robust"], n_iterations, stop_flag=stop_flag)
    if device:
        import torch
        dv = tab["kf_Tcw"].device
        up = [torch.as_tensor(np.ascontiguousarray(poses7).reshape(-1)).to(dv), torch.as_tensor(np.ascontiguousarray(pts3).reshape(-1)).to(dv)]
        applied = global_ba_apply_device(asm["cam_kf"], asm["gpt_pt"], up[0], up[1], tab, stage=stage, normals=normals, out=out, n=(c[0], c[1]))
        applied["_uploads"] = up
    else:
        applied = global_ba_apply(asm["cam_kf"], asm["gpt_pt"], poses7, pts3, tab, stage=stage, normals=normals, out=out)
    return dict(assembled=asm, poses7=poses7, pts3=pts3, summary=summary, applied=applied)


# ---- ComputeSim3's front: SearchByBoW, the gate and Sim3Solver's constructor data for every candidate ---------------------------------
LS_OFFSETS, LS_KF, LS_PT, LS_LEVEL, LS_CAP, LS_SLOT = 1, 2, 4, 8, 16, 32        # *d_status bits of orbl_loop_sim3_candidates_device
LS_KEPT, LS_BAD_KEYFRAME, LS_FEW_MATCHES = 0, 1, 2                              # cand_status
# (key, dtype, width) of the tables, in the order the entry takes them
_LS_KF = (("kf_bad", np.uint8, 1), ("kf_Tcw", np.float64, 12), ("kf_K4", np.float32, 4))
_LS_SLOT = (("kf_slot_off", np.int32, 1), ("kf_slot_pt", np.int32, 1), ("kf_slot_level", np.int32, 1), ("kf_slot_angle", np.float32, 1), ("kf_slot_desc", np.uint8, 32))
_LS_FV = (("kf_fv_off", np.int32, 1), ("fv_node", np.uint32, 1), ("fv_ent_off", np.int32, 1), ("fv_ent", np.int32, 1))
_LS_PT = (("pt_bad", np.uint8, 1), ("X", np.float64, 3))
_LS_OBS = (("obs_off", np.int32, 1), ("obs_kf", np.int32, 1), ("obs_slot", np.int32, 1))
# (key, dtype, elements per candidate / per row, which of the two)
_LS_OUT = (("match12", np.int32, None, "cand"), ("nmatches", np.int32, 1, "cand"), ("cand_status", np.int32, 1, "cand"), ("K1", np.float32, 4, "cand"),
           ("K2", np.float32, 4, "cand"), ("off", np.int32, None, "off"), ("X1c", np.float64, 3, "row"), ("X2c", np.float64, 3, "row"), ("max_err1", np.float32, 1, "row"),
           ("max_err2", np.float32, 1, "row"), ("row_i1", np.int32, 1, "row"), ("row_pt1", np.int32, 1, "row"), ("row_pt2", np.int32, 1, "row"), ("counts", np.int32, None, "two"))


def _ls_out_size(kind, per, n_cand, cap1, cap_rows):
    return {"cand": n_cand * (cap1 if per is None else per), "off": n_cand + 1, "row": cap_rows * (per or 1), "two": 2}[kind]


def sim3_candidates(tab, cur_kf, cand_kf, nnratio=0.75, check_ori=True, min_matches=20, cap1=None, cap_rows=None, device=False, **kw):
    """ComputeSim3's front for every candidate in one call (orbl_loop_sim3_candidates; include/orbslam_hip.h states the inputs and the
    semantics): SearchByBoW(cur_kf, candidate), the min_matches gate and the rows Sim3Solver's constructor builds.  tab: the map tables
    kf_bad (may be None), kf_Tcw [nkf, 12], kf_K4 [nkf, 4], kf_slot_off / kf_slot_pt / kf_slot_level / kf_slot_angle / kf_slot_desc
    [nslots, 32], kf_fv_off / fv_node / fv_ent_off / fv_ent, pt_bad, X [npts, 3], obs_off / obs_kf / obs_slot, level_sigma2.  cap1
    defaults to the current keyframe's slot count, cap_rows to n_cand times that.  Returns a dict: match12 [n_cand, cap1], nmatches,
    cand_status, K1, K2 [n_cand, 4], off [n_cand + 1], counts = {rows, candidates kept} and, cut to counts[0] rows, X1c, X2c [rows, 3],
    max_err1, max_err2, row_i1, row_pt1, row_pt2.  Raises OrbHipError (ORBHIP_ECAP) when a capacity is too small.
    device=True: sim3_candidates_device on torch CUDA tensors."""
    if device:
        return sim3_candidates_device(tab, cur_kf, cand_kf, nnratio=nnratio, check_ori=check_ori, min_matches=min_matches, cap1=cap1, cap_rows=cap_rows, **kw)
    L = _lib.load()
    ck = _c(cand_kf, np.int32).reshape(-1)
    t = {k: _flat(tab.get(k), dt) for k, dt, _ in _LS_KF + _LS_SLOT + _LS_FV + _LS_PT + _LS_OBS}
    sig = _c(tab["level_sigma2"], np.float32).reshape(-1)
    so = t["kf_slot_off"]
    nkf, npts = len(so) - 1, len(t["pt_bad"])
    assert len(t["kf_Tcw"]) == 12 * nkf and len(t["kf_K4"]) == 4 * nkf and len(t["kf_fv_off"]) == nkf + 1 and len(t["X"]) == 3 * npts and len(t["obs_off"]) == npts + 1
    assert all(len(t[k]) == w * so[-1] for k, _, w in _LS_SLOT[1:]) and len(t["fv_ent_off"]) == len(t["fv_node"]) + 1
    n1 = int(so[cur_kf + 1] - so[cur_kf]) if 0 <= cur_kf < nkf else 0
    cap1 = n1 if cap1 is None else int(cap1)
    cap_rows = len(ck) * n1 if cap_rows is None else int(cap_rows)
    o = {k: np.zeros(_ls_out_size(kind, per, len(ck), cap1, cap_rows), dt) for k, dt, per, kind in _LS_OUT}
    _lib.check(L.orbl_loop_sim3_candidates(int(cur_kf), len(ck), _p(ck), nkf, *[_p(t[k]) for k, _, _ in _LS_KF + _LS_SLOT + _LS_FV], npts,
                                           *[_p(t[k]) for k, _, _ in _LS_PT + _LS_OBS], _p(sig), len(sig), float(nnratio), int(bool(check_ori)), int(min_matches),
                                           cap1, cap_rows, *[_p(o[k]) for k, _, _, _ in _LS_OUT]), "orbl_loop_sim3_candidates")
    rows = int(o["counts"][0])
    for k, _, per, kind in _LS_OUT:
        if kind == "row":
            o[k] = o[k][:rows * per].reshape((rows, per) if per > 1 else (rows,))
        elif kind == "cand" and per != 1:
            o[k] = o[k].reshape(len(ck), -1)
    return o


def sim3_candidates_device(tab, cur_kf, cand_kf, nnratio=0.75, check_ori=True, min_matches=20, cap1=None, cap_rows=None, out=None, workspace=None):
    """orbl_loop_sim3_candidates_device on torch CUDA tensors (the tables of sim3_candidates, flat or shaped, in its dtypes; cand_kf an
    int32 tensor), enqueued on the current stream, nothing synchronised and nothing read back: cap1 and cap_rows are therefore the
    caller's to give (cap1 at least the current keyframe's slot count).  out: optional dict of preset output tensors; workspace: an
    optional uint8 tensor to reuse.  Returns a dict of device tensors: match12 [n_cand, cap1], nmatches, cand_status, K1, K2, off, X1c,
    X2c [cap_rows, 3], max_err1, max_err2, row_i1, row_pt1, row_pt2 [cap_rows], counts [2], status (the LS_* bits) and the workspace
    under "_workspace".  X1c, X2c, max_err1, max_err2, off, K1, K2 go to sim3solver.iterate_batch_device as they are."""
    import torch
    L = _lib.load()
    assert cap1 is not None and cap_rows is not None, "the device form reads nothing back: give cap1 and cap_rows"
    dev = tab["kf_Tcw"].device
    n_cand = cand_kf.numel()
    tt = {torch.uint8: np.uint8, torch.int32: np.int32, torch.float32: np.float32, torch.float64: np.float64}
    for k, dt, _ in _LS_KF + _LS_SLOT + _LS_FV + _LS_PT + _LS_OBS + (("level_sigma2", np.float32, 1),):
        v = tab.get(k)
        assert v is None or (v.is_contiguous() and (tt.get(v.dtype) == dt or (dt == np.uint32 and v.dtype == torch.int32))), k
    assert cand_kf.dtype == torch.int32 and cand_kf.is_contiguous()
    nkf, nslots, nfv, nent = tab["kf_slot_off"].numel() - 1, tab["kf_slot_pt"].numel(), tab["fv_node"].numel(), tab["fv_ent"].numel()
    npts, nobs = tab["pt_bad"].numel(), tab["obs_kf"].numel()
    ws = _lib.workspace("orbl_loop_sim3_candidates_workspace", n_cand, int(cap1), device=dev, min_bytes=16, reuse=workspace)
    to = {np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}
    o = {} if out is None else dict(out)
    sizes = [(k, to[dt], _ls_out_size(kind, per, n_cand, int(cap1), int(cap_rows))) for k, dt, per, kind in _LS_OUT] + [("status", torch.int32, 1)]
    for k, dt, n in sizes:
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 1), dtype=dt, device=dev)[:n]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == n, k
    g = tab.get
    _lib.check(L.orbl_loop_sim3_candidates_device(int(cur_kf), n_cand, _p(cand_kf), nkf, _p(g("kf_bad")), _p(g("kf_Tcw")), _p(g("kf_K4")), nslots, _p(g("kf_slot_off")),
                                                  _pn(g("kf_slot_pt")), _pn(g("kf_slot_level")), _pn(g("kf_slot_angle")), _pn(g("kf_slot_desc")), nfv, _p(g("kf_fv_off")),
                                                  _pn(g("fv_node")), nent, _p(g("fv_ent_off")), _pn(g("fv_ent")), npts, _pn(g("pt_bad")), _pn(g("X")), nobs,
                                                  _p(g("obs_off")), _pn(g("obs_kf")), _pn(g("obs_slot")), _p(g("level_sigma2")), g("level_sigma2").numel(), float(nnratio),
                                                  int(bool(check_ori)), int(min_matches), int(cap1), int(cap_rows), *[_pn(o[k]) for k, _, _, _ in _LS_OUT], _p(o["status"]),
                                                  _p(ws), _lib.stream()), "orbl_loop_sim3_candidates_device")
    r = dict(o)
    r["match12"] = r["match12"].view(n_cand, -1) if cap1 else r["match12"]
    for k in ("K1", "K2"):
        r[k] = r[k].view(n_cand, 4)
    for k in ("X1c", "X2c"):
        r[k] = r[k].view(-1, 3)
    r["_workspace"] = ws                                                                # (kept alive until the caller synchronises)
    return r
