"""Host mirror of the LocalMapping thread's device-resident steps (include/orbslam_hip.h: orbl_*; reference
src/LocalMapping.cc:196-396 CreateNewMapPoints, :398-505 SearchInNeighbors, :576-637 KeyFrameCulling; src/KeyFrame.cc:314-398 UpdateConnections).
Thin ctypes layer: arrays in, arrays out."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import carray as _c, flat as _flat, ptr as _p, ptr_nonempty as _pn


class _KF(C.Structure):              # orbl_keyframe
    _fields_ = [("kps", C.c_void_p), ("desc", C.c_void_p), ("unmapped", C.c_void_p), ("n", C.c_int),
                ("fv_node", C.c_void_p), ("fv_off", C.c_void_p), ("fv_idx", C.c_void_p), ("fv_n", C.c_int),
                ("Tcw", C.c_double * 12), ("K4", C.c_float * 4), ("F12", C.c_double * 9), ("ex", C.c_float), ("ey", C.c_float)]


class _FuseKF(C.Structure):          # orbl_fuse_keyframe
    _fields_ = [("kps", C.c_void_p), ("desc", C.c_void_p), ("n", C.c_int), ("bounds", C.c_float * 4)]


def prepare_create_new_map_points(cur, neighbours, scale_factors, level_sigma2, ratio_factor, stop=None):
    """Marshals the arguments of orbl_create_new_map_points once and returns call() -> (match12, ok, x3D, n_processed): what a C++
    caller holds anyway (tools/api_latency.py times call() alone)."""
    L = _lib.load()
    keep = []                                                   # the arrays the structs point at

    def hold(a, dt):
        a = _c(a, dt); keep.append(a); return a
    k1 = hold(cur["kps"], np.float32).reshape(-1, 4); n1 = len(k1)
    d1 = hold(cur["desc"], np.uint8).reshape(-1, 32)
    u1 = hold(cur["unmapped"], np.uint8) if cur.get("unmapped") is not None else None
    f1 = [hold(x, np.uint32) for x in cur["fv"]]
    T1 = hold(np.asarray(cur["Tcw"], np.float64).reshape(-1)[:12], np.float64); K1 = hold(cur["K4"], np.float32)
    nb = (_KF * max(len(neighbours), 1))()
    for k, q in enumerate(neighbours):
        kk = hold(q["kps"], np.float32).reshape(-1, 4); dd = hold(q["desc"], np.uint8).reshape(-1, 32)
        uu = hold(q["unmapped"], np.uint8) if q.get("unmapped") is not None else None
        ff = [hold(x, np.uint32) for x in q["fv"]]
        assert len(dd) == len(kk) and len(ff[1]) == len(ff[0]) + 1
        s = nb[k]
        s.kps, s.desc, s.unmapped, s.n = kk.ctypes.data, dd.ctypes.data, (uu.ctypes.data if uu is not None else None), len(kk)
        s.fv_node, s.fv_off, s.fv_idx, s.fv_n = ff[0].ctypes.data, ff[1].ctypes.data, ff[2].ctypes.data, len(ff[0])
        s.Tcw[:] = np.asarray(q["Tcw"], np.float64).reshape(-1)[:12].tolist(); s.K4[:] = _c(q["K4"], np.float32).tolist()
        s.F12[:] = np.asarray(q["F12"], np.float64).reshape(9).tolist()
        s.ex, s.ey = float(q["epipole"][0]), float(q["epipole"][1])
    sf = hold(scale_factors, np.float32); ls = hold(level_sigma2, np.float32)
    nn = len(neighbours)
    m = np.full((max(nn, 1), max(n1, 1)), -1, np.int32); ok = np.zeros((max(nn, 1), max(n1, 1)), np.uint8); X = np.zeros((max(nn, 1), max(n1, 1), 3), np.float64)
    npr = C.c_int(0)
    st = None
    if stop is not None:
        assert stop.dtype == np.uint8 and stop.size >= 1
        st = _p(stop)
    a = (_p(k1), _p(d1), _p(u1), n1, _p(f1[0]), _p(f1[1]), _p(f1[2]), len(f1[0]), _p(T1), _p(K1), C.cast(nb, C.c_void_p), nn, _p(sf), _p(ls),
         len(sf), float(ratio_factor), st, _p(m), _p(ok), _p(X), C.byref(npr))

    def call():
        _lib.check(L.orbl_create_new_map_points(*a), "orbl_create_new_map_points")
        return m[:nn, :n1], ok[:nn, :n1].view(np.bool_), X[:nn, :n1], npr.value
    call._keep = (keep, nb)
    return call


def create_new_map_points(cur, neighbours, scale_factors, level_sigma2, ratio_factor, stop=None):
    """LocalMapping::CreateNewMapPoints for the current keyframe and its neighbours, in order, in one call.
    cur = dict(kps[n1,4] {x, y, octave, angle}, desc[n1,32], unmapped[n1] (or None), fv=(nodes, offsets, indices), Tcw[3,4], K4);
    each neighbour the same plus F12[3,3] and epipole=(ex, ey).  stop: optional 1-element uint8 array (CheckNewKeyFrames).
    Returns (match12[nb, n1] int32, ok[nb, n1] bool, x3D[nb, n1, 3] float64, n_processed)."""
    return prepare_create_new_map_points(cur, neighbours, scale_factors, level_sigma2, ratio_factor, stop)()


def fuse_batch(keyframes, q_uv, q_radius, q_level, mp_desc, inv_level_sigma2, sim3=False, n_levels=8):
    """ORBmatcher::Fuse candidate selection for T keyframes x M map points (orbl_fuse_batch; sim3=True: orbl_fuse_batch_sim3, the form of
    LoopClosing::SearchAndFuse without the chi-square gate, inv_level_sigma2 unused).  keyframes: dicts(kps[n,4], desc[n,32],
    bounds[4]); q_uv[T,M,2], q_radius[T,M], q_level[T,M] (-1: not projected), mp_desc[M,32].  Returns (best_idx[T,M], best_dist[T,M])."""
    L = _lib.load()
    keep = []
    T = len(keyframes)
    if T == 0:
        return np.zeros((0, 0), np.int32), np.zeros((0, 0), np.int32)
    kf = (_FuseKF * max(T, 1))()
    for t, q in enumerate(keyframes):
        kk = _c(q["kps"], np.float32).reshape(-1, 4); dd = _c(q["desc"], np.uint8).reshape(-1, 32); keep += [kk, dd]
        kf[t].kps, kf[t].desc, kf[t].n = kk.ctypes.data, dd.ctypes.data, len(kk)
        kf[t].bounds[:] = _c(q["bounds"], np.float32).tolist()
    uv = _c(q_uv, np.float32).reshape(T, -1, 2); M = uv.shape[1]
    rad = _c(q_radius, np.float32).reshape(T, M); lvl = _c(q_level, np.int32).reshape(T, M)
    md = _c(mp_desc, np.uint8).reshape(M, 32)
    bi = np.full((max(T, 1), max(M, 1)), -1, np.int32); bd = np.full((max(T, 1), max(M, 1)), 256, np.int32)
    if sim3:
        _lib.check(L.orbl_fuse_batch_sim3(C.cast(kf, C.c_void_p), T, _p(uv), _p(rad), _p(lvl), M, _p(md), int(n_levels), _p(bi), _p(bd)),
                   "orbl_fuse_batch_sim3")
        return bi[:T, :M], bd[:T, :M]
    ils = _c(inv_level_sigma2, np.float32)
    _lib.check(L.orbl_fuse_batch(C.cast(kf, C.c_void_p), T, _p(uv), _p(rad), _p(lvl), M, _p(md), _p(ils), len(ils), _p(bi), _p(bd)),
               "orbl_fuse_batch")
    return bi[:T, :M], bd[:T, :M]


MP_DESC = 1                          # ORBL_MP_DESC
MP_NORMAL_DEPTH = 2                  # ORBL_MP_NORMAL_DEPTH


def update_map_points(obs_off, obs_desc=None, obs_kf_good=None, X=None, ref_kf=None, ref_level=None, obs_kf=None, kf_center=None,
                      scale_factors=None, pt_good=None, what=MP_DESC | MP_NORMAL_DEPTH, out=None):
    """MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth for a batch of points (orbl_update_map_points).
    obs_off[npts+1] CSR offsets into the observation arrays (list order = the point's std::map order); obs_desc[nobs,32],
    obs_kf_good[nobs] (None = all good) for the descriptor; X[npts,3], ref_kf[npts], ref_level[npts], obs_kf[nobs],
    kf_center[nkf,3], scale_factors[n_levels] for the normal and depth; pt_good[npts] (None = all good).
    out: optional dict of preset output arrays (best_obs, desc, normal, min_max, nd_written); entries the call leaves unchanged
    keep their values.  Returns that dict: best_obs[npts] int32 (-1 = descriptor unchanged), desc[npts,32] uint8,
    normal[npts,3] float64, min_max[npts,2] float32 {min, max}, nd_written[npts] uint8."""
    L = _lib.load()
    off = _c(obs_off, np.int32).reshape(-1)
    npts = len(off) - 1
    nobs = int(off[-1]) if npts >= 0 and len(off) else 0
    o = {} if out is None else out
    o.setdefault("best_obs", np.full(max(npts, 0), -1, np.int32)); o.setdefault("desc", np.zeros((max(npts, 0), 32), np.uint8))
    o.setdefault("normal", np.zeros((max(npts, 0), 3), np.float64)); o.setdefault("min_max", np.zeros((max(npts, 0), 2), np.float32))
    o.setdefault("nd_written", np.zeros(max(npts, 0), np.uint8))
    for k, dt in (("best_obs", np.int32), ("desc", np.uint8), ("normal", np.float64), ("min_max", np.float32), ("nd_written", np.uint8)):
        assert o[k].dtype == dt and o[k].flags.c_contiguous, k
    desc = _c(obs_desc, np.uint8).reshape(-1, 32) if obs_desc is not None else None
    kg = _c(obs_kf_good, np.uint8) if obs_kf_good is not None else None
    Xa = _c(X, np.float64).reshape(-1, 3) if X is not None else None
    rk = _c(ref_kf, np.int32) if ref_kf is not None else None
    rl = _c(ref_level, np.int32) if ref_level is not None else None
    ok_ = _c(obs_kf, np.int32) if obs_kf is not None else None
    kc = _c(kf_center, np.float64).reshape(-1, 3) if kf_center is not None else None
    sf = _c(scale_factors, np.float32) if scale_factors is not None else None
    pg = _c(pt_good, np.uint8) if pt_good is not None else None
    _lib.check(L.orbl_update_map_points(npts, _p(off), _p(Xa), _p(rk), _p(rl), _p(pg), nobs, _p(ok_), _p(desc), _p(kg),
                                        len(kc) if kc is not None else 0, _p(kc), _p(sf), len(sf) if sf is not None else 0, int(what),
                                        _p(o["best_obs"]), _p(o["desc"]), _p(o["normal"]), _p(o["min_max"]), _p(o["nd_written"])),
               "orbl_update_map_points")
    return o


def update_map_points_device(obs_off, obs_desc, obs_kf_good, X, ref_kf, ref_level, obs_kf, kf_center, scale_factors, pt_good, what, out):
    """orbl_update_map_points_device on torch CUDA tensors (the same arguments as update_map_points; None where a pointer may be
    NULL); out = dict of device tensors (best_obs, desc, normal, min_max, nd_written), written on the current stream."""
    L = _lib.load()
    npts = obs_off.numel() - 1
    nobs = obs_desc.shape[0] if obs_desc is not None else (obs_kf.numel() if obs_kf is not None else 0)
    ws = _lib.workspace("orbl_update_map_points_workspace", npts, device=obs_off.device, min_bytes=16)
    _lib.check(L.orbl_update_map_points_device(npts, _p(obs_off), _p(X), _p(ref_kf), _p(ref_level), _p(pt_good), nobs, _p(obs_kf), _p(obs_desc), _p(obs_kf_good),
                                               kf_center.shape[0] if kf_center is not None else 0, _p(kf_center), _p(scale_factors),
                                               scale_factors.numel() if scale_factors is not None else 0, int(what), _p(out.get("best_obs")), _p(out.get("desc")),
                                               _p(out.get("normal")), _p(out.get("min_max")), _p(out.get("nd_written")), _p(ws),
                                               _lib.stream()), "orbl_update_map_points_device")
    out["_workspace"] = ws                                       # (kept alive until the caller synchronises)
    return out


class CullingResult:
    """What orbl_keyframe_culling reports: culled[ncand] uint8, n_redundant[ncand] / n_map_points[ncand] int32 as seen at each
    candidate's turn, and the final state pt_bad[npts] uint8, pt_nobs[npts] int32, obs_erased[nobs] uint8 (None where not asked for);
    status: the device form's d_status tensor (None in the host form)."""
    __slots__ = ("culled", "n_redundant", "n_map_points", "pt_bad", "pt_nobs", "obs_erased", "status", "_workspace")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def keyframe_culling(cand_kf, cand_flags, slot_off, slot_pt, slot_level, nkf, obs_off, obs_kf, obs_level, pt_bad=None, pt_nobs=None,
                     th_obs=3, ratio=0.9, final_state=True, out=None):
    """LocalMapping::KeyFrameCulling for the whole candidate list with the reference's sequential semantics (orbl_keyframe_culling;
    include/orbslam_hip.h states the inputs).  cand_kf[ncand], cand_flags[ncand] (None = all 0; bit 0: id_ == 0, bit 1:
    do_not_erase_), slot_off[ncand + 1], slot_pt / slot_level[nslots], obs_off[npts + 1], obs_kf / obs_level[nobs], pt_bad[npts]
    (None = none bad), pt_nobs[npts] (None = the list lengths).  final_state=False passes NULL for the three state outputs.
    out: optional dict of preset output arrays (every element is overwritten).  Returns a CullingResult."""
    L = _lib.load()
    ck = _c(cand_kf, np.int32).reshape(-1); ncand = len(ck)
    cf = _c(cand_flags, np.uint8).reshape(-1) if cand_flags is not None else None
    so = _c(slot_off, np.int32).reshape(-1); sp = _c(slot_pt, np.int32).reshape(-1); sl = _c(slot_level, np.int32).reshape(-1)
    oo = _c(obs_off, np.int32).reshape(-1); ok_ = _c(obs_kf, np.int32).reshape(-1); ol = _c(obs_level, np.int32).reshape(-1)
    npts = len(oo) - 1
    assert len(so) == ncand + 1 and npts >= 0 and (cf is None or len(cf) == ncand) and len(sp) == len(sl) and len(ok_) == len(ol)
    assert len(sp) >= (so[-1] if ncand else 0) and len(ok_) >= (oo[-1] if npts else 0)     # (the library checks the rest)
    pb = _c(pt_bad, np.uint8).reshape(-1) if pt_bad is not None else None
    pn = _c(pt_nobs, np.int32).reshape(-1) if pt_nobs is not None else None
    assert (pb is None or len(pb) == npts) and (pn is None or len(pn) == npts)
    o = {} if out is None else out
    o.setdefault("culled", np.zeros(ncand, np.uint8)); o.setdefault("n_redundant", np.zeros(ncand, np.int32)); o.setdefault("n_map_points", np.zeros(ncand, np.int32))
    if final_state:
        o.setdefault("pt_bad", np.zeros(npts, np.uint8)); o.setdefault("pt_nobs", np.zeros(npts, np.int32)); o.setdefault("obs_erased", np.zeros(len(ok_), np.uint8))
    for k, dt, n in (("culled", np.uint8, ncand), ("n_redundant", np.int32, ncand), ("n_map_points", np.int32, ncand), ("pt_bad", np.uint8, npts),
                     ("pt_nobs", np.int32, npts), ("obs_erased", np.uint8, len(ok_))):
        assert o.get(k) is None or (o[k].dtype == dt and o[k].flags.c_contiguous and o[k].size == n), k
    _lib.check(L.orbl_keyframe_culling(ncand, _p(ck), _p(cf), _p(so), _p(sp), _p(sl), int(nkf), npts, _p(oo), _p(ok_), _p(ol), _p(pb),
                                       _p(pn), int(th_obs), float(ratio), _p(o["culled"]), _p(o["n_redundant"]), _p(o["n_map_points"]),
                                       _p(o.get("pt_bad")), _p(o.get("pt_nobs")), _p(o.get("obs_erased"))), "orbl_keyframe_culling")
    return CullingResult(**o)


def keyframe_culling_device(cand_kf, cand_flags, slot_off, slot_pt, slot_level, nkf, obs_off, obs_kf, obs_level, pt_bad=None, pt_nobs=None,
                            th_obs=3, ratio=0.9, final_state=True, out=None):
    """orbl_keyframe_culling_device on torch CUDA tensors (int32 / uint8 as in keyframe_culling; None where a pointer may be NULL),
    enqueued on the current stream.  out: optional dict of preset device tensors.  Returns a CullingResult of device tensors whose
    status (uint32 as int32[1]) is 0 when every entry was in range; the workspace is kept alive by the result."""
    import torch
    L = _lib.load()
    dev = cand_kf.device
    ncand, nslots, npts, nobs = cand_kf.numel(), slot_pt.numel(), obs_off.numel() - 1, obs_kf.numel()
    ws = _lib.workspace("orbl_keyframe_culling_workspace", ncand, nslots, npts, nobs, device=dev)
    o = {} if out is None else out
    for k, dt, n in (("culled", torch.uint8, ncand), ("n_redundant", torch.int32, ncand), ("n_map_points", torch.int32, ncand)) + \
            ((("pt_bad", torch.uint8, npts), ("pt_nobs", torch.int32, npts), ("obs_erased", torch.uint8, nobs)) if final_state else ()):
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 1), dtype=dt, device=dev)[:n]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == n, k
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(L.orbl_keyframe_culling_device(ncand, _p(cand_kf), _p(cand_flags), nslots, _p(slot_off), _p(slot_pt), _p(slot_level), int(nkf), npts, nobs, _p(obs_off),
                                              _p(obs_kf), _p(obs_level), _p(pt_bad), _p(pt_nobs), int(th_obs), float(ratio), _p(o["culled"]), _p(o["n_redundant"]),
                                              _p(o["n_map_points"]), _p(o.get("pt_bad")), _p(o.get("pt_nobs")), _p(o.get("obs_erased")), _p(status), _p(ws),
                                              _lib.stream()), "orbl_keyframe_culling_device")
    return CullingResult(status=status, _workspace=ws, **o)


ECAP = -4                            # ORBHIP_ECAP
UC_OFFSETS, UC_INDEX, UC_CAP_AFF, UC_CAP_CONN, UC_CAP_ORD, UC_CAP_LINK = 1, 2, 4, 8, 16, 32      # *d_status bits of orbl_update_connections_device


def _uc_default_caps(ntgt, nkf, nconn, links):
    """capacities no call can exceed: a final map is a counter (at most nkf - 1 entries) or an input row plus one entry per target"""
    cap = min(nkf * max(nkf - 1, 0), nconn + 2 * ntgt * nkf)
    return nkf, cap, cap, (ntgt * nkf if links else 0)


def update_connections(tgt_kf, slot_off, slot_pt, nkf, obs_off, obs_kf, conn_off, conn_kf, conn_w, tgt_flags=None, pt_bad=None, kf_rank=None,
                       prev_off=None, prev_kf=None, th=15, links=None, caps=None, out=None, check=True):
    """KeyFrame::UpdateConnections on the keyframes tgt_kf, one after the other, in one call (orbl_update_connections;
    include/orbslam_hip.h states the inputs and the semantics).  tgt_flags, pt_bad, kf_rank and the pair prev_off / prev_kf may be None;
    links (default: whether prev is given) asks for the loop links.  caps = (cap_aff, cap_conn, cap_ord, cap_link), default: bounds no call
    exceeds.  out: optional dict of preset output arrays of those capacities (aff_kf, conn_off, conn_kf, conn_w, ord_off, ord_kf, ord_w,
    link_off, link_kf, tgt_status, tgt_parent, counts).  Returns a dict of int32 arrays trimmed to the written counts, with counts =
    {n_aff, n_conn, n_ord, n_link} and rc; check=False returns rc = ORBHIP_ECAP with only counts filled instead of raising."""
    L = _lib.load()
    tk = _c(tgt_kf, np.int32).reshape(-1); ntgt = len(tk)
    tf = _c(tgt_flags, np.uint8).reshape(-1) if tgt_flags is not None else None
    so = _c(slot_off, np.int32).reshape(-1); sp = _c(slot_pt, np.int32).reshape(-1)
    oo = _c(obs_off, np.int32).reshape(-1); ok_ = _c(obs_kf, np.int32).reshape(-1)
    pb = _c(pt_bad, np.uint8).reshape(-1) if pt_bad is not None else None
    kr = _c(kf_rank, np.int32).reshape(-1) if kf_rank is not None else None
    co = _c(conn_off, np.int32).reshape(-1); ck = _c(conn_kf, np.int32).reshape(-1); cw = _c(conn_w, np.int32).reshape(-1)
    po = _c(prev_off, np.int32).reshape(-1) if prev_off is not None else None
    pk = _c(prev_kf, np.int32).reshape(-1) if prev_kf is not None else None
    if pk is not None and pk.size == 0:
        pk = np.zeros(1, np.int32)                              # (an empty list still needs a pointer: the pair is given or not)
    npts = len(oo) - 1
    assert len(so) == ntgt + 1 and npts >= 0 and len(co) == int(nkf) + 1 and len(ck) == len(cw) and (tf is None or len(tf) == ntgt)
    assert (pb is None or len(pb) == npts) and (kr is None or len(kr) == nkf) and (po is None or len(po) == ntgt + 1)
    assert len(sp) >= so[-1] and len(ok_) >= oo[-1] and len(ck) >= co[-1] and (po is None or pk is None or len(pk) >= po[-1])      # (the library checks the rest)
    links = po is not None if links is None else links
    cap_aff, cap_conn, cap_ord, cap_link = _uc_default_caps(ntgt, int(nkf), len(ck), links) if caps is None else caps
    o = {} if out is None else out
    sizes = dict(tgt_status=ntgt, tgt_parent=ntgt, aff_kf=cap_aff, conn_off=cap_aff + 1, conn_kf=cap_conn, conn_w=cap_conn, ord_off=cap_aff + 1, ord_kf=cap_ord,
                 ord_w=cap_ord, counts=4)
    if links:
        sizes.update(link_off=ntgt + 1, link_kf=cap_link)
    for k, n in sizes.items():
        o.setdefault(k, np.zeros(n, np.int32))
        assert o[k].dtype == np.int32 and o[k].flags.c_contiguous and o[k].size == n, k
    rc = L.orbl_update_connections(ntgt, _p(tk), _p(tf), _p(so), _p(sp), int(nkf), npts, _p(oo), _p(ok_), _p(pb), _p(kr), _p(co), _p(ck),
                                   _p(cw), _p(po), _p(pk), int(th), cap_aff, cap_conn, cap_ord, cap_link, _p(o["tgt_status"]), _p(o["tgt_parent"]),
                                   _p(o["aff_kf"]), _p(o["conn_off"]), _p(o["conn_kf"]), _p(o["conn_w"]), _p(o["ord_off"]), _p(o["ord_kf"]),
                                   _p(o["ord_w"]), _p(o.get("link_off")), _p(o.get("link_kf")), _p(o["counts"]))
    if rc == ECAP and not check:
        return dict(rc=rc, counts=o["counts"])
    _lib.check(rc, "orbl_update_connections")
    n_aff, n_conn, n_ord, n_link = (int(v) for v in o["counts"])
    r = dict(rc=0, counts=o["counts"], tgt_status=o["tgt_status"], tgt_parent=o["tgt_parent"], aff_kf=o["aff_kf"][:n_aff], conn_off=o["conn_off"][:n_aff + 1],
             conn_kf=o["conn_kf"][:n_conn], conn_w=o["conn_w"][:n_conn], ord_off=o["ord_off"][:n_aff + 1], ord_kf=o["ord_kf"][:n_ord], ord_w=o["ord_w"][:n_ord],
             link_off=None, link_kf=None)
    if links:
        r.update(link_off=o["link_off"], link_kf=o["link_kf"][:n_link])
    return r


def update_connections_device(tgt_kf, slot_off, slot_pt, nkf, obs_off, obs_kf, conn_off, conn_kf, conn_w, tgt_flags=None, pt_bad=None, kf_rank=None,
                              prev_off=None, prev_kf=None, th=15, links=None, caps=None, out=None, workspace=None):
    """orbl_update_connections_device on torch CUDA tensors (int32 / uint8 as in update_connections; None where a pointer may be NULL),
    enqueued on the current stream, nothing synchronised.  out: optional dict of preset device tensors of the capacities; workspace:
    optional uint8 tensor to reuse (it is cleared by every call).  Returns a dict of device tensors of FULL capacity - counts[4] holds
    the wanted sizes, status (uint32 as int32[1]) the UC_* bits - and the workspace under "_workspace"."""
    import torch
    L = _lib.load()
    dev = tgt_kf.device
    ntgt, nslots, npts, nobs, nconn = tgt_kf.numel(), slot_pt.numel(), obs_off.numel() - 1, obs_kf.numel(), conn_kf.numel()
    nprev = prev_kf.numel() if prev_kf is not None else 0
    links = prev_off is not None if links is None else links
    cap_aff, cap_conn, cap_ord, cap_link = _uc_default_caps(ntgt, int(nkf), nconn, links) if caps is None else caps
    ws = _lib.workspace("orbl_update_connections_workspace", ntgt, int(nkf), npts, nslots, nconn, device=dev, reuse=workspace)
    o = {} if out is None else out
    sizes = dict(tgt_status=ntgt, tgt_parent=ntgt, aff_kf=cap_aff, conn_off=cap_aff + 1, conn_kf=cap_conn, conn_w=cap_conn, ord_off=cap_aff + 1, ord_kf=cap_ord,
                 ord_w=cap_ord, counts=4, status=1)
    if links:
        sizes.update(link_off=ntgt + 1, link_kf=cap_link)
    for k, n in sizes.items():
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
        assert o[k].dtype == torch.int32 and o[k].is_contiguous() and o[k].numel() == n, k
    _lib.check(L.orbl_update_connections_device(ntgt, _p(tgt_kf), _p(tgt_flags), nslots, _p(slot_off), _p(slot_pt), int(nkf), npts, nobs, _p(obs_off), _p(obs_kf), _p(pt_bad),
                                                _p(kf_rank), nconn, _p(conn_off), _p(conn_kf), _p(conn_w), nprev, _p(prev_off), _p(prev_kf), int(th), cap_aff, cap_conn,
                                                cap_ord, cap_link, _p(o["tgt_status"]), _p(o["tgt_parent"]), _p(o["aff_kf"]), _p(o["conn_off"]), _p(o["conn_kf"]),
                                                _p(o["conn_w"]), _p(o["ord_off"]), _p(o["ord_kf"]), _p(o["ord_w"]), _p(o.get("link_off")), _p(o.get("link_kf")),
                                                _p(o["counts"]), _p(o["status"]), _p(ws), _lib.stream()),
               "orbl_update_connections_device")
    r = dict(o)
    r.setdefault("link_off", None); r.setdefault("link_kf", None)
    r["_workspace"] = ws                                         # (kept alive until the caller synchronises)
    return r


BF_OFFSETS, BF_INDEX, BF_TARGET, BF_ROW, BF_CAP_ORD, BF_CAP_CHILD = 1, 2, 4, 8, 16, 32      # *d_status bits of orbl_set_bad_keyframes_device

_BF_KF = (("kf_bad", np.uint8), ("kf_parent", np.int32), ("kf_rank", np.int32), ("kf_Tcw", np.float64), ("child_off", np.int32), ("child_kf", np.int32),
          ("conn_off", np.int32), ("conn_kf", np.int32), ("conn_w", np.int32), ("ord_off", np.int32), ("ord_kf", np.int32), ("ord_w", np.int32))
_BF_PT = (("kf_slot_off", np.int32), ("kf_slot_pt", np.int32), ("pt_bad", np.uint8), ("pt_nobs", np.int32), ("pt_ref_kf", np.int32), ("obs_off", np.int32),
          ("obs_kf", np.int32), ("obs_slot", np.int32))
_BF_INOUT = ("kf_bad", "kf_parent", "kf_slot_pt", "pt_bad", "pt_nobs", "pt_ref_kf")
_BF_OUT = ("tgt_status", "tgt_Tcp", "oconn_off", "oconn_kf", "oconn_w", "oord_off", "oord_kf", "oord_w", "ochild_off", "ochild_kf", "counts")


class BadFlagResult:
    """What orbl_set_bad_keyframes reports: tgt_status[ntgt], tgt_Tcp[ntgt][12]; the tables it changed in place kf_bad, kf_parent and -
    with the point set - kf_slot_pt, pt_bad, pt_nobs, pt_ref_kf, obs_erased; the whole new tables oconn_*, oord_*, ochild_* (the host form
    trims them to the written counts, the device form returns them at full capacity); counts[6] = {n_bad, n_conn_out, n_ord_out,
    n_child_out, n_adopted, n_fallback}; rc; status: the device form's d_status tensor (None in the host form)."""
    __slots__ = _BF_OUT + _BF_INOUT + ("obs_erased", "rc", "status", "_workspace")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _bf_default_caps(nkf, nchild, nconn, nord, ntgt):
    """capacities no call can exceed: a list is copied or becomes what is left of its row; every turn adds at most one row entry per child
    of its target"""
    return nconn + nord, nchild + ntgt * nkf


def set_bad_keyframes(tgt_kf, tables, tgt_flags=None, tgt_mask=None, caps=None, out=None, check=True):
    """KeyFrame::SetBadFlag on the keyframes tgt_kf, one after the other, in one call (orbl_set_bad_keyframes; include/orbslam_hip.h states
    the inputs and the semantics).  tables: a dict with kf_bad, kf_parent, kf_rank (may be None), kf_Tcw, child_off / child_kf, conn_off /
    conn_kf / conn_w, ord_off / ord_kf / ord_w and - all of them or none - kf_slot_off, kf_slot_pt, pt_bad, pt_nobs, pt_ref_kf, obs_off,
    obs_kf, obs_slot.  The in/out tables are COPIED: the changed ones come back in the result, the caller's arrays stay.  caps = (cap_ord,
    cap_child), default: bounds no call exceeds.  out: optional dict of preset output arrays of those capacities.  Returns a BadFlagResult;
    check=False returns rc = ORBHIP_ECAP with counts and the (then unchanged) copies of the in/out tables instead of raising."""
    L = _lib.load()
    tk = _c(tgt_kf, np.int32).reshape(-1); ntgt = len(tk)
    tf = _c(tgt_flags, np.uint8).reshape(-1) if tgt_flags is not None else None
    tm = _c(tgt_mask, np.uint8).reshape(-1) if tgt_mask is not None else None
    assert (tf is None or len(tf) == ntgt) and (tm is None or len(tm) == ntgt)
    points = tables.get("kf_slot_off") is not None
    a = {}
    for k, dt in _BF_KF + (_BF_PT if points else ()):
        v = tables.get(k)
        a[k] = None if v is None else (np.array(v, dt).reshape(-1) if k in _BF_INOUT else _c(v, dt).reshape(-1))
    nkf = len(a["kf_bad"])
    assert len(a["kf_parent"]) == nkf and len(a["kf_Tcw"]) == 12 * nkf and (a["kf_rank"] is None or len(a["kf_rank"]) == nkf)
    for off, ent in (("child_off", ("child_kf",)), ("conn_off", ("conn_kf", "conn_w")), ("ord_off", ("ord_kf", "ord_w"))):
        assert len(a[off]) == nkf + 1 and all(len(a[e]) >= a[off][-1] for e in ent), off      # (the library checks the rest)
    npts = 0
    if points:
        npts = len(a["obs_off"]) - 1
        assert len(a["kf_slot_off"]) == nkf + 1 and len(a["kf_slot_pt"]) >= a["kf_slot_off"][-1] and npts >= 0
        assert len(a["pt_bad"]) == npts and len(a["pt_nobs"]) == npts and len(a["pt_ref_kf"]) == npts
        assert len(a["obs_kf"]) >= a["obs_off"][-1] and len(a["obs_slot"]) == len(a["obs_kf"])
        a["obs_erased"] = np.zeros(len(a["obs_kf"]), np.uint8)
    nconn = len(a["conn_kf"])
    cap_ord, cap_child = _bf_default_caps(nkf, len(a["child_kf"]), nconn, len(a["ord_kf"]), ntgt) if caps is None else caps
    o = dict(tgt_status=np.zeros(ntgt, np.int32), tgt_Tcp=np.zeros((ntgt, 12), np.float64), oconn_off=np.zeros(nkf + 1, np.int32), oconn_kf=np.zeros(nconn, np.int32),
             oconn_w=np.zeros(nconn, np.int32), oord_off=np.zeros(nkf + 1, np.int32), oord_kf=np.zeros(cap_ord, np.int32), oord_w=np.zeros(cap_ord, np.int32),
             ochild_off=np.zeros(nkf + 1, np.int32), ochild_kf=np.zeros(cap_child, np.int32), counts=np.zeros(6, np.int32))
    for k, v in ({} if out is None else out).items():
        assert v.dtype == o[k].dtype and v.flags.c_contiguous and v.size == o[k].size, k
        o[k] = v
    rc = L.orbl_set_bad_keyframes(ntgt, _p(tk), _p(tf), _p(tm), nkf, *[_p(a[k]) for k, _ in _BF_KF], npts, *[_p(a.get(k)) for k, _ in _BF_PT],
                                  _p(a.get("obs_erased")), int(cap_ord), int(cap_child), *[_p(o[k]) for k in _BF_OUT])
    if rc == ECAP and not check:
        return BadFlagResult(rc=rc, counts=o["counts"], obs_erased=a.get("obs_erased"), **{k: a.get(k) for k in _BF_INOUT})
    _lib.check(rc, "orbl_set_bad_keyframes")
    _, n_conn, n_ord, n_child = (int(v) for v in o["counts"][:4])
    o.update(oconn_kf=o["oconn_kf"][:n_conn], oconn_w=o["oconn_w"][:n_conn], oord_kf=o["oord_kf"][:n_ord], oord_w=o["oord_w"][:n_ord], ochild_kf=o["ochild_kf"][:n_child])
    return BadFlagResult(rc=0, obs_erased=a.get("obs_erased"), **{k: a.get(k) for k in _BF_INOUT}, **o)


def set_bad_keyframes_device(tgt_kf, tables, tgt_flags=None, tgt_mask=None, caps=None, out=None, workspace=None):
    """orbl_set_bad_keyframes_device on torch CUDA tensors (dtypes as in set_bad_keyframes; None where a pointer may be NULL), enqueued on
    the current stream, nothing synchronised.  The in/out tables of `tables` are changed IN PLACE.  tgt_mask may be the d_culled tensor
    of keyframe_culling_device.  out: optional dict of preset device tensors of the capacities (and obs_erased); workspace: optional
    uint8 tensor to reuse (it is cleared by every call).  Returns a BadFlagResult of device tensors of FULL capacity - counts[6] holds
    the wanted sizes, status (uint32 as int32[1]) the BF_* bits."""
    import torch
    L = _lib.load()
    dev = tgt_kf.device
    points = tables.get("kf_slot_off") is not None
    a = {k: tables.get(k) for k, _ in _BF_KF + _BF_PT}
    ntgt, nkf = tgt_kf.numel(), a["kf_bad"].numel()
    nchild, nconn, nord = a["child_kf"].numel(), a["conn_kf"].numel(), a["ord_kf"].numel()
    npts, nslots, nobs = (a["obs_off"].numel() - 1, a["kf_slot_pt"].numel(), a["obs_kf"].numel()) if points else (0, 0, 0)
    cap_ord, cap_child = _bf_default_caps(nkf, nchild, nconn, nord, ntgt) if caps is None else caps
    ws = _lib.workspace("orbl_set_bad_keyframes_workspace", ntgt, nkf, nchild, nconn, nobs, device=dev, reuse=workspace)
    o = {} if out is None else out
    sizes = dict(tgt_status=ntgt, oconn_off=nkf + 1, oconn_kf=nconn, oconn_w=nconn, oord_off=nkf + 1, oord_kf=cap_ord, oord_w=cap_ord, ochild_off=nkf + 1,
                 ochild_kf=cap_child, counts=6, status=1)
    for k, n in sizes.items():
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
        assert o[k].dtype == torch.int32 and o[k].is_contiguous() and o[k].numel() == n, k
    if o.get("tgt_Tcp") is None:
        o["tgt_Tcp"] = torch.empty((max(ntgt, 1), 12), dtype=torch.float64, device=dev)[:ntgt]
    if points and o.get("obs_erased") is None:
        o["obs_erased"] = torch.empty(max(nobs, 1), dtype=torch.uint8, device=dev)[:nobs]
    _lib.check(L.orbl_set_bad_keyframes_device(ntgt, _p(tgt_kf), _p(tgt_flags), _p(tgt_mask), nkf, _p(a["kf_bad"]), _p(a["kf_parent"]), _p(a["kf_rank"]), _p(a["kf_Tcw"]),
                                               nchild, _p(a["child_off"]), _p(a["child_kf"]), nconn, _p(a["conn_off"]), _p(a["conn_kf"]), _p(a["conn_w"]), nord,
                                               _p(a["ord_off"]), _p(a["ord_kf"]), _p(a["ord_w"]), npts, nslots, _p(a["kf_slot_off"]), _p(a["kf_slot_pt"]), _p(a["pt_bad"]),
                                               _p(a["pt_nobs"]), _p(a["pt_ref_kf"]), nobs, _p(a["obs_off"]), _p(a["obs_kf"]), _p(a["obs_slot"]), _p(o.get("obs_erased")),
                                               int(cap_ord), int(cap_child), *[_p(o[k]) for k in _BF_OUT], _p(o["status"]), _p(ws),
                                               _lib.stream()), "orbl_set_bad_keyframes_device")
    return BadFlagResult(rc=0, status=o["status"], obs_erased=o.get("obs_erased"), _workspace=ws, **{k: a.get(k) for k in _BF_INOUT}, **{k: o[k] for k in _BF_OUT})


# op_kind values of orbl_apply_map_edits and the *d_status bits of orbl_apply_map_edits_device
ME_NOP, ME_ADD, ME_REPLACE, ME_SET_BAD, ME_FUSE, ME_FIND_OR_ADD, ME_REPLACE_FOUND = range(7)
ME_OFFSETS, ME_KF, ME_PT, ME_SLOT, ME_CAP = 1, 2, 4, 8, 16

_ME_OPS = ("op_kind", "op_pt", "op_arg", "op_kf", "op_slot")
_ME_IN = (("kf_slot_off", np.int32), ("kf_rank", np.int32), ("kf_slot_pt", np.int32), ("kf_slot_level", np.int32), ("kf_slot_uv", np.float32), ("pt_bad", np.uint8),
          ("pt_nobs", np.int32), ("pt_found", np.int32), ("pt_visible", np.int32), ("pt_replaced", np.int32), ("obs_off", np.int32), ("obs_kf", np.int32),
          ("obs_slot", np.int32), ("obs_dead", np.uint8))
_ME_INOUT = ("kf_slot_pt", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced")
_ME_OUT = (("op_status", np.int32), ("op_found", np.int32), ("pt_touched", np.uint8), ("oobs_off", np.int32), ("oobs_kf", np.int32), ("oobs_slot", np.int32),
           ("oobs_src", np.int32), ("oobs_level", np.int32), ("oobs_uv", np.float32), ("counts", np.int32))


class MapEditResult:
    """What orbl_apply_map_edits reports: op_status[nops], op_found[nops], pt_touched[npts]; the tables it changed in place kf_slot_pt,
    pt_bad, pt_nobs and - when given - pt_found, pt_visible, pt_replaced; the whole new observation tables oobs_off[npts + 1], oobs_kf,
    oobs_slot, oobs_src and - with the kf_slot_level pair - oobs_level, oobs_uv (the host form trims them to counts[0], the device form
    returns them at full capacity); counts[8] = {n_obs_out, n_obs_added, n_replace, n_set_bad, n_fused, n_touched, n_late_adds, 0}; rc;
    status: the device form's d_status tensor (None in the host form)."""
    __slots__ = tuple(k for k, _ in _ME_OUT) + _ME_INOUT + ("rc", "status", "_workspace")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _me_sizes(nops, npts, cap_obs, attrs):
    return dict(op_status=nops, op_found=nops, pt_touched=npts, oobs_off=npts + 1, oobs_kf=cap_obs, oobs_slot=cap_obs, oobs_src=cap_obs,
                oobs_level=cap_obs if attrs else None, oobs_uv=2 * cap_obs if attrs else None, counts=8)


def apply_map_edits(ops, tables, cap_obs=None, out=None, check=True):
    """An ordered list of map-point edits - AddObservation, Replace, SetBadFlag, both Fuse forms - replayed on the map tables in one call,
    which returns the whole new observation tables (orbl_apply_map_edits; include/orbslam_hip.h states the kinds and the semantics).
    ops: a dict with op_kind, op_pt, op_arg, op_kf, op_slot (equal lengths; empty lists = the pure rebuild).  tables: a dict with
    kf_slot_off, kf_rank (may be None), kf_slot_pt, pt_bad, pt_nobs, obs_off, obs_kf, obs_slot and - each may be None or missing -
    obs_dead, the pair kf_slot_level / kf_slot_uv, the pair pt_found / pt_visible, pt_replaced.  The in/out tables are COPIED: the
    changed ones come back in the result, the caller's arrays stay.  cap_obs: default nobs + nops, which no call exceeds.  out: optional
    dict of preset output arrays of that capacity.  Returns a MapEditResult; check=False returns rc = ORBHIP_ECAP with counts and the
    (then unchanged) copies of the in/out tables instead of raising."""
    L = _lib.load()
    op = [_c(ops[k], np.int32).reshape(-1) for k in _ME_OPS]
    nops = len(op[0])
    assert all(len(v) == nops for v in op)
    a = {}
    for k, dt in _ME_IN:
        v = tables.get(k)
        a[k] = None if v is None else (np.array(v, dt).reshape(-1) if k in _ME_INOUT else _c(v, dt).reshape(-1))
    nkf, npts, nobs = len(a["kf_slot_off"]) - 1, len(a["obs_off"]) - 1, len(a["obs_kf"])
    assert nkf >= 0 and npts >= 0 and len(a["obs_slot"]) == nobs and len(a["pt_bad"]) == npts and len(a["pt_nobs"]) == npts     # (the library checks the rest)
    assert len(a["kf_slot_pt"]) >= a["kf_slot_off"][-1] and nobs >= a["obs_off"][-1] and (a["kf_rank"] is None or len(a["kf_rank"]) == nkf)
    for k in ("pt_found", "pt_visible", "pt_replaced"):
        assert a[k] is None or len(a[k]) == npts, k
    assert a["obs_dead"] is None or len(a["obs_dead"]) == nobs
    attrs = a["kf_slot_level"] is not None
    assert not attrs or (a["kf_slot_uv"] is not None and len(a["kf_slot_level"]) == len(a["kf_slot_pt"]) and len(a["kf_slot_uv"]) == 2 * len(a["kf_slot_pt"]))
    cap_obs = nobs + nops if cap_obs is None else int(cap_obs)
    sizes = _me_sizes(nops, npts, cap_obs, attrs)
    o = {k: None if sizes[k] is None else np.zeros(sizes[k], dt) for k, dt in _ME_OUT}
    for k, v in ({} if out is None else out).items():
        assert k in o and o[k] is not None, "out[%r]: no such output (oobs_level / oobs_uv need the kf_slot_level pair)" % k
        assert v.dtype == o[k].dtype and v.flags.c_contiguous and v.size == o[k].size, k
        o[k] = v
    rc = L.orbl_apply_map_edits(nops, *[_p(v) for v in op], nkf, *[_p(a[k]) for k in ("kf_slot_off", "kf_rank", "kf_slot_pt", "kf_slot_level", "kf_slot_uv")],
                                npts, *[_p(a[k]) for k in ("pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced", "obs_off", "obs_kf", "obs_slot", "obs_dead")],
                                cap_obs, *[_p(o[k]) for k, _ in _ME_OUT])
    if rc == ECAP and not check:
        return MapEditResult(rc=rc, counts=o["counts"], **{k: a[k] for k in _ME_INOUT})
    _lib.check(rc, "orbl_apply_map_edits")
    n = int(o["counts"][0])
    o.update(oobs_kf=o["oobs_kf"][:n], oobs_slot=o["oobs_slot"][:n], oobs_src=o["oobs_src"][:n])
    if attrs:
        o.update(oobs_level=o["oobs_level"][:n], oobs_uv=o["oobs_uv"].reshape(-1, 2)[:n])
    return MapEditResult(rc=0, **{k: a[k] for k in _ME_INOUT}, **o)


def apply_map_edits_device(ops, tables, cap_obs=None, out=None, workspace=None):
    """orbl_apply_map_edits_device on torch CUDA tensors (dtypes as in apply_map_edits; None where a pointer may be NULL), enqueued on the
    current stream, nothing synchronised.  The in/out tables of `tables` are changed IN PLACE.  obs_dead may be the obs_erased tensor of
    set_bad_keyframes_device, keyframe_culling_device or local_ba_apply_device.  out: optional dict of preset device tensors of the
    capacity - the dict is FILLED IN with the tensors the call creates, so passing the same dict again reuses them; workspace: optional
    uint8 tensor to reuse (it is cleared by every call).  Returns a MapEditResult of device tensors of FULL
    capacity - counts[8] holds the wanted sizes, status (uint32 as int32[1]) the ME_* bits."""
    import torch
    L = _lib.load()
    op = [ops[k] for k in _ME_OPS]
    a = {k: tables.get(k) for k, _ in _ME_IN}
    dev = a["obs_off"].device
    nops, nkf, npts = op[0].numel(), a["kf_slot_off"].numel() - 1, a["obs_off"].numel() - 1
    nslots, nobs = a["kf_slot_pt"].numel(), a["obs_kf"].numel()
    attrs = a["kf_slot_level"] is not None
    cap_obs = nobs + nops if cap_obs is None else int(cap_obs)
    ws = _lib.workspace("orbl_apply_map_edits_workspace", nops, nkf, npts, nslots, nobs, device=dev, reuse=workspace)
    o = {} if out is None else out
    sizes = dict(_me_sizes(nops, npts, cap_obs, attrs), status=1)
    tdt = {np.int32: torch.int32, np.uint8: torch.uint8, np.float32: torch.float32}
    for k, dt in _ME_OUT + (("status", np.int32),):
        n = sizes[k]
        if n is None:
            assert o.get(k) is None, "out[%r] needs the kf_slot_level pair" % k
            o[k] = None
            continue
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 1), dtype=tdt[dt], device=dev)[:n]
        assert o[k].dtype == tdt[dt] and o[k].is_contiguous() and o[k].numel() == n, k
    _lib.check(L.orbl_apply_map_edits_device(nops, *[_p(v) for v in op], nkf, _p(a["kf_slot_off"]), _p(a["kf_rank"]), nslots, _p(a["kf_slot_pt"]), _p(a["kf_slot_level"]),
                                             _p(a["kf_slot_uv"]), npts, _p(a["pt_bad"]), _p(a["pt_nobs"]), _p(a["pt_found"]), _p(a["pt_visible"]), _p(a["pt_replaced"]), nobs,
                                             _p(a["obs_off"]), _p(a["obs_kf"]), _p(a["obs_slot"]), _p(a["obs_dead"]), cap_obs, *[_p(o[k]) for k, _ in _ME_OUT], _p(o["status"]),
                                             _p(ws), _lib.stream()), "orbl_apply_map_edits_device")
    return MapEditResult(rc=0, status=o["status"], _workspace=ws, **{k: a[k] for k in _ME_INOUT}, **{k: o[k] for k, _ in _ME_OUT})


# *d_status bits of orbl_local_ba_assemble_device and orbl_local_ba_apply_device
LA_OFFSETS, LA_KF, LA_PT, LA_RANK, LA_LEVEL, LA_CAP_CAM, LA_CAP_PTS, LA_CAP_OBS, LA_OBS = 1, 2, 4, 8, 16, 32, 64, 128, 256

_LA_IN = (("kf_id", np.int32), ("kf_bad", np.uint8), ("kf_rank", np.int32), ("kf_Tcw", np.float64), ("kf_K4", np.float64), ("kf_slot_off", np.int32),
          ("kf_slot_pt", np.int32), ("X", np.float64), ("pt_bad", np.uint8), ("pt_rank", np.int32), ("obs_off", np.int32), ("obs_kf", np.int32),
          ("obs_uv", np.float32), ("obs_level", np.int32), ("inv_level_sigma2", np.float32))
# (name, dtype, entries per element, which capacity)
_LA_OUT = (("cam_kf", np.int32, 1, 0), ("K4", np.float64, 4, 0), ("poses7", np.float64, 7, 0), ("cam_fixed", np.uint8, 1, 0), ("cam_local", np.uint8, 1, 0),
           ("lpt_pt", np.int32, 1, 1), ("pts3", np.float64, 3, 1), ("lobs_cam", np.int32, 1, 2), ("lobs_pt", np.int32, 1, 2), ("lobs_uv", np.float64, 2, 2),
           ("lobs_inv_sigma2", np.float32, 1, 2), ("lobs_src", np.int32, 1, 2))
_LA_SHAPE = dict(K4=(-1, 4), poses7=(-1, 7), pts3=(-1, 3), lobs_uv=(-1, 2))
_AP_INOUT = (("kf_Tcw", np.float64), ("kf_center", np.float64), ("kf_slot_pt", np.int32), ("X", np.float64), ("pt_bad", np.uint8), ("pt_nobs", np.int32),
             ("pt_ref_kf", np.int32))
_AP_IN = (("kf_slot_off", np.int32), ("obs_off", np.int32), ("obs_kf", np.int32), ("obs_slot", np.int32), ("obs_level", np.int32), ("kf_level0", np.int32),
          ("scale_factors", np.float32))


def local_ba_assemble(cur_kf, nbr_kf, tab, caps=None, out=None, check=True, device=False, **kw):
    """The problem of CeresOptimizer::LocalBundleAdjustment from the map tables (orbl_local_ba_assemble; include/orbslam_hip.h states the
    inputs and the semantics).  tab: dict of the tables kf_id, kf_bad, kf_rank, kf_Tcw [nkf, 12], kf_K4 [nkf, 4], kf_slot_off, kf_slot_pt,
    X [npts, 3], pt_bad, pt_rank, obs_off, obs_kf, obs_uv [nobs, 2], obs_level, inv_level_sigma2 (kf_bad, kf_rank, pt_bad, pt_rank may be
    None or missing).  caps = (cap_cam, cap_pts, cap_obs), default (nkf, npts, nobs): bounds no call exceeds.  out: optional dict of preset
    output arrays of those capacities.  Returns a dict trimmed to the written counts: cam_kf, K4 [ncam, 4], poses7 [ncam, 7], cam_fixed,
    cam_local, lpt_pt, pts3, lobs_cam, lobs_pt, lobs_uv, lobs_inv_sigma2, lobs_src, kf_role [nkf], pt_local [npts], counts = {ncam,
    n_local_cam, npts_local, nobs_local} and rc; check=False returns rc = ORBHIP_ECAP with only counts filled instead of raising.
    device=True: local_ba_assemble_device on torch CUDA tensors."""
    if device:
        return local_ba_assemble_device(cur_kf, nbr_kf, tab, caps=caps, out=out, **kw)
    L = _lib.load()
    t = {k: _flat(tab.get(k), dt) for k, dt in _LA_IN}
    nb = _c(nbr_kf, np.int32).reshape(-1)
    nkf, npts, nobs = len(t["kf_id"]), len(t["X"]) // 3, len(t["obs_kf"])
    assert len(t["kf_Tcw"]) == 12 * nkf and len(t["kf_K4"]) == 4 * nkf and len(t["kf_slot_off"]) == nkf + 1 and len(t["obs_off"]) == npts + 1
    assert len(t["obs_uv"]) == 2 * nobs and len(t["obs_level"]) == nobs and nobs >= (t["obs_off"][-1] if npts else 0)
    assert len(t["kf_slot_pt"]) >= (t["kf_slot_off"][-1] if nkf else 0)                      # (the library checks the rest)
    for k, n in (("kf_bad", nkf), ("kf_rank", nkf), ("pt_bad", npts), ("pt_rank", npts)):
        assert t[k] is None or len(t[k]) == n, k
    cap = (nkf, npts, nobs) if caps is None else tuple(int(c) for c in caps)
    o = {} if out is None else out
    for k, dt, w, c in _LA_OUT:
        o.setdefault(k, np.zeros(w * cap[c], dt))
        assert o[k].dtype == dt and o[k].flags.c_contiguous and o[k].size == w * cap[c], k
    o.setdefault("kf_role", np.zeros(nkf, np.uint8)); o.setdefault("pt_local", np.zeros(npts, np.uint8)); o.setdefault("counts", np.zeros(4, np.int32))
    rc = L.orbl_local_ba_assemble(int(cur_kf), len(nb), _pn(nb), nkf, *[_pn(t[k]) for k in ("kf_id", "kf_bad", "kf_rank", "kf_Tcw", "kf_K4")], _p(t["kf_slot_off"]),
                                  _pn(t["kf_slot_pt"]), npts, _pn(t["X"]), _pn(t["pt_bad"]), _pn(t["pt_rank"]), _p(t["obs_off"]), _pn(t["obs_kf"]), _pn(t["obs_uv"]),
                                  _pn(t["obs_level"]), _pn(t["inv_level_sigma2"]), len(t["inv_level_sigma2"]), cap[0], cap[1], cap[2], _p(o["counts"]),
                                  *[_pn(o[k]) for k, _, _, _ in _LA_OUT], _pn(o["kf_role"]), _pn(o["pt_local"]))
    if rc == ECAP and not check:
        return dict(rc=rc, counts=o["counts"])
    _lib.check(rc, "orbl_local_ba_assemble")
    n = (int(o["counts"][0]), int(o["counts"][2]), int(o["counts"][3]))
    r = dict(rc=0, counts=o["counts"], kf_role=o["kf_role"], pt_local=o["pt_local"])
    for k, _, w, c in _LA_OUT:
        r[k] = o[k][:w * n[c]].reshape(_LA_SHAPE.get(k, (-1,)))
    return r


def local_ba_assemble_device(cur_kf, nbr_kf, tab, caps=None, out=None, workspace=None):
    """orbl_local_ba_assemble_device on torch CUDA tensors (dtypes as in local_ba_assemble; None where a pointer may be NULL), enqueued on
    the current stream, nothing synchronised.  Returns a dict of device tensors of FULL capacity - counts[4] holds the wanted sizes,
    status (uint32 as int32[1]) the LA_* bits - with kf_role, pt_local and the workspace under "_workspace"."""
    import torch
    L = _lib.load()
    g = tab.get
    dev = tab["kf_id"].device
    n_nbr = nbr_kf.numel() if nbr_kf is not None else 0
    nkf, npts, nobs, nslots = tab["kf_id"].numel(), tab["X"].numel() // 3, tab["obs_kf"].numel(), tab["kf_slot_pt"].numel()
    cap = (nkf, npts, nobs) if caps is None else tuple(int(c) for c in caps)
    ws = _lib.workspace("orbl_local_ba_assemble_workspace", nkf, npts, device=dev, reuse=workspace)
    o = {} if out is None else dict(out)
    tdt = {np.int32: torch.int32, np.float64: torch.float64, np.float32: torch.float32, np.uint8: torch.uint8}
    sizes = [(k, tdt[dt], w * cap[c]) for k, dt, w, c in _LA_OUT] + [("kf_role", torch.uint8, nkf), ("pt_local", torch.uint8, npts), ("counts", torch.int32, 4),
                                                                     ("status", torch.int32, 1)]
    for k, dt, n in sizes:
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 1), dtype=dt, device=dev)[:n]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == n, k
    _lib.check(L.orbl_local_ba_assemble_device(int(cur_kf), n_nbr, _pn(nbr_kf), nkf, _pn(g("kf_id")), _pn(g("kf_bad")), _pn(g("kf_rank")), _pn(g("kf_Tcw")), _pn(g("kf_K4")), nslots,
                                               _p(tab["kf_slot_off"]), _pn(g("kf_slot_pt")), npts, _pn(g("X")), _pn(g("pt_bad")), _pn(g("pt_rank")), nobs,
                                               _p(tab["obs_off"]), _pn(g("obs_kf")), _pn(g("obs_uv")), _pn(g("obs_level")), _pn(g("inv_level_sigma2")),
                                               tab["inv_level_sigma2"].numel(), cap[0], cap[1], cap[2], _pn(o["counts"]), *[_pn(o[k]) for k, _, _, _ in _LA_OUT],
                                               _pn(o["kf_role"]), _pn(o["pt_local"]), _pn(o["status"]), _pn(ws), _lib.stream()),
               "orbl_local_ba_assemble_device")
    r = dict(o)
    r["_workspace"] = ws                                         # (kept alive until the caller synchronises)
    return r


def local_ba_apply(asm, poses7, pts3, obs_erase, tab, normals=True, out=None, device=False, **kw):
    """The write-back of CeresOptimizer::LocalBundleAdjustment on the map tables (orbl_local_ba_apply; include/orbslam_hip.h states the
    inputs and the semantics).  asm: what local_ba_assemble returned (cam_kf, cam_local, lpt_pt, lobs_src are read); poses7 [ncam, 7],
    pts3 [npts_local, 3], obs_erase [nobs_local] from optimizer.local_bundle_adjustment.  tab: dict of the tables kf_Tcw, kf_center, kf_slot_off,
    kf_slot_pt, X, pt_bad, pt_nobs, pt_ref_kf, obs_off, obs_kf, obs_slot, obs_level, kf_level0 (may be None), scale_factors.  normals=False
    leaves step 4 out.  out: optional dict of preset normal [npts, 3], min_max [npts, 2], nd_written [npts] arrays, of which only the rows of
    points with a new normal are rewritten (nd_written wholly).  Returns a dict: new copies of kf_Tcw, kf_center, kf_slot_pt, X, pt_bad,
    pt_nobs, pt_ref_kf; obs_erased [nobs], normal, min_max, nd_written, counts = {n_erased, n_points_turned_bad, n_observations_dead,
    n_normals_written}.  device=True: local_ba_apply_device on torch CUDA tensors, in place."""
    if device:
        return local_ba_apply_device(asm, poses7, pts3, obs_erase, tab, normals=normals, out=out, **kw)
    L = _lib.load()
    io = {k: (None if tab.get(k) is None else np.array(tab[k], dtype=dt, order="C").reshape(-1)) for k, dt in _AP_INOUT}       # (always copies)
    t = {k: _flat(tab.get(k), dt) for k, dt in _AP_IN}
    ck = _flat(asm["cam_kf"], np.int32); cl = _flat(asm["cam_local"], np.uint8); lp = _flat(asm["lpt_pt"], np.int32); ls = _flat(asm["lobs_src"], np.int32)
    p7 = _flat(poses7, np.float64); p3 = _flat(pts3, np.float64); er = _flat(obs_erase, np.uint8)
    ncam, npl, nol = len(ck), len(lp), len(ls)
    nkf, npts, nobs = len(io["kf_Tcw"]) // 12, len(io["X"]) // 3, len(t["obs_kf"])
    assert len(cl) == ncam and len(p7) == 7 * ncam and len(p3) == 3 * npl and len(er) >= nol
    assert len(t["kf_slot_off"]) == nkf + 1 and len(t["obs_off"]) == npts + 1 and len(t["obs_slot"]) == nobs and nobs >= (t["obs_off"][-1] if npts else 0)
    assert len(io["pt_bad"]) == npts and len(io["pt_nobs"]) == npts and len(io["pt_ref_kf"]) == npts and (io["kf_center"] is None or len(io["kf_center"]) == 3 * nkf)
    assert len(io["kf_slot_pt"]) >= (t["kf_slot_off"][-1] if nkf else 0)
    o = {} if out is None else out
    o["obs_erased"] = np.zeros(nobs, np.uint8); o["counts"] = np.zeros(4, np.int32)
    if normals:
        o.setdefault("normal", np.zeros((npts, 3))); o.setdefault("min_max", np.zeros((npts, 2), np.float32)); o.setdefault("nd_written", np.zeros(npts, np.uint8))
        for k, dt, n in (("normal", np.float64, 3 * npts), ("min_max", np.float32, 2 * npts), ("nd_written", np.uint8, npts)):
            assert o[k].dtype == dt and o[k].flags.c_contiguous and o[k].size == n, k
        assert len(t["obs_level"]) == nobs
    else:
        o.update(normal=None, min_max=None, nd_written=None)
    sf = t["scale_factors"] if normals else None
    _lib.check(L.orbl_local_ba_apply(ncam, _pn(ck), _pn(cl), _pn(p7), npl, _pn(lp), _pn(p3), nol, _pn(ls), _pn(er), nkf, _pn(io["kf_Tcw"]), _pn(io["kf_center"]), _p(t["kf_slot_off"]),
                                     _pn(io["kf_slot_pt"]), npts, _pn(io["X"]), _pn(io["pt_bad"]), _pn(io["pt_nobs"]), _pn(io["pt_ref_kf"]), _p(t["obs_off"]), _pn(t["obs_kf"]),
                                     _pn(t["obs_slot"]), _pn(t["obs_level"]), _pn(t["kf_level0"]), _p(sf), len(sf) if sf is not None else 0, _pn(o["obs_erased"]),
                                     _p(o["normal"]), _p(o["min_max"]), _p(o["nd_written"]), _p(o["counts"])), "orbl_local_ba_apply")
    r = dict(o)
    r.update(io)
    r["kf_Tcw"] = io["kf_Tcw"].reshape(-1, 12); r["X"] = io["X"].reshape(-1, 3)
    if io["kf_center"] is not None:
        r["kf_center"] = io["kf_center"].reshape(-1, 3)
    return r


def local_ba_apply_device(asm, poses7, pts3, obs_erase, tab, normals=True, out=None, n=None, workspace=None):
    """orbl_local_ba_apply_device on torch CUDA tensors, enqueued on the current stream, nothing synchronised.  The tables kf_Tcw,
    kf_center, kf_slot_pt, X, pt_bad, pt_nobs, pt_ref_kf change IN PLACE.  n = (ncam, npts_local, nobs_local) as host integers; default:
    read from asm["counts"], which waits for the stream.  Returns a dict of device tensors: those tables, obs_erased, normal, min_max,
    nd_written, counts[4], status (the LA_* bits), and the workspace under "_workspace"."""
    import torch
    L = _lib.load()
    g = tab.get
    dev = tab["kf_Tcw"].device
    if n is None:
        c = asm["counts"].cpu().tolist()
        n = (c[0], c[2], c[3])
    ncam, npl, nol = (int(v) for v in n)
    nkf, npts, nobs, nslots = tab["kf_Tcw"].numel() // 12, tab["X"].numel() // 3, tab["obs_kf"].numel(), tab["kf_slot_pt"].numel()
    ws = _lib.workspace("orbl_local_ba_apply_workspace", nobs, device=dev, reuse=workspace)
    o = {} if out is None else dict(out)
    sizes = [("obs_erased", torch.uint8, nobs), ("counts", torch.int32, 4), ("status", torch.int32, 1)]
    if normals:
        sizes += [("normal", torch.float64, 3 * npts), ("min_max", torch.float32, 2 * npts), ("nd_written", torch.uint8, npts)]
    for k, dt, m in sizes:
        if o.get(k) is None:
            o[k] = torch.empty(max(m, 1), dtype=dt, device=dev)[:m]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == m, k
    for k, _ in _AP_INOUT:
        assert g(k) is None or g(k).is_contiguous(), k
    sf = g("scale_factors") if normals else None
    _lib.check(L.orbl_local_ba_apply_device(ncam, _pn(asm["cam_kf"]), _pn(asm["cam_local"]), _pn(poses7), npl, _pn(asm["lpt_pt"]), _pn(pts3), nol, _pn(asm["lobs_src"]), _pn(obs_erase),
                                            nkf, _pn(g("kf_Tcw")), _pn(g("kf_center")), nslots, _p(tab["kf_slot_off"]), _pn(g("kf_slot_pt")), npts, _pn(g("X")),
                                            _pn(g("pt_bad")), _pn(g("pt_nobs")), _pn(g("pt_ref_kf")), nobs, _p(tab["obs_off"]), _pn(g("obs_kf")), _pn(g("obs_slot")),
                                            _pn(g("obs_level")), _pn(g("kf_level0")), _p(sf), sf.numel() if sf is not None else 0,
                                            _pn(o["obs_erased"]), *[_p(o.get(k)) for k in ("normal", "min_max", "nd_written")],
                                            _pn(o["counts"]), _pn(o["status"]), _pn(ws), _lib.stream()), "orbl_local_ba_apply_device")
    r = dict(o)
    for k in ("normal", "min_max", "nd_written"):
        r.setdefault(k, None)
    r.update({k: g(k) for k, _ in _AP_INOUT})
    r["_workspace"] = ws                                         # (kept alive until the caller synchronises)
    return r


def local_bundle_adjustment_on_tables(cur_kf, nbr_kf, tab, stop_flag=None, normals=True, device=False, out=None):
    """CeresOptimizer::LocalBundleAdjustment on the map tables: local_ba_assemble, optimizer.local_bundle_adjustment on the compact problem
    (its structure pass is host code: the problem crosses to the host between the two calls), local_ba_apply - which is skipped when the
    stop flag aborted the solve (src/CeresOptimizer.cc:509-512), so that the tables stay as they are.  tab holds the tables of both calls.
    Returns dict(aborted, assembled, solved = (poses7, pts3, obs_erase) or None, applied = what local_ba_apply returned or None,
    summaries)."""
    from . import optimizer
    asm = local_ba_assemble(cur_kf, nbr_kf, tab, device=device)
    if device:
        c = asm["counts"].cpu().tolist()                         # (waits for the stream: the solver's structure pass reads the problem on the host)
        n = (c[0], c[2], c[3])
        w = dict(K4=4, poses7=7, cam_fixed=1, cam_local=1, pts3=3, lobs_cam=1, lobs_pt=1, lobs_uv=2, lobs_inv_sigma2=1)
        cap = dict(K4=0, poses7=0, cam_fixed=0, cam_local=0, pts3=1, lobs_cam=2, lobs_pt=2, lobs_uv=2, lobs_inv_sigma2=2)
        h = {k: asm[k][:w[k] * n[cap[k]]].cpu().numpy() for k in w}
    else:
        h = asm
    if stop_flag is not None and stop_flag.reshape(-1)[0]:       # (:509-512)
        return dict(aborted=1, assembled=asm, solved=None, applied=None, summaries=None)
    aborted, poses7, pts3, erase, s1, s2 = optimizer.local_bundle_adjustment(h["K4"], np.asarray(h["poses7"]).reshape(-1, 7), h["cam_fixed"], h["cam_local"], h["pts3"],
                                                                             h["lobs_cam"], h["lobs_pt"], h["lobs_uv"], h["lobs_inv_sigma2"], stop_flag=stop_flag)
    if aborted:
        return dict(aborted=aborted, assembled=asm, solved=(poses7, pts3, erase), applied=None, summaries=(s1, s2))
    if device:
        import torch
        dev = tab["kf_Tcw"].device
        up = [torch.as_tensor(np.ascontiguousarray(v)).to(dev) for v in (poses7, pts3, erase)]
        applied = local_ba_apply_device(asm, up[0], up[1], up[2], tab, normals=normals, out=out, n=n)
        applied["_uploads"] = up
    else:
        applied = local_ba_apply(asm, poses7, pts3, erase, tab, normals=normals, out=out)
    return dict(aborted=0, assembled=asm, solved=(poses7, pts3, erase), applied=applied, summaries=(s1, s2))


# ---- LocalMapping::SearchInNeighbors on the resident tables (include/orbslam_hip.h: orbl_fuse_targets*, orbl_fuse_rows*, orbl_fuse_candidates*,
# orbl_update_map_points_on_tables*)
SN_OFFSETS, SN_KF, SN_PT, SN_LEVEL, SN_CAP, SN_SLOT = 1, 2, 4, 8, 16, 32         # *d_status bits of the device forms
LOG_SCALE_FACTOR = 0.18232159316539764                                          # log_scale_factor_ = logf(1.2f), the float 0x1.756506p-3 (numpy's log is one ulp off)

_SN_TAB = (("kf_bad", np.uint8), ("kf_rank", np.int32), ("kf_Tcw", np.float64), ("kf_center", np.float64), ("kf_K4", np.float32), ("kf_bounds", np.float32),
           ("kf_slot_off", np.int32), ("kf_slot_pt", np.int32), ("kf_slot_uv", np.float32), ("kf_slot_level", np.int32), ("kf_slot_desc", np.uint8), ("X", np.float64),
           ("pt_normal", np.float64), ("pt_min_dist", np.float32), ("pt_max_dist", np.float32), ("pt_desc", np.uint8), ("pt_bad", np.uint8), ("pt_nobs", np.int32),
           ("pt_found", np.int32), ("pt_visible", np.int32), ("pt_replaced", np.int32), ("pt_ref_kf", np.int32), ("obs_off", np.int32), ("obs_kf", np.int32),
           ("obs_slot", np.int32), ("ord_off", np.int32), ("ord_kf", np.int32), ("conn_off", np.int32), ("conn_kf", np.int32), ("conn_w", np.int32),
           ("kf_fuse_target", np.int32), ("pt_fuse_cand", np.int32), ("scale_factors", np.float32), ("inv_level_sigma2", np.float32))
_SN_ROWS = ("op_kind", "op_pt", "op_arg", "op_kf", "op_slot", "best_idx", "best_dist", "q_uv", "q_level")


def _sn_host(tab, keys):
    dt = dict(_SN_TAB)
    return {k: (None if tab.get(k) is None else _c(tab[k], dt[k]).reshape(-1)) for k in keys}


def _sn_dev_out(o, sizes, dev):
    import torch
    tdt = {np.int32: torch.int32, np.uint8: torch.uint8, np.float32: torch.float32}
    for k, dt, n in sizes:
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 1), dtype=tdt[dt], device=dev)[:n]
        assert o[k].dtype == tdt[dt] and o[k].is_contiguous() and o[k].numel() == n, k
    return o


def fuse_targets(cur_kf, cur_id, tab, nn=20, nn2=5, cap_tgt=None, device=False, out=None):
    """The target keyframes of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:400-431; orbl_fuse_targets, include/orbslam_hip.h states
    the semantics).  tab: kf_bad (may be None), ord_off, ord_kf, kf_fuse_target.  cap_tgt: default nn (1 + nn2), which no call exceeds.
    Host form: returns dict(tgt_kf trimmed, counts[2], kf_fuse_target = a new copy of the stamps).  device=True: torch CUDA tensors, the
    stamps change IN PLACE, enqueued on the current stream, nothing synchronised; tgt_kf comes at full capacity with counts and status."""
    L = _lib.load()
    cap = nn * (1 + nn2) if cap_tgt is None else int(cap_tgt)
    if device:
        dev = tab["ord_off"].device
        o = _sn_dev_out({} if out is None else out, (("tgt_kf", np.int32, cap), ("counts", np.int32, 2), ("status", np.int32, 1)), dev)
        _lib.check(L.orbl_fuse_targets_device(int(cur_kf), int(cur_id), tab["ord_off"].numel() - 1, _pn(tab.get("kf_bad")), tab["ord_kf"].numel(),
                                              _p(tab["ord_off"]), _pn(tab["ord_kf"]), _p(tab["kf_fuse_target"]), int(nn), int(nn2),
                                              cap, _pn(o["tgt_kf"]), _pn(o["counts"]), _pn(o["status"]), None, _lib.stream()), "orbl_fuse_targets_device")
        return dict(o, kf_fuse_target=tab["kf_fuse_target"])
    t = _sn_host(tab, ("kf_bad", "ord_off", "ord_kf"))
    stamp = np.array(tab["kf_fuse_target"], np.int32).reshape(-1)
    tgt, counts = np.zeros(max(cap, 1), np.int32), np.zeros(2, np.int32)
    _lib.check(L.orbl_fuse_targets(int(cur_kf), int(cur_id), len(t["ord_off"]) - 1, _pn(t["kf_bad"]), _p(t["ord_off"]), _pn(t["ord_kf"]), _p(stamp), int(nn),
                                   int(nn2), cap, _p(tgt) if cap else None, _p(counts)), "orbl_fuse_targets")
    return dict(tgt_kf=tgt[:counts[0]], counts=counts, kf_fuse_target=stamp)


_SN_ROW_KF = ("kf_Tcw", "kf_center", "kf_K4", "kf_bounds", "kf_slot_off")
_SN_ROW_SLOT = ("kf_slot_uv", "kf_slot_level", "kf_slot_desc")
_SN_ROW_PT = ("X", "pt_normal", "pt_min_dist", "pt_max_dist", "pt_desc", "scale_factors", "inv_level_sigma2")


def fuse_rows(kf, pts, tab, th=3.0, log_scale_factor=None, device=False, out=None, extras=True):
    """The search of ORBmatcher::Fuse(pKF, vpMapPoints, th) for one keyframe and a list of points, as edit rows for apply_map_edits
    (orbl_fuse_rows; include/orbslam_hip.h states the arithmetic and the row layout).  pts[n], -1 = null.  tab: kf_Tcw [nkf, 12], kf_center
    [nkf, 3], kf_K4 [nkf, 4] and kf_bounds [nkf, 4] (float32), kf_slot_off, kf_slot_uv [nslots, 2], kf_slot_level, kf_slot_desc [nslots, 32],
    X [npts, 3], pt_normal, pt_min_dist, pt_max_dist, pt_desc [npts, 32], scale_factors, inv_level_sigma2.  extras=False leaves best_idx,
    best_dist, q_uv, q_level out.  Host form: kf an integer; returns a dict of arrays.  device=True: kf a device int32 tensor holding the
    index (a view of a target list will do), everything a torch CUDA tensor, enqueued on the current stream, nothing synchronised."""
    L = _lib.load()
    lsf = LOG_SCALE_FACTOR if log_scale_factor is None else float(log_scale_factor)
    names = _SN_ROWS if extras else _SN_ROWS[:5]
    if device:
        n, dev = pts.numel(), pts.device
        o = _sn_dev_out({} if out is None else out, [(k, np.float32 if k == "q_uv" else np.int32, 2 * n if k == "q_uv" else n) for k in names] + [("status", np.int32, 1)],
                        dev)
        assert tab["kf_K4"].element_size() == 4 and tab["kf_bounds"].element_size() == 4, "kf_K4 and kf_bounds are float32 tables"
        _lib.check(L.orbl_fuse_rows_device(_p(kf), n, _pn(pts), tab["kf_slot_off"].numel() - 1, *[_pn(tab[k]) for k in _SN_ROW_KF[:4]],
                                           _p(tab["kf_slot_off"]), tab["kf_slot_level"].numel(), *[_pn(tab[k]) for k in _SN_ROW_SLOT],
                                           tab["pt_max_dist"].numel(), *[_pn(tab[k]) for k in _SN_ROW_PT], lsf, tab["scale_factors"].numel(), float(th),
                                           *[_pn(o.get(k)) for k in _SN_ROWS], _pn(o["status"]), None, _lib.stream()), "orbl_fuse_rows_device")
        return o
    t = _sn_host(tab, _SN_ROW_KF + _SN_ROW_SLOT + _SN_ROW_PT)
    pl = _c(pts, np.int32).reshape(-1)
    n = len(pl)
    o = {k: np.zeros(2 * n if k == "q_uv" else n, np.float32 if k == "q_uv" else np.int32) for k in names}
    _lib.check(L.orbl_fuse_rows(int(kf), n, _pn(pl), len(t["kf_slot_off"]) - 1, *[_pn(t[k]) for k in _SN_ROW_KF[:4]], _p(t["kf_slot_off"]),
                                *[_pn(t[k]) for k in _SN_ROW_SLOT], len(t["pt_max_dist"]), *[_pn(t[k]) for k in _SN_ROW_PT], lsf, len(t["scale_factors"]), float(th),
                                *[_pn(o.get(k)) for k in _SN_ROWS]), "orbl_fuse_rows")
    if extras:
        o["q_uv"] = o["q_uv"].reshape(-1, 2)
    return o


def fuse_candidates(tgt_kf, cur_id, tab, cap_cand=None, device=False, out=None, workspace=None):
    """The candidates of SearchInNeighbors' second direction (src/LocalMapping.cc:445-470; orbl_fuse_candidates): the first occurrence of
    every point of the listed targets that is not null, not bad and not stamped cur_id, in the reference's order.  tab: kf_slot_off,
    kf_slot_pt, pt_bad, pt_fuse_cand.  cap_cand: default npts, which no call exceeds.  Host form: returns dict(cand_pt trimmed, counts[2],
    pt_fuse_cand = a new copy of the stamps).  device=True: torch CUDA tensors (tgt_kf trimmed to the targets: its count is a host
    integer), the stamps change IN PLACE, enqueued on the current stream, nothing synchronised; cand_pt comes at full capacity."""
    L = _lib.load()
    if device:
        dev = tab["kf_slot_off"].device
        n_tgt, nkf, nslots, npts = tgt_kf.numel(), tab["kf_slot_off"].numel() - 1, tab["kf_slot_pt"].numel(), tab["pt_bad"].numel()
        cap = npts if cap_cand is None else int(cap_cand)
        ws = _lib.workspace("orbl_fuse_candidates_workspace", n_tgt, npts, device=dev, reuse=workspace)
        o = _sn_dev_out({} if out is None else out, (("cand_pt", np.int32, cap), ("counts", np.int32, 2), ("status", np.int32, 1)), dev)
        _lib.check(L.orbl_fuse_candidates_device(n_tgt, _pn(tgt_kf), nkf, _p(tab["kf_slot_off"]), nslots, _pn(tab["kf_slot_pt"]), npts,
                                                 _pn(tab["pt_bad"]), _pn(tab["pt_fuse_cand"]), int(cur_id), cap, _pn(o["cand_pt"]), _pn(o["counts"]),
                                                 _pn(o["status"]), _p(ws), _lib.stream()), "orbl_fuse_candidates_device")
        return dict(o, pt_fuse_cand=tab["pt_fuse_cand"], _workspace=ws)
    t = _sn_host(tab, ("kf_slot_off", "kf_slot_pt", "pt_bad"))
    tg = _c(tgt_kf, np.int32).reshape(-1)
    stamp = np.array(tab["pt_fuse_cand"], np.int32).reshape(-1)
    npts = len(t["pt_bad"])
    cap = npts if cap_cand is None else int(cap_cand)
    cand, counts = np.zeros(max(cap, 1), np.int32), np.zeros(2, np.int32)
    _lib.check(L.orbl_fuse_candidates(len(tg), _pn(tg), len(t["kf_slot_off"]) - 1, _p(t["kf_slot_off"]), _pn(t["kf_slot_pt"]), npts, _pn(t["pt_bad"]),
                                      _pn(stamp), int(cur_id), cap, _p(cand) if cap else None, _p(counts)), "orbl_fuse_candidates")
    return dict(cand_pt=cand[:counts[0]], counts=counts, pt_fuse_cand=stamp)


_SN_UPD_IN = ("kf_bad", "kf_center", "kf_slot_off", "kf_slot_pt", "kf_slot_level", "kf_slot_desc", "pt_bad", "X", "pt_ref_kf", "obs_off", "obs_kf", "obs_slot",
              "scale_factors")
_SN_UPD_INOUT = ("pt_desc", "pt_normal", "pt_min_dist", "pt_max_dist")


def update_map_points_on_tables(what, tab, pt_mask=None, mask_kf=-1, device=False, out=None, workspace=None):
    """MapPoint::ComputeDistinctiveDescriptors and / or UpdateNormalAndDepth (what = MP_DESC, MP_NORMAL_DEPTH or both) for the points that
    pt_mask[npts] and / or the non-null slots of keyframe mask_kf select, read from the tables (orbl_update_map_points_on_tables).  tab:
    kf_bad (may be None), kf_center, kf_slot_off, kf_slot_pt, kf_slot_level, kf_slot_desc, pt_bad, X, pt_ref_kf, obs_off, obs_kf, obs_slot,
    scale_factors and the tables it rewrites: pt_desc, pt_normal, pt_min_dist, pt_max_dist.  Host form: those four come back as new copies
    with best_obs and nd_written.  device=True: torch CUDA tensors, the four tables change IN PLACE, enqueued on the current stream,
    nothing synchronised; returns best_obs, nd_written, status and the workspace."""
    L = _lib.load()
    desc, nd = bool(what & MP_DESC), bool(what & MP_NORMAL_DEPTH)
    if device:
        g = tab.get
        dev = tab["obs_off"].device
        nkf, nslots, npts, nobs = tab["kf_slot_off"].numel() - 1, tab["kf_slot_desc"].numel() // 32, tab["pt_bad"].numel(), tab["obs_kf"].numel()
        ws = _lib.workspace("orbl_update_map_points_on_tables_workspace", npts, nobs, device=dev, min_bytes=16, reuse=workspace)
        o = _sn_dev_out({} if out is None else out, (("best_obs", np.int32, npts), ("nd_written", np.uint8, npts), ("status", np.int32, 1)), dev)
        sf = g("scale_factors")
        _lib.check(L.orbl_update_map_points_on_tables_device(int(what), _pn(pt_mask), int(mask_kf), nkf, _pn(g("kf_bad")), _pn(g("kf_center")),
                                                             _p(tab["kf_slot_off"]), nslots, _pn(g("kf_slot_pt")), _pn(g("kf_slot_level")),
                                                             _pn(tab["kf_slot_desc"]), npts, _pn(tab["pt_bad"]), _pn(g("X")), _pn(g("pt_ref_kf")), nobs,
                                                             _p(tab["obs_off"]), _pn(tab["obs_kf"]), _pn(tab["obs_slot"]), _pn(sf),
                                                             sf.numel() if sf is not None else 0, *[_pn(g(k)) for k in _SN_UPD_INOUT], _pn(o["best_obs"]),
                                                             _pn(o["nd_written"]), _pn(o["status"]), _p(ws), _lib.stream()),
                   "orbl_update_map_points_on_tables_device")
        return dict(o, _workspace=ws, **{k: g(k) for k in _SN_UPD_INOUT})
    t = _sn_host(tab, _SN_UPD_IN)
    dt = dict(_SN_TAB)
    io = {k: (None if tab.get(k) is None else np.array(tab[k], dt[k]).reshape(-1)) for k in _SN_UPD_INOUT}                     # (always copies)
    npts = len(t["pt_bad"])
    pm = None if pt_mask is None else _c(pt_mask, np.uint8).reshape(-1)
    assert pm is None or len(pm) == npts
    best, wrote = np.full(npts, -1, np.int32), np.zeros(npts, np.uint8)
    sf = t["scale_factors"]
    _lib.check(L.orbl_update_map_points_on_tables(int(what), _pn(pm), int(mask_kf), len(t["kf_slot_off"]) - 1, _pn(t["kf_bad"]), _pn(t["kf_center"]),
                                                  _p(t["kf_slot_off"]), _pn(t["kf_slot_pt"]), _pn(t["kf_slot_level"]), _pn(t["kf_slot_desc"]), npts,
                                                  _pn(t["pt_bad"]), _pn(t["X"]), _pn(t["pt_ref_kf"]), _p(t["obs_off"]), _pn(t["obs_kf"]), _pn(t["obs_slot"]),
                                                  _pn(sf), len(sf) if sf is not None else 0, *[_pn(io[k]) for k in _SN_UPD_INOUT], _pn(best) if desc else None,
                                                  _pn(wrote) if nd else None), "orbl_update_map_points_on_tables")
    r = dict(io, best_obs=best, nd_written=wrote)
    if r["pt_desc"] is not None:
        r["pt_desc"] = r["pt_desc"].reshape(-1, 32)
    if r["pt_normal"] is not None:
        r["pt_normal"] = r["pt_normal"].reshape(-1, 3)
    return r


def search_in_neighbors_on_tables(cur_kf, cur_id, tab, device=True, nn=20, nn2=5, th=3.0, log_scale_factor=None, conn_th=15):
    """LocalMapping::SearchInNeighbors (src/LocalMapping.cc:398-488) on the resident map tables, with the reference's sequential semantics:
      1. fuse_targets; n_tgt is read back.
      2. a snapshot of the current keyframe's slot row (map_point_matches is taken once, :435, and the row changes during the loop).
      3. per target, in list order: fuse_rows for the snapshot -> apply_map_edits_device -> update_map_points_on_tables(MP_DESC, pt_touched);
         the 32 bytes of counts are read back for the next call's nobs, and the observation tables are swapped for the rebuilt ones.
      4. fuse_candidates; the count is read back.
      5. fuse_rows for the current keyframe over the candidates -> apply_map_edits_device.
      6. the descriptors of the touched points.
      7. update_map_points_on_tables(MP_DESC | MP_NORMAL_DEPTH, the non-null slots of cur_kf) (:474-485).
      8. update_connections_device for the one keyframe (:487).
    Those count read-backs - one per target keyframe plus three - are the ONLY host reads before the end; no table crosses to the host.
    tab: a dict of torch CUDA tensors that is changed IN PLACE - every table named in fuse_targets, fuse_rows, fuse_candidates,
    update_map_points_on_tables and apply_map_edits_device (kf_rank, pt_found / pt_visible, pt_replaced may be None), plus conn_off,
    conn_kf, conn_w for update_connections_device; kf_K4 may be the float64 table of the BA builders (it is narrowed once).  The entries
    obs_off, obs_kf, obs_slot are REPLACED by the rebuilt tables.  device=False: the tables are numpy arrays; they are uploaded, the same
    chain runs, and a dict of new numpy tables comes back (a GPU is needed either way).
    Returns dict(tab, tgt_kf (host list), n_fused: the reference's return value of every Fuse call - one per target, then the current
    keyframe's -, cand_pt (host array), connections = what update_connections_device returned (its own status word included), status = the
    OR of the status words of every other call: 0 unless some table entry was out of range)."""
    import torch
    if not device:
        dt = dict(_SN_TAB)
        up = {k: (None if v is None else (torch.as_tensor(_c(v, dt[k])).cuda() if k in dt else v)) for k, v in tab.items()}
        r = search_in_neighbors_on_tables(cur_kf, cur_id, up, True, nn, nn2, th, log_scale_factor, conn_th)
        torch.cuda.synchronize()
        r["tab"] = {k: (v.cpu().numpy() if hasattr(v, "data_ptr") else v) for k, v in r["tab"].items()}
        r["connections"] = {k: (v.cpu().numpy() if hasattr(v, "data_ptr") else v) for k, v in r["connections"].items() if k != "_workspace"}
        return r
    t = dict(tab)
    if t["kf_K4"].dtype != torch.float32:
        t["kf_K4"] = t["kf_K4"].to(torch.float32)
    dev = t["obs_off"].device
    statuses, n_fused, keep = [], [], []
    tg = fuse_targets(cur_kf, cur_id, t, nn, nn2, device=True)
    statuses.append(tg["status"])
    n_tgt = int(tg["counts"][:1].cpu()[0])                             # host read 1
    lo, hi = (int(v) for v in t["kf_slot_off"][int(cur_kf):int(cur_kf) + 2].cpu())       # (the offsets are static: read once, with n_tgt)
    snapshot = t["kf_slot_pt"][lo:hi].clone()

    def fuse(kf_word, pts):
        rows = fuse_rows(kf_word, pts, t, th, log_scale_factor, device=True, extras=False)
        ed = apply_map_edits_device(rows, dict(t, kf_slot_level=None, kf_slot_uv=None))          # (no oobs_level / oobs_uv: nothing here reads them)
        t["obs_off"], full = ed.oobs_off, (ed.oobs_kf, ed.oobs_slot)
        c = ed.counts.cpu()                                            # the 32 bytes of counts: the next call's nobs
        n = int(c[0])
        t["obs_kf"], t["obs_slot"] = full[0][:n], full[1][:n]
        up = update_map_points_on_tables(MP_DESC, t, pt_mask=ed.pt_touched, device=True)
        statuses.extend((rows["status"], ed.status, up["status"]))
        keep.extend((rows, ed, up))
        n_fused.append(int(c[4]))

    for i in range(n_tgt):
        fuse(tg["tgt_kf"][i:i + 1], snapshot)
    cd = fuse_candidates(tg["tgt_kf"][:n_tgt], cur_id, t, device=True)
    statuses.append(cd["status"])
    n_cand = int(cd["counts"][:1].cpu()[0])
    cur_word = torch.tensor([int(cur_kf)], dtype=torch.int32, device=dev)
    fuse(cur_word, cd["cand_pt"][:n_cand])
    up = update_map_points_on_tables(MP_DESC | MP_NORMAL_DEPTH, t, mask_kf=int(cur_kf), device=True)
    statuses.append(up["status"])
    row_off = torch.tensor([0, hi - lo], dtype=torch.int32, device=dev)              # (update_connections takes the slot rows of its targets only)
    conn = update_connections_device(cur_word, row_off, t["kf_slot_pt"][lo:hi], t["kf_slot_off"].numel() - 1, t["obs_off"], t["obs_kf"], t["conn_off"], t["conn_kf"],
                                     t["conn_w"], pt_bad=t["pt_bad"], kf_rank=t.get("kf_rank"), th=conn_th)
    status = 0
    for s in torch.stack([s.reshape(-1)[0] for s in statuses]).cpu().tolist():
        status |= int(s) & 0xFFFFFFFF
    for k in ("obs_off", "obs_kf", "obs_slot"):
        tab[k] = t[k]
    return dict(tab=tab, tgt_kf=tg["tgt_kf"][:n_tgt].cpu().tolist(), n_fused=n_fused, cand_pt=cd["cand_pt"][:n_cand].cpu().numpy(), connections=conn, status=status,
                _keep=(keep, up, cd, tg, snapshot, cur_word, row_off))
