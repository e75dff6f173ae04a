"""Host mirror of the LocalMapping thread's device-resident steps (include/orbslam_hip.h: orbl_*; reference
src/LocalMapping.cc:196-396 CreateNewMapPoints, :398-505 SearchInNeighbors, :576-637 KeyFrameCulling; src/KeyFrame.cc:314-398 UpdateConnections).
Thin ctypes layer: arrays in, arrays out."""
import ctypes as C

import numpy as np

from . import _lib


class _KF(C.Structure):              # orbl_keyframe
    _fields_ = [("kps", C.c_void_p), ("desc", C.c_void_p), ("unmapped", C.c_void_p), ("n", C.c_int),
                ("fv_node", C.c_void_p), ("fv_off", C.c_void_p), ("fv_idx", C.c_void_p), ("fv_n", C.c_int),
                ("Tcw", C.c_double * 12), ("K4", C.c_float * 4), ("F12", C.c_double * 9), ("ex", C.c_float), ("ey", C.c_float)]


class _FuseKF(C.Structure):          # orbl_fuse_keyframe
    _fields_ = [("kps", C.c_void_p), ("desc", C.c_void_p), ("n", C.c_int), ("bounds", C.c_float * 4)]


def _c(a, dt):
    return np.ascontiguousarray(a, dt)


def _addr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


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
        st = C.c_void_p(stop.ctypes.data)
    L.orbl_create_new_map_points.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    a = (_addr(k1), _addr(d1), _addr(u1), n1, _addr(f1[0]), _addr(f1[1]), _addr(f1[2]), len(f1[0]), _addr(T1), _addr(K1), C.cast(nb, C.c_void_p), nn, _addr(sf), _addr(ls),
         len(sf), float(ratio_factor), st, _addr(m), _addr(ok), _addr(X), C.byref(npr))

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
        L.orbl_fuse_batch_sim3.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.check(L.orbl_fuse_batch_sim3(C.cast(kf, C.c_void_p), T, _addr(uv), _addr(rad), _addr(lvl), M, _addr(md), int(n_levels), _addr(bi), _addr(bd)),
                   "orbl_fuse_batch_sim3")
        return bi[:T, :M], bd[:T, :M]
    ils = _c(inv_level_sigma2, np.float32)
    L.orbl_fuse_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    _lib.check(L.orbl_fuse_batch(C.cast(kf, C.c_void_p), T, _addr(uv), _addr(rad), _addr(lvl), M, _addr(md), _addr(ils), len(ils), _addr(bi), _addr(bd)),
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
    vp, i32 = C.c_void_p, C.c_int
    L.orbl_update_map_points.argtypes = [i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    _lib.check(L.orbl_update_map_points(npts, _addr(off), _addr(Xa), _addr(rk), _addr(rl), _addr(pg), nobs, _addr(ok_), _addr(desc), _addr(kg),
                                        len(kc) if kc is not None else 0, _addr(kc), _addr(sf), len(sf) if sf is not None else 0, int(what),
                                        _addr(o["best_obs"]), _addr(o["desc"]), _addr(o["normal"]), _addr(o["min_max"]), _addr(o["nd_written"])),
               "orbl_update_map_points")
    return o


def update_map_points_device(obs_off, obs_desc, obs_kf_good, X, ref_kf, ref_level, obs_kf, kf_center, scale_factors, pt_good, what, out):
    """orbl_update_map_points_device on torch CUDA tensors (the same arguments as update_map_points; None where a pointer may be
    NULL); out = dict of device tensors (best_obs, desc, normal, min_max, nd_written), written on the current stream."""
    import torch
    L = _lib.load()
    npts = obs_off.numel() - 1
    nobs = obs_desc.shape[0] if obs_desc is not None else (obs_kf.numel() if obs_kf is not None else 0)
    nbytes = C.c_size_t(0)
    _lib.check(L.orbl_update_map_points_workspace(npts, C.byref(nbytes)), "orbl_update_map_points_workspace")
    ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=obs_off.device)

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())
    vp, i32 = C.c_void_p, C.c_int
    L.orbl_update_map_points_device.argtypes = [i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    _lib.check(L.orbl_update_map_points_device(npts, p(obs_off), p(X), p(ref_kf), p(ref_level), p(pt_good), nobs, p(obs_kf), p(obs_desc), p(obs_kf_good),
                                               kf_center.shape[0] if kf_center is not None else 0, p(kf_center), p(scale_factors),
                                               scale_factors.numel() if scale_factors is not None else 0, int(what), p(out.get("best_obs")), p(out.get("desc")),
                                               p(out.get("normal")), p(out.get("min_max")), p(out.get("nd_written")), p(ws),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), "orbl_update_map_points_device")
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
    _lib.check(L.orbl_keyframe_culling(ncand, _addr(ck), _addr(cf), _addr(so), _addr(sp), _addr(sl), int(nkf), npts, _addr(oo), _addr(ok_), _addr(ol), _addr(pb),
                                       _addr(pn), int(th_obs), float(ratio), _addr(o["culled"]), _addr(o["n_redundant"]), _addr(o["n_map_points"]),
                                       _addr(o.get("pt_bad")), _addr(o.get("pt_nobs")), _addr(o.get("obs_erased"))), "orbl_keyframe_culling")
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
    nbytes = C.c_size_t(0)
    _lib.check(L.orbl_keyframe_culling_workspace(ncand, nslots, npts, nobs, C.byref(nbytes)), "orbl_keyframe_culling_workspace")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    o = {} if out is None else out
    for k, dt, n in (("culled", torch.uint8, ncand), ("n_redundant", torch.int32, ncand), ("n_map_points", torch.int32, ncand)) + \
            ((("pt_bad", torch.uint8, npts), ("pt_nobs", torch.int32, npts), ("obs_erased", torch.uint8, nobs)) if final_state else ()):
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 1), dtype=dt, device=dev)[:n]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == n, k
    status = torch.empty(1, dtype=torch.int32, device=dev)

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())
    _lib.check(L.orbl_keyframe_culling_device(ncand, p(cand_kf), p(cand_flags), nslots, p(slot_off), p(slot_pt), p(slot_level), int(nkf), npts, nobs, p(obs_off),
                                              p(obs_kf), p(obs_level), p(pt_bad), p(pt_nobs), int(th_obs), float(ratio), p(o["culled"]), p(o["n_redundant"]),
                                              p(o["n_map_points"]), p(o.get("pt_bad")), p(o.get("pt_nobs")), p(o.get("obs_erased")), p(status), p(ws),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)), "orbl_keyframe_culling_device")
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
    rc = L.orbl_update_connections(ntgt, _addr(tk), _addr(tf), _addr(so), _addr(sp), int(nkf), npts, _addr(oo), _addr(ok_), _addr(pb), _addr(kr), _addr(co), _addr(ck),
                                   _addr(cw), _addr(po), _addr(pk), int(th), cap_aff, cap_conn, cap_ord, cap_link, _addr(o["tgt_status"]), _addr(o["tgt_parent"]),
                                   _addr(o["aff_kf"]), _addr(o["conn_off"]), _addr(o["conn_kf"]), _addr(o["conn_w"]), _addr(o["ord_off"]), _addr(o["ord_kf"]),
                                   _addr(o["ord_w"]), _addr(o.get("link_off")), _addr(o.get("link_kf")), _addr(o["counts"]))
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
    nbytes = C.c_size_t(0)
    _lib.check(L.orbl_update_connections_workspace(ntgt, int(nkf), npts, nslots, nconn, C.byref(nbytes)), "orbl_update_connections_workspace")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev) if workspace is None else workspace
    assert ws.numel() >= nbytes.value
    o = {} if out is None else out
    sizes = dict(tgt_status=ntgt, tgt_parent=ntgt, aff_kf=cap_aff, conn_off=cap_aff + 1, conn_kf=cap_conn, conn_w=cap_conn, ord_off=cap_aff + 1, ord_kf=cap_ord,
                 ord_w=cap_ord, counts=4, status=1)
    if links:
        sizes.update(link_off=ntgt + 1, link_kf=cap_link)
    for k, n in sizes.items():
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
        assert o[k].dtype == torch.int32 and o[k].is_contiguous() and o[k].numel() == n, k

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())
    _lib.check(L.orbl_update_connections_device(ntgt, p(tgt_kf), p(tgt_flags), nslots, p(slot_off), p(slot_pt), int(nkf), npts, nobs, p(obs_off), p(obs_kf), p(pt_bad),
                                                p(kf_rank), nconn, p(conn_off), p(conn_kf), p(conn_w), nprev, p(prev_off), p(prev_kf), int(th), cap_aff, cap_conn,
                                                cap_ord, cap_link, p(o["tgt_status"]), p(o["tgt_parent"]), p(o["aff_kf"]), p(o["conn_off"]), p(o["conn_kf"]),
                                                p(o["conn_w"]), p(o["ord_off"]), p(o["ord_kf"]), p(o["ord_w"]), p(o.get("link_off")), p(o.get("link_kf")),
                                                p(o["counts"]), p(o["status"]), p(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "orbl_update_connections_device")
    r = dict(o)
    r.setdefault("link_off", None); r.setdefault("link_kf", None)
    r["_workspace"] = ws                                         # (kept alive until the caller synchronises)
    return r
