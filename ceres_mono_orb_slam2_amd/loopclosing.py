"""LoopClosing's two map-moving steps on the GPU (include/orbslam_hip.h: orbl_correct_loop*, orbl_propagate_global_ba*): the pose and
point correction of CorrectLoop (src/LoopClosing.cc:437-523) and the write-back of the global bundle adjustment (:681-739).
There is no CPU fallback: without the library or a GPU the calls raise."""
import ctypes as C

import numpy as np

from . import _lib

ML_OFFSETS, ML_KF, ML_PT, ML_RANK, ML_LEVEL, ML_SCW = 1, 2, 4, 8, 16, 32        # *d_status bits of orbl_correct_loop_device
GB_KF, GB_CYCLE, GB_STALE = 1, 2, 4                                             # *d_status bits of orbl_propagate_global_ba_device


def _c(a, dt):
    return np.ascontiguousarray(a, dt)


def _copy(a, dt, shape):
    return np.array(a, dtype=dt, order="C").reshape(shape)          # (always a copy: the in/out tables are returned, the caller's stay)


def _opt(a, dt):
    return None if a is None else _c(a, dt).reshape(-1)


def _addr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


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
    cr = _opt(conn_rank, np.int32)
    S = _c(Scw, np.float64).reshape(-1)
    so = _c(slot_off, np.int32).reshape(-1); sp = _c(slot_pt, np.int32).reshape(-1)
    Xn = _copy(X, np.float64, (-1, 3)); npts = len(Xn)
    pb = _opt(pt_bad, np.uint8); pd = _opt(pt_done, np.uint8)
    oo = _opt(obs_off, np.int32); ok_ = _opt(obs_kf, np.int32); rk = _opt(ref_kf, np.int32); rl = _opt(ref_level, np.int32); sf = _opt(scale_factors, np.float32)
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
    _lib.check(L.orbl_correct_loop(nkf, _addr(T), _addr(Cn), nconn, _addr(ck), _addr(cr), _addr(S), _addr(so), _addr(sp), npts, _addr(Xn), _addr(pb), _addr(pd),
                                   _addr(oo), _addr(ok_) if nd else None, _addr(rk), _addr(rl), _addr(sf), len(sf) if nd else 0, _addr(o["corrected"]),
                                   _addr(o["non_corrected"]), _addr(o["pt_owner"]), _addr(o["normal"]), _addr(o["min_max"]), _addr(o["nd_written"]),
                                   _addr(o["counts"])), "orbl_correct_loop")
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
    nbytes = C.c_size_t(0)
    _lib.check(L.orbl_correct_loop_workspace(nkf, nconn, npts, C.byref(nbytes)), "orbl_correct_loop_workspace")
    ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=dev) if workspace is None else workspace
    assert ws.numel() >= nbytes.value
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

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())
    for t in (kf_Tcw, kf_center, X):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float64)
    _lib.check(L.orbl_correct_loop_device(nkf, p(kf_Tcw), p(kf_center), nconn, p(conn_kf), p(conn_rank), p(Scw), nslots, p(slot_off), p(slot_pt), npts, p(X),
                                          p(pt_bad), p(pt_done), nobs, p(obs_off), p(obs_kf), p(ref_kf), p(ref_level), p(scale_factors),
                                          scale_factors.numel() if scale_factors is not None else 0, p(o["corrected"]), p(o["non_corrected"]), p(o["pt_owner"]),
                                          p(o.get("normal")), p(o.get("min_max")), p(o.get("nd_written")), p(o["counts"]), p(o["status"]), p(ws),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "orbl_correct_loop_device")
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
    pb = _opt(pt_bad, np.uint8); pin = _opt(pt_in_gba, np.uint8)
    pgx = None if pt_gba_X is None else _c(pt_gba_X, np.float64).reshape(-1, 3)
    ref = _c(pt_ref_kf, np.int32).reshape(-1)
    assert len(G) == nkf and len(F) == nkf and len(par) == nkf and (Cn is None or len(Cn) == nkf) and len(ref) == npts
    assert (pb is None or len(pb) == npts) and (pin is None or len(pin) == npts) and (pgx is None or len(pgx) == npts)
    bef = np.zeros((nkf, 12)) if kf_bef_Tcw is None else kf_bef_Tcw
    assert bef.dtype == np.float64 and bef.flags.c_contiguous and bef.size == 12 * nkf
    o = dict(kf_bef_Tcw=bef, kf_reached=np.zeros(nkf, np.uint8), pt_moved=np.zeros(npts, np.uint8), counts=np.zeros(4, np.int32))
    _lib.check(L.orbl_propagate_global_ba(nkf, _addr(T), _addr(G), _addr(F), _addr(par), len(org), _addr(org), _addr(Cn), npts, _addr(Xn), _addr(pb), _addr(pin),
                                          _addr(pgx), _addr(ref), _addr(bef), _addr(o["kf_reached"]), _addr(o["pt_moved"]), _addr(o["counts"])),
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
    nbytes = C.c_size_t(0)
    _lib.check(L.orbl_propagate_global_ba_workspace(nkf, npts, C.byref(nbytes)), "orbl_propagate_global_ba_workspace")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev) if workspace is None else workspace
    assert ws.numel() >= nbytes.value
    o = {} if out is None else dict(out)
    if kf_bef_Tcw is not None:
        o["kf_bef_Tcw"] = kf_bef_Tcw
    for k, dt, n in (("kf_bef_Tcw", torch.float64, 12 * nkf), ("kf_reached", torch.uint8, nkf), ("pt_moved", torch.uint8, npts), ("counts", torch.int32, 4),
                     ("status", torch.int32, 1)):
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 1), dtype=dt, device=dev)[:n]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == n, k

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())
    for t in (kf_Tcw, kf_gba_Tcw, kf_center, X):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float64)
    _lib.check(L.orbl_propagate_global_ba_device(nkf, p(kf_Tcw), p(kf_gba_Tcw), p(kf_in_gba), p(kf_parent), n_origin, p(origin_kf), p(kf_center), npts, p(X),
                                                 p(pt_bad), p(pt_in_gba), p(pt_gba_X), p(pt_ref_kf), p(o["kf_bef_Tcw"]), p(o["kf_reached"]), p(o["pt_moved"]),
                                                 p(o["counts"]), p(o["status"]), p(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "orbl_propagate_global_ba_device")
    r = dict(o)
    r.update(kf_Tcw=kf_Tcw, kf_gba_Tcw=kf_gba_Tcw, kf_in_gba=kf_in_gba, kf_center=kf_center, X=X, _workspace=ws)
    return r
