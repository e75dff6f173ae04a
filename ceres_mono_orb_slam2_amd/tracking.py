"""Tracking::TrackWithMotionModel's data-parallel core as ONE device-resident call (reference src/Tracking.cc:616-646):
Frame construction (ORBextractor::operator(), grid), ORBmatcher::SearchByProjection(current_frame_, last_frame_, th) and
CeresOptimizer::PoseOptimization - include/orbslam_hip.h::orbt_track_with_motion_model, csrc/orb_track.hip."""
import ctypes as C
import threading

import numpy as np

from . import _lib
from .extractor import KP_DTYPE


class TrackResult(C.Structure):                # orbt_result
    _fields_ = [("n_keypoints", C.c_int32), ("nmatches", C.c_int32), ("n_correspondences", C.c_int32), ("n_inliers", C.c_int32),
                ("greedy_rounds", C.c_int32), ("reserved", C.c_int32), ("pose7", C.c_double * 7)]


def _c(a, dt):
    """C-contiguous array of dtype dt without a copy (or a call into numpy) when it already is one"""
    if type(a) is np.ndarray and a.dtype == dt and a.flags.c_contiguous:
        return a
    return np.ascontiguousarray(a, dt)


def _addr(a):
    return a.__array_interface__["data"][0]


def image_bounds(w, h, K4, dist5):
    """Frame::ComputeImageBounds (include/orbslam_hip.h::orbt_image_bounds; reference src/Frame.cc:357-385): {min_x, max_x, min_y, max_y}
    float32 of a w x h image under the distortion dist5 = (k1, k2, p1, p2, k3) - the `bounds` of every track_* call of that camera."""
    L = _lib.load()
    K4 = _c(K4, np.float32); d = _c(dist5, np.float32)
    assert K4.size == 4 and d.size == 5
    out = np.zeros(4, np.float32)
    _lib.check(L.orbt_image_bounds(int(w), int(h), _addr(K4), _addr(d), _addr(out)), "orbt_image_bounds")
    return out


def set_distortion(extractor, dist5):
    """orbt_set_distortion: every later track_* call of THIS thread that extracts a frame with `extractor` undistorts its keypoints with
    dist5 = (k1, k2, p1, p2, k3) before the grid is built (Frame::UndistortKeyPoints).  None, or k1 == 0: no distortion (the default).
    Set the coefficients of an extractor through THIS function, not through the library's orbt_set_distortion on extractor._h:
    track_with_motion_model asks the library for kps_undistorted only for extractors that got coefficients here (for all others it
    returns the raw coordinates as they lie in kps, without a call), so coefficients set behind its back would leave kps_undistorted raw.
    A call that goes on with a resident frame (track_local_map, image=None) after the coefficients changed is refused."""
    L = _lib.load()
    if dist5 is None:
        _lib.check(L.orbt_set_distortion(extractor._h, None), "orbt_set_distortion")
        return
    d = _c(dist5, np.float32)
    assert d.size == 5
    _lib.check(L.orbt_set_distortion(extractor._h, _addr(d)), "orbt_set_distortion")
    # Never cleared: the coefficients are per THREAD in the library, so another thread may still hold some when this one drops its own.
    # An extractor that never had any takes track_with_motion_model's shortcut (the raw coordinates as a view of kps, no call).
    extractor._had_distortion = True


def _last_undistorted(L, extractor, cap):
    """undistort_keypoints_[i].pt of the frame the call before produced (orbt_last_undistorted_keypoints): (n, 2) float32"""
    und = np.zeros((cap, 2), np.float32); n = C.c_int(0)
    _lib.check(L.orbt_last_undistorted_keypoints(extractor._h, _addr(und), cap, C.byref(n)), "orbt_last_undistorted_keypoints")
    return und[:n.value]


def track_with_motion_model(extractor, image, K4, bounds, Tcw_pred, last_Xw, last_desc, last_octave, last_angle, last_valid, th=15.0,
                            check_ori=True, copy=True):
    """extractor: ORBextractor; image (H, W) uint8; Tcw_pred (3 or 4, 4); the last frame's per-feature arrays (see the header).
    Returns dict(kps, kps_undistorted, desc, match, owner, outlier, pose7, nmatches, n_inliers, n_correspondences, greedy_rounds); kps
    are the raw keypoints, kps_undistorted (n, 2) float32 their undistorted coordinates (set_distortion; the raw ones without).  copy=True (the
    default) returns private arrays.  copy=False is for the latency-critical caller: the arrays are then READ-ONLY VIEWS of two
    alternating buffer sets kept with the extractor - frame N's arrays are overwritten by frame N + 2 - so anything kept longer
    (keyframe bookkeeping) must be copied by the caller.  Calls on one extractor are serialised by a lock kept with it."""
    L = _lib.load()
    img = _c(image, np.uint8)
    h, w = img.shape
    K4 = _c(K4, np.float32); bounds = _c(bounds, np.float32)
    T = np.ascontiguousarray(np.asarray(Tcw_pred, np.float64).reshape(-1)[:12])
    X = _c(last_Xw, np.float64).reshape(-1, 3); n = len(X)
    D = _c(last_desc, np.uint8).reshape(-1, 32); O = _c(last_octave, np.int32)
    A = _c(last_angle, np.float32); V = _c(last_valid, np.uint8)
    assert len(D) == n and len(O) == n and len(A) == n and len(V) == n
    # The output buffers (and their addresses) live with the extractor, two sets used alternately: a per-frame call must not spend
    # its time in allocations, page faults and copies (190 us of Python per call at first, ~25 now).
    with _extractor_lock(extractor):
        return _track_locked(L, extractor, img, w, h, K4, bounds, T, X, D, O, A, V, n, th, check_ori, copy)


def _extractor_lock(extractor):
    """One lock per extractor: every entry point that runs an extraction on it (pyramid / blur buffers, side stream and events of
    the context are per-extractor state) takes it, so calls on one extractor from several Python threads are serialised."""
    lock = extractor.__dict__.get("_track_lock")
    if lock is None:
        lock = extractor.__dict__.setdefault("_track_lock", threading.Lock())
    return lock


def _track_locked(L, extractor, img, w, h, K4, bounds, T, X, D, O, A, V, n, th, check_ori, copy):
    cap = extractor.max_keypoints
    S = getattr(extractor, "_track_bufs", None)
    if S is None or S["cap"] != cap or S["nq"] < n:
        nq = max(n, 1, S["nq"] if S else 0)
        def mk():
            b = dict(kps=np.zeros(cap, KP_DTYPE), desc=np.zeros((cap, 32), np.uint8), match=np.full(nq, -1, np.int32),
                     owner=np.full(cap, -1, np.int32), outl=np.zeros(cap, np.uint8), res=TrackResult(), und=np.zeros((cap, 2), np.float32), nund=C.c_int(0))
            b["p"] = tuple(_addr(b[k]) for k in ("kps", "desc", "match", "owner", "outl"))
            b["pres"] = C.byref(b["res"]); b["pund"] = _addr(b["und"]); b["pnund"] = C.byref(b["nund"])
            b["raw_xy"] = np.ndarray((cap, 2), np.float32, b["kps"], 0, (b["kps"].itemsize, 4))      # {x, y} of the keypoint records in place
            return b
        S = dict(cap=cap, nq=nq, sets=(mk(), mk()), turn=0)
        extractor._track_bufs = S
    S["turn"] ^= 1
    B = S["sets"][S["turn"]]
    pk, pd, pm, po, pl = B["p"]
    res = B["res"]
    _lib.check(L.orbt_track_with_motion_model(extractor._h, _addr(img), w, h, img.strides[0], _addr(K4), _addr(bounds), _addr(T), _addr(X),
                                              _addr(D), _addr(O), _addr(A), _addr(V), n, float(th), int(bool(check_ori)), pk, pd, cap, pm, po, pl,
                                              B["pres"]), "orbt_track_with_motion_model")
    und = B["raw_xy"]                                          # without distortion undistort_keypoints_ ARE keypoints_ (src/Frame.cc:330-333)
    if getattr(extractor, "_had_distortion", False):
        _lib.check(L.orbt_last_undistorted_keypoints(extractor._h, B["pund"], cap, B["pnund"]), "orbt_last_undistorted_keypoints")
        und = B["und"]
    k = res.n_keypoints
    out = dict(kps=B["kps"][:k], kps_undistorted=und[:k], desc=B["desc"][:k], match=B["match"][:n], owner=B["owner"][:k], outlier=B["outl"][:k].view(np.bool_),
               pose7=np.array(res.pose7[:], np.float64), nmatches=res.nmatches, n_inliers=res.n_inliers,
               n_correspondences=res.n_correspondences, greedy_rounds=res.greedy_rounds)
    for key in ("kps", "kps_undistorted", "desc", "match", "owner", "outlier"):
        if copy:
            out[key] = out[key].copy()
        else:
            v = out[key].view(); v.flags.writeable = False; out[key] = v
    return out


def track_local_map(extractor, K4, bounds, Tcw, log_scale_factor, mp_Xw, mp_normal, mp_min_dist, mp_max_dist, mp_desc, mp_state, slot_Xw, slot_state,
                    th=1.0, nnratio=0.8):
    """Tracking::TrackLocalMap's data-parallel core on the frame the last track_with_motion_model call of THIS thread left on the
    device (include/orbslam_hip.h::orbt_track_local_map; reference src/Tracking.cc:673-750, :793-842, src/ORBmatcher.cc:42-119).
    Returns dict(in_view, match, owner, outlier, pose7, nmatches, n_inliers, n_correspondences, n_in_view, greedy_rounds)."""
    L = _lib.load()
    K4 = _c(K4, np.float32); bounds = _c(bounds, np.float32)
    T = np.ascontiguousarray(np.asarray(Tcw, np.float64).reshape(-1)[:12])
    X = _c(mp_Xw, np.float64).reshape(-1, 3); n = len(X)
    N = _c(mp_normal, np.float64).reshape(-1, 3); mn = _c(mp_min_dist, np.float32); mx = _c(mp_max_dist, np.float32)
    D = _c(mp_desc, np.uint8).reshape(-1, 32); S = _c(mp_state, np.uint8)
    SX = _c(slot_Xw, np.float64).reshape(-1, 3); SS = _c(slot_state, np.uint8); nk = len(SS)
    assert len(N) == n and len(mn) == n and len(mx) == n and len(D) == n and len(S) == n and len(SX) == nk
    in_view = np.zeros(max(n, 1), np.uint8); match = np.full(max(n, 1), -1, np.int32)
    owner = np.full(max(nk, 1), -1, np.int32); outl = np.zeros(max(nk, 1), np.uint8)
    res = TrackResult()
    _lib.check(L.orbt_track_local_map(extractor._h, _addr(K4), _addr(bounds), _addr(T), float(log_scale_factor), _addr(X), _addr(N), _addr(mn), _addr(mx), _addr(D),
                                      _addr(S), n, _addr(SX), _addr(SS), nk, float(th), float(nnratio), _addr(in_view), _addr(match), _addr(owner), _addr(outl),
                                      C.byref(res)), "orbt_track_local_map")
    return dict(in_view=in_view[:n].view(np.bool_), match=match[:n], owner=owner[:nk], outlier=outl[:nk].view(np.bool_), pose7=np.array(res.pose7[:], np.float64),
                nmatches=res.nmatches, n_inliers=res.n_inliers, n_correspondences=res.n_correspondences, n_in_view=res.reserved, greedy_rounds=res.greedy_rounds)


def track_reference_keyframe(extractor, vocabulary, image, K4, bounds, Tcw_last, kf_desc, kf_valid, kf_angle, kf_Xw, kf_fv, nnratio=0.7, check_ori=True):
    """Tracking::TrackReferenceKeyFrame's data-parallel core (include/orbslam_hip.h::orbt_track_reference_keyframe; reference
    src/Tracking.cc:566-615).  image None: the frame of the last orbt_* call of this thread.  kf_fv = (node ids, offsets, indices).
    Returns dict(kps, kps_undistorted, desc (None without image), bow=(words, values), fv=(nodes, offsets, indices), match, owner, outlier, pose7, ...)."""
    L = _lib.load()
    K4 = _c(K4, np.float32); bounds = _c(bounds, np.float32)
    T = np.ascontiguousarray(np.asarray(Tcw_last, np.float64).reshape(-1)[:12])
    D = _c(kf_desc, np.uint8).reshape(-1, 32); n = len(D)
    V = _c(kf_valid, np.uint8); A = _c(kf_angle, np.float32); X = _c(kf_Xw, np.float64).reshape(-1, 3)
    fn, fo, fi = [_c(x, np.uint32) for x in kf_fv]
    assert len(V) == n and len(A) == n and len(X) == n and len(fo) == len(fn) + 1
    cap = extractor.max_keypoints
    kps = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8)
    bw = np.zeros(cap, np.uint32); bv = np.zeros(cap, np.float64); nw = C.c_int(0)
    on = np.zeros(cap, np.uint32); oo = np.zeros(cap + 2, np.uint32); oi = np.zeros(cap, np.uint32); nf = C.c_int(0)
    match = np.full(max(n, 1), -1, np.int32); owner = np.full(cap, -1, np.int32); outl = np.zeros(cap, np.uint8)
    res = TrackResult()
    if image is not None:
        img = _c(image, np.uint8); h, w = img.shape; ip, st = _addr(img), img.strides[0]
    else:
        img, h, w, ip, st = None, 0, 0, None, 0
    import contextlib
    with (_extractor_lock(extractor) if img is not None else contextlib.nullcontext()):      # (with an image the call runs an extraction on this extractor)
        _lib.check(L.orbt_track_reference_keyframe(extractor._h, vocabulary._h, ip, w, h, st, _addr(K4), _addr(bounds), _addr(T), _addr(D), _addr(V), _addr(A), _addr(X), n,
                                                   _addr(fn), _addr(fo), _addr(fi), len(fn), float(nnratio), int(bool(check_ori)), _addr(kps), _addr(desc), cap,
                                                   _addr(bw), _addr(bv), C.byref(nw), _addr(on), _addr(oo), _addr(oi), C.byref(nf), _addr(match), _addr(owner), _addr(outl),
                                                   C.byref(res)), "orbt_track_reference_keyframe")
        und = _last_undistorted(L, extractor, cap) if img is not None else None
    k = res.n_keypoints
    return dict(kps=kps[:k] if img is not None else None, kps_undistorted=und, desc=desc[:k] if img is not None else None, bow=(bw[:nw.value], bv[:nw.value]),
                fv=(on[:nf.value], oo[:nf.value + 1], oi[:oo[nf.value]]), match=match[:n], owner=owner[:k], outlier=outl[:k].view(np.bool_),
                pose7=np.array(res.pose7[:], np.float64), nmatches=res.nmatches, n_inliers=res.n_inliers, n_correspondences=res.n_correspondences, n_keypoints=k)


def last_call_ms():
    """orbt_last_call_ms: wall time of this thread's most recent track_* call inside the library (a Python caller adds its own
    interpreter-lock waits around the call when other threads are busy)."""
    return float(_lib.load().orbt_last_call_ms())


class _RelocKF(C.Structure):         # orbt_reloc_keyframe
    _fields_ = [("desc", C.c_void_p), ("valid", C.c_void_p), ("angle", C.c_void_p), ("n", C.c_int),
                ("fv_node", C.c_void_p), ("fv_off", C.c_void_p), ("fv_idx", C.c_void_p), ("fv_n", C.c_int)]


def relocalization_search_by_bow(extractor, vocabulary, image, K4, bounds, candidates, nnratio=0.75, check_ori=True):
    """Tracking::Relocalization, first stage (include/orbslam_hip.h::orbt_relocalization_search_by_bow; reference src/Tracking.cc:979-1029):
    ComputeBoW of the frame + SearchByBoW(keyframe, frame) for every candidate keyframe in one call.  candidates: dicts(desc[n,32],
    valid[n], angle[n], fv=(nodes, offsets, indices)).  image None: the frame of the last orbt_* call of this thread.
    Returns dict(kps, kps_undistorted, desc (None without image), bow, fv, owner[n_cand, n_keypoints], nmatches[n_cand])."""
    import contextlib
    L = _lib.load()
    K4 = _c(K4, np.float32); bounds = _c(bounds, np.float32)
    keep = []
    nc = len(candidates)
    cs = (_RelocKF * max(nc, 1))()
    for i, q in enumerate(candidates):
        D = _c(q["desc"], np.uint8).reshape(-1, 32); V = _c(q["valid"], np.uint8); A = _c(q["angle"], np.float32)
        fn, fo, fi = [_c(x, np.uint32) for x in q["fv"]]
        assert len(V) == len(D) and len(A) == len(D) and len(fo) == len(fn) + 1
        keep += [D, V, A, fn, fo, fi]
        cs[i].desc, cs[i].valid, cs[i].angle, cs[i].n = D.ctypes.data, V.ctypes.data, A.ctypes.data, len(D)
        cs[i].fv_node, cs[i].fv_off, cs[i].fv_idx, cs[i].fv_n = fn.ctypes.data, fo.ctypes.data, fi.ctypes.data, len(fn)
    cap = extractor.max_keypoints
    kps = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8)
    bw = np.zeros(cap, np.uint32); bv = np.zeros(cap, np.float64); nw = C.c_int(0)
    on = np.zeros(cap, np.uint32); oo = np.zeros(cap + 2, np.uint32); oi = np.zeros(cap, np.uint32); nf = C.c_int(0)
    owner = np.full((max(nc, 1), cap), -1, np.int32); nm = np.zeros(max(nc, 1), np.int32); nk = C.c_int(0)
    if image is not None:
        img = _c(image, np.uint8); h, w = img.shape; ip, st = _addr(img), img.strides[0]
    else:
        img, h, w, ip, st = None, 0, 0, None, 0
    with (_extractor_lock(extractor) if img is not None else contextlib.nullcontext()):
        _lib.check(L.orbt_relocalization_search_by_bow(extractor._h, vocabulary._h, ip, w, h, st, _addr(K4), _addr(bounds), C.cast(cs, C.c_void_p), nc, float(nnratio),
                                                       int(bool(check_ori)), _addr(kps), _addr(desc), cap, _addr(bw), _addr(bv), C.byref(nw), _addr(on), _addr(oo), _addr(oi),
                                                       C.byref(nf), _addr(owner), _addr(nm), C.byref(nk)), "orbt_relocalization_search_by_bow")
        und = _last_undistorted(L, extractor, cap) if img is not None else None
    k = nk.value
    return dict(kps=kps[:k] if img is not None else None, kps_undistorted=und, desc=desc[:k] if img is not None else None, bow=(bw[:nw.value], bv[:nw.value]),
                fv=(on[:nf.value], oo[:nf.value + 1], oi[:oo[nf.value]]), owner=owner[:nc, :k], nmatches=nm[:nc], n_keypoints=k)


# ---- Tracking::Relocalization behind a PnP pose (reference src/Tracking.cc:1056-1126) ----
RR_MAX_CANDIDATES = 64
RR_NO_POSE, RR_FEW_INLIERS, RR_MATCH_FIRST, RR_MATCH_SECOND, RR_MATCH_THIRD, RR_FAIL_WIDE, RR_FAIL_SECOND, RR_FAIL_NARROW, RR_FAIL_THIRD = range(9)


class _RefineCand(C.Structure):      # orbt_reloc_refine_candidate
    _fields_ = [("pt", C.c_void_p), ("Xw", C.c_void_p), ("desc", C.c_void_p), ("min_dist", C.c_void_p), ("max_dist", C.c_void_p), ("angle", C.c_void_p),
                ("n", C.c_int32), ("reserved", C.c_int32), ("Tcw", C.c_void_p), ("slot_kf", C.c_void_p)]


class _RefineResult(C.Structure):    # orbt_reloc_refine_result
    _fields_ = [("stage", C.c_int32), ("matched", C.c_int32), ("narrow_passes", C.c_int32), ("reserved", C.c_int32), ("n_good", C.c_int32 * 3),
                ("n_additional", C.c_int32 * 2), ("n_correspondences", C.c_int32 * 3), ("pose7", C.c_double * 7)]


def relocalization_refine(extractor, K4, bounds, candidates, log_scale_factor, check_ori=True, narrow_in_loop=True, n_kp=None, out=None):
    """Everything Tracking::Relocalization does behind a PnP pose, for every candidate of a round in one call on the frame the last
    extracting track_* / relocalization_search_by_bow call of THIS thread left on the device (include/orbslam_hip.h::
    orbt_relocalization_refine).  candidates: dicts(pt[n] point ids or -1, Xw[n, 3], desc[n, 32], min_dist[n], max_dist[n], angle[n],
    Tcw (3 or 4, 4) or None, slot_kf[n_kp] or None without a pose).  n_kp: the frame's keypoint count (default: the length of the first
    slot_kf).  out: optional (slot_kf_out, outlier) int32 / uint8 arrays of n_cand x n_kp entries to write into.
    Returns dict(first_match, results = one dict per candidate (stage, matched, narrow_passes, n_good[3], n_additional[2],
    n_correspondences[3], pose7, slot_kf[n_kp], outlier[n_kp]))."""
    L = _lib.load()
    K4 = _c(K4, np.float32); bounds = _c(bounds, np.float32)
    nc = len(candidates)
    if n_kp is None:
        n_kp = next((len(q["slot_kf"]) for q in candidates if q.get("slot_kf") is not None), 0)
    n_kp = int(n_kp)
    cs = (_RefineCand * max(nc, 1))()
    keep = []
    for i, q in enumerate(candidates):
        P = _c(q["pt"], np.int32).reshape(-1); n = len(P)
        X = _c(q["Xw"], np.float64).reshape(-1, 3); D = _c(q["desc"], np.uint8).reshape(-1, 32)
        mn = _c(q["min_dist"], np.float32).reshape(-1); mx = _c(q["max_dist"], np.float32).reshape(-1); A = _c(q["angle"], np.float32).reshape(-1)
        assert len(X) == n and len(D) == n and len(mn) == n and len(mx) == n and len(A) == n
        keep += [P, X, D, mn, mx, A]
        cs[i].pt, cs[i].Xw, cs[i].desc, cs[i].min_dist, cs[i].max_dist, cs[i].angle, cs[i].n = _addr(P), _addr(X), _addr(D), _addr(mn), _addr(mx), _addr(A), n
        if q.get("Tcw") is not None:
            T = np.ascontiguousarray(np.asarray(q["Tcw"], np.float64).reshape(-1)[:12]); S = _c(q["slot_kf"], np.int32).reshape(-1)
            assert len(S) == n_kp
            keep += [T, S]
            cs[i].Tcw, cs[i].slot_kf = _addr(T), _addr(S)
    res = (_RefineResult * max(nc, 1))()
    if out is None:
        slot = np.full((max(nc, 1), max(n_kp, 1)), -1, np.int32); outl = np.zeros((max(nc, 1), max(n_kp, 1)), np.uint8)
    else:
        slot, outl = out
        assert slot.dtype == np.int32 and outl.dtype == np.uint8 and slot.flags.c_contiguous and outl.flags.c_contiguous and slot.size >= nc * n_kp and outl.size >= nc * n_kp
    first = C.c_int32(-1)
    _lib.check(L.orbt_relocalization_refine(extractor._h, _addr(K4), _addr(bounds), float(log_scale_factor), C.cast(cs, C.c_void_p), nc, n_kp, int(bool(check_ori)),
                                            int(bool(narrow_in_loop)), C.cast(res, C.c_void_p), _addr(slot), _addr(outl), C.byref(first)), "orbt_relocalization_refine")
    fs = slot.reshape(-1)[:nc * n_kp].reshape(nc, n_kp); fo = outl.reshape(-1)[:nc * n_kp].reshape(nc, n_kp)
    results = [dict(stage=r.stage, matched=bool(r.matched), narrow_passes=r.narrow_passes, n_good=list(r.n_good), n_additional=list(r.n_additional),
                    n_correspondences=list(r.n_correspondences), pose7=np.array(r.pose7[:], np.float64), slot_kf=fs[i], outlier=fo[i].view(np.bool_))
               for i, r in enumerate(res[:nc])]
    return dict(first_match=first.value, results=results)


# ---- Tracking::UpdateLocalMap (reference src/Tracking.cc:838-977; include/orbslam_hip.h states the tables and the semantics) ----
ULM_OK, ULM_NO_VOTES = 0, 1
_PACKED = (("mp_Xw", np.float64, 3), ("mp_normal", np.float64, 3), ("mp_min_dist", np.float32, 1), ("mp_max_dist", np.float32, 1), ("mp_desc", np.uint8, 32),
           ("mp_state", np.uint8, 1), ("slot_Xw", np.float64, 3), ("slot_state", np.uint8, 1))


def _i32(a):
    return None if a is None else _c(a, np.int32).reshape(-1)


def _a(a):
    return None if a is None else _addr(a)


def update_local_keyframes(frame_pt, pt_bad, obs_off, obs_kf, kf_bad, kf_rank, kf_parent, cov_off, cov_kf, child_off, child_kf, prev_local_kf, cap_kf=None,
                           votes=True, out=None, check=True):
    """Tracking::UpdateLocalKeyFrames over the graph alone (orbt_update_local_keyframes).  kf_rank None = index order.  out: optional dict
    of preset output arrays (frame_pt_out, local_kf[cap_kf], votes).  Returns dict(frame_pt_out, local_kf (the list), n_local_kf, ref_kf
    (-1 = leave reference_keyframe_ alone), status (ULM_OK / ULM_NO_VOTES), votes).  check=False: a failing call returns dict(rc, n_local_kf)
    instead of raising (ORBHIP_ECAP writes the count alone)."""
    L = _lib.load()
    fp = _i32(frame_pt); pb = _c(pt_bad, np.uint8).reshape(-1); oo = _i32(obs_off); ok_ = _i32(obs_kf)
    kb = _c(kf_bad, np.uint8).reshape(-1); kr = _i32(kf_rank); kp = _i32(kf_parent); co = _i32(cov_off); ck = _i32(cov_kf); ho = _i32(child_off); hk = _i32(child_kf)
    pv = _i32(prev_local_kf)
    npts, nkf = len(pb), len(kb)
    assert (npts == 0 or len(oo) == npts + 1) and len(kp) == nkf and (kr is None or len(kr) == nkf) and (nkf == 0 or (len(co) == nkf + 1 and len(ho) == nkf + 1))
    assert (npts == 0 or len(ok_) >= oo[-1]) and (nkf == 0 or (len(ck) >= co[-1] and len(hk) >= ho[-1]))          # (the library checks the rest)
    cap = max(nkf, len(pv)) if cap_kf is None else int(cap_kf)
    o = {} if out is None else out
    o.setdefault("frame_pt_out", np.full(len(fp), -1, np.int32)); o.setdefault("local_kf", np.full(cap, -1, np.int32))
    if votes:
        o.setdefault("votes", np.zeros(nkf, np.int32))
    for k, n in (("frame_pt_out", len(fp)), ("local_kf", cap), ("votes", nkf)):
        assert o.get(k) is None or (o[k].dtype == np.int32 and o[k].flags.c_contiguous and o[k].size == n), k
    n = C.c_int(0); ref = C.c_int(-1); st = C.c_int(0)
    rc = L.orbt_update_local_keyframes(len(fp), _a(fp), npts, _a(pb), _a(oo), _a(ok_), nkf, _a(kb), _a(kr), _a(kp), _a(co), _a(ck), _a(ho), _a(hk), len(pv), _a(pv),
                                       cap, _a(o["frame_pt_out"]), _a(o["local_kf"]), C.byref(n), C.byref(ref), C.byref(st), _a(o.get("votes")))
    if not check and rc:
        return dict(rc=rc, n_local_kf=n.value)
    _lib.check(rc, "orbt_update_local_keyframes")
    return dict(frame_pt_out=o["frame_pt_out"], local_kf=o["local_kf"][:n.value], n_local_kf=n.value, ref_kf=ref.value, status=st.value, votes=o.get("votes"))


def update_local_points(kf_slot_off, kf_slot_pt, pt_bad, pt_nobs, pt_Xw, pt_normal, pt_min_dist, pt_max_dist, pt_desc, frame_pt, seen_pt, cap_pt, packed=True, out=None,
                        check=True):
    """Tracking::UpdateLocalPoints over the slot tables of the local keyframes (row i = the i-th local keyframe) and, with packed=True,
    the arrays track_local_map takes (orbt_update_local_points).  out: optional dict of preset output arrays.  Returns dict(local_pt (the
    list), n_local_pt, and the eight packed arrays at their full capacity: mp_*[cap_pt], slot_*[n_kp])."""
    L = _lib.load()
    so = _i32(kf_slot_off); sp = _i32(kf_slot_pt); pb = _c(pt_bad, np.uint8).reshape(-1); fp = _i32(frame_pt); se = _i32(seen_pt)
    npts, nl, nk, cap = len(pb), len(so) - 1, len(fp), int(cap_pt)
    assert nl >= 0 and len(sp) >= so[-1]
    rec = [None] * 6
    if packed:
        rec = [_i32(pt_nobs), _c(pt_Xw, np.float64).reshape(-1, 3), _c(pt_normal, np.float64).reshape(-1, 3), _c(pt_min_dist, np.float32).reshape(-1),
               _c(pt_max_dist, np.float32).reshape(-1), _c(pt_desc, np.uint8).reshape(-1, 32)]
        assert all(len(r) == npts for r in rec)
    o = {} if out is None else out
    o.setdefault("local_pt", np.full(cap, -1, np.int32))
    assert o["local_pt"].dtype == np.int32 and o["local_pt"].size == cap
    if packed:
        for k, dt, w in _PACKED:
            n = (nk if k.startswith("slot") else cap) * w
            o.setdefault(k, np.zeros(n, dt))
            assert o[k].dtype == dt and o[k].flags.c_contiguous and o[k].size == n, k
    n = C.c_int(0)
    rc = L.orbt_update_local_points(nl, _a(so), _a(sp), npts, _a(pb), *[_a(r) for r in rec], nk, _a(fp), len(se), _a(se), cap, _a(o["local_pt"]), C.byref(n),
                                    *[_a(o.get(k)) for k, _, _ in _PACKED])
    if not check and rc:
        return dict(rc=rc, n_local_pt=n.value)
    _lib.check(rc, "orbt_update_local_points")
    r = dict(local_pt=o["local_pt"][:n.value], n_local_pt=n.value)
    for k, _, w in _PACKED:
        r[k] = None if o.get(k) is None else (o[k].reshape(-1, w) if w > 1 else o[k])
    return r


def update_local_map_device(T, cap_kf, cap_pt, max_local_slots=None, packed=True, votes=True, out=None):
    """orbt_update_local_map_device on torch CUDA tensors, enqueued on the current stream, no synchronisation.  T: dict of the resident
    tables, named as in the header: frame_pt, seen_pt, prev_local_kf, pt_bad, pt_nobs, obs_off, obs_kf, pt_Xw, pt_normal, pt_min_dist,
    pt_max_dist, pt_desc, kf_bad, kf_rank (or None), kf_parent, cov_off, cov_kf, child_off, child_kf, kf_slot_off, kf_slot_pt (int32 /
    uint8 / float64 / float32 as there).  max_local_slots None = all slots.  out: optional dict of preset device tensors.  Returns a
    dict of device tensors: frame_pt_out, local_kf[cap_kf], local_pt[cap_pt], counts[4] = (n_local_kf, ref_kf, n_local_pt, status), votes,
    the eight packed arrays, status (the d_status word as int32[1]); the workspace is kept alive by the result."""
    import torch
    L = _lib.load()
    dev = T["pt_bad"].device
    n_kp, n_seen, n_prev = T["frame_pt"].numel(), T["seen_pt"].numel(), T["prev_local_kf"].numel()
    npts, nkf = T["pt_bad"].numel(), T["kf_bad"].numel()
    nobs, ncov, nchild, nslots = T["obs_kf"].numel(), T["cov_kf"].numel(), T["child_kf"].numel(), T["kf_slot_pt"].numel()
    mls = nslots if max_local_slots is None else int(max_local_slots)
    ws = _lib.workspace("orbt_update_local_map_workspace", nkf, npts, mls, device=dev)
    o = {} if out is None else out
    tdt = {np.float64: torch.float64, np.float32: torch.float32, np.uint8: torch.uint8}
    want = [("frame_pt_out", torch.int32, n_kp), ("local_kf", torch.int32, cap_kf), ("local_pt", torch.int32, cap_pt), ("counts", torch.int32, 4)]
    if votes:
        want.append(("votes", torch.int32, nkf))
    if packed:
        want += [(k, tdt[dt], (n_kp if k.startswith("slot") else cap_pt) * w) for k, dt, w in _PACKED]
    for k, dt, n in want:
        if o.get(k) is None:
            o[k] = torch.empty(max(n, 4), dtype=dt, device=dev)[:n]
        assert o[k].dtype == dt and o[k].is_contiguous() and o[k].numel() == n, k
    status = torch.empty(1, dtype=torch.int32, device=dev)
    p = _lib.ptr
    g = T.get
    _lib.check(L.orbt_update_local_map_device(
        n_kp, p(g("frame_pt")), n_seen, p(g("seen_pt")), n_prev, p(g("prev_local_kf")), npts, p(g("pt_bad")), p(g("pt_nobs")), nobs, p(g("obs_off")), p(g("obs_kf")),
        p(g("pt_Xw")), p(g("pt_normal")), p(g("pt_min_dist")), p(g("pt_max_dist")), p(g("pt_desc")), nkf, p(g("kf_bad")), p(g("kf_rank")), p(g("kf_parent")), ncov,
        p(g("cov_off")), p(g("cov_kf")), nchild, p(g("child_off")), p(g("child_kf")), nslots, p(g("kf_slot_off")), p(g("kf_slot_pt")), mls, int(cap_kf), int(cap_pt),
        p(o["frame_pt_out"]), p(o["local_kf"]), p(o["local_pt"]), p(o["counts"]), p(o.get("votes")), *[p(o.get(k)) for k, _, _ in _PACKED],
        p(status), p(ws), _lib.stream()), "orbt_update_local_map_device")
    r = dict(o)
    for k, _, w in _PACKED:
        if r.get(k) is not None and w > 1:
            r[k] = r[k].view(-1, w)
    r["status"] = status; r["_workspace"] = ws
    return r


def track_local_map_device(extractor, K4, bounds, Tcw, log_scale_factor, packed, n_mp, th=1.0, nnratio=0.8):
    """track_local_map on the packed DEVICE arrays update_local_map_device returned (`packed`: that dict, or any dict of torch CUDA tensors
    mp_Xw, mp_normal, mp_min_dist, mp_max_dist, mp_desc, mp_state, slot_Xw, slot_state) - orbt_track_local_map_device.  n_mp: the number
    of rows to run over, at least the count of local map points (the capacity is always right: padding rows have mp_state 0).  The
    arrays are taken as the current torch stream leaves them.  Returns what track_local_map returns."""
    L = _lib.load()
    K4 = _c(K4, np.float32); bounds = _c(bounds, np.float32)
    T = np.ascontiguousarray(np.asarray(Tcw, np.float64).reshape(-1)[:12])
    n = int(n_mp); nk = packed["slot_state"].numel()
    assert packed["mp_state"].numel() >= n and packed["mp_desc"].numel() >= 32 * n and packed["mp_Xw"].numel() >= 3 * n and packed["slot_Xw"].numel() == 3 * nk
    in_view = np.zeros(max(n, 1), np.uint8); match = np.full(max(n, 1), -1, np.int32)
    owner = np.full(max(nk, 1), -1, np.int32); outl = np.zeros(max(nk, 1), np.uint8)
    res = TrackResult()
    p = lambda k: _lib.ptr(packed[k])                                               # noqa: E731
    _lib.check(L.orbt_track_local_map_device(extractor._h, _addr(K4), _addr(bounds), _addr(T), float(log_scale_factor), p("mp_Xw"), p("mp_normal"), p("mp_min_dist"),
                                             p("mp_max_dist"), p("mp_desc"), p("mp_state"), n, p("slot_Xw"), p("slot_state"), nk, float(th), float(nnratio),
                                             _lib.stream(), _addr(in_view), _addr(match), _addr(owner), _addr(outl), C.byref(res)),
               "orbt_track_local_map_device")
    return dict(in_view=in_view[:n].view(np.bool_), match=match[:n], owner=owner[:nk], outlier=outl[:nk].view(np.bool_), pose7=np.array(res.pose7[:], np.float64),
                nmatches=res.nmatches, n_inliers=res.n_inliers, n_correspondences=res.n_correspondences, n_in_view=res.reserved, greedy_rounds=res.greedy_rounds)
