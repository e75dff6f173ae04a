"""The staged round trip of the seven map-maintenance host entries (csrc/common.h: RoundTrip) on the MI355X: orbl_update_map_points,
orbl_keyframe_culling, orbl_update_connections, orbl_correct_loop, orbl_propagate_global_ba, orbt_update_local_keyframes and
orbt_update_local_points, where the staging itself can go wrong rather than the kernels:
  1. the smallest shapes, where a piece of the upload or of the result block is empty and a device pointer is NULL;
  2. counts that put the end of a uint8 piece on either side of the 256-byte boundary of the next one (255, 256, 257 points) and leave
     the float64 tables off it (11 keyframes), with every caller array between two guard bands of 64 elements;
  3. a larger call followed by a smaller one on the same thread, whose staging the second call reuses.
The problems come from the builders of the entries' own tests and every result is compared with the restatements those tests use
(tests/np*.py), bit for bit; nothing is restated here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import connectioncases as ucc  # noqa: E402
from tests import cullingcases as kcc  # noqa: E402
from tests import localmapcases as lmc  # noqa: E402
from tests import mapcorrectcases as mcc  # noqa: E402
from tests import npconnections as npu  # noqa: E402
from tests import npculling as npk  # noqa: E402
from tests import nplocalmap as npl  # noqa: E402
from tests import npmapcorrect as npc  # noqa: E402
from tests import npmappoint as npm  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = dict(int32=-77, uint8=0xA5, float64=-1.5e300, float32=-2.5e30)       # values no call writes
BOTH = npm.DESC | npm.NORMAL_DEPTH
NKF = 11                                                            # 11 x 12 and 11 x 3 doubles: neither ends on a 256-byte boundary
SIZES = (255, 256, 257)                                             # a uint8 per point: one short of, on and one past the boundary


class Guarded:
    """caller arrays, each the middle of an allocation with GUARD elements of the sentinel on both sides"""

    def __init__(self):
        self.whole = {}

    def new(self, name, shape, dt, init=None):
        n = int(np.prod(shape))
        w = np.full(n + 2 * GUARD, SENTINEL[np.dtype(dt).name], dt)
        v = w[GUARD:GUARD + n].reshape(shape)
        if init is not None:
            v[...] = np.asarray(init).reshape(shape)
        self.whole[name] = w
        return v

    def check(self, what):
        for name, w in self.whole.items():
            s = SENTINEL[w.dtype.name]
            assert (w[:GUARD] == s).all() and (w[-GUARD:] == s).all(), (what, name, "a guard band was written")


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _equal(got, exp, what, keys):
    for k in keys:
        if exp[k] is None:
            assert got[k] is None, (what, k)
            continue
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.dtype == e.dtype and g.size == e.size and np.array_equal(_bits(g), _bits(e)), (what, k)


def _dev(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).cuda()              # (a copy: an empty tensor's pointer is NULL)


def _np(t):
    return None if t is None else t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- update_map_points
MP_KEYS = ("best_obs", "desc", "normal", "min_max", "nd_written")


def _mp_outputs(npts, G):
    return dict(best_obs=G.new("best_obs", (npts,), np.int32), desc=G.new("desc", (npts, 32), np.uint8), normal=G.new("normal", (npts, 3), np.float64),
                min_max=G.new("min_max", (npts, 2), np.float32), nd_written=G.new("nd_written", (npts,), np.uint8))


def _mp_host(b, what, label):
    from ceres_mono_orb_slam2_amd import localmapping
    npts = len(b["obs_off"]) - 1
    G = Guarded()
    out = _mp_outputs(npts, G)
    exp = npm.update_map_points(b, what, out)                       # (from copies of the sentinel-filled arrays: rows left alone stay sentinel)
    got = localmapping.update_map_points(b["obs_off"], b["obs_desc"], b["obs_kf_good"], b["X"], b["ref_kf"], b["ref_level"], b["obs_kf"], b["kf_center"],
                                         b["scale_factors"], b["pt_good"], what, out)
    assert all(got[k] is out[k] for k in MP_KEYS)
    _equal(got, exp, label, MP_KEYS)
    G.check(label)
    return exp


def _mp_device(b, what, exp, label):
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    npts = len(b["obs_off"]) - 1
    out = {k: _dev(v) for k, v in _mp_outputs(npts, Guarded()).items()}
    localmapping.update_map_points_device(*[_dev(b[k]) for k in ("obs_off", "obs_desc", "obs_kf_good", "X", "ref_kf", "ref_level", "obs_kf", "kf_center", "scale_factors",
                                                                "pt_good")], what, out)
    torch.cuda.synchronize()
    d = {k: _np(out[k]).reshape(exp[k].shape) for k in MP_KEYS}
    # the device form writes every row of best_obs / nd_written and the rows of the rest that it computed: as the host form
    _equal(d, exp, label, MP_KEYS)


# ------------------------------------------------------------------------------------------------------------------ keyframe_culling
KC_KEYS = ("culled", "n_redundant", "n_map_points", "pt_bad", "pt_nobs", "obs_erased")


def _kc_host(pr, label, exp=None):
    from ceres_mono_orb_slam2_amd import localmapping
    exp = npk.culling(pr) if exp is None else exp
    ncand, npts, nobs = len(pr["cand_kf"]), pr["npts"], len(pr["obs_kf"])
    G = Guarded()
    out = dict(culled=G.new("culled", (ncand,), np.uint8), n_redundant=G.new("n_redundant", (ncand,), np.int32), n_map_points=G.new("n_map_points", (ncand,), np.int32),
               pt_bad=G.new("pt_bad", (npts,), np.uint8), pt_nobs=G.new("pt_nobs", (npts,), np.int32), obs_erased=G.new("obs_erased", (nobs,), np.uint8))
    r = localmapping.keyframe_culling(pr["cand_kf"], pr["cand_flags"], pr["slot_off"], pr["slot_pt"], pr["slot_level"], pr["nkf"], pr["obs_off"], pr["obs_kf"],
                                      pr["obs_level"], pr["pt_bad"], pr["pt_nobs"], out=out)
    assert all(getattr(r, k) is out[k] for k in KC_KEYS)
    _equal(out, exp, label, KC_KEYS)
    G.check(label)
    return exp


def _kc_device(pr, exp, label):
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    d = localmapping.keyframe_culling_device(*[_dev(pr[k]) for k in ("cand_kf", "cand_flags", "slot_off", "slot_pt", "slot_level")], pr["nkf"],
                                             *[_dev(pr[k]) for k in ("obs_off", "obs_kf", "obs_level", "pt_bad", "pt_nobs")])
    torch.cuda.synchronize()
    _equal({k: _np(getattr(d, k)) for k in KC_KEYS}, exp, label, KC_KEYS)
    assert int(d.status.item()) == 0, label


# --------------------------------------------------------------------------------------------------------------- update_connections
UC_KEYS = ("tgt_status", "tgt_parent", "counts", "aff_kf", "conn_off", "conn_kf", "conn_w", "ord_off", "ord_kf", "ord_w", "link_off", "link_kf")
UC_LISTS = dict(aff_kf=0, conn_kf=1, conn_w=1, ord_kf=2, ord_w=2, link_kf=3)       # output -> the entry of counts[] that is its length


def _uc_args(pr, conv=lambda a: a):
    a = [conv(pr[k]) for k in ("tgt_kf", "slot_off", "slot_pt")] + [pr["nkf"]] + [conv(pr[k]) for k in ("obs_off", "obs_kf", "conn_off", "conn_kf", "conn_w")]
    kw = dict(tgt_flags=conv(pr["tgt_flags"]), pt_bad=conv(pr["pt_bad"]), kf_rank=conv(pr["kf_rank"]), prev_off=conv(pr["prev_off"]), prev_kf=conv(pr["prev_kf"]), th=pr["th"])
    return a, kw


def _uc_host(pr, label, exp=None):
    from ceres_mono_orb_slam2_amd import localmapping
    exp = npu.connections(pr) if exp is None else exp
    ntgt, nkf, links = len(pr["tgt_kf"]), pr["nkf"], pr["prev_off"] is not None
    cap_aff, cap_conn, cap_ord, cap_link = caps = localmapping._uc_default_caps(ntgt, nkf, len(pr["conn_kf"]), links)
    sizes = dict(tgt_status=ntgt, tgt_parent=ntgt, aff_kf=cap_aff, conn_off=cap_aff + 1, conn_kf=cap_conn, conn_w=cap_conn, ord_off=cap_aff + 1, ord_kf=cap_ord, ord_w=cap_ord,
                 counts=4)
    if links:
        sizes.update(link_off=ntgt + 1, link_kf=cap_link)
    G = Guarded()
    out = {k: G.new(k, (n,), np.int32) for k, n in sizes.items()}
    a, kw = _uc_args(pr)
    r = localmapping.update_connections(*a, caps=caps, out=out, **kw)
    _equal(r, exp, label, UC_KEYS)
    c = exp["counts"]
    for k, i in UC_LISTS.items():                                   # behind a list's count the caller's array is not touched
        if k in out:
            assert (out[k][c[i]:] == SENTINEL["int32"]).all(), (label, k, "written behind its count")
    for k in ("conn_off", "ord_off"):
        assert (out[k][c[0] + 1:] == SENTINEL["int32"]).all(), (label, k, "written behind its count")
    G.check(label)
    return exp


def _uc_device(pr, exp, label):
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    a, kw = _uc_args(pr, _dev)
    r = localmapping.update_connections_device(*a, **kw)
    torch.cuda.synchronize()
    c = _np(r["counts"])
    d = dict(counts=c, tgt_status=_np(r["tgt_status"]), tgt_parent=_np(r["tgt_parent"]), conn_off=_np(r["conn_off"])[:c[0] + 1], ord_off=_np(r["ord_off"])[:c[0] + 1],
             link_off=_np(r.get("link_off")))
    for k, i in UC_LISTS.items():
        d[k] = None if r.get(k) is None else _np(r[k])[:c[i]]
    _equal(d, exp, label, UC_KEYS)
    assert int(r["status"].item()) == 0, label


def _uc_with_points(pr, npts):
    """the problem with points nobody observes and no slot names appended, up to npts"""
    q = dict(pr)
    extra = npts - pr["npts"]
    assert extra >= 0
    q["npts"] = npts
    q["obs_off"] = np.concatenate([pr["obs_off"], np.full(extra, pr["obs_off"][-1], np.int32)])
    q["pt_bad"] = np.concatenate([pr["pt_bad"], np.zeros(extra, np.uint8)])
    return q


# --------------------------------------------------------------------------------------------- correct_loop and propagate_global_ba
ML_KEYS = ("kf_Tcw", "kf_center", "X", "corrected", "non_corrected", "pt_owner", "counts", "normal", "min_max", "nd_written")
GB_KEYS = ("kf_Tcw", "kf_gba_Tcw", "kf_in_gba", "kf_center", "X", "kf_bef_Tcw", "kf_reached", "pt_moved", "counts")


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _ml_presets(pr):
    n = pr["npts"]
    if pr["obs_off"] is None:
        return {}
    return dict(normal=np.full((n, 3), SENTINEL["float64"]), min_max=np.full((n, 2), SENTINEL["float32"], np.float32), nd_written=np.full(n, SENTINEL["uint8"], np.uint8))


def _ml_host(pr, label, exp=None):
    """the C entry itself, so that the tables and every output lie between guard bands"""
    from ceres_mono_orb_slam2_amd import _lib
    exp = npc.correct_loop(pr, **_ml_presets(pr)) if exp is None else exp
    nkf, nc, n, nd = pr["nkf"], len(pr["conn_kf"]), pr["npts"], pr["obs_off"] is not None
    G = Guarded()
    v = dict(kf_Tcw=G.new("kf_Tcw", (nkf, 12), np.float64, pr["kf_Tcw"]), kf_center=None if pr["kf_center"] is None else G.new("kf_center", (nkf, 3), np.float64, pr["kf_center"]),
             X=G.new("X", (n, 3), np.float64, pr["X"]), corrected=G.new("corrected", (nc, 7), np.float64), non_corrected=G.new("non_corrected", (nc, 7), np.float64),
             pt_owner=G.new("pt_owner", (n,), np.int32), counts=G.new("counts", (2,), np.int32), normal=None, min_max=None, nd_written=None)
    if nd:
        v.update(normal=G.new("normal", (n, 3), np.float64), min_max=G.new("min_max", (n, 2), np.float32), nd_written=G.new("nd_written", (n,), np.uint8))
    i = {k: (None if pr[k] is None else np.ascontiguousarray(pr[k])) for k in ("conn_kf", "conn_rank", "Scw", "slot_off", "slot_pt", "pt_bad", "pt_done", "obs_off", "obs_kf",
                                                                              "ref_kf", "ref_level", "scale_factors")}
    rc = _lib.load().orbl_correct_loop(nkf, _ptr(v["kf_Tcw"]), _ptr(v["kf_center"]), nc, _ptr(i["conn_kf"]), _ptr(i["conn_rank"]), _ptr(i["Scw"]), _ptr(i["slot_off"]),
                                       _ptr(i["slot_pt"]), n, _ptr(v["X"]), _ptr(i["pt_bad"]), _ptr(i["pt_done"]), _ptr(i["obs_off"]), _ptr(i["obs_kf"]), _ptr(i["ref_kf"]),
                                       _ptr(i["ref_level"]), _ptr(i["scale_factors"]), len(i["scale_factors"]) if nd else 0, _ptr(v["corrected"]), _ptr(v["non_corrected"]),
                                       _ptr(v["pt_owner"]), _ptr(v["normal"]), _ptr(v["min_max"]), _ptr(v["nd_written"]), _ptr(v["counts"]))
    _lib.check(rc, "orbl_correct_loop")
    _equal(v, exp, label, ML_KEYS)
    G.check(label)
    return exp


def _ml_device(pr, exp, label):
    import torch
    from ceres_mono_orb_slam2_amd import loopclosing
    if pr["npts"] == 0 and pr["obs_off"] is not None:               # (tensors without elements have no pointer: the set cannot be given, and has nothing to say)
        pr = dict(pr, obs_off=None, obs_kf=None, ref_kf=None, ref_level=None, scale_factors=None)
        exp = dict(exp, normal=None, min_max=None, nd_written=None)
    kw = {k: _dev(a) for k, a in _ml_presets(pr).items()}
    r = loopclosing.correct_loop_device(_dev(pr["kf_Tcw"]), _dev(pr["conn_kf"]), _dev(pr["Scw"]), _dev(pr["slot_off"]), _dev(pr["slot_pt"]), _dev(pr["X"]),
                                        **{k: _dev(pr[k]) for k in ("kf_center", "conn_rank", "pt_bad", "pt_done", "obs_off", "obs_kf", "ref_kf", "ref_level", "scale_factors")}, **kw)
    torch.cuda.synchronize()
    e = dict(exp)
    if e["nd_written"] is not None:                                  # (the device form writes nd_written of every point: 0 where it did not move)
        e["nd_written"] = np.where(e["pt_owner"] >= 0, e["nd_written"], 0).astype(np.uint8)
    _equal({k: _np(r.get(k)) for k in ML_KEYS}, e, label, ML_KEYS)
    assert int(r["status"].item()) == 0, label


def _gb_host(pr, label, exp=None):
    from ceres_mono_orb_slam2_amd import _lib
    nkf, n = pr["nkf"], pr["npts"]
    exp = npc.propagate_global_ba(pr, kf_bef_Tcw=np.full((nkf, 12), SENTINEL["float64"])) if exp is None else exp
    G = Guarded()
    v = dict(kf_Tcw=G.new("kf_Tcw", (nkf, 12), np.float64, pr["kf_Tcw"]), kf_gba_Tcw=G.new("kf_gba_Tcw", (nkf, 12), np.float64, pr["kf_gba_Tcw"]),
             kf_in_gba=G.new("kf_in_gba", (nkf,), np.uint8, pr["kf_in_gba"]), kf_center=None if pr["kf_center"] is None else G.new("kf_center", (nkf, 3), np.float64, pr["kf_center"]),
             X=G.new("X", (n, 3), np.float64, pr["X"]), kf_bef_Tcw=G.new("kf_bef_Tcw", (nkf, 12), np.float64), kf_reached=G.new("kf_reached", (nkf,), np.uint8),
             pt_moved=G.new("pt_moved", (n,), np.uint8), counts=G.new("counts", (4,), np.int32))
    i = {k: (None if pr[k] is None else np.ascontiguousarray(pr[k])) for k in ("kf_parent", "origin_kf", "pt_bad", "pt_in_gba", "pt_gba_X", "pt_ref_kf")}
    rc = _lib.load().orbl_propagate_global_ba(nkf, _ptr(v["kf_Tcw"]), _ptr(v["kf_gba_Tcw"]), _ptr(v["kf_in_gba"]), _ptr(i["kf_parent"]), len(i["origin_kf"]), _ptr(i["origin_kf"]),
                                              _ptr(v["kf_center"]), n, _ptr(v["X"]), _ptr(i["pt_bad"]), _ptr(i["pt_in_gba"]), _ptr(i["pt_gba_X"]), _ptr(i["pt_ref_kf"]),
                                              _ptr(v["kf_bef_Tcw"]), _ptr(v["kf_reached"]), _ptr(v["pt_moved"]), _ptr(v["counts"]))
    _lib.check(rc, "orbl_propagate_global_ba")
    _equal(v, exp, label, GB_KEYS)
    G.check(label)
    return exp


def _gb_device(pr, exp, label):
    import torch
    from ceres_mono_orb_slam2_amd import loopclosing
    r = loopclosing.propagate_global_ba_device(*[_dev(pr[k]) for k in ("kf_Tcw", "kf_gba_Tcw", "kf_in_gba", "kf_parent", "origin_kf", "X", "pt_ref_kf")],
                                               **{k: _dev(pr[k]) for k in ("kf_center", "pt_bad", "pt_in_gba", "pt_gba_X")},
                                               kf_bef_Tcw=_dev(np.full((pr["nkf"], 12), SENTINEL["float64"])))
    torch.cuda.synchronize()
    _equal({k: _np(r.get(k)) for k in GB_KEYS}, exp, label, GB_KEYS)
    assert int(r["status"].item()) == (loopclosing.GB_STALE if exp["counts"][3] else 0), label


# ------------------------------------------------------------------------------------- update_local_keyframes / update_local_points
LM_LISTS = ("mp_Xw", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_desc")
LM_WIDTH = dict(mp_Xw=3, mp_normal=3, mp_min_dist=1, mp_max_dist=1, mp_desc=32, mp_state=1, slot_Xw=3, slot_state=1)
LM_TYPE = dict(mp_Xw=np.float64, mp_normal=np.float64, mp_min_dist=np.float32, mp_max_dist=np.float32, mp_desc=np.uint8, mp_state=np.uint8, slot_Xw=np.float64,
               slot_state=np.uint8)


def _lm_host(pr, cap_kf, cap_pt, label):
    """the two host calls as the drop-in chains them (tests/test_gpu_local_map.py), every output between guard bands"""
    from ceres_mono_orb_slam2_amd import tracking
    exp = npl.update_local_map(pr, cap_pt=cap_pt)
    nkf, n_kp = len(pr["kf_bad"]), len(pr["frame_pt"])
    G = Guarded()
    o1 = dict(frame_pt_out=G.new("frame_pt_out", (n_kp,), np.int32), local_kf=G.new("local_kf", (cap_kf,), np.int32), votes=G.new("votes", (nkf,), np.int32))
    a = tracking.update_local_keyframes(pr["frame_pt"], pr["pt_bad"], pr["obs_off"], pr["obs_kf"], pr["kf_bad"], pr["kf_rank"], pr["kf_parent"], pr["cov_off"], pr["cov_kf"],
                                        pr["child_off"], pr["child_kf"], pr["prev_local_kf"], cap_kf=cap_kf, out=o1)
    for k in ("n_local_kf", "ref_kf", "status"):
        assert a[k] == exp[k], (label, k)
    _equal(a, exp, label, ("frame_pt_out", "local_kf", "votes"))
    assert (o1["local_kf"][exp["n_local_kf"]:] == SENTINEL["int32"]).all(), (label, "local_kf behind the count")
    rows = [pr["kf_slot_pt"][pr["kf_slot_off"][k]:pr["kf_slot_off"][k + 1]] for k in a["local_kf"]]
    off, val = lmc._csr(rows)
    o2 = dict(local_pt=G.new("local_pt", (cap_pt,), np.int32))
    o2.update({k: G.new(k, ((n_kp if k.startswith("slot") else cap_pt) * w,), LM_TYPE[k]) for k, w in LM_WIDTH.items()})
    b = tracking.update_local_points(off, val, pr["pt_bad"], pr["pt_nobs"], pr["pt_Xw"], pr["pt_normal"], pr["pt_min_dist"], pr["pt_max_dist"], pr["pt_desc"],
                                     a["frame_pt_out"], pr["seen_pt"], cap_pt, out=o2)
    n = exp["n_local_pt"]
    assert b["n_local_pt"] == n, label
    _equal(dict(local_pt=b["local_pt"], mp_state=o2["mp_state"], slot_state=o2["slot_state"], slot_Xw=o2["slot_Xw"]), exp, label, ("local_pt", "mp_state", "slot_state", "slot_Xw"))
    assert (o2["local_pt"][n:] == SENTINEL["int32"]).all(), (label, "local_pt behind the count")
    for k in LM_LISTS:                                              # the packed rows up to the count, the caller's bytes behind it
        g = o2[k].reshape(cap_pt, LM_WIDTH[k])
        assert np.array_equal(_bits(g[:n]), _bits(np.asarray(exp[k]).reshape(n, LM_WIDTH[k]))), (label, k)
        assert (g[n:] == SENTINEL[g.dtype.name]).all(), (label, k, "rows behind the count were written")
    G.check(label)
    return exp


def _lm_device(pr, cap_kf, cap_pt, exp, label):
    import torch
    from ceres_mono_orb_slam2_amd import tracking
    packed = len(pr["frame_pt"]) > 0                                # (tensors without elements have no pointer, and the packed outputs are given all or none)
    d = tracking.update_local_map_device({k: _dev(v) for k, v in pr.items()}, cap_kf, cap_pt, packed=packed)
    torch.cuda.synchronize()
    c = _np(d["counts"])
    assert [int(x) for x in c] == [exp["n_local_kf"], exp["ref_kf"], exp["n_local_pt"], exp["status"]] and int(d["status"].item()) == 0, label
    n = exp["n_local_pt"]
    got = dict(frame_pt_out=_np(d["frame_pt_out"]), local_kf=_np(d["local_kf"])[:c[0]], votes=_np(d["votes"]), local_pt=_np(d["local_pt"])[:n])
    if packed:
        got.update(mp_state=_np(d["mp_state"]), slot_state=_np(d["slot_state"]), slot_Xw=_np(d["slot_Xw"]))
    _equal(got, exp, label, tuple(got))
    for k in LM_LISTS if packed else ():
        assert np.array_equal(_bits(_np(d[k]).reshape(cap_pt, LM_WIDTH[k])[:n]), _bits(np.asarray(exp[k]).reshape(n, LM_WIDTH[k]))), (label, k)


def _lm_caps(pr, slack=3):
    exp = npl.update_local_map(pr)
    return max(exp["n_local_kf"], len(pr["prev_local_kf"])) + slack, exp["n_local_pt"] + slack


# ================================================================================================================ 1. empty and minimal
def test_update_map_points_without_points_and_without_observations():
    from ceres_mono_orb_slam2_amd import localmapping
    # no point: the call returns before any device work, host and device form alike
    b = npm.make_batch(5, [], nkf=NKF)
    exp = _mp_host(b, BOTH, "npts 0")
    _mp_device(b, BOTH, exp, "npts 0 device")
    assert all(v.size == 0 for v in exp.values())
    # points without a single observation: the descriptor and observer pieces are empty, every point is left alone
    b = npm.make_batch(6, [0, 0, 0], nkf=NKF)
    for what in (BOTH, npm.DESC, npm.NORMAL_DEPTH):
        exp = _mp_host(b, what, "nobs 0")
        _mp_device(b, what, exp, "nobs 0 device")
    # no optional array at all
    b = npm.make_batch(7, [3, 0, 70, 1], nkf=NKF)
    b["pt_good"] = None; b["obs_kf_good"] = None
    exp = _mp_host(b, BOTH, "no flags")
    _mp_device(b, BOTH, exp, "no flags device")
    assert localmapping.MP_DESC == npm.DESC


def test_keyframe_culling_without_candidates_and_without_points():
    obs = [[(0, 0), (1, 0), (2, 0), (3, 0)]] * 4
    slots = [[(p, 0) for p in range(4)] for _ in range(5)]
    for label, pr in (("ncand 0", kcc.flatten(5, obs, slots, [], [])),                       # the map state comes back as it went in
                      ("ncand 0, npts 0", kcc.flatten(5, [], slots, [], [])),                # an empty result block
                      ("npts 0", kcc.flatten(5, [], [[] for _ in range(5)], [1, 3], [0, 2])),      # candidates that hold nothing
                      ("no flags", kcc.flatten(5, obs, slots, [0, 1], [0, 0]))):
        exp = npk.culling(pr)
        if label == "no flags":                                     # (NULL stands for all zero, which is what the restatement was given)
            pr = dict(pr, cand_flags=None)
        _kc_host(pr, label, exp)
        _kc_device(pr, exp, label + " device")
    # the three state outputs not asked for and no candidate: nothing comes back at all
    from ceres_mono_orb_slam2_amd import localmapping
    pr = kcc.flatten(5, obs, slots, [], [])
    r = localmapping.keyframe_culling(pr["cand_kf"], pr["cand_flags"], pr["slot_off"], pr["slot_pt"], pr["slot_level"], pr["nkf"], pr["obs_off"], pr["obs_kf"],
                                      pr["obs_level"], final_state=False)
    assert r.culled.size == 0 and r.pt_bad is None


def test_update_connections_without_targets_points_or_tables():
    full = ucc.make(3, nkf=NKF, sparse=False, per_kf=12)
    obs = [full["obs_kf"][full["obs_off"][p]:full["obs_off"][p + 1]].tolist() for p in range(full["npts"])]
    conn = [{1: 3}, {0: 3, 2: 1}, {1: 1}] + [{} for _ in range(NKF - 3)]
    cases = (("ntgt 0", ucc.flatten(NKF, obs, [], [], conn=conn, prev=[], pt_bad=[0] * len(obs))),
             ("ntgt 0, no links", ucc.flatten(NKF, obs, [], [], conn=conn, pt_bad=[0] * len(obs))),
             ("npts 0", ucc.flatten(NKF, [], [2, 0], [[-1, -1], []], conn=conn, prev=[[1], []], flags=[1, 0])),
             ("nothing at entry", ucc.flatten(NKF, obs, [0, 1], [[0, 1, 2], [0, 1]], prev=[[], []], th=1)),
             ("nkf 0", ucc.flatten(0, [], [], [], prev=[])))
    for label, pr in cases:
        exp = _uc_host(pr, label)
        _uc_device(pr, exp, label + " device")


def test_correct_loop_without_points_and_without_observations():
    T = [mcc._pose((0.5, -1.0, 2.0))]
    Scw = [0.0, 0.0, 0.0, 1.0, 0.25, 0.0, -0.5]
    cases = (("nkf 1, nconn 1, npts 0, normals asked for", mcc.loop_problem(T, [0], Scw, [[]], np.zeros((0, 3)), obs=[], ref_kf=[], ref_level=[])),
             ("nkf 1, nconn 1, npts 0", mcc.loop_problem(T, [0], Scw, [[]], np.zeros((0, 3)))),
             ("npts 1, nobs 0, normals asked for", mcc.loop_problem(T, [0], Scw, [[0]], [[1.0, 2.0, 3.0]], obs=[[]], ref_kf=[0], ref_level=[0])),
             ("no slot", mcc.loop_problem(T, [0], Scw, [[]], [[1.0, 2.0, 3.0]], obs=[[0]], ref_kf=[0], ref_level=[1], pt_bad=[0], pt_done=[0])),
             ("no centres", mcc.loop_problem(T, [0], Scw, [[0]], [[1.0, 2.0, 3.0]], centres=False)))
    for label, pr in cases:
        exp = _ml_host(pr, label)
        _ml_device(pr, exp, label + " device")
    assert exp["pt_owner"].tolist() == [0]


def test_propagate_global_ba_without_keyframes_and_without_origins():
    T = [mcc._pose((float(k), 0.0, 0.0)) for k in range(3)]
    G = [mcc._pose((float(k), 10.0, 0.0)) for k in range(3)]
    none = np.zeros((0, 12))
    cases = (("nkf 0, npts 0", mcc.gba_problem(none, none, [], [], [], np.zeros((0, 3)), [])),
             ("nkf 0, points of the BA", mcc.gba_problem(none, none, [], [], [], [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], [0, 0], pt_bad=[0, 1], pt_in_gba=[1, 1],
                                                         pt_gba_X=[[9.0, 9.0, 9.0], [8.0, 8.0, 8.0]])),
             ("n_origin 0", mcc.gba_problem(T, G, [1, 1, 0], [-1, 0, 1], [], [[1.0, 2.0, 3.0]], [1])),
             ("npts 0", mcc.gba_problem(T, G, [1, 1, 0], [-1, 0, 1], [0], np.zeros((0, 3)), [], centres=False)))
    for label, pr in cases:
        exp = _gb_host(pr, label)
        _gb_device(pr, exp, label + " device")
    assert exp["counts"].tolist() == [3, 1, 0, 0]


def test_update_local_map_pair_without_keypoints_points_or_keyframes():
    chain = dict(cov={0: [1], 1: [0, 2], 2: [1]}, children={0: [1], 1: [2]}, parent={1: 0, 2: 1})
    cases = (("n_kp 0, the previous list stays", lmc.build(3, [[0, 1], [1, 2], [2, 3]], [], prev=[2, 0], seen=[1], **chain)),
             ("n_kp 0, no previous list", lmc.build(3, [[0, 1], [1, 2], [2, 3]], [], **chain)),
             ("empty slot tables", lmc.build(3, [[], [], []], [0, 1], obs=[[0], [0, 1]], npts=2, **chain)),
             ("npts 0", lmc.build(3, [[], [-1], []], [-1, -1], npts=0, prev=[1], **chain)),
             ("nkf 0", lmc.build(0, [], [-1], npts=0)))
    for label, pr in cases:
        cap_kf, cap_pt = _lm_caps(pr)
        exp = _lm_host(pr, cap_kf, cap_pt, label)
        _lm_device(pr, cap_kf, cap_pt, exp, label + " device")


# ===================================================================================================== 2. sizes across a piece boundary
@pytest.mark.parametrize("npts", SIZES)
def test_pieces_that_end_around_a_256_byte_boundary(npts):
    rng = np.random.default_rng(npts)
    label = "npts %d" % npts
    b = npm.make_batch(npts, rng.integers(0, 9, npts), nkf=NKF, bad_pt_frac=0.05)
    for what in (BOTH, npm.DESC, npm.NORMAL_DEPTH):
        _mp_host(b, what, "map points, " + label)
    exp = _kc_host(kcc.make(npts, nkf=NKF, npts=npts, span=4, q=0.9), "culling, " + label)
    assert exp["culled"].size == NKF - 1
    pr = _uc_with_points(ucc.make(npts, nkf=NKF, sparse=False, per_kf=60), npts)
    assert pr["npts"] == npts and len(pr["pt_bad"]) == npts
    _uc_host(pr, "connections, " + label)
    exp = _ml_host(mcc.make_loop(npts, nconn=5, npts=npts, nkf=NKF, max_slots=120), "correct loop, " + label)
    assert exp["counts"][0] > 0 and 0 < exp["nd_written"][exp["pt_owner"] >= 0].sum() and (exp["pt_owner"] < 0).any()
    exp = _gb_host(mcc.make_gba(npts, NKF, npts=npts), "global BA, " + label)
    assert 0 < exp["kf_reached"].sum() and (exp["pt_moved"] == 0).any() and (exp["pt_moved"] != 0).any()
    pr = lmc.make(npts, nkf=NKF, npts=npts, n_kp=npts)
    exp = _lm_host(pr, NKF, npts, "local map, " + label)              # (cap_pt = npts: mp_state is a uint8 per row of the capacity)
    assert 0 < exp["n_local_pt"] < npts


# ============================================================================================================== 3. a warm second call
def test_a_smaller_call_after_a_larger_one_on_the_same_thread():
    for size, nkf, label in ((900, 40, "larger"), (70, 9, "smaller")):
        rng = np.random.default_rng(size)
        b = npm.make_batch(size, rng.integers(0, 12, size), nkf=nkf, bad_pt_frac=0.05)
        _mp_host(b, BOTH, "map points, " + label)
        _kc_host(kcc.make(size, nkf=nkf, npts=size, span=4, q=0.9), "culling, " + label)
        _uc_host(ucc.make(size, nkf=nkf, per_kf=size // 20), "connections, " + label)
        _ml_host(mcc.make_loop(size, nconn=nkf // 2, npts=size, nkf=nkf, max_slots=100), "correct loop, " + label)
        _gb_host(mcc.make_gba(size, nkf, npts=size), "global BA, " + label)
        pr = lmc.make(size, nkf=nkf, npts=size, n_kp=size // 3)
        cap_kf, cap_pt = _lm_caps(pr)
        _lm_host(pr, cap_kf, cap_pt, "local map, " + label)
