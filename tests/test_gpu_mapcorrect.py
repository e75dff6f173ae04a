"""orbl_correct_loop(_device) and orbl_propagate_global_ba(_device) on the MI355X against the restatement tests/npmapcorrect.py (the literal
loops of src/LoopClosing.cc:446-523 and :681-739): every output is compared bit for bit, as uint8 views - the arithmetic is IEEE +, *, /
and sqrt in a stated order, without fused multiply-add, which tests/test_gpu_mappoints.py already holds the normal and depth to.  Rows a
call must leave alone are poisoned first.  tests/test_mapcorrect_restatement.py shows that the problems tell the loops' order dependence
from an order-blind implementation."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import mapcorrectcases as mc  # noqa: E402
from tests import npmapcorrect as npm  # noqa: E402

pytestmark = pytest.mark.gpu

ML_KEYS = ("kf_Tcw", "kf_center", "X", "corrected", "non_corrected", "pt_owner", "counts", "normal", "min_max", "nd_written")
GB_KEYS = ("kf_Tcw", "kf_gba_Tcw", "kf_in_gba", "kf_center", "X", "kf_bef_Tcw", "kf_reached", "pt_moved", "counts")
HAND_LOOP = mc.hand_loop_cases()
HAND_GBA = mc.hand_gba_cases()
_SEEDED = {}


def _poison_loop(pr):
    n = pr["npts"]
    return dict(normal=np.full((n, 3), mc.POISON), min_max=np.full((n, 2), mc.POISON, np.float32), nd_written=np.full(n, 77, np.uint8))


def _expect_loop(pr):
    return npm.correct_loop(pr, **(_poison_loop(pr) if pr["obs_off"] is not None else {}))


def _expect_gba(pr):
    return npm.propagate_global_ba(pr, kf_bef_Tcw=np.full((pr["nkf"], 12), mc.POISON))


def _seeded(kind):
    """every seeded problem with its restated outputs, computed once and shared"""
    if kind not in _SEEDED:
        _SEEDED[kind] = [(name, pr, (_expect_loop if kind == "loop" else _expect_gba)(pr)) for name, pr in (mc.seeded_loop() if kind == "loop" else mc.seeded_gba())]
        for _, pr, exp in _SEEDED[kind]:
            for v in list(pr.values()) + list(exp.values()):
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _SEEDED[kind]


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _same(got, exp, what, keys):
    for k in keys:
        if exp[k] is None:
            assert got[k] is None, (what, k)
            continue
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.dtype == e.dtype and g.size == e.size, (what, k, g.dtype, e.dtype)
        if not np.array_equal(_bits(g), _bits(e)):
            bad = np.nonzero(g.reshape(-1) != e.reshape(-1))[0]
            raise AssertionError((what, k, "first differences at", bad[:5].tolist(), g.reshape(-1)[bad[:5]].tolist(), e.reshape(-1)[bad[:5]].tolist()))


def _t(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).cuda()              # (a copy: the shared problems are read-only)


def _loop_host(pr):
    from ceres_mono_orb_slam2_amd import loopclosing
    kw = _poison_loop(pr) if pr["obs_off"] is not None else {}
    return loopclosing.correct_loop(pr["kf_Tcw"], pr["conn_kf"], pr["Scw"], pr["slot_off"], pr["slot_pt"], pr["X"], kf_center=pr["kf_center"], conn_rank=pr["conn_rank"],
                                    pt_bad=pr["pt_bad"], pt_done=pr["pt_done"], obs_off=pr["obs_off"], obs_kf=pr["obs_kf"], ref_kf=pr["ref_kf"], ref_level=pr["ref_level"],
                                    scale_factors=pr["scale_factors"], **kw)


def _loop_device_enqueue(pr, tables=None):
    """tables: device tensors (kf_Tcw, kf_center, X) that replace the problem's - what an earlier call on the stream left"""
    from ceres_mono_orb_slam2_amd import loopclosing
    nd = pr["obs_off"] is not None
    kw = {k: _t(v) for k, v in _poison_loop(pr).items()} if nd else {}
    T, Cn, X = tables if tables is not None else (_t(pr["kf_Tcw"]), _t(pr["kf_center"]), _t(pr["X"]))
    return loopclosing.correct_loop(T, _t(pr["conn_kf"]), _t(pr["Scw"]), _t(pr["slot_off"]), _t(pr["slot_pt"]), X, kf_center=Cn, conn_rank=_t(pr["conn_rank"]),
                                    pt_bad=_t(pr["pt_bad"]), pt_done=_t(pr["pt_done"]), obs_off=_t(pr["obs_off"]), obs_kf=_t(pr["obs_kf"]), ref_kf=_t(pr["ref_kf"]),
                                    ref_level=_t(pr["ref_level"]), scale_factors=_t(pr["scale_factors"]), device=True, **kw)


def _down(r, keys, shapes):
    import torch
    torch.cuda.synchronize()
    o = {k: (None if r.get(k) is None else r[k].cpu().numpy()) for k in keys}
    o["status"] = int(r["status"].item()) & 0xFFFFFFFF
    for k, s in shapes.items():
        if o.get(k) is not None:
            o[k] = o[k].reshape(s)
    return o


def _loop_device(pr):
    return _down(_loop_device_enqueue(pr), ML_KEYS, dict(kf_Tcw=(-1, 12), kf_center=(-1, 3), X=(-1, 3), corrected=(-1, 7), non_corrected=(-1, 7), normal=(-1, 3), min_max=(-1, 2)))


def _device_view(exp):
    """what the device form writes where the host form leaves the caller's bytes: nd_written of every point (0 where it did not move)"""
    e = dict(exp)
    if e["nd_written"] is not None:
        e["nd_written"] = np.where(e["pt_owner"] >= 0, e["nd_written"], 0).astype(np.uint8)
    return e


def _loop_both(pr, what, exp=None):
    exp = _expect_loop(pr) if exp is None else exp
    h, d = _loop_host(pr), _loop_device(pr)
    _same(h, exp, what + " host", ML_KEYS)
    _same(d, _device_view(exp), what + " device", ML_KEYS)
    assert d["status"] == 0, what
    return exp


def _gba_args(pr, conv):
    a = [conv(pr[k]) for k in ("kf_Tcw", "kf_gba_Tcw", "kf_in_gba", "kf_parent", "origin_kf", "X", "pt_ref_kf")]
    kw = {k: conv(pr[k]) for k in ("kf_center", "pt_bad", "pt_in_gba", "pt_gba_X")}
    return a, kw


def _gba_host(pr):
    from ceres_mono_orb_slam2_amd import loopclosing
    a, kw = _gba_args(pr, lambda v: v)
    return loopclosing.propagate_global_ba(*a, kf_bef_Tcw=np.full((pr["nkf"], 12), mc.POISON), **kw)


def _gba_device_enqueue(pr):
    from ceres_mono_orb_slam2_amd import loopclosing
    a, kw = _gba_args(pr, _t)
    return loopclosing.propagate_global_ba(*a, kf_bef_Tcw=_t(np.full((pr["nkf"], 12), mc.POISON)), device=True, **kw)


GB_SHAPES = dict(kf_Tcw=(-1, 12), kf_gba_Tcw=(-1, 12), kf_center=(-1, 3), X=(-1, 3), kf_bef_Tcw=(-1, 12))


def _gba_both(pr, what, exp=None):
    exp = _expect_gba(pr) if exp is None else exp
    h, d = _gba_host(pr), _down(_gba_device_enqueue(pr), GB_KEYS, GB_SHAPES)
    _same(h, exp, what + " host", GB_KEYS)
    _same(d, exp, what + " device", GB_KEYS)
    from ceres_mono_orb_slam2_amd import loopclosing
    assert d["status"] == (loopclosing.GB_STALE if exp["counts"][3] else 0), what
    return exp


@pytest.mark.parametrize("name", sorted(HAND_LOOP))
def test_correct_loop_hand_cases_host_and_device(name):
    pr, hand = HAND_LOOP[name]
    exp = _loop_both(pr, name)
    assert exp["pt_owner"].tolist() == hand["pt_owner"].tolist() and exp["counts"].tolist() == hand["counts"]


def test_correct_loop_seeded_host_and_device_equal_the_restatement():
    for name, pr, exp in _seeded("loop"):
        _loop_both(pr, name, exp)


def test_correct_loop_without_the_optional_arguments():
    pr = dict(mc.make_loop(31, nconn=7, npts=300))
    pr.update(conn_rank=None, pt_bad=None, pt_done=None, obs_off=None, obs_kf=None, ref_kf=None, ref_level=None, scale_factors=None)
    _loop_both(pr, "no rank, flags or normals")
    pr["kf_center"] = None
    _loop_both(pr, "no centres either")


@pytest.mark.parametrize("name", sorted(HAND_GBA))
def test_propagate_global_ba_hand_cases_host_and_device(name):
    pr, hand = HAND_GBA[name]
    exp = _gba_both(pr, name)
    assert exp["counts"].tolist() == hand["counts"] and exp["kf_reached"].tolist() == hand["kf_reached"]


def test_propagate_global_ba_seeded_host_and_device_equal_the_restatement():
    for name, pr, exp in _seeded("gba"):
        _gba_both(pr, name, exp)


def test_propagate_global_ba_without_the_optional_arguments_and_with_a_cycle():
    from ceres_mono_orb_slam2_amd import loopclosing
    pr = dict(mc.make_gba(41, 70))
    pr.update(kf_center=None, pt_bad=None, pt_in_gba=None, pt_gba_X=None)
    _gba_both(pr, "no centres, flags or BA positions")
    # a cycle: two keyframes that are each other's parent, and a third hanging on them, are not reached (the device form says so)
    pr = dict(mc.make_gba(42, 70))
    par = pr["kf_parent"].copy()
    loose = [int(k) for k in np.nonzero(par >= 0)[0] if not np.any(par == k)][:3]                # (three leaves)
    par[loose[0]] = loose[1]; par[loose[1]] = loose[0]; par[loose[2]] = loose[0]
    pr["kf_parent"] = par
    exp = _expect_gba(pr)
    assert exp["kf_reached"][loose].tolist() == [0, 0, 0]
    h, d = _gba_host(pr), _down(_gba_device_enqueue(pr), GB_KEYS, GB_SHAPES)
    _same(h, exp, "cycle host", GB_KEYS)
    _same(d, exp, "cycle device", GB_KEYS)
    assert d["status"] & loopclosing.GB_CYCLE


def _drop_connected(pr, c):
    """the problem without the connected keyframe at list position c (the relative rank order of the others is kept)"""
    q = dict(pr)
    keep = [i for i in range(len(pr["conn_kf"])) if i != c]
    q["conn_kf"] = pr["conn_kf"][keep]
    q["conn_rank"] = np.argsort(np.argsort(pr["conn_rank"][keep])).astype(np.int32)
    rows = [pr["slot_pt"][pr["slot_off"][i]:pr["slot_off"][i + 1]].tolist() for i in keep]
    q["slot_off"], q["slot_pt"] = mc._csr(rows)
    return q, keep


def test_correct_loop_device_status_bits_and_absent_entries():
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    pr = mc.make_loop(51, nconn=9, npts=400)
    base = _device_view(_expect_loop(pr))
    nkf, npts, nconn = pr["nkf"], pr["npts"], len(pr["conn_kf"])
    moved = [p for p in range(npts) if base["pt_owner"][p] >= 0 and base["nd_written"][p]]

    def run(**changes):
        q = dict(pr)
        for k, (at, v) in changes.items():
            q[k] = pr[k].copy(); q[k][at] = v
        return _loop_device(q)

    def without_normal(p):
        e = dict(base)
        e["normal"] = base["normal"].copy(); e["normal"][p] = mc.POISON
        e["min_max"] = base["min_max"].copy(); e["min_max"][p] = mc.POISON
        e["nd_written"] = base["nd_written"].copy(); e["nd_written"][p] = 0
        return e
    # a slot naming a point out of range is an empty slot
    s = int(np.nonzero(pr["slot_pt"] >= 0)[0][5])
    q = dict(pr); q["slot_pt"] = pr["slot_pt"].copy(); q["slot_pt"][s] = -1
    for v in (npts, -2, 2 ** 30):
        d = run(slot_pt=(s, v))
        assert d["status"] == lc.ML_PT
        _same(d, _device_view(_expect_loop(q)), "slot point %d" % v, ML_KEYS)
    # an observer, a reference keyframe or a level out of range: that point is moved but gets no normal
    p = moved[3]
    for key, at, v, bit in (("obs_kf", int(pr["obs_off"][p]), nkf, lc.ML_KF), ("obs_kf", int(pr["obs_off"][p + 1]) - 1, -1, lc.ML_KF), ("ref_kf", p, nkf + 7, lc.ML_KF),
                            ("ref_kf", p, -1, lc.ML_KF), ("ref_level", p, 8, lc.ML_LEVEL), ("ref_level", p, -1, lc.ML_LEVEL)):
        d = run(**{key: (at, v)})
        assert d["status"] == bit, (key, v)
        _same(d, without_normal(p), "%s %d" % (key, v), ML_KEYS)
    # a connected keyframe out of range is not in the group: zeros in its two Sim3 rows
    c = 2
    q, keep = _drop_connected(pr, c)
    e = _device_view(_expect_loop(q))
    for k in ("corrected", "non_corrected"):
        full = np.zeros((nconn, 7)); full[keep] = e[k]; e[k] = full
    for v in (nkf, -1):
        d = run(conn_kf=(c, v))
        assert d["status"] == lc.ML_KF
        _same(d, e, "connected keyframe %d" % v, ML_KEYS)
    # the last row's end beyond nslots: the current keyframe's slots are not there
    last = nconn - 1
    rows = [pr["slot_pt"][pr["slot_off"][i]:pr["slot_off"][i + 1]].tolist() for i in range(nconn)]
    q = dict(pr); q["slot_off"], q["slot_pt"] = mc._csr(rows[:last] + [[]])
    d = run(slot_off=(nconn, len(pr["slot_pt"]) + 3))
    assert d["status"] == lc.ML_OFFSETS
    e = _device_view(_expect_loop(q))
    _same(d, e, "slot_off", ML_KEYS)
    # a rank that repeats: the bit is set; list position breaks the tie, so the owners are decided all the same
    holder = np.argsort(pr["conn_rank"])
    r = next(r for r in range(nconn - 1) if holder[r] < holder[r + 1])
    d = run(conn_rank=(holder[r + 1], r))
    assert d["status"] == lc.ML_RANK
    _same(d, base, "rank repeats", ("kf_Tcw", "kf_center", "X", "corrected", "non_corrected", "pt_owner", "counts"))
    d = run(conn_rank=(0, nconn))
    assert d["status"] & lc.ML_RANK
    # an Scw that is not finite: the bit, nothing else is promised
    assert run(Scw=(2, np.nan))["status"] == lc.ML_SCW and run(Scw=(slice(0, 4), 0.0))["status"] == lc.ML_SCW


def test_propagate_global_ba_device_status_bits_and_absent_entries():
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    pr = mc.make_gba(61, 80)
    nkf = pr["nkf"]

    def run(q):
        return _down(_gba_device_enqueue(q), GB_KEYS, GB_SHAPES)
    stale = lc.GB_STALE if _expect_gba(pr)["counts"][3] else 0
    # an origin out of range is not an origin
    q = dict(pr); q["origin_kf"] = np.append(pr["origin_kf"], [nkf, -1]).astype(np.int32)
    d = run(q)
    assert d["status"] == lc.GB_KF | stale
    _same(d, _expect_gba(pr), "origin", GB_KEYS)
    # a parent out of range is no parent
    child = int(np.nonzero(pr["kf_parent"] >= 0)[0][7])
    e = dict(pr); e["kf_parent"] = pr["kf_parent"].copy(); e["kf_parent"][child] = -1
    exp = _expect_gba(e)
    for v in (nkf, -2):
        q = dict(pr); q["kf_parent"] = pr["kf_parent"].copy(); q["kf_parent"][child] = v
        d = run(q)
        assert d["status"] & lc.GB_KF and not d["status"] & lc.GB_CYCLE
        _same(d, exp, "parent %d" % v, GB_KEYS)
    # a reference keyframe out of range: the point stays
    base = _expect_gba(pr)
    p = int(np.nonzero(base["pt_moved"] == 2)[0][0])
    for v in (nkf, -1):
        q = dict(pr); q["pt_ref_kf"] = pr["pt_ref_kf"].copy(); q["pt_ref_kf"][p] = v
        d = run(q)
        assert d["status"] == lc.GB_KF | stale
        e = dict(base)
        e["X"] = base["X"].copy(); e["X"][p] = pr["X"][p]
        e["pt_moved"] = base["pt_moved"].copy(); e["pt_moved"][p] = 0
        e["counts"] = base["counts"].copy(); e["counts"][2] -= 1
        _same(d, e, "reference keyframe %d" % v, GB_KEYS)


def test_propagate_then_correct_loop_on_one_stream_without_synchronisation():
    import torch
    pg = mc.make_gba(71, 64, npts=400)
    pl = dict(mc.make_loop(72, nconn=10, npts=400, nkf=64))
    eg = _expect_gba(pg)
    pl.update(kf_Tcw=eg["kf_Tcw"], kf_center=eg["kf_center"], X=eg["X"])
    el = _device_view(_expect_loop(pl))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rg = _gba_device_enqueue(pg)
        rl = _loop_device_enqueue(pl, tables=(rg["kf_Tcw"], rg["kf_center"], rg["X"]))
    s.synchronize()
    d = _down(rl, ML_KEYS, dict(kf_Tcw=(-1, 12), kf_center=(-1, 3), X=(-1, 3), corrected=(-1, 7), non_corrected=(-1, 7), normal=(-1, 3), min_max=(-1, 2)))
    _same(d, el, "loop after propagation", ML_KEYS)
    g = _down(rg, ("kf_gba_Tcw", "kf_in_gba", "kf_bef_Tcw", "kf_reached", "pt_moved", "counts"), dict(kf_gba_Tcw=(-1, 12), kf_bef_Tcw=(-1, 12)))
    _same(g, eg, "propagation", ("kf_gba_Tcw", "kf_in_gba", "kf_bef_Tcw", "kf_reached", "pt_moved", "counts"))
