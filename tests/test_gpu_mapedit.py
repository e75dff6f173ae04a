"""orbl_apply_map_edits(_device) on the MI355X against the restatement tests/npmapedit.py (the literal sequential replay of
MapPoint::AddObservation / Replace / SetBadFlag over the edit list): every output is compared byte for byte, the lists trimmed to counts.
tests/test_mapedit_restatement.py shows that the problems take every path of the replay and tell it from an order-blind implementation."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import badflagcases as bc  # noqa: E402
from tests import mapeditcases as mc  # noqa: E402
from tests import npbadflag as npb  # noqa: E402
from tests import npculling  # noqa: E402
from tests import npmapedit as npm  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("op_status", "op_found", "pt_touched", "kf_slot_pt", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced", "oobs_off", "oobs_kf", "oobs_slot", "oobs_src",
        "oobs_level", "oobs_uv", "counts")
LISTS = ("oobs_kf", "oobs_slot", "oobs_src", "oobs_level", "oobs_uv")
INOUT = ("kf_slot_pt", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced")
HAND = mc.hand_cases()
POISON = -7777
ECAP = -4
_SEEDED = None


def _seeded():
    """every seeded problem with its restated outputs, computed once and shared"""
    global _SEEDED
    if _SEEDED is None:
        _SEEDED = [(name, pr, npm.apply_map_edits(pr)) for name, pr in mc.seeded().items()]
        for _, pr, exp in _SEEDED:
            for v in list(pr.values()) + list(exp.values()):
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _SEEDED


def _host(pr, **kw):
    from ceres_mono_orb_slam2_amd import localmapping
    r = localmapping.apply_map_edits({k: pr[k] for k in mc.OP_KEYS}, {k: pr.get(k) for k in mc.TABLES}, **kw)
    return {k: getattr(r, k) for k in r.__slots__}


def _t(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).cuda()             # (a copy: the shared problems are read-only)


def _device_raw(pr, **kw):
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    r = localmapping.apply_map_edits_device({k: _t(pr[k]) for k in mc.OP_KEYS}, {k: _t(pr.get(k)) for k in mc.TABLES}, **kw)
    torch.cuda.synchronize()
    return r


def _trim(r):
    """the device form's full-capacity tensors cut to the written count, as the host form returns them"""
    o = {k: (None if getattr(r, k) is None else getattr(r, k).cpu().numpy()) for k in KEYS}
    o["status"] = int(r.status.item()) & 0xFFFFFFFF
    n = int(o["counts"][0])
    for k in LISTS:
        if o[k] is not None:
            o[k] = o[k].reshape(-1, 2)[:n] if k == "oobs_uv" else o[k][:n]
    return o


def _device(pr, **kw):
    return _trim(_device_raw(pr, **kw))


def _same(got, exp, what, keys=KEYS):
    for k in keys:
        if exp[k] is None:
            assert got[k] is None, (what, k)
            continue
        g, e = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        assert g.dtype == e.dtype and g.shape == e.shape and g.tobytes() == e.tobytes(), (what, k, got[k], exp[k])


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_worked_cases_host_and_device(name):
    pr, exp = HAND[name]
    h, d = _host(pr), _device(pr)
    _same(h, exp, name + " host")
    _same(d, exp, name + " device")
    assert d["status"] == 0, name


def test_seeded_maps_host_and_device_equal_the_restatement():
    for name, pr, exp in _seeded():
        h, d = _host(pr), _device(pr)
        _same(h, exp, name + " host")
        _same(d, exp, name + " device")
        assert d["status"] == 0, name


def test_nullable_arguments_left_out():
    name, pr, _ = _seeded()[0]
    q = dict(pr, kf_rank=None, kf_slot_level=None, kf_slot_uv=None, pt_found=None, pt_visible=None, pt_replaced=None)
    exp = npm.apply_map_edits(q)
    _same(_host(q), exp, name + " host")
    _same(_device(q), exp, name + " device")


def test_two_runs_give_identical_bytes():
    name, pr, exp = _seeded()[-1]
    a, b = _device(pr), _device(pr)
    _same(a, b, name)
    _same(_host(pr), a, name)


def test_nothing_is_written_beyond_the_count():
    import torch
    name, pr, exp = _seeded()[1]
    cap = len(pr["obs_kf"]) + len(pr["op_kind"])
    n = int(exp["counts"][0])
    assert n < cap
    dt = dict(oobs_uv=torch.float32)
    out = {k: torch.full(((2 if k == "oobs_uv" else 1) * cap,), POISON, dtype=dt.get(k, torch.int32)).cuda() for k in LISTS}
    r = _device_raw(pr, out=out)
    _same(_trim(r), exp, name)
    for k in LISTS:
        v = out[k].cpu().numpy()
        assert (v[(2 if k == "oobs_uv" else 1) * n:] == POISON).all(), (name, k)
    hout = {k: np.full((2 if k == "oobs_uv" else 1) * cap, POISON, np.float32 if k == "oobs_uv" else np.int32) for k in LISTS}
    _same(_host(pr, out=hout), exp, name + " host")
    for k in LISTS:
        assert (hout[k][(2 if k == "oobs_uv" else 1) * n:] == POISON).all(), (name, k)


def test_capacity_one_short():
    import torch
    name, pr, exp = _seeded()[2]
    n = int(exp["counts"][0])
    out = {k: np.full((2 if k == "oobs_uv" else 1) * (n - 1), POISON, np.float32 if k == "oobs_uv" else np.int32) for k in LISTS}
    out["oobs_off"] = np.full(pr["npts"] + 1, POISON, np.int32)
    h = _host(pr, cap_obs=n - 1, out=out, check=False)
    assert h["rc"] == ECAP and np.array_equal(h["counts"], exp["counts"]), name
    assert all((v == POISON).all() for v in out.values()), name
    for k in INOUT:                                                  # the in/out tables are untouched
        assert np.array_equal(h[k], pr[k]), (name, k)
    # the device form: the bit, every element below the capacity, nothing beyond it
    big = {k: torch.full(((2 if k == "oobs_uv" else 1) * (n - 1 + 8),), POISON, dtype=torch.float32 if k == "oobs_uv" else torch.int32).cuda() for k in LISTS}
    r = _device_raw(pr, cap_obs=n - 1, out={k: v[:v.numel() - (16 if k == "oobs_uv" else 8)] for k, v in big.items()})
    assert int(r.status.item()) == npm.ST_CAP and np.array_equal(r.counts.cpu().numpy(), exp["counts"]), name
    for k, v in big.items():
        v = v.cpu().numpy()
        w = 2 if k == "oobs_uv" else 1
        assert (v[-8 * w:] == POISON).all() and np.array_equal(v[:-8 * w], np.ascontiguousarray(exp[k]).reshape(-1)[:len(v) - 8 * w]), (name, k)
    _same(_host(pr, cap_obs=n), exp, name + " exact capacity")


def test_an_out_of_range_op_is_absent_and_sets_its_bit():
    name, pr, exp = _seeded()[0]
    ops = mc.ops_of(pr)
    at = (3, 11, 20, 29, 35)
    extra = [(mc.ADD, pr["npts"], 0, 0, 0), (mc.FUSE, 1, 0, pr["nkf"], 0), (mc.FIND_OR_ADD, 1, 0, 0, int(pr["kf_slot_off"][1])), (9, 0, 0, 0, 0), (mc.REPLACE, 2, -1, 0, 0)]
    bad, shift = [], []
    for i, o in enumerate(ops):
        for a, x in zip(at, extra):
            if a == i:
                bad.append(x)
        shift.append(len(bad))
        bad.append(o)
    bad = [(k, p, shift[a] if k == mc.REPLACE_FOUND else a, kf, s) for k, p, a, kf, s in bad]      # (a REPLACE_FOUND keeps naming its FIND_OR_ADD)
    bad.append((mc.REPLACE_FOUND, 1, shift[at[0]] - 1, 0, 0))            # ... and this one names the ADD above: no FIND_OR_ADD
    q = mc.with_ops(pr, bad)
    want = npm.apply_map_edits(q)
    assert want["status"] == npm.ST_KF | npm.ST_PT | npm.ST_SLOT and (want["op_status"] == 10).sum() == 6
    d = _device(q)
    assert d["status"] == want["status"], name
    # the other ops are unaffected: only the numbers of the created observations move with the op indices
    keep = [i for i in range(len(bad)) if want["op_status"][i] != 10]
    assert np.array_equal(d["op_status"][keep], exp["op_status"]) and np.array_equal(d["op_found"][keep], exp["op_found"])
    _same(d, want, name)
    _same(d, exp, name, keys=("kf_slot_pt", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced", "pt_touched", "oobs_off", "oobs_kf", "oobs_slot", "oobs_level"))


def test_culling_enqueued_behind_the_edits_reads_their_tables():
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    seen = set()
    for name, pr, exp in _seeded():
        so, nkf = pr["kf_slot_off"], pr["nkf"]
        cand = np.arange(0, nkf, max(1, nkf // 8), dtype=np.int32)
        rows = [[s for s in range(so[k], so[k + 1]) if exp["kf_slot_pt"][s] >= 0] for k in cand]
        flat = np.array([s for r in rows for s in r], np.int64)
        cp = dict(nkf=nkf, npts=pr["npts"], cand_kf=cand, cand_flags=np.zeros(len(cand), np.uint8),
                  slot_off=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32), slot_pt=exp["kf_slot_pt"][flat].astype(np.int32),
                  slot_level=pr["kf_slot_level"][flat].astype(np.int32), obs_off=exp["oobs_off"], obs_kf=exp["oobs_kf"], obs_level=exp["oobs_level"],
                  pt_bad=exp["pt_bad"], pt_nobs=exp["pt_nobs"])
        want = npculling.culling(cp, th_obs=3, ratio=0.3)
        seen |= set(int(v) for v in want["culled"])
        args = [_t(cp[k]) for k in ("cand_kf", "cand_flags", "slot_off", "slot_pt", "slot_level")]
        # the culling checks every element of the arrays it is given, and nothing is written beyond n_obs_out: the tail is preset in range
        cap = len(pr["obs_kf"]) + len(pr["op_kind"])
        zeros = {k: torch.zeros(cap, dtype=torch.int32).cuda() for k in ("oobs_kf", "oobs_level")}
        r = localmapping.apply_map_edits_device({k: _t(pr[k]) for k in mc.OP_KEYS}, {k: _t(pr.get(k)) for k in mc.TABLES}, out=zeros)
        c = localmapping.keyframe_culling_device(*args, nkf, r.oobs_off, r.oobs_kf, r.oobs_level, pt_bad=r.pt_bad, pt_nobs=r.pt_nobs, th_obs=3, ratio=0.3)
        torch.cuda.synchronize()                                     # (enqueued on the same stream, nothing synchronised in between)
        n = int(exp["counts"][0])
        assert int(c.status.item()) == 0 and int(r.status.item()) == 0, name
        for k in ("culled", "n_redundant", "n_map_points", "pt_bad", "pt_nobs"):
            assert np.array_equal(getattr(c, k).cpu().numpy(), want[k]), (name, k)
        assert np.array_equal(c.obs_erased.cpu().numpy()[:n], want["obs_erased"]), name
    assert seen == {0, 1}


def test_obs_erased_of_set_bad_keyframes_as_obs_dead_equals_compacting_on_the_host():
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    pr = bc.make(3, nkf=40, ntgt=6)
    want = npb.set_bad_keyframes(pr)
    assert want["obs_erased"].any() and pr["kf_rank"] is not None
    tables = {k: _t(pr.get(k)) for k in ("kf_bad", "kf_parent", "kf_rank", "kf_Tcw", "child_off", "child_kf", "conn_off", "conn_kf", "conn_w", "ord_off", "ord_kf", "ord_w",
                                         "kf_slot_off", "kf_slot_pt", "pt_bad", "pt_nobs", "pt_ref_kf", "obs_off", "obs_kf", "obs_slot")}
    b = localmapping.set_bad_keyframes_device(_t(pr["tgt_kf"]), tables, tgt_flags=_t(pr["tgt_flags"]), tgt_mask=_t(pr["tgt_mask"]))
    empty = {k: torch.empty(0, dtype=torch.int32).cuda() for k in mc.OP_KEYS}
    r = localmapping.apply_map_edits_device(empty, dict(tables, obs_dead=b.obs_erased))          # (same stream, the tables the first call changed in place)
    torch.cuda.synchronize()
    d = _trim(r)
    assert d["status"] == 0 and np.array_equal(b.obs_erased.cpu().numpy(), want["obs_erased"])
    rank, off, okf, oslot, osrc = pr["kf_rank"], [0], [], [], []
    for p in range(pr["npts"]):                                      # compacting on the host
        es = [e for e in range(pr["obs_off"][p], pr["obs_off"][p + 1]) if not want["obs_erased"][e]]
        for e in sorted(es, key=lambda e: rank[pr["obs_kf"][e]]):
            okf.append(pr["obs_kf"][e]); oslot.append(pr["obs_slot"][e]); osrc.append(e)
        off.append(len(okf))
    exp = dict(oobs_off=np.array(off, np.int32), oobs_kf=np.array(okf, np.int32), oobs_slot=np.array(oslot, np.int32), oobs_src=np.array(osrc, np.int32),
               kf_slot_pt=want["kf_slot_pt"], pt_bad=want["pt_bad"], pt_nobs=want["pt_nobs"], counts=np.array([len(okf), 0, 0, 0, 0, 0, 0, 0], np.int32))
    _same(d, exp, "rebuild", keys=tuple(exp))
