"""orbl_set_bad_keyframes(_device) on the MI355X against the restatement tests/npbadflag.py (the literal sequential loop of
src/KeyFrame.cc:460-553): every output is compared byte for byte, tgt_Tcp included - it is the same FP64 operations in the same order.
tests/test_badflag_restatement.py shows that the problems take every path of the loop and tell it from an order-blind implementation."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import badflagcases as bc  # noqa: E402
from tests import npbadflag as npb  # noqa: E402
from tests import npculling  # noqa: E402

pytestmark = pytest.mark.gpu

KF_KEYS = ("tgt_status", "tgt_Tcp", "kf_bad", "kf_parent", "counts", "oconn_off", "oconn_kf", "oconn_w", "oord_off", "oord_kf", "oord_w", "ochild_off", "ochild_kf")
PT_KEYS = ("kf_slot_pt", "pt_bad", "pt_nobs", "pt_ref_kf", "obs_erased")
LISTS = dict(oconn_kf=1, oconn_w=1, oord_kf=2, oord_w=2, ochild_kf=3)           # output -> the entry of counts[] that is its length
TABLES = ("kf_bad", "kf_parent", "kf_rank", "kf_Tcw", "child_off", "child_kf", "conn_off", "conn_kf", "conn_w", "ord_off", "ord_kf", "ord_w", "kf_slot_off",
          "kf_slot_pt", "pt_bad", "pt_nobs", "pt_ref_kf", "obs_off", "obs_kf", "obs_slot")
HAND = bc.hand_cases()
POISON = -7777
ECAP = -4
_SEEDED = None


def _seeded():
    """every seeded problem with its restated outputs (with and without the point set), computed once and shared"""
    global _SEEDED
    if _SEEDED is None:
        _SEEDED = [(name, pr, npb.set_bad_keyframes(pr), npb.set_bad_keyframes(pr, points=False)) for name, pr in bc.seeded().items()]
        for _, pr, e1, e2 in _SEEDED:
            for v in list(pr.values()) + list(e1.values()) + list(e2.values()):
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _SEEDED


def _keys(pr):
    return KF_KEYS + (PT_KEYS if pr.get("kf_slot_off") is not None else ())


def _host(pr, **kw):
    from ceres_mono_orb_slam2_amd import localmapping
    r = localmapping.set_bad_keyframes(pr["tgt_kf"], {k: pr.get(k) for k in TABLES}, tgt_flags=pr["tgt_flags"], tgt_mask=pr["tgt_mask"], **kw)
    return {k: getattr(r, k) for k in r.__slots__}


def _device_raw(pr, mask=None, **kw):
    import torch
    from ceres_mono_orb_slam2_amd import localmapping

    def t(a):
        return None if a is None else torch.as_tensor(np.array(a)).cuda()          # (a copy: the shared problems are read-only)
    r = localmapping.set_bad_keyframes_device(t(pr["tgt_kf"]), {k: t(pr.get(k)) for k in TABLES}, tgt_flags=t(pr["tgt_flags"]),
                                              tgt_mask=t(pr["tgt_mask"]) if mask is None else mask, **kw)
    torch.cuda.synchronize()
    return r


def _trim(r):
    """the device form's full-capacity tensors cut to the written counts, as the host form returns them"""
    o = {k: (None if getattr(r, k) is None else getattr(r, k).cpu().numpy()) for k in KF_KEYS + PT_KEYS}
    o["status"] = int(r.status.item()) & 0xFFFFFFFF
    for k, i in LISTS.items():
        o[k] = o[k][:o["counts"][i]]
    return o


def _device(pr, **kw):
    return _trim(_device_raw(pr, **kw))


def _same(got, exp, what, keys):
    for k in keys:
        g, e = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        assert g.dtype == e.dtype and g.shape == e.shape and g.tobytes() == e.tobytes(), (what, k, got[k], exp[k])


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_worked_cases_host_and_device(name):
    pr, exp = HAND[name]
    exp = dict(exp, tgt_Tcp=npb.set_bad_keyframes(pr, points="kf_slot_off" in pr)["tgt_Tcp"])      # (the restated bytes: the hand values are equal, -0.0 aside)
    assert np.array_equal(exp["tgt_Tcp"], HAND[name][1]["tgt_Tcp"])
    h, d = _host(pr), _device(pr)
    _same(h, exp, name + " host", _keys(pr))
    _same(d, exp, name + " device", _keys(pr))
    assert d["status"] == 0, name


def test_seeded_maps_host_and_device_equal_the_restatement_with_and_without_points():
    for name, pr, exp, exp_np in _seeded():
        h, d = _host(pr), _device(pr)
        _same(h, exp, name + " host", _keys(pr))
        _same(d, exp, name + " device", _keys(pr))
        assert d["status"] == 0, name
        q = bc.without_points(pr)
        h, d = _host(q), _device(q)
        _same(h, exp_np, name + " host, no points", KF_KEYS)
        _same(d, exp_np, name + " device, no points", KF_KEYS)
        assert d["status"] == 0 and d["pt_bad"] is None, name


def test_two_runs_give_identical_bytes():
    name, pr, exp, _ = _seeded()[-1]
    a, b = _device(pr), _device(pr)
    _same(a, b, name, _keys(pr))
    _same(_host(pr), a, name, _keys(pr))


def _culling_problem(pr):
    """LocalMapping::KeyFrameCulling over the targets as its candidates: their non-null slots, every keypoint on level 0"""
    so = pr["kf_slot_off"]
    rows = [[int(p) for p in pr["kf_slot_pt"][so[k]:so[k + 1]] if p >= 0] for k in pr["tgt_kf"]]
    slot_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    slot_pt = np.array([p for r in rows for p in r], np.int32)
    flags = np.zeros(len(rows), np.uint8) if pr["tgt_flags"] is None else pr["tgt_flags"]
    return dict(nkf=pr["nkf"], npts=pr["npts"], cand_kf=pr["tgt_kf"], cand_flags=flags, slot_off=slot_off, slot_pt=slot_pt, slot_level=np.zeros(len(slot_pt), np.int32),
                obs_off=pr["obs_off"], obs_kf=pr["obs_kf"], obs_level=np.zeros(len(pr["obs_kf"]), np.int32), pt_bad=None, pt_nobs=pr["pt_nobs"])


def test_enqueued_behind_the_culling_with_its_mask_on_the_device():
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    seen = set()
    for name, pr, _, _ in _seeded()[3:6]:
        cp = _culling_problem(pr)
        culled = npculling.culling(cp, th_obs=3, ratio=0.65)["culled"]
        seen |= set(int(v) for v in culled)
        exp = npb.set_bad_keyframes(dict(pr, tgt_mask=culled))

        def t(a):
            return torch.as_tensor(np.array(a)).cuda()
        c = localmapping.keyframe_culling_device(t(cp["cand_kf"]), t(cp["cand_flags"]), t(cp["slot_off"]), t(cp["slot_pt"]), t(cp["slot_level"]), cp["nkf"], t(cp["obs_off"]),
                                                 t(cp["obs_kf"]), t(cp["obs_level"]), pt_nobs=t(cp["pt_nobs"]), th_obs=3, ratio=0.65, final_state=False)
        d = _trim(_device_raw(pr, mask=c.culled))                    # (enqueued on the same stream, nothing synchronised in between)
        assert np.array_equal(c.culled.cpu().numpy(), culled), name
        _same(d, exp, name, _keys(pr))
        assert d["status"] == 0, name
    assert seen == {0, 1}                                            # (both values of the mask were met)


def test_capacities_one_short():
    import torch
    name, pr, exp, _ = _seeded()[5]
    n_ord, n_child = int(exp["counts"][2]), int(exp["counts"][3])
    assert n_ord > 1 and n_child > 1
    for caps, bit in (((n_ord - 1, n_child), 16), ((n_ord, n_child - 1), 32)):
        out = {k: np.full(n, POISON, np.int32) for k, n in (("oord_kf", caps[0]), ("oord_w", caps[0]), ("ochild_kf", caps[1]), ("oconn_off", pr["nkf"] + 1))}
        h = _host(pr, caps=caps, out=out, check=False)
        assert h["rc"] == ECAP and np.array_equal(h["counts"], exp["counts"]), name
        assert all((v == POISON).all() for v in out.values()), name
        for k in ("kf_bad", "kf_parent") + PT_KEYS[:4]:
            assert np.array_equal(h[k], pr[k]), (name, k)
        assert not h["obs_erased"].any()
        # the device form: the bit, every element below the capacity, nothing beyond it
        big = {k: torch.full((n + 8,), POISON, dtype=torch.int32).cuda() for k, n in (("oord_kf", caps[0]), ("oord_w", caps[0]), ("ochild_kf", caps[1]))}
        r = _device_raw(pr, caps=caps, out={k: v[:v.numel() - 8] for k, v in big.items()})
        assert int(r.status.item()) == bit and np.array_equal(r.counts.cpu().numpy(), exp["counts"]), name
        for k, v in big.items():
            v = v.cpu().numpy()
            assert (v[-8:] == POISON).all() and np.array_equal(v[:-8], exp[k][:len(v) - 8]), (name, k)
    full = _host(pr, caps=(n_ord, n_child))
    _same(full, exp, name + " exact capacities", _keys(pr))


def _drop(pr, off, ents, i):
    """the problem without entry i of the CSR table (off, ents)"""
    q = dict(pr)
    row = int(np.searchsorted(pr[off], i, side="right")) - 1
    o = np.array(pr[off]); o[row + 1:] -= 1
    q[off] = o
    for e in ents:
        q[e] = np.delete(pr[e], i)
    return q


def test_corrupted_indices_count_as_absent_and_set_the_status_bits():
    from ceres_mono_orb_slam2_amd import localmapping as lm
    name, pr, _, _ = _seeded()[4]
    nkf = pr["nkf"]
    ic, ih, io = len(pr["conn_kf"]) // 2, len(pr["child_kf"]) // 2, len(pr["ord_kf"]) // 3
    bad = dict(pr, conn_kf=np.array(pr["conn_kf"]), child_kf=np.array(pr["child_kf"]), ord_kf=np.array(pr["ord_kf"]))
    bad["conn_kf"][ic] = nkf + 5; bad["child_kf"][ih] = -3; bad["ord_kf"][io] = nkf
    bad["tgt_kf"] = np.concatenate([pr["tgt_kf"][:1], [nkf + 1], pr["tgt_kf"][1:]]).astype(np.int32)
    for k in ("tgt_flags", "tgt_mask"):
        bad[k] = np.concatenate([pr[k][:1], [k == "tgt_mask"], pr[k][1:]]).astype(np.uint8)
    clean = _drop(_drop(_drop(pr, "conn_off", ("conn_kf", "conn_w"), ic), "child_off", ("child_kf",), ih), "ord_off", ("ord_kf", "ord_w"), io)
    exp = npb.set_bad_keyframes(clean)
    d = _device(bad)
    assert d["status"] == lm.BF_INDEX | lm.BF_TARGET, name
    assert d["tgt_status"][1] == 4 and not d["tgt_Tcp"][1].any()
    d["tgt_status"] = np.delete(d["tgt_status"], 1); d["tgt_Tcp"] = np.delete(d["tgt_Tcp"], 1, axis=0)
    _same(d, exp, name, _keys(pr))
    # a duplicate among the status-0 targets: the first instance counts, the second is skipped with status 4
    dup = dict(pr, tgt_kf=np.concatenate([pr["tgt_kf"], pr["tgt_kf"][:1]]).astype(np.int32))
    for k in ("tgt_flags", "tgt_mask"):
        dup[k] = np.concatenate([pr[k], [k == "tgt_mask"]]).astype(np.uint8)
    d = _device(dup)
    exp = npb.set_bad_keyframes(pr)
    assert d["status"] == lm.BF_TARGET and d["tgt_status"][-1] == 4 and not d["tgt_Tcp"][-1].any()
    d["tgt_status"] = d["tgt_status"][:-1]; d["tgt_Tcp"] = d["tgt_Tcp"][:-1]
    _same(d, exp, name + " duplicate", _keys(pr))
