"""orbl_keyframe_culling(_device) on the MI355X against the restatement tests/npculling.py (src/LocalMapping.cc:576-637 with the state
changes of KeyFrame::SetBadFlag and MapPoint::EraseObservation between candidates): the decisions, the counts seen at every
candidate's turn and the final map state, all integer, all compared with ==.  tests/test_culling_restatement.py shows that the
problems tell the sequential semantics from an order-blind scoring."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import cullingcases as cc  # noqa: E402
from tests import npculling as npc  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("culled", "n_redundant", "n_map_points", "pt_bad", "pt_nobs", "obs_erased")
HAND = cc.hand_cases()
_SEEDED = None


def _seeded():
    """every seeded problem with its restated outputs, computed once and shared"""
    global _SEEDED
    if _SEEDED is None:
        _SEEDED = [(name, pr, npc.culling(pr)) for name, pr in cc.seeded()]
        for _, pr, exp in _SEEDED:
            for v in list(pr.values()) + list(exp.values()):
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _SEEDED


def _poisoned(pr):
    ncand, npts, nobs = len(pr["cand_kf"]), pr["npts"], len(pr["obs_kf"])
    return dict(culled=np.full(ncand, 0xA5, np.uint8), n_redundant=np.full(ncand, -77, np.int32), n_map_points=np.full(ncand, -78, np.int32),
                pt_bad=np.full(npts, 0xA5, np.uint8), pt_nobs=np.full(npts, -79, np.int32), obs_erased=np.full(nobs, 0xA5, np.uint8))


def _host(pr, **kw):
    from ceres_mono_orb_slam2_amd import localmapping
    return localmapping.keyframe_culling(pr["cand_kf"], pr["cand_flags"], pr["slot_off"], pr["slot_pt"], pr["slot_level"], pr["nkf"], pr["obs_off"],
                                         pr["obs_kf"], pr["obs_level"], pr["pt_bad"], pr["pt_nobs"], **kw)


def _device(pr, **kw):
    import torch
    from ceres_mono_orb_slam2_amd import localmapping

    def t(a):
        return None if a is None else torch.as_tensor(np.array(a)).cuda()          # (a copy: the shared problems are read-only)
    r = localmapping.keyframe_culling_device(t(pr["cand_kf"]), t(pr["cand_flags"]), t(pr["slot_off"]), t(pr["slot_pt"]), t(pr["slot_level"]), pr["nkf"],
                                             t(pr["obs_off"]), t(pr["obs_kf"]), t(pr["obs_level"]), t(pr["pt_bad"]), t(pr["pt_nobs"]), **kw)
    torch.cuda.synchronize()
    return r


def _same(got, exp, what=""):
    for k in KEYS:
        g = getattr(got, k)
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == exp[k].dtype and np.array_equal(g, exp[k]), (what, k)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_worked_cases_host_and_device(name):
    pr, exp = HAND[name]
    _same(_host(pr, out=_poisoned(pr)), exp, name)                  # (poisoned outputs: every element must be overwritten)
    d = _device(pr)
    _same(d, exp, name)
    assert int(d.status.item()) == 0


def test_seeded_problems_host_equals_restatement():
    for name, pr, exp in _seeded():
        _same(_host(pr, out=_poisoned(pr)), exp, name)


def test_seeded_problems_device_equals_host():
    import torch
    for name, pr, exp in _seeded():
        h = _host(pr)
        out = {k: torch.from_numpy(v).cuda() for k, v in _poisoned(pr).items()}
        d = _device(pr, out=out)
        _same(d, {k: getattr(h, k) for k in KEYS}, name)
        _same(d, exp, name)
        assert int(d.status.item()) == 0


def test_fat_keyframes_more_slots_than_one_workgroup_pass():
    for kw, culls in ((cc.FAT, False), (cc.FAT_CULL, True)):
        pr = cc.make(0, **kw)
        assert np.diff(pr["slot_off"]).max() > 2048
        exp = npc.culling(pr)
        assert not culls or (exp["culled"].sum() >= 1 and exp["pt_bad"].sum() >= 100)
        _same(_host(pr, out=_poisoned(pr)), exp, "fat")
        _same(_device(pr), exp, "fat")


def test_every_candidate_order_of_case_e():
    """the map of case (e) with keyframes 2 and 3 as candidates too: all 24 orders, and all orders of every subset"""
    pr0, _ = HAND["e_order_AB"]
    obs = [[(int(pr0["obs_kf"][e]), int(pr0["obs_level"][e])) for e in range(pr0["obs_off"][p], pr0["obs_off"][p + 1])] for p in range(pr0["npts"])]
    slots = [[(p, l) for p in range(len(obs)) for k2, l in obs[p] if k2 == k] for k in range(5)]
    n = 0
    for r in (1, 2, 3, 4):
        for cand in itertools.permutations(range(4), r):
            pr = cc.flatten(5, obs, slots, list(cand), [0] * r)
            exp = npc.culling(pr)
            assert list(exp["culled"]) == [1] + [0] * (r - 1)        # whoever comes first goes, the rest stay
            _same(_host(pr), exp, cand)
            n += 1
    assert n == 64


def test_null_optional_arguments():
    name, pr, exp = _seeded()[4]                                    # small-0
    h = _host(pr, final_state=False)
    assert h.pt_bad is None and h.pt_nobs is None and h.obs_erased is None
    for k in KEYS[:3]:
        assert np.array_equal(getattr(h, k), exp[k])
    d = _device(pr, final_state=False)
    for k in KEYS[:3]:
        assert np.array_equal(getattr(d, k).cpu().numpy(), exp[k])
    # no flags array: as all zero; an explicit pt_bad of zeros and pt_nobs of the list lengths: as NULL
    q = dict(pr); q["cand_flags"] = None
    z = dict(pr); z["cand_flags"] = np.zeros_like(pr["cand_flags"])
    _same(_host(q), npc.culling(z), "no flags")
    q = dict(pr); q["pt_bad"] = np.zeros(pr["npts"], np.uint8); q["pt_nobs"] = np.diff(pr["obs_off"]).astype(np.int32)
    _same(_host(q), exp, "explicit state")


def test_initially_bad_points_are_ignored():
    name, pr, _ = _seeded()[5]
    q = dict(pr); q["pt_bad"] = (np.arange(pr["npts"]) % 7 == 0).astype(np.uint8)
    exp = npc.culling(q)
    assert not np.array_equal(exp["culled"], npc.culling(pr)["culled"]) or not np.array_equal(exp["n_map_points"], npc.culling(pr)["n_map_points"])
    _same(_host(q), exp, "bad points")
    _same(_device(q), exp, "bad points")


def test_device_form_out_of_range_entries_set_status_and_do_not_fault():
    import torch
    name, pr, exp = _seeded()[4]
    for key, value, bit in (("slot_pt", 10 ** 6, 2), ("slot_pt", -5, 2), ("obs_kf", pr["nkf"], 2), ("obs_kf", -1, 2), ("cand_kf", pr["nkf"] + 3, 2),
                            ("slot_level", -1, 4), ("obs_level", -2, 4), ("slot_off", 10 ** 7, 1), ("obs_off", -9, 1)):
        q = dict(pr); q[key] = pr[key].copy(); q[key][len(q[key]) // 2] = value
        d = _device(q)
        assert int(d.status.item()) & bit, (key, value)
        assert d.culled.cpu().numpy().max() <= 1
    torch.cuda.synchronize()
    # an absent slot is a slot that is not there: the same answer as the problem without it
    q = dict(pr); q["slot_pt"] = pr["slot_pt"].copy(); q["slot_pt"][3] = pr["npts"]
    c = int(np.searchsorted(pr["slot_off"], 3, side="right") - 1)
    w = dict(pr); w["slot_pt"] = np.delete(pr["slot_pt"], 3); w["slot_level"] = np.delete(pr["slot_level"], 3)
    w["slot_off"] = pr["slot_off"].copy(); w["slot_off"][c + 1:] -= 1
    d = _device(q)
    e = npc.culling(w)
    for k in KEYS[:3]:
        assert np.array_equal(getattr(d, k).cpu().numpy(), e[k]), k
    _same(_device(pr), exp, "a clean call afterwards")
