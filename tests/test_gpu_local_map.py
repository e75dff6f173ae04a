"""orbt_update_local_keyframes / orbt_update_local_points / orbt_update_local_map_device on the MI355X against the restatement
tests/nplocalmap.py (Tracking::UpdateLocalMap, src/Tracking.cc:838-977, and SearchLocalPoints' skip rule): every list, count, status,
frame_pt_out, votes and packed array, all integers or copies, all compared with ==.  Output buffers are pre-filled with a poison
pattern: what the contract says is written is written (the mp_state padding included) and nothing beyond a capacity is."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import localmapcases as lc  # noqa: E402
from tests import nplocalmap as nlm  # noqa: E402

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(ROOT, "ceres_mono_orb_slam2_amd", "csrc", "orb_localupdate.inc")).read()
T = int(re.search(r"#define ULM_T (\d+)", _SRC).group(1))          # the compaction tile of k_ulm_first / k_ulm_count / k_ulm_scatter
B = int(re.search(r"#define ULM_B (\d+)", _SRC).group(1))          # frame slots per workgroup of k_ulm_marks
ECAP = -4
PACKED = ("mp_Xw", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_desc")
POISON = dict(int32=-77, uint8=0xA5, float64=-1.5e300, float32=-2.5e30)
HAND = lc.hand_cases()
_SEEDED = None


def _seeded():
    """every seeded problem, computed once and shared (read-only)"""
    global _SEEDED
    if _SEEDED is None:
        _SEEDED = lc.seeded()
        for _, pr in _SEEDED:
            for v in pr.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _SEEDED


def _poison(shape, dt):
    return np.full(shape, POISON[np.dtype(dt).name], dt)


def _packed_poison(cap_pt, n_kp):
    return dict(mp_Xw=_poison(3 * cap_pt, np.float64), mp_normal=_poison(3 * cap_pt, np.float64), mp_min_dist=_poison(cap_pt, np.float32),
                mp_max_dist=_poison(cap_pt, np.float32), mp_desc=_poison(32 * cap_pt, np.uint8), mp_state=_poison(cap_pt, np.uint8),
                slot_Xw=_poison(3 * n_kp, np.float64), slot_state=_poison(n_kp, np.uint8))


def _host(pr, cap_kf, cap_pt):
    """the two host calls as the drop-in chains them: the graph first, then the slot tables of the returned keyframes only"""
    from ceres_mono_orb_slam2_amd import tracking
    nkf, n_kp = len(pr["kf_bad"]), len(pr["frame_pt"])
    o1 = dict(frame_pt_out=_poison(n_kp, np.int32), local_kf=_poison(cap_kf, np.int32), votes=_poison(nkf, np.int32))
    a = tracking.update_local_keyframes(pr["frame_pt"], pr["pt_bad"], pr["obs_off"], pr["obs_kf"], pr["kf_bad"], pr["kf_rank"], pr["kf_parent"], pr["cov_off"], pr["cov_kf"],
                                        pr["child_off"], pr["child_kf"], pr["prev_local_kf"], cap_kf=cap_kf, out=o1)
    assert (o1["local_kf"][a["n_local_kf"]:] == POISON["int32"]).all()
    rows = [pr["kf_slot_pt"][pr["kf_slot_off"][k]:pr["kf_slot_off"][k + 1]] for k in a["local_kf"]]
    off, val = lc._csr(rows)
    o2 = dict(local_pt=_poison(cap_pt, np.int32), **_packed_poison(cap_pt, n_kp))
    b = tracking.update_local_points(off, val, pr["pt_bad"], pr["pt_nobs"], pr["pt_Xw"], pr["pt_normal"], pr["pt_min_dist"], pr["pt_max_dist"], pr["pt_desc"],
                                     a["frame_pt_out"], pr["seen_pt"], cap_pt, out=o2)
    r = dict(a); r.update(b); r["local_pt_full"] = o2["local_pt"]
    return r


def _tables(pr):
    import torch
    return {k: (None if v is None else torch.as_tensor(np.array(v)).cuda()) for k, v in pr.items()}


def _device(pr, cap_kf, cap_pt, max_local_slots=None):
    import torch
    from ceres_mono_orb_slam2_amd import tracking
    nkf, n_kp = len(pr["kf_bad"]), len(pr["frame_pt"])
    out = dict(frame_pt_out=_poison(n_kp, np.int32), local_kf=_poison(cap_kf, np.int32), local_pt=_poison(cap_pt, np.int32), counts=_poison(4, np.int32),
               votes=_poison(nkf, np.int32), **_packed_poison(cap_pt, n_kp))
    out = {k: torch.from_numpy(v).cuda() for k, v in out.items()}
    d = tracking.update_local_map_device(_tables(pr), cap_kf, cap_pt, max_local_slots=max_local_slots, out=out)
    torch.cuda.synchronize()
    r = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items() if k != "_workspace"}
    c = r["counts"]
    r.update(n_local_kf=int(c[0]), ref_kf=int(c[1]), n_local_pt=int(c[2]), status=int(c[3]), d_status=int(r["status"][0]), local_pt_full=r["local_pt"], local_kf_full=r["local_kf"])
    r["local_kf"] = r["local_kf"][:max(0, min(cap_kf, r["n_local_kf"]))]; r["local_pt"] = r["local_pt"][:max(0, min(cap_pt, r["n_local_pt"]))]
    return r


def _same(got, pr, cap_pt, what=""):
    exp = nlm.update_local_map(pr, cap_pt=cap_pt)
    for k in ("n_local_kf", "ref_kf", "status", "n_local_pt"):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    for k in ("frame_pt_out", "local_kf", "votes", "local_pt", "mp_state", "slot_state"):
        g = np.asarray(got[k]).reshape(-1)
        assert g.dtype == exp[k].dtype and np.array_equal(g, exp[k]), (what, k)
    n = exp["n_local_pt"]
    assert np.array_equal(np.asarray(got["slot_Xw"]).reshape(-1, 3), exp["slot_Xw"]), (what, "slot_Xw")
    for k in PACKED:
        g = np.asarray(got[k]); g = g.reshape(cap_pt, -1) if g.size else g.reshape(0, 1)
        e = np.asarray(exp[k]).reshape(n, -1)
        assert g.dtype == e.dtype and np.array_equal(g[:n], e), (what, k)
        assert (g[n:] == POISON[g.dtype.name]).all(), (what, k, "rows beyond the count were written")
    assert (got["local_pt_full"][n:] == POISON["int32"]).all(), (what, "local_pt beyond the count")
    return exp


def _caps(pr, slack=3):
    exp = nlm.update_local_map(pr)
    return max(exp["n_local_kf"], len(pr["prev_local_kf"])) + slack, exp["n_local_pt"] + slack


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_worked_cases_host_and_device(name):
    pr, want = HAND[name]
    cap_kf, cap_pt = _caps(pr)
    for how, got in (("host", _host(pr, cap_kf, cap_pt)), ("device", _device(pr, cap_kf, cap_pt))):
        _same(got, pr, cap_pt, (name, how))
        for k, v in want.items():                                   # the hand-written values themselves
            g = np.asarray(got[k]).reshape(-1)
            assert np.array_equal(g[:len(np.atleast_1d(v))] if k == "mp_state" else g, np.asarray(v).reshape(-1)), (name, how, k)
    assert got["d_status"] == 0 and (got["local_kf_full"][got["n_local_kf"]:] == POISON["int32"]).all()


def test_seeded_maps_host_and_device_equal_the_restatement():
    for name, pr in _seeded():
        cap_kf, cap_pt = _caps(pr)
        exp = _same(_host(pr, cap_kf, cap_pt), pr, cap_pt, (name, "host"))
        d = _device(pr, cap_kf, cap_pt)
        _same(d, pr, cap_pt, (name, "device"))
        assert d["d_status"] == 0
        assert (exp["n_local_kf"], exp["n_local_pt"]) == lc.TABLE[name][:2]


def _seam(total, n_kp, seed=0):
    """Two voted keyframes whose slot tables hold `total` slots together: every fifth slot is empty, every seventh repeats the point three
    slots before, the top point id sits in the last slot and in the frame, one point is bad."""
    rng = np.random.default_rng(seed + total)
    npts = total + 3
    ids = [int(p) for p in rng.permutation(npts - 1)]
    slots = []
    for i in range(total):
        slots.append(-1 if i % 5 == 4 else (slots[i - 3] if i % 7 == 6 and slots[i - 3] >= 0 else ids[i]))
    slots[-1] = npts - 1                                            # the top id is used
    cut = total // 3
    frame = ([npts - 1] + [slots[i % total] if i % 3 else -1 for i in range(1, n_kp)])[:n_kp]
    obs = [[0, 1]] * npts
    return lc.build(2, [slots[:cut], slots[cut:]], frame, obs=obs, npts=npts, pt_bad=[ids[1]], seen=[ids[2]])


@pytest.mark.parametrize("total", [1, T - 1, T, T + 1, 2 * T + 3])
def test_slot_totals_around_the_compaction_tile(total):
    pr = _seam(total, n_kp=1 if total <= T else B + 1)
    assert pr["kf_slot_off"][-1] == total and pr["kf_slot_pt"].max() == len(pr["pt_bad"]) - 1
    cap_kf, cap_pt = _caps(pr, slack=T + 1)
    _same(_host(pr, cap_kf, cap_pt), pr, cap_pt, ("host", total))
    _same(_device(pr, cap_kf, cap_pt), pr, cap_pt, ("device", total))
    _same(_device(pr, cap_kf, cap_pt, max_local_slots=total), pr, cap_pt, ("device, exact slot bound", total))


def test_first_occurrence_behind_a_tile_of_empty_slots_and_duplicate_in_a_later_tile():
    # tile 0: three points and empty slots; tile 1: empty throughout; tile 2: the first occurrence of points 3, 4, then fresh points; tile 3: 3 again
    slots = [0, 1, 2] + [-1] * (2 * T - 3) + [3, 4] + list(range(5, 5 + T)) + [3, 4, 0]
    pr = lc.build(1, [slots], [0])
    exp = nlm.update_local_map(pr)
    assert list(exp["local_pt"]) == list(range(5 + T))
    cap_pt = 5 + T
    _same(_host(pr, 1, cap_pt), pr, cap_pt, "host")
    _same(_device(pr, 1, cap_pt), pr, cap_pt, "device")


@pytest.mark.parametrize("n_kp", [1, B + 1])
def test_frame_sizes_around_the_vote_block(n_kp):
    name, pr0 = _seeded()[4]                                        # small-1
    pr = dict(pr0)
    pr["frame_pt"] = np.resize(pr0["frame_pt"][pr0["frame_pt"] >= 0], n_kp).astype(np.int32)
    pr["frame_pt"][-1] = len(pr["pt_bad"]) - 1                      # the top point id, held by the last lane
    cap_kf, cap_pt = _caps(pr)
    _same(_host(pr, cap_kf, cap_pt), pr, cap_pt, ("host", n_kp))
    _same(_device(pr, cap_kf, cap_pt), pr, cap_pt, ("device", n_kp))


def test_capacities_exact_fit_and_one_short():
    from ceres_mono_orb_slam2_amd import tracking
    name, pr = _seeded()[3]                                         # small-0
    exp = nlm.update_local_map(pr)
    nk, npt, n_kp = exp["n_local_kf"], exp["n_local_pt"], len(pr["frame_pt"])
    _same(_host(pr, nk, npt), pr, npt, "host, exact")
    d = _device(pr, nk, npt)
    _same(d, pr, npt, "device, exact")
    assert d["d_status"] == 0
    # one short, host: ORBHIP_ECAP and only the count is written
    o1 = dict(frame_pt_out=_poison(n_kp, np.int32), local_kf=_poison(nk - 1, np.int32), votes=_poison(len(pr["kf_bad"]), np.int32))
    r = tracking.update_local_keyframes(pr["frame_pt"], pr["pt_bad"], pr["obs_off"], pr["obs_kf"], pr["kf_bad"], pr["kf_rank"], pr["kf_parent"], pr["cov_off"], pr["cov_kf"],
                                        pr["child_off"], pr["child_kf"], pr["prev_local_kf"], cap_kf=nk - 1, out=o1, check=False)
    assert r == dict(rc=ECAP, n_local_kf=nk)
    assert all((v == POISON["int32"]).all() for v in o1.values())
    rows = [pr["kf_slot_pt"][pr["kf_slot_off"][k]:pr["kf_slot_off"][k + 1]] for k in exp["local_kf"]]
    off, val = lc._csr(rows)
    o2 = dict(local_pt=_poison(npt - 1, np.int32), **_packed_poison(npt - 1, n_kp))
    r = tracking.update_local_points(off, val, pr["pt_bad"], pr["pt_nobs"], pr["pt_Xw"], pr["pt_normal"], pr["pt_min_dist"], pr["pt_max_dist"], pr["pt_desc"],
                                     exp["frame_pt_out"], pr["seen_pt"], npt - 1, out=o2, check=False)
    assert r == dict(rc=ECAP, n_local_pt=npt)
    assert all((v == POISON[v.dtype.name]).all() for v in o2.values())
    # one short, device: the wanted counts, a status bit, nothing beyond the capacity, every packed row padding
    d = _device(pr, nk, npt - 1)
    assert d["n_local_pt"] == npt and d["n_local_kf"] == nk and d["d_status"] == 8
    assert np.array_equal(d["local_pt_full"], exp["local_pt"][:npt - 1]) and (d["mp_state"] == 0).all() and (d["mp_min_dist"] == POISON["float32"]).all()
    d = _device(pr, nk - 1, npt)
    assert d["n_local_kf"] == nk and d["ref_kf"] == exp["ref_kf"] and d["d_status"] == 4 and d["n_local_pt"] == 0 and (d["mp_state"] == 0).all()
    assert np.array_equal(d["local_kf_full"], _poison(nk - 1, np.int32)) and (d["local_pt_full"] == POISON["int32"]).all()
    total = int(sum(len(x) for x in rows))
    d = _device(pr, nk, npt, max_local_slots=total - 1)
    assert d["d_status"] == 16 and d["n_local_pt"] == 0 and np.array_equal(d["local_kf"], exp["local_kf"])
    _same(_device(pr, nk, npt, max_local_slots=total), pr, npt, "device, exact slot bound")


def test_device_form_out_of_range_entries_set_status_and_do_not_fault():
    name, pr = _seeded()[4]
    cap_kf, cap_pt = _caps(pr)
    big = 10 ** 6
    exp = nlm.update_local_map(pr)
    kf0 = int(exp["local_kf"][0])                                   # the first voted keyframe: the walk always visits it, its slots are always read
    p0 = int(exp["frame_pt_out"][exp["frame_pt_out"] >= 0][0])      # a point the frame holds: its observers are always read
    where = dict(frame_pt=int(np.nonzero(pr["frame_pt"] >= 0)[0][0]), obs_kf=int(pr["obs_off"][p0]), seen_pt=0, kf_slot_pt=int(pr["kf_slot_off"][kf0]),
                 cov_kf=slice(None), child_kf=slice(None), kf_parent=slice(None), kf_rank=3, obs_off=p0, kf_slot_off=kf0, cov_off=kf0)
    for key, value, bit in (("frame_pt", big, 2), ("frame_pt", -5, 2), ("obs_kf", len(pr["kf_bad"]), 2), ("obs_kf", -1, 2), ("seen_pt", big, 2), ("kf_slot_pt", big, 2),
                            ("cov_kf", big, 2), ("child_kf", -3, 2), ("kf_parent", big, 2), ("kf_rank", big, 2), ("obs_off", -9, 1), ("kf_slot_off", 10 ** 7, 1),
                            ("cov_off", 10 ** 7, 1)):
        q = dict(pr); q[key] = pr[key].copy()
        q[key][where[key]] = value
        d = _device(q, len(pr["kf_bad"]), len(pr["pt_bad"]))
        assert d["d_status"] & bit, (key, value)
        assert 0 <= d["n_local_pt"] <= len(pr["pt_bad"]) and 0 <= d["n_local_kf"] <= len(pr["kf_bad"])
    q = dict(pr); q["kf_rank"] = pr["kf_rank"].copy(); q["kf_rank"][0] = q["kf_rank"][1]          # not a permutation
    assert _device(q, len(pr["kf_bad"]), len(pr["pt_bad"]))["d_status"] & 2
    d = _device(pr, cap_kf, cap_pt)                                 # a clean call afterwards
    _same(d, pr, cap_pt, "clean")
    assert d["d_status"] == 0


def test_index_order_when_no_rank_is_given_and_lists_only_without_packed_outputs():
    import torch
    from ceres_mono_orb_slam2_amd import tracking
    name, pr0 = _seeded()[5]
    pr = dict(pr0); pr["kf_rank"] = None
    cap_kf, cap_pt = _caps(pr)
    _same(_host(pr, cap_kf, cap_pt), pr, cap_pt, "host, index order")
    _same(_device(pr, cap_kf, cap_pt), pr, cap_pt, "device, index order")
    exp = nlm.update_local_map(pr)
    d = tracking.update_local_map_device(_tables(pr), cap_kf, cap_pt, packed=False, votes=False)
    torch.cuda.synchronize()
    c = d["counts"].cpu().numpy()
    assert list(c) == [exp["n_local_kf"], exp["ref_kf"], exp["n_local_pt"], exp["status"]] and "mp_state" not in d
    assert np.array_equal(d["local_pt"].cpu().numpy()[:c[2]], exp["local_pt"])
    rows = [pr["kf_slot_pt"][pr["kf_slot_off"][k]:pr["kf_slot_off"][k + 1]] for k in exp["local_kf"]]
    off, val = lc._csr(rows)
    b = tracking.update_local_points(off, val, pr["pt_bad"], None, None, None, None, None, None, exp["frame_pt_out"], pr["seen_pt"], cap_pt, packed=False)
    assert np.array_equal(b["local_pt"], exp["local_pt"]) and b["mp_state"] is None
