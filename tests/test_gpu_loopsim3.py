"""orbl_loop_sim3_candidates (host and device forms) on the MI355X against the restatement tests/nploopsim3.py, the literal front of
LoopClosing::ComputeSim3.  EVERYTHING here is compared byte for byte: the integer outputs are exact by definition, and X1c / X2c /
max_err have a fixed operation order without fused multiply-add - so there is no tolerance anywhere in this file.
tests/test_loopsim3_restatement.py shows that the restatement's search is the oracle's and that the cases take the paths these
comparisons rely on."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import loopsim3cases as lc  # noqa: E402
from tests import nploopsim3 as NL  # noqa: E402

pytestmark = pytest.mark.gpu

PER_CAND = ("match12", "nmatches", "cand_status", "K1", "K2", "off", "counts")
PER_ROW = ("X1c", "X2c", "max_err1", "max_err2", "row_i1", "row_pt1", "row_pt2")
FILL = dict(X1c=0.0, X2c=0.0, max_err1=0.0, max_err2=0.0, row_i1=-1, row_pt1=-1, row_pt2=-1)
_CACHE = {}


def _lc():
    from ceres_mono_orb_slam2_amd import loopclosing
    return loopclosing


def _frozen(tab):
    for v in tab.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return tab


def _seeded(seed):
    """a seeded map and its restatement, computed once, shared and read-only"""
    if seed not in _CACHE:
        m = lc.make(seed)
        mm = 90 if seed % 2 else 20                                  # (odd seeds: the gate discards several candidates)
        _CACHE[seed] = (_frozen(m["tab"]), m["cur_kf"], m["cand_kf"], dict(min_matches=mm), NL.sim3_candidates(m["tab"], m["cur_kf"], m["cand_kf"], min_matches=mm))
    return _CACHE[seed]


def _seam(check_ori):
    key = ("seam", check_ori)
    if key not in _CACHE:
        m = lc.seam_case()
        cand = m["cand_kf"] if check_ori else m["cand_kf"][:2]
        kw = dict(min_matches=10, check_ori=check_ori)
        _CACHE[key] = (_frozen(m["tab"]), m["cur_kf"], cand, kw, NL.sim3_candidates(m["tab"], m["cur_kf"], cand, **kw))
    return _CACHE[key]


def _first(exp, n, cap1):
    """the expectation for the first n candidates alone: every candidate's row is computed on its own"""
    rows = int(exp["off"][n])
    o = {k: exp[k][:n] for k in ("match12", "nmatches", "cand_status", "K1", "K2")}
    o.update({k: exp[k][:rows] for k in PER_ROW})
    o["off"] = exp["off"][:n + 1]
    o["counts"] = np.array([rows, int((exp["cand_status"][:n] == 0).sum())], np.int32)
    return o


def _dev_tab(tab):
    import torch
    return {k: (None if v is None else torch.from_numpy(np.array(v).view(np.int32) if v.dtype == np.uint32 else np.array(v)).cuda()) for k, v in tab.items()}     # (copies: the shared tables are read-only)


def _status(d):
    return int(d["status"].cpu()[0]) & 0xFFFFFFFF


def _same(got, exp, what):
    g, e = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert g.dtype == e.dtype and g.shape == e.shape and g.tobytes() == e.tobytes(), (what, got, exp)


def _check_host(h, exp, what):
    for k in PER_CAND + PER_ROW:
        _same(h[k], exp[k], (what, "host", k))


def _check_device(d, exp, what, bits=0):
    """every element of every output: the expected rows, then the fill"""
    import torch
    torch.cuda.synchronize()
    assert _status(d) == bits, (what, _status(d))
    for k in PER_CAND:
        _same(d[k].cpu().numpy().reshape(np.asarray(exp[k]).shape), exp[k], (what, "device", k))
    rows = int(exp["counts"][0])
    for k in PER_ROW:
        g = d[k].cpu().numpy()
        _same(g[:rows], exp[k], (what, "device", k))
        assert np.all(g[rows:] == FILL[k]), (what, "device fill", k)


def _run_both(tab, cur, cand, exp, what, cap1=None, cap_rows=None, **kw):
    import torch
    L = _lc()
    cand = np.asarray(cand, np.int32)
    n1 = int(tab["kf_slot_off"][cur + 1] - tab["kf_slot_off"][cur])
    _check_host(L.sim3_candidates(tab, cur, cand, cap1=cap1, cap_rows=cap_rows, **kw), exp, what)
    d = L.sim3_candidates_device(_dev_tab(tab), cur, torch.from_numpy(np.array(cand, np.int32)).cuda(), cap1=n1 if cap1 is None else cap1,
                                 cap_rows=int(exp["counts"][0]) + 3 if cap_rows is None else cap_rows, **kw)
    _check_device(d, exp, what)
    return d


# ------------------------------------------------------------------------------------------------------------------ the cases
def test_hand_cases_host_and_device():
    for name, tab, cur, cand, want in lc.hand_cases():
        exp = NL.sim3_candidates(tab, cur, cand, **want["args"])
        for k, v in want.items():                                 # (the worked values themselves, not only the restatement)
            if k != "args":
                assert np.array_equal(np.asarray(exp[k], np.float64), np.asarray(v, np.float64)), (name, k)
        _run_both(tab, cur, cand, exp, name, **want["args"])


def test_the_gate_19_and_20_matches():
    tab, cur, cand, want = lc.gate_case()
    exp = NL.sim3_candidates(tab, cur, cand)
    assert exp["nmatches"].tolist() == want["nmatches"] and exp["cand_status"].tolist() == want["cand_status"] and exp["off"].tolist() == want["off"]
    _run_both(tab, cur, cand, exp, "gate")


@pytest.mark.parametrize("seed", lc.SEEDS)
def test_seeded_maps_host_and_device(seed):
    tab, cur, cand, kw, exp = _seeded(seed)
    assert exp["counts"][0] > 100 and 1 in exp["cand_status"] and (seed not in (101, 103, 109) or 2 in exp["cand_status"])
    _run_both(tab, cur, cand, exp, seed, **kw)


@pytest.mark.parametrize("n_cand", (1, 2, 7))
def test_seam_shapes(n_cand):
    """candidate node lists of 1, 63, 64, 65, 256, 257 and 300 entries, current node lists of 64, 65 and 130, a keyframe without nodes"""
    tab, cur, cand, kw, exp = _seam(True)
    assert len(cand) == 7 and exp["nmatches"][6] == 0 and min(exp["nmatches"][:2]) > 40
    n1 = int(tab["kf_slot_off"][cur + 1] - tab["kf_slot_off"][cur])
    _run_both(tab, cur, cand[:n_cand], _first(exp, n_cand, n1), ("seam", n_cand), **kw)


def test_seam_shapes_without_the_rotation_check():
    tab, cur, cand, kw, exp = _seam(False)
    with_ori = _seam(True)[4]
    assert exp["nmatches"][0] > with_ori["nmatches"][0], "the rotation check had something to reject"
    _run_both(tab, cur, cand, exp, "seam, check_ori 0", **kw)


# ------------------------------------------------------------------------------------------------------------------ the contract
def _poisoned(n_cand, cap1, cap_rows, guard=8):
    """preset outputs filled with 0xA5 bytes, each a view of a larger buffer whose tail must stay as it is"""
    import torch
    L = _lc()
    big, out = {}, {}
    to = {np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}
    for k, dt, per, kind in L._LS_OUT:
        n = L._ls_out_size(kind, per, n_cand, cap1, cap_rows)
        b = torch.full(((n + guard) * np.dtype(dt).itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        big[k] = (b, n * np.dtype(dt).itemsize)
        out[k] = b.view(to[dt])[:n]
    return big, out


def _guards_intact(big):
    return all(bool((b[n:] == 0xA5).all()) for b, n in big.values())


def test_poisoned_outputs_are_overwritten_and_two_runs_agree():
    import torch
    tab, cur, cand, kw, exp = _seeded(lc.SEEDS[1])
    n1 = int(tab["kf_slot_off"][cur + 1] - tab["kf_slot_off"][cur])
    cap1, cap_rows = n1 + 37, int(exp["counts"][0]) + 300
    wide = dict(exp)
    wide["match12"] = np.full((len(cand), cap1), -1, np.int32)
    wide["match12"][:, :n1] = exp["match12"]
    dt, dc = _dev_tab(tab), torch.from_numpy(np.array(cand, np.int32)).cuda()
    runs = []
    for _ in range(2):
        big, out = _poisoned(len(cand), cap1, cap_rows)
        d = _lc().sim3_candidates_device(dt, cur, dc, cap1=cap1, cap_rows=cap_rows, out=out, **kw)
        _check_device(d, wide, "poisoned")
        assert _guards_intact(big)
        runs.append({k: big[k][0].cpu().numpy().tobytes() for k in big})
    assert runs[0] == runs[1]


def test_each_capacity_one_too_small():
    import torch
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = _lc()
    tab, cur, cand, kw, exp = _seeded(lc.SEEDS[2])
    n1, rows = int(tab["kf_slot_off"][cur + 1] - tab["kf_slot_off"][cur]), int(exp["counts"][0])
    dt, dc = _dev_tab(tab), torch.from_numpy(np.array(cand, np.int32)).cuda()
    with pytest.raises(OrbHipError, match=r"code -4\): orbl_loop_sim3_candidates: wanted %d rows; capacity %d" % (rows, rows - 1)):
        L.sim3_candidates(tab, cur, cand, cap_rows=rows - 1, **kw)
    with pytest.raises(OrbHipError, match=r"code -4\): orbl_loop_sim3_candidates: the current keyframe has %d slots; cap1 is %d" % (n1, n1 - 1)):
        L.sim3_candidates(tab, cur, cand, cap1=n1 - 1, **kw)
    # device, cap_rows: off[] and counts[] state what was wanted, the rows that fit are there, nothing lies beyond
    big, out = _poisoned(len(cand), n1, rows - 1)
    d = L.sim3_candidates_device(dt, cur, dc, cap1=n1, cap_rows=rows - 1, out=out, **kw)
    torch.cuda.synchronize()
    assert _status(d) == L.LS_CAP and _guards_intact(big)
    for k in PER_CAND:
        _same(d[k].cpu().numpy().reshape(np.asarray(exp[k]).shape), exp[k], ("cap_rows", k))
    for k in PER_ROW:
        _same(d[k].cpu().numpy(), exp[k][:rows - 1], ("cap_rows", k))
    # device, cap1: nothing is searched
    big, out = _poisoned(len(cand), n1 - 1, rows)
    d = L.sim3_candidates_device(dt, cur, dc, cap1=n1 - 1, cap_rows=rows, out=out, **kw)
    torch.cuda.synchronize()
    assert _status(d) == L.LS_CAP and _guards_intact(big)
    assert d["counts"].cpu().tolist() == [0, 0] and not d["off"].cpu().any() and not d["nmatches"].cpu().any() and bool((d["match12"].cpu() == -1).all())
    assert d["cand_status"].cpu().tolist() == [1 if s == 1 else 2 for s in exp["cand_status"]]
    assert bool((d["row_i1"].cpu() == -1).all()) and not d["X1c"].cpu().any()


def test_corrupted_indices_raise_status_and_count_as_absent():
    import torch
    L = _lc()
    tab, cur, cand, kw, exp = _seeded(lc.SEEDS[3])
    n1 = int(tab["kf_slot_off"][cur + 1] - tab["kf_slot_off"][cur])
    nkf, npts = len(tab["kf_slot_off"]) - 1, len(tab["pt_bad"])
    c0 = int(np.argmax(exp["cand_status"] == 0))                   # the first kept candidate and its first row: what it was built from
    r0 = exp["_rows"][0]
    lo1, lo2 = int(tab["kf_slot_off"][cur]), int(tab["kf_slot_off"][cand[c0]])
    obs_e = next(e for e in range(int(tab["obs_off"][r0["pt1"]]), int(tab["obs_off"][r0["pt1"] + 1])) if tab["obs_kf"][e] == cur)
    ent_e = int(tab["fv_ent_off"][tab["kf_fv_off"][cur]])          # the first entry of the current keyframe's first node
    edits = [("kf_fv_off", cand[c0] + 1, -5, L.LS_OFFSETS), ("fv_ent_off", int(tab["kf_fv_off"][cur]) + 1, 10 ** 9, L.LS_OFFSETS), ("obs_off", r0["pt1"] + 1, -1, L.LS_OFFSETS),
             ("kf_slot_pt", lo1 + r0["i1"], npts, L.LS_PT), ("kf_slot_pt", lo2 + int(exp["match12"][c0][r0["i1"]]), -7, L.LS_PT),
             ("kf_slot_level", lo1 + r0["x1"], 99, L.LS_LEVEL), ("kf_slot_level", lo2 + r0["x2"], -1, L.LS_LEVEL), ("fv_ent", ent_e, 100000, L.LS_SLOT),
             ("fv_ent", ent_e, -1, L.LS_SLOT), ("obs_slot", obs_e, 100000, L.LS_SLOT), ("obs_kf", obs_e, nkf, L.LS_KF)]
    base = _dev_tab(tab)
    dc = torch.from_numpy(np.array(cand, np.int32)).cuda()
    for key, at, value, bit in edits:
        t = dict(base)
        t[key] = base[key].clone()
        t[key].view(-1)[at] = value
        d = L.sim3_candidates_device(t, cur, dc, cap1=n1, cap_rows=int(exp["counts"][0]) + 3, **kw)
        torch.cuda.synchronize()
        assert _status(d) == bit, (key, at, value, _status(d))
        assert int(d["counts"].cpu()[0]) <= exp["counts"][0]
    # a candidate that is no keyframe counts as a bad one; the others are computed as before
    c2 = cand.copy(); c2[0] = nkf
    d = L.sim3_candidates_device(base, cur, torch.from_numpy(np.array(c2, np.int32)).cuda(), cap1=n1, cap_rows=int(exp["counts"][0]) + 3, **kw)
    torch.cuda.synchronize()
    assert _status(d) == L.LS_KF and d["cand_status"].cpu().tolist() == [1] + exp["cand_status"][1:].tolist()
    assert d["nmatches"].cpu().tolist() == [0] + exp["nmatches"][1:].tolist() and bool((d["match12"][1:].cpu() == torch.as_tensor(exp["match12"][1:])).all())
    # a current keyframe that is none: nothing matches
    d = L.sim3_candidates_device(base, nkf, dc, cap1=n1, cap_rows=8, **kw)
    torch.cuda.synchronize()
    assert _status(d) == L.LS_KF and d["counts"].cpu().tolist() == [0, 0] and not d["nmatches"].cpu().any() and not d["K1"].cpu().any()


def test_a_reused_workspace():
    import torch
    L = _lc()
    a, b = _seeded(lc.SEEDS[4]), _seeded(lc.SEEDS[5])
    caps = [(int(t[0]["kf_slot_off"][t[1] + 1] - t[0]["kf_slot_off"][t[1]]), int(t[4]["counts"][0]) + 3) for t in (a, b)]
    nbytes = max(L.sim3_candidates_device(_dev_tab(t[0]), t[1], torch.from_numpy(np.array(t[2], np.int32)).cuda(), cap1=c[0], cap_rows=c[1], **t[3])["_workspace"].numel() for t, c in zip((a, b), caps))
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    for t, c in ((a, caps[0]), (b, caps[1]), (a, caps[0])):
        d = L.sim3_candidates_device(_dev_tab(t[0]), t[1], torch.from_numpy(np.array(t[2], np.int32)).cuda(), cap1=c[0], cap_rows=c[1], workspace=ws, **t[3])
        assert d["_workspace"] is ws
        _check_device(d, t[4], "reused workspace")


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_the_outputs_feed_iterate_batch_device_unchanged():
    """orbl_loop_sim3_candidates_device -> orbt_sim3_iterate_batch_device with no host step between them but the read of off[] that
    draws the sets; every candidate's result and masks equal sim3solver.iterate on the rows the restatement builds"""
    import torch
    from ceres_mono_orb_slam2_amd import sim3solver as S
    tab, cur, cand, kw, exp = _seeded(lc.SEEDS[6])
    nc, n1 = len(cand), int(tab["kf_slot_off"][cur + 1] - tab["kf_slot_off"][cur])
    cap_rows = int(exp["counts"][0]) + 5
    d = _lc().sim3_candidates_device(_dev_tab(tab), cur, torch.from_numpy(np.array(cand, np.int32)).cuda(), cap1=n1, cap_rows=cap_rows, **kw)
    off = d["off"].cpu().numpy()                                   # (the one inherent read: N per candidate)
    _same(off, exp["off"], "off")
    iterations, min_inliers = 12, 20
    rng = np.random.default_rng(3)
    sets = np.zeros((nc, iterations, 3), np.int32)
    for c in range(nc):
        n = int(off[c + 1] - off[c])
        if n >= 3:
            sets[c] = S.draw_sets(n, iterations, lambda lo, hi: int(rng.integers(lo, hi + 1)))
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()      # noqa: E731
    st = dict(fix_scale=up(np.zeros(nc, np.int32)), min_inliers=up(np.full(nc, min_inliers, np.int32)), n_sets=up(np.full(nc, iterations, np.int32)), sets=up(sets),
              best_count=up(np.zeros(nc, np.int32)), best_mask=torch.zeros(cap_rows, dtype=torch.uint8, device="cuda"), best_R=up(np.tile(np.eye(3), (nc, 1, 1))),
              best_t=up(np.zeros((nc, 3))), best_scale=up(np.ones(nc, np.float32)), result=torch.zeros(S.result_bytes(nc), dtype=torch.uint8, device="cuda"),
              inliers=torch.zeros(cap_rows, dtype=torch.uint8, device="cuda"))
    ws = S.iterate_batch_device(d["X1c"], d["X2c"], d["max_err1"], d["max_err2"], d["off"], d["K1"], d["K2"], **st)
    torch.cuda.synchronize()
    del ws
    res = S.decode_results(st["result"].cpu().numpy())
    inl, bm = st["inliers"].cpu().numpy(), st["best_mask"].cpu().numpy()
    found = 0
    for c in range(nc):
        a, b = int(off[c]), int(off[c + 1])
        if b - a < min_inliers:
            assert res[c]["status"] == S.TOO_FEW, c
            continue
        ref = S.iterate(exp["X1c"][a:b], exp["X2c"][a:b], exp["max_err1"][a:b], exp["max_err2"][a:b], exp["K1"][c], exp["K2"][c], False, min_inliers, sets[c])
        for k in ("status", "consumed", "n_inliers"):
            assert res[c][k] == ref[k], (c, k)
        for k in ("scale", "T12", "R", "t"):
            _same(res[c][k], ref[k], (c, k))
        _same(inl[a:b].astype(bool), ref["inliers"], (c, "inliers"))
        _same(bm[a:b], ref["state"].best_mask, (c, "best_mask"))
        found += ref["status"] == S.FOUND
    assert found > 0
