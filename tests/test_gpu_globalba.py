"""orbl_global_ba_assemble(_device) and orbl_global_ba_apply(_device) on the MI355X against the restatement tests/npglobalba.py (the
literal loops of src/CeresOptimizer.cc:59-225 in the drop-in's reading): every output is compared bit for bit, as uint8 views - the
64-bit arithmetic is IEEE +, *, / and sqrt in a stated order, without fused multiply-add.  Rows a call must leave alone are poisoned
first.  tests/test_globalba_restatement.py shows that the maps tell the stated orders from an order-blind implementation."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import globalbacases as gc  # noqa: E402
from tests import npglobalba as npg  # noqa: E402
from tests import npmapcorrect as npm  # noqa: E402
from tests.test_globalba_restatement import SEEDED  # noqa: E402

pytestmark = pytest.mark.gpu

ASM_DT = dict(cam_kf=(np.int32, 1, 0), K4=(np.float64, 4, 0), poses7=(np.float64, 7, 0), cam_fixed=(np.uint8, 1, 0), gpt_pt=(np.int32, 1, 1), pts3=(np.float64, 3, 1),
              gobs_cam=(np.int32, 1, 2), gobs_pt=(np.int32, 1, 2), gobs_uv=(np.float64, 2, 2), gobs_weight=(np.float64, 1, 2), gobs_robust=(np.uint8, 1, 2),
              gobs_src=(np.int32, 1, 2))
ASM_KEYS = tuple(ASM_DT) + ("kf_cam", "pt_idx", "counts")
AP0_KEYS = ("kf_Tcw", "kf_center", "X", "normal", "min_max", "nd_written", "counts")
AP1_KEYS = ("kf_gba_Tcw", "kf_in_gba", "pt_gba_X", "pt_in_gba", "counts")
TABLES = ("kf_id", "kf_bad", "kf_Tcw", "kf_K4", "X", "pt_bad", "obs_off", "obs_kf", "obs_uv", "obs_level", "inv_level_sigma2", "kf_center", "pt_ref_kf", "ref_level",
          "scale_factors", "kf_gba_Tcw", "pt_gba_X")
HAND = gc.hand_assemble_cases()
_EXPECT = {}


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _same(got, exp, what, keys):
    for k in keys:
        if exp[k] is None:
            assert got.get(k) is None, (what, k)
            continue
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.dtype == e.dtype and g.size == e.size, (what, k, g.dtype, e.dtype, g.size, e.size)
        if not np.array_equal(_bits(g), _bits(e)):
            bad = np.nonzero(g.reshape(-1) != e.reshape(-1))[0]
            raise AssertionError((what, k, "first differences at", bad[:5].tolist(), g.reshape(-1)[bad[:5]].tolist(), e.reshape(-1)[bad[:5]].tolist()))


def _t(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).cuda()              # (a copy: the shared maps are read-only)


def _tab(m, conv=lambda v: v):
    return {k: conv(m.get(k)) for k in TABLES}


def _expect(name, m, rob=1):
    """the restatement's problem, computed once per map and left unchanged"""
    if (name, rob) not in _EXPECT:
        _EXPECT[(name, rob)] = npg.assemble(m, is_robust=rob)
    return _EXPECT[(name, rob)]


def _caps(m):
    return (m["nkf"] if m["ba_kf"] is None else min(m["nkf"], len(m["ba_kf"]))), (m["npts"] if m["ba_pt"] is None else min(m["npts"], len(m["ba_pt"]))), len(m["obs_kf"])


def _poison_lists(cap):
    return {k: np.full(w * cap[c], 99 if dt == np.uint8 else gc.POISON, dt) for k, (dt, w, c) in ASM_DT.items()}


def _asm_host(m, rob=1, caps=None, **kw):
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    cap = _caps(m) if caps is None else caps
    pres = _poison_lists(cap)
    r = lc.global_ba_assemble(_tab(m), ba_kf=m["ba_kf"], ba_pt=m["ba_pt"], is_robust=rob, caps=cap, out=pres, **kw)
    n = [int(v) for v in r["counts"]] if r["rc"] == 0 else [0, 0, 0]
    for k, (dt, w, c) in ASM_DT.items():                            # what lies behind the lists is not touched
        assert np.all(pres[k][w * n[c]:] == (99 if dt == np.uint8 else dt(gc.POISON))), k
    return r


def _asm_device(m, rob=1, caps=None, tab=None):
    import torch
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    cap = _caps(m) if caps is None else caps
    pres = {k: _t(v) for k, v in _poison_lists(cap).items()}
    r = lc.global_ba_assemble(_tab(m, _t) if tab is None else tab, ba_kf=_t(m["ba_kf"]), ba_pt=_t(m["ba_pt"]), is_robust=rob, caps=cap, out=pres, device=True)
    torch.cuda.synchronize()
    o = {k: r[k].cpu().numpy() for k in ASM_KEYS}
    o["status"] = int(r["status"].item()) & 0xFFFFFFFF
    n = [int(v) for v in o["counts"]]
    for k, (dt, w, c) in ASM_DT.items():
        m_ = min(n[c], cap[c])
        assert np.all(o[k][w * m_:] == (99 if dt == np.uint8 else dt(gc.POISON))), k
        o[k] = o[k][:w * m_]
    return o


def _asm_both(m, what, exp, rob=1):
    _same(_asm_host(m, rob), exp, what + " host", ASM_KEYS)
    d = _asm_device(m, rob)
    _same(d, exp, what + " device", ASM_KEYS)
    assert d["status"] == 0, what


def _poison_nd(m):
    n = m["npts"]
    return dict(normal=np.full((n, 3), gc.POISON), min_max=np.full((n, 2), gc.POISON, np.float32), nd_written=np.full(n, 77, np.uint8))


def _expect_apply(m, prob, stage, normals=True):
    kw = {k: v for k, v in _poison_nd(m).items() if k != "nd_written"} if (normals and stage == 0) else {}
    return npg.apply(m, *prob, stage=stage, normals=normals, **kw)


def _ap_host(m, prob, stage, normals=True):
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    r = lc.global_ba_apply(*prob, _tab(m), stage=stage, normals=normals, out=_poison_nd(m) if (normals and stage == 0) else None)
    for k, s in (("kf_Tcw", (-1, 12)), ("kf_center", (-1, 3)), ("X", (-1, 3)), ("kf_gba_Tcw", (-1, 12)), ("pt_gba_X", (-1, 3))):
        if r.get(k) is not None:
            r[k] = r[k].reshape(s)
    return r


def _ap_device(m, prob, stage, normals=True, tab=None, n=None):
    import torch
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    out = {k: _t(v) for k, v in _poison_nd(m).items()} if (normals and stage == 0) else None
    tab = _tab(m, _t) if tab is None else tab
    if stage and tab.get("kf_gba_Tcw") is not None:
        tab["kf_in_gba"] = _t(np.full(m["nkf"], 55, np.uint8)); tab["pt_in_gba"] = _t(np.full(m["npts"], 55, np.uint8))
    r = lc.global_ba_apply(*[_t(v) for v in prob], tab, stage=stage, normals=normals, out=out, device=True, n=n)
    torch.cuda.synchronize()
    o = {k: (None if r.get(k) is None else r[k].cpu().numpy()) for k in (AP1_KEYS if stage else AP0_KEYS)}
    o["status"] = int(r["status"].item()) & 0xFFFFFFFF
    return o


def _ap_both(m, prob, stage, what, normals=True):
    exp = _expect_apply(m, prob, stage, normals)
    keys = AP1_KEYS if stage else AP0_KEYS
    h = _ap_host(m, prob, stage, normals)
    _same(h, exp, what + " host", keys)
    d = _ap_device(m, prob, stage, normals)
    _same(d, exp, what + " device", keys)
    assert d["status"] == 0, what
    return exp, h


@pytest.mark.parametrize("name", sorted(HAND))
def test_assemble_hand_cases_host_and_device(name):
    m, rob, hand = HAND[name]
    exp = _expect("hand " + name, m, rob)
    for k, v in hand.items():
        assert np.array_equal(exp[k], np.asarray(v, exp[k].dtype).reshape(exp[k].shape)), k
    _asm_both(m, name, exp, rob)


@pytest.mark.parametrize("name,m", SEEDED, ids=[n for n, _ in SEEDED])
def test_assemble_seeded_host_and_device(name, m):
    _asm_both(m, name, _expect(name, m))


def test_assemble_same_bytes_on_two_runs():
    name, m = SEEDED[3]
    a, b = _asm_device(m), _asm_device(m)
    for k in ASM_KEYS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize("which", [0, 1, 2])
def test_capacity_one_short(which):
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    name, m = SEEDED[1]
    exp = _expect(name, m)
    cap = [int(v) for v in exp["counts"]]
    cap[which] -= 1
    r = _asm_host(m, caps=tuple(cap), check=False)                    # (_asm_host: every list still holds its poison)
    assert r["rc"] == lc.ECAP and r["counts"].tolist() == exp["counts"].tolist() and set(r) == {"rc", "counts"}
    with pytest.raises(Exception, match="wanted"):
        _asm_host(m, caps=tuple(cap))
    d = _asm_device(m, caps=tuple(cap))                              # (_asm_device: nothing behind the capacity is written)
    assert d["status"] == (lc.GA_CAP_CAM, lc.GA_CAP_PTS, lc.GA_CAP_OBS)[which] and d["counts"].tolist() == exp["counts"].tolist()
    for k, (dt, w, c) in ASM_DT.items():
        e = np.asarray(exp[k]).reshape(-1)[:w * cap[c]]
        assert np.array_equal(_bits(d[k]), _bits(e)), k
    assert np.array_equal(d["kf_cam"], exp["kf_cam"]) and np.array_equal(d["pt_idx"], exp["pt_idx"])


def test_device_out_of_range_entries_count_as_absent():
    """inputs the kernels bounds-check: every one sets its status bit and the rest of the problem is what the restatement gives without it"""
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    name, m = SEEDED[0]
    nkf, npts = m["nkf"], m["npts"]

    def run(changed, absent, bit):
        d = _asm_device(changed)
        _same(d, npg.assemble(absent), str(bit), ASM_KEYS)
        assert d["status"] == bit, (bit, d["status"])
    # a list entry out of range: the entry is not there
    q = dict(m); q["ba_kf"] = m["ba_kf"].copy(); q["ba_kf"][2] = nkf
    a = dict(m); a["ba_kf"] = np.delete(m["ba_kf"], 2)
    d = _asm_device(q); e = npg.assemble(a)
    assert d["status"] == lc.GA_KF and np.array_equal(d["cam_kf"], e["cam_kf"]) and np.array_equal(d["gobs_src"], e["gobs_src"]) and np.array_equal(d["gpt_pt"], e["gpt_pt"])
    q = dict(m); q["ba_pt"] = m["ba_pt"].copy(); q["ba_pt"][5] = -3
    a = dict(m); a["ba_pt"] = np.delete(m["ba_pt"], 5)
    run(q, a, lc.GA_PT)
    # a point twice: its first position counts
    q = dict(m); q["ba_pt"] = np.concatenate([m["ba_pt"], m["ba_pt"][:3]])
    d = _asm_device(q, caps=_caps(m))
    _same(d, _expect(name, m), "repeat", ASM_KEYS)
    assert d["status"] == lc.GA_REPEAT
    # an observer or a level out of range: the observation gives no row
    exp = _expect(name, m)
    e0 = int(exp["gobs_src"][4])
    for key, val, bit in (("obs_kf", nkf + 5, lc.GA_KF), ("obs_level", 8, lc.GA_LEVEL), ("obs_level", -1, lc.GA_LEVEL)):
        q = dict(m); q[key] = m[key].copy(); q[key][e0] = val
        d = _asm_device(q)
        assert d["status"] == bit and e0 not in d["gobs_src"].tolist() and d["counts"][2] == exp["counts"][2] - 1
    # offsets that leave the array: the point has no list
    p = int(exp["gpt_pt"][2])
    q = dict(m); q["obs_off"] = m["obs_off"].copy(); q["obs_off"][p + 1] = len(m["obs_kf"]) + 7
    d = _asm_device(q)
    assert d["status"] & lc.GA_OFFSETS and d["pt_idx"][p] == -1


@pytest.mark.parametrize("stage", [0, 1])
def test_apply_hand_case_host_and_device(stage):
    m, prob, s0, s1 = gc.hand_apply_case()
    exp, _ = _ap_both(m, prob, stage, "hand stage %d" % stage)
    hand = s1 if stage else s0
    for k, v in hand.items():
        if k not in ("normal6", "min_max6"):
            assert np.array_equal(exp[k], np.asarray(v, exp[k].dtype).reshape(exp[k].shape)), k
    if stage == 0:
        assert np.array_equal(exp["normal"][6], hand["normal6"]) and np.array_equal(exp["min_max"][6], np.array(hand["min_max6"], np.float32))
        _ap_both(m, prob, 0, "hand without normals", normals=False)


@pytest.mark.parametrize("name,m", SEEDED[:5], ids=[n for n, _ in SEEDED[:5]])
@pytest.mark.parametrize("stage", [0, 1])
def test_apply_seeded_host_and_device(name, m, stage):
    from ceres_mono_orb_slam2_amd import localmapping as lm
    asm = _expect(name, m)
    p7, p3 = gc.solver_result(11, asm)
    w = gc.turned_bad(12, m, asm)
    w["kf_gba_Tcw"] = np.full((m["nkf"], 12), gc.POISON); w["pt_gba_X"] = np.full((m["npts"], 3), gc.POISON)
    exp, got = _ap_both(w, (asm["cam_kf"], asm["gpt_pt"], p7, p3), stage, name)
    assert 0 < exp["counts"][0] < asm["counts"][0] and 0 < exp["counts"][1] < asm["counts"][1]
    if stage:
        return
    # normals and depth ranges: orbl_update_map_points on the call's own output, bit for bit
    wrote_pt = np.zeros(m["npts"], bool); wrote_pt[asm["gpt_pt"]] = True; wrote_pt &= w["pt_bad"] == 0
    good = (wrote_pt & (m["pt_ref_kf"] >= 0)).astype(np.uint8)
    ref = lm.update_map_points(m["obs_off"], X=got["X"], ref_kf=m["pt_ref_kf"], ref_level=m["ref_level"], obs_kf=m["obs_kf"], kf_center=got["kf_center"],
                               scale_factors=m["scale_factors"], pt_good=good, what=lm.MP_NORMAL_DEPTH, out=_poison_nd(m))
    wn = np.asarray(got["nd_written"]) != 0
    assert wn.sum() == exp["counts"][2] > 0 and np.array_equal(wn, (ref["nd_written"] == 1) & wrote_pt)
    assert np.array_equal(_bits(got["normal"][wn]), _bits(ref["normal"][wn])) and np.array_equal(_bits(got["min_max"][wn]), _bits(ref["min_max"][wn]))
    assert np.all(got["normal"][~wn] == gc.POISON) and np.all(got["min_max"][~wn] == np.float32(gc.POISON))      # rows of other points are untouched


def test_apply_device_status_bits():
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    name, m = SEEDED[0]
    asm = _expect(name, m)
    p7, p3 = gc.solver_result(13, asm)
    ck, gp = asm["cam_kf"], asm["gpt_pt"]
    base = npg.apply(m, ck, gp, p7, p3, stage=1)
    # a pose that is not finite, a zero quaternion: the camera is not written
    for at, val in ((7 * 2 + 1, np.nan), (7 * 2 + 5, np.inf), (slice(7 * 2 + 3, 7 * 2 + 7), 0.0)):
        q7 = p7.copy(); q7.reshape(-1)[at] = val
        d = _ap_device(m, (ck, gp, q7, p3), 1)
        assert d["status"] == lc.GA_POSE and d["kf_in_gba"][ck[2]] == 0 and d["counts"][0] == base["counts"][0] - 1
        keep = np.arange(len(ck)) != 2
        _same(d, npg.apply(m, ck[keep], gp, p7[keep], p3, stage=1), "pose", AP1_KEYS)
    # a keyframe listed twice: the last one counts; out-of-range entries are absent
    ck2 = np.concatenate([ck, ck[:1]]); q7 = np.concatenate([p7, p7[3:4]])
    d = _ap_device(m, (ck2, gp, q7, p3), 1)
    assert d["status"] == lc.GA_KF
    _same(d, npg.apply(m, ck2, gp, q7, p3, stage=1), "twice", AP1_KEYS)
    ck3 = ck.copy(); ck3[1] = m["nkf"]
    gp3 = gp.copy(); gp3[0] = -1
    d = _ap_device(m, (ck3, gp3, p7, p3), 0)
    assert d["status"] == lc.GA_KF | lc.GA_PT
    keep = np.arange(len(ck)) != 1
    e = _expect_apply(m, (ck[keep], gp[1:], p7[keep], p3[1:]), 0)
    _same(d, e, "absent", AP0_KEYS)


def _chain_tables(m, asm, seed):
    """a parent tree rooted at the first camera's keyframe (the map's keyframe 0: in the BA, not bad), for orbl_propagate_global_ba"""
    rng = np.random.RandomState(seed)
    nkf = m["nkf"]
    root = int(asm["cam_kf"][0])
    order = [root] + [k for k in rng.permutation(nkf) if k != root]
    parent = np.full(nkf, -1, np.int32)
    for i in range(1, nkf):
        parent[order[i]] = order[int(rng.randint(max(0, i - 4), i))]
    return parent, np.array([root], np.int32), np.where(m["pt_ref_kf"] < 0, 0, m["pt_ref_kf"]).astype(np.int32)


@pytest.mark.parametrize("name,m", [SEEDED[0], SEEDED[3]], ids=[SEEDED[0][0], SEEDED[3][0]])
def test_chain_on_device_tables_to_propagate_global_ba(name, m):
    """assemble on the device, solve ONCE, apply that one solution with stage 1 through the device and through the restatement, feed both to
    propagate_global_ba (device and tests/npmapcorrect.py): every table bit for bit.  No step depends on the solver repeating its bits."""
    import torch
    from ceres_mono_orb_slam2_amd import loopclosing as lc, optimizer
    exp = _expect(name, m)
    tab = _tab(m, _t)
    tab["kf_gba_Tcw"] = None; tab["pt_gba_X"] = None
    asm = lc.global_ba_assemble(tab, ba_kf=_t(m["ba_kf"]), ba_pt=_t(m["ba_pt"]), device=True)
    torch.cuda.synchronize()
    assert int(asm["status"].item()) == 0
    n = [int(v) for v in asm["counts"].cpu()]
    for k, (dt, w, c) in ASM_DT.items():
        assert np.array_equal(_bits(asm[k][:w * n[c]].cpu().numpy()), _bits(exp[k])), k
    p7, p3, _ = optimizer.bundle_adjustment(exp["K4"], exp["poses7"], exp["cam_fixed"], exp["pts3"], exp["gobs_cam"], exp["gobs_pt"], exp["gobs_uv"], exp["gobs_weight"],
                                            exp["gobs_robust"], n_iterations=10)
    assert np.all(np.isfinite(p7)) and np.all(np.isfinite(p3))          # (whatever the solve left is written back; the maps' rows are not a consistent scene)
    ap = lc.global_ba_apply(asm["cam_kf"], asm["gpt_pt"], _t(p7.reshape(-1)), _t(p3.reshape(-1)), tab, stage=1, device=True, n=(n[0], n[1]))
    ea = npg.apply(m, exp["cam_kf"], exp["gpt_pt"], p7, p3, stage=1)
    snap = {k: ap[k].clone() for k in AP1_KEYS}                       # (propagate_global_ba completes kf_gba_Tcw and kf_in_gba in place)
    parent, origins, ref = _chain_tables(m, exp, 21)
    g = lc.propagate_global_ba(tab["kf_Tcw"], ap["kf_gba_Tcw"], ap["kf_in_gba"], _t(parent), _t(origins), tab["X"], _t(ref), kf_center=tab["kf_center"], pt_bad=tab["pt_bad"],
                               pt_in_gba=ap["pt_in_gba"], pt_gba_X=ap["pt_gba_X"], device=True)
    torch.cuda.synchronize()
    assert int(ap["status"].item()) == 0 and int(g["status"].item()) == 0
    _same({k: snap[k].cpu().numpy() for k in AP1_KEYS}, ea, name + " apply", AP1_KEYS)
    pr = dict(nkf=m["nkf"], npts=m["npts"], kf_Tcw=m["kf_Tcw"], kf_gba_Tcw=ea["kf_gba_Tcw"], kf_in_gba=ea["kf_in_gba"], kf_parent=parent, origin_kf=origins,
              kf_center=m["kf_center"], X=m["X"], pt_bad=m["pt_bad"], pt_in_gba=ea["pt_in_gba"], pt_gba_X=ea["pt_gba_X"], pt_ref_kf=ref)
    eg = npm.propagate_global_ba(pr)
    assert eg["counts"][0] == m["nkf"] and eg["counts"][1] > 0 and eg["counts"][2] > 0
    _same({k: g[k].cpu().numpy() for k in ("kf_Tcw", "kf_gba_Tcw", "kf_in_gba", "kf_center", "X", "kf_reached", "pt_moved", "counts")}, eg, name + " propagate",
          ("kf_Tcw", "kf_gba_Tcw", "kf_in_gba", "kf_center", "X", "kf_reached", "pt_moved", "counts"))


def test_on_tables_host_and_device_and_no_camera():
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    name, m = SEEDED[0]
    stop = np.ones(1, np.uint8)                                       # a raised stop flag: the write-back still runs
    r = lc.global_bundle_adjustment_on_tables(_tab(m), ba_kf=m["ba_kf"], ba_pt=m["ba_pt"], n_iterations=5, stop_flag=stop, stage=1)
    exp = _expect(name, m)
    assert r["applied"] is not None and r["applied"]["counts"].tolist() == [int(exp["counts"][0]), int(exp["counts"][1]), 0]
    tab = _tab(m, _t)
    d = lc.global_bundle_adjustment_on_tables(tab, ba_kf=_t(m["ba_kf"]), ba_pt=_t(m["ba_pt"]), n_iterations=5, stage=0, device=True)
    e = npg.apply(m, exp["cam_kf"], exp["gpt_pt"], d["poses7"], d["pts3"], stage=0)
    _same({k: d["applied"][k].cpu().numpy() for k in ("kf_Tcw", "kf_center", "X", "normal", "min_max", "nd_written", "counts")}, e, "on tables", AP0_KEYS)
    none = lc.global_bundle_adjustment_on_tables(_tab(m), ba_kf=np.zeros(0, np.int32), ba_pt=m["ba_pt"])
    assert none["applied"] is None and none["summary"] is None and none["assembled"]["counts"].tolist() == [0, 0, 0]
