"""orbl_local_ba_assemble(_device) and orbl_local_ba_apply(_device) on the MI355X against the restatement tests/nplocalba.py (the literal
loops of src/CeresOptimizer.cc:346-406, :423-506, :573-598): every output is compared bit for bit, as uint8 views - the 64-bit arithmetic
is IEEE +, *, / and sqrt in a stated order, without fused multiply-add.  Rows a call must leave alone are poisoned first.
tests/test_localba_restatement.py shows that the maps tell the reference's orders from an order-blind implementation."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import localbacases as lc  # noqa: E402
from tests import nplocalba as npl  # noqa: E402
from tests.test_localba_restatement import seeded  # noqa: E402

pytestmark = pytest.mark.gpu

ASM_LISTS = ("cam_kf", "K4", "poses7", "cam_fixed", "cam_local", "lpt_pt", "pts3", "lobs_cam", "lobs_pt", "lobs_uv", "lobs_inv_sigma2", "lobs_src")
ASM_KEYS = ASM_LISTS + ("kf_role", "pt_local", "counts")
ASM_DT = dict(cam_kf=(np.int32, 1, 0), K4=(np.float64, 4, 0), poses7=(np.float64, 7, 0), cam_fixed=(np.uint8, 1, 0), cam_local=(np.uint8, 1, 0), lpt_pt=(np.int32, 1, 1),
              pts3=(np.float64, 3, 1), lobs_cam=(np.int32, 1, 2), lobs_pt=(np.int32, 1, 2), lobs_uv=(np.float64, 2, 2), lobs_inv_sigma2=(np.float32, 1, 2), lobs_src=(np.int32, 1, 2))
AP_KEYS = ("kf_Tcw", "kf_center", "kf_slot_pt", "X", "pt_bad", "pt_nobs", "pt_ref_kf", "obs_erased", "normal", "min_max", "nd_written", "counts")
TABLES = ("kf_id", "kf_bad", "kf_rank", "kf_Tcw", "kf_K4", "kf_slot_off", "kf_slot_pt", "X", "pt_bad", "pt_rank", "obs_off", "obs_kf", "obs_uv", "obs_level", "inv_level_sigma2",
          "kf_center", "pt_nobs", "pt_ref_kf", "obs_slot", "kf_level0", "scale_factors")
HAND = lc.hand_assemble_cases()


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


def _tab(m, conv=lambda v: v, apply=False):
    t = {k: conv(m.get(k)) for k in TABLES}
    if apply and m.get("pt_bad") is None:
        t["pt_bad"] = conv(np.zeros(m["npts"], np.uint8))
    return t


def _caps(m):
    return m["nkf"], m["npts"], len(m["obs_kf"])


def _poison_lists(m, caps=None):
    cap = _caps(m) if caps is None else caps
    return {k: np.full(w * cap[c], 99 if dt == np.uint8 else lc.POISON, dt) for k, (dt, w, c) in ASM_DT.items()}


def _asm_host(m, **kw):
    from ceres_mono_orb_slam2_amd import localmapping as lm
    pres = _poison_lists(m, kw.get("caps"))
    r = lm.local_ba_assemble(m["cur_kf"], m["nbr_kf"], _tab(m), out=pres, **kw)
    if r["rc"] == 0:
        n = (int(r["counts"][0]), int(r["counts"][2]), int(r["counts"][3]))
        for k, (dt, w, c) in ASM_DT.items():                        # what lies behind the lists is not touched
            assert np.all(pres[k][w * n[c]:] == (99 if dt == np.uint8 else dt(lc.POISON))), k
    return r


def _asm_device(m, caps=None):
    import torch
    from ceres_mono_orb_slam2_amd import localmapping as lm
    cap = _caps(m) if caps is None else caps
    pres = {k: _t(v) for k, v in _poison_lists(m, cap).items()}
    r = lm.local_ba_assemble(m["cur_kf"], _t(m["nbr_kf"]), _tab(m, _t), caps=cap, out=pres, device=True)
    torch.cuda.synchronize()
    o = {k: r[k].cpu().numpy() for k in ASM_KEYS}
    o["status"] = int(r["status"].item()) & 0xFFFFFFFF
    n = (int(o["counts"][0]), int(o["counts"][2]), int(o["counts"][3]))
    for k, (dt, w, c) in ASM_DT.items():
        m_ = min(n[c], cap[c])
        assert np.all(o[k][w * m_:] == (99 if dt == np.uint8 else dt(lc.POISON))), k
        o[k] = o[k][:w * m_]
    return o


def _asm_both(m, what, exp=None):
    exp = npl.assemble(m) if exp is None else exp
    _same(_asm_host(m), exp, what + " host", ASM_KEYS)
    d = _asm_device(m)
    _same(d, exp, what + " device", ASM_KEYS)
    assert d["status"] == 0, what
    return exp


def _poison_nd(m):
    n = m["npts"]
    return dict(normal=np.full((n, 3), lc.POISON), min_max=np.full((n, 2), lc.POISON, np.float32), nd_written=np.full(n, 77, np.uint8))


def _expect_apply(m, asm, res, normals=True):
    kw = {k: v for k, v in _poison_nd(m).items() if k != "nd_written"} if normals else {}
    return npl.apply(m, asm, *res, normals=normals, **kw)


def _ap_host(m, asm, res, normals=True):
    from ceres_mono_orb_slam2_amd import localmapping as lm
    r = lm.local_ba_apply(asm, *res, _tab(m, apply=True), normals=normals, out=_poison_nd(m) if normals else None)
    for k, s in (("kf_Tcw", (-1, 12)), ("kf_center", (-1, 3)), ("X", (-1, 3))):
        r[k] = None if r[k] is None else r[k].reshape(s)
    return r


def _ap_device_enqueue(m, asm, res, normals=True, tab=None, n=None):
    from ceres_mono_orb_slam2_amd import localmapping as lm
    a = {k: _t(asm[k]) for k in ("cam_kf", "cam_local", "lpt_pt", "lobs_src")}
    n = (len(asm["cam_kf"]), len(asm["lpt_pt"]), len(asm["lobs_src"])) if n is None else n
    out = {k: _t(v) for k, v in _poison_nd(m).items()} if normals else None
    return lm.local_ba_apply(a, _t(res[0]), _t(res[1]), _t(res[2]), _tab(m, _t, apply=True) if tab is None else tab, normals=normals, out=out, device=True, n=n)


def _down(r, keys):
    import torch
    torch.cuda.synchronize()
    o = {k: (None if r.get(k) is None else r[k].cpu().numpy()) for k in keys}
    o["status"] = int(r["status"].item()) & 0xFFFFFFFF
    return o


def _ap_both(m, asm, res, what, exp=None, normals=True):
    exp = _expect_apply(m, asm, res, normals) if exp is None else exp
    _same(_ap_host(m, asm, res, normals), exp, what + " host", AP_KEYS)
    d = _down(_ap_device_enqueue(m, asm, res, normals), AP_KEYS)
    _same(d, exp, what + " device", AP_KEYS)
    assert d["status"] == 0, what
    return exp


@pytest.mark.parametrize("name", sorted(HAND))
def test_assemble_hand_cases_host_and_device(name):
    m, hand = HAND[name]
    exp = _asm_both(m, name)
    for k, v in hand.items():
        assert exp[k].tolist() == v, (name, k)


def test_apply_hand_case_host_and_device():
    m, res, hand = lc.hand_apply_case()
    exp = _ap_both(m, npl.assemble(m), res, "hand apply")
    for k in ("kf_slot_pt", "pt_bad", "pt_nobs", "pt_ref_kf", "obs_erased", "counts", "nd_written"):
        assert exp[k].tolist() == hand[k], k


def test_seeded_maps_host_and_device_equal_the_restatement():
    for name, m, asm, res, out in seeded():
        _asm_both(m, name, asm)
        exp = _expect_apply(m, asm, res)
        assert np.array_equal(exp["pt_nobs"], out["pt_nobs"])
        _ap_both(m, asm, res, name, exp)


def test_without_the_optional_arguments():
    name, m, asm, res, _ = seeded()[0]
    q = dict(m); q.update(kf_bad=None, kf_rank=None, pt_bad=None, pt_rank=None, kf_level0=None)
    a = _asm_both(q, "no flags or ranks")
    r = lc.solver_result(77, q, a)
    _ap_both(q, a, r, "no kf_level0")
    _ap_both(q, a, r, "no normals", normals=False)
    q["kf_center"] = None
    _ap_both(q, a, r, "no centres either", normals=False)


def test_capacities_ecap_with_the_wanted_counts_and_cap_bits():
    from ceres_mono_orb_slam2_amd import localmapping as lm
    name, m, asm, res, _ = seeded()[1]
    want = asm["counts"].tolist()
    full = (want[0], want[2], want[3])
    _same(_asm_host(m, caps=full), asm, "exact capacities", ASM_KEYS)
    for i, bit in ((0, lm.LA_CAP_CAM), (1, lm.LA_CAP_PTS), (2, lm.LA_CAP_OBS)):
        cap = list(full); cap[i] -= 1
        r = _asm_host(m, caps=tuple(cap), check=False)
        assert r["rc"] == lm.ECAP and r["counts"].tolist() == want and set(r) == {"rc", "counts"}
        d = _asm_device(m, caps=tuple(cap))
        assert d["status"] == bit and d["counts"].tolist() == want
        for k, (dt, w, c) in ASM_DT.items():                        # what fits is written, in its place
            assert np.array_equal(_bits(d[k]), _bits(np.asarray(asm[k]).reshape(-1)[:w * cap[c]])), (k, i)
    with pytest.raises(lm._lib.OrbHipError, match="wanted %d cameras" % want[0]):
        _asm_host(m, caps=(0, 0, 0))


def test_assemble_device_status_bits_and_absent_entries():
    from ceres_mono_orb_slam2_amd import localmapping as lm
    name, m, asm, res, _ = seeded()[3]
    nkf, npts = m["nkf"], m["npts"]

    def changed(**ch):
        q = dict(m)
        for k, (at, v) in ch.items():
            q[k] = np.array(m[k]); q[k][at] = v
        return q
    # a neighbour out of range is not in the list
    q = dict(m); q["nbr_kf"] = np.concatenate([[nkf, -1], m["nbr_kf"], [2 ** 30]]).astype(np.int32)
    d = _asm_device(q)
    assert d["status"] == lm.LA_KF
    _same(d, asm, "neighbour", ASM_KEYS)
    # a slot naming a point out of range is an empty slot
    s = int(m["kf_slot_off"][m["cur_kf"]]) + int(np.nonzero(m["kf_slot_pt"][m["kf_slot_off"][m["cur_kf"]]:m["kf_slot_off"][m["cur_kf"] + 1]] >= 0)[0][0])
    exp = npl.assemble(changed(kf_slot_pt=(s, -1)))
    for v in (npts, -2):
        d = _asm_device(changed(kf_slot_pt=(s, v)))
        assert d["status"] == lm.LA_PT
        _same(d, exp, "slot point %d" % v, ASM_KEYS)
    # an observer or a level out of range: the observation gives no row (as if a bad neighbour, stamped and without a camera, held it)
    row = next(i for i in range(len(asm["lobs_src"])) if asm["cam_local"][asm["lobs_cam"][i]])
    e = int(asm["lobs_src"][row])
    exp = npl.assemble(changed(obs_kf=(e, int(np.nonzero(asm["kf_role"] == 3)[0][0]))))
    for key, v, bit in (("obs_kf", nkf, lm.LA_KF), ("obs_kf", -1, lm.LA_KF), ("obs_level", 8, lm.LA_LEVEL), ("obs_level", -1, lm.LA_LEVEL)):
        d = _asm_device(changed(**{key: (e, v)}))
        assert d["status"] == bit, (key, v)
        _same(d, exp, "%s %d" % (key, v), ASM_KEYS)
    # a keyframe whose slots run past nslots has none; a point whose list does is not read
    d = _asm_device(changed(kf_slot_off=(nkf, len(m["kf_slot_pt"]) + 5)))
    assert d["status"] & lm.LA_OFFSETS
    # ranks that are no permutations: the bit
    assert _asm_device(changed(kf_rank=(0, int(m["kf_rank"][1]))))["status"] & lm.LA_RANK
    assert _asm_device(changed(pt_rank=(3, npts)))["status"] & lm.LA_RANK


def test_apply_device_status_bits_and_absent_entries():
    from ceres_mono_orb_slam2_amd import localmapping as lm
    name, m, asm, res, _ = seeded()[2]
    base = _expect_apply(m, asm, res)
    nobs = len(m["obs_kf"])
    # a row naming an observation out of range erases nothing
    i = int(np.nonzero(res[2] == 0)[0][0])
    for v in (nobs, -1):
        a = dict(asm); a["lobs_src"] = asm["lobs_src"].copy(); a["lobs_src"][i] = v
        r = (res[0], res[1], res[2].copy()); r[2][i] = 1
        d = _down(_ap_device_enqueue(m, a, r), AP_KEYS)
        assert d["status"] == lm.LA_OBS
        _same(d, base, "lobs_src %d" % v, AP_KEYS)
    # an observation naming a slot its keyframe does not have: the observation dies, no slot is written
    e = int(np.nonzero(base["obs_erased"])[0][0])
    k = int(m["obs_kf"][e])
    q = dict(m); q["obs_slot"] = m["obs_slot"].copy(); q["obs_slot"][e] = int(m["kf_slot_off"][k + 1] - m["kf_slot_off"][k])
    d = _down(_ap_device_enqueue(q, asm, res), AP_KEYS)
    assert d["status"] == lm.LA_OBS
    exp = dict(base); exp["kf_slot_pt"] = base["kf_slot_pt"].copy()
    s = int(m["kf_slot_off"][k]) + int(m["obs_slot"][e])
    if not any(base["obs_erased"][f] and f != e and int(m["kf_slot_off"][m["obs_kf"][f]]) + int(m["obs_slot"][f]) == s for f in range(nobs)):
        exp["kf_slot_pt"][s] = m["kf_slot_pt"][s]
    _same(d, exp, "obs_slot", AP_KEYS)
    # a camera or a local point out of range is not moved
    c = int(np.nonzero(asm["cam_local"])[0][0])
    a = dict(asm); a["cam_kf"] = asm["cam_kf"].copy(); a["cam_kf"][c] = m["nkf"]
    assert _down(_ap_device_enqueue(m, a, res), AP_KEYS)["status"] & lm.LA_KF
    a = dict(asm); a["lpt_pt"] = asm["lpt_pt"].copy(); a["lpt_pt"][0] = -1
    assert _down(_ap_device_enqueue(m, a, res), AP_KEYS)["status"] & lm.LA_PT


def test_chain_on_resident_tensors_and_the_abort_path():
    """device assemble -> optimizer.local_bundle_adjustment -> device apply on resident tables, against the restatement's apply fed the SAME
    downloaded solver outputs (nothing rests on the solver being bit-reproducible); with the stop flag up every table stays bit-identical"""
    import torch
    from ceres_mono_orb_slam2_amd import localmapping as lm
    m = _ba_map()
    asm = npl.assemble(m)
    tab = _tab(m, _t, apply=True)
    before = {k: (None if v is None else v.clone()) for k, v in tab.items()}
    stop = np.ones(1, np.uint8)
    r = lm.local_bundle_adjustment_on_tables(m["cur_kf"], _t(m["nbr_kf"]), tab, stop_flag=stop, device=True)
    torch.cuda.synchronize()
    assert r["aborted"] == 1 and r["applied"] is None
    for k, v in before.items():
        assert v is None or torch.equal(v, tab[k]), k
    r = lm.local_bundle_adjustment_on_tables(m["cur_kf"], _t(m["nbr_kf"]), tab, out={k: _t(v) for k, v in _poison_nd(m).items()}, device=True)
    assert r["aborted"] == 0 and 0 < int(r["solved"][2].sum()) < len(r["solved"][2])
    d = _down(r["assembled"], ASM_KEYS)
    n = (int(d["counts"][0]), int(d["counts"][2]), int(d["counts"][3]))
    for k, (dt, w, c) in ASM_DT.items():
        d[k] = d[k][:w * n[c]]
    _same(d, asm, "chain assemble", ASM_KEYS)
    exp = _expect_apply(m, asm, r["solved"])
    _same(_down(r["applied"], AP_KEYS), exp, "chain apply", AP_KEYS)


def _ba_map():
    """a map whose observations are the projections of its points (a pixel of noise, a few gross outliers), so that the solve converges and
    erases some rows: 10 keyframes on a line looking down z, 400 points in front of them"""
    rng = np.random.RandomState(5)
    nkf, npts = 10, 400
    Tcw = np.array([lc._pose((-0.3 * k, 0.02 * rng.randn(), 0.0)) for k in range(nkf)])
    X = np.column_stack([rng.uniform(-1, 4, npts), rng.uniform(-1.5, 1.5, npts), rng.uniform(4, 9, npts)])
    slots = [[] for _ in range(nkf)]
    obs, uv, lvl = [], [], []
    for p in range(npts):
        ks = sorted(rng.permutation(nkf)[:int(rng.randint(3, 8))].tolist())
        obs.append(ks)
        for k in ks:
            slots[k].append(p)
            T = Tcw[k].reshape(3, 4)
            xc = T[:, :3] @ X[p] + T[:, 3]
            u = lc.K4[0] * xc[0] / xc[2] + lc.K4[2] + rng.randn() * 0.5; v = lc.K4[1] * xc[1] / xc[2] + lc.K4[3] + rng.randn() * 0.5
            if rng.rand() < 0.03:
                u += 40.0
            uv.append((u, v)); lvl.append(int(rng.randint(0, 3)))
    return lc.table_map(7, [6, 8, 5, 9, 4], Tcw, np.arange(nkf) + 1, slots, X + 0.02 * rng.randn(npts, 3), obs, obs_uv=uv, obs_level=lvl, kf_level0=[0] * nkf)


def test_apply_empty_inputs_host_and_device():
    """no points, no observations, no rows: one local camera is still moved; then nothing at all"""
    m, _ = HAND["empty inputs"]
    asm = npl.assemble(m)
    res = (np.array([[-5.0, 1.0, 2.0, 0.0, 0.0, 0.0, 2.0]]), np.zeros((0, 3)), np.zeros(0, np.uint8))
    exp = _ap_both(m, asm, res, "empty apply")
    assert exp["kf_center"].tolist() == [[5.0, -1.0, -2.0]] and exp["counts"].tolist() == [0, 0, 0, 0] and exp["obs_erased"].size == 0
    none = dict(asm); none.update(cam_kf=asm["cam_kf"][:0], cam_local=asm["cam_local"][:0])
    exp = _ap_both(m, none, (np.zeros((0, 7)), res[1], res[2]), "nothing to apply")
    assert np.array_equal(exp["kf_Tcw"], m["kf_Tcw"])


def test_apply_device_offsets_bit():
    """a point whose list runs past the observation arrays has no list: nothing of it is erased, it gets no normal, its position is still set"""
    from ceres_mono_orb_slam2_amd import localmapping as lm
    name, m, asm, res, _ = seeded()[0]
    npts, nobs = m["npts"], len(m["obs_kf"])
    p = npts - 1
    assert m["obs_off"][p] < nobs                                # (the last point has a list)
    mine = np.array([int(m["obs_off"][p]) <= int(e) < nobs for e in asm["lobs_src"]])
    r = (res[0], res[1], np.where(mine, 0, res[2]).astype(np.uint8))
    q = dict(m); q["obs_off"] = m["obs_off"].copy(); q["obs_off"][npts] = nobs + 3
    e = dict(m); e["obs_off"] = m["obs_off"].copy(); e["obs_off"][npts] = m["obs_off"][p]
    d = _down(_ap_device_enqueue(q, asm, r), AP_KEYS)
    assert d["status"] == lm.LA_OFFSETS
    _same(d, _expect_apply(e, asm, r), "obs_off past nobs", AP_KEYS)
