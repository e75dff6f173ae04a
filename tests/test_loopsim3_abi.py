"""CPU checks of orbl_loop_sim3_candidates / _device / _workspace (include/orbslam_hip.h): the symbols are exported, declared and bound,
every argument error is ORBHIP_EINVAL before any device work, a valid call without a GPU is ORBHIP_ENODEV (no CPU fallback), and the
workspace size is the documented host arithmetic."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import loopsim3cases as lc  # noqa: E402

EINVAL, ENODEV, ECAP = -1, -2, -4
NAMES = ["orbl_loop_sim3_candidates" + s for s in ("", "_device", "_workspace")]
KF = ("kf_bad", "kf_Tcw", "kf_K4", "kf_slot_off", "kf_slot_pt", "kf_slot_level", "kf_slot_angle", "kf_slot_desc", "kf_fv_off", "fv_node", "fv_ent_off", "fv_ent")
PT = ("pt_bad", "X", "obs_off", "obs_kf", "obs_slot")
OUT = (("match12", np.int32), ("nmatches", np.int32), ("cand_status", np.int32), ("K1", np.float32), ("K2", np.float32), ("off", np.int32), ("X1c", np.float64),
       ("X2c", np.float64), ("max_err1", np.float32), ("max_err2", np.float32), ("row_i1", np.int32), ("row_pt1", np.int32), ("row_pt2", np.int32), ("counts", np.int32))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def case():
    tab, cur, cand, _ = lc.gate_case()
    return {k: np.ascontiguousarray(v) for k, v in tab.items()}, cur, np.array(cand, np.int32)


def _changed(t, key, at, value):
    q = dict(t); q[key] = t[key].copy(); q[key].reshape(-1)[at] = value
    return q


def _call(lib, t, cur, cand, n_cand=None, nkf=None, npts=None, n_levels=8, nnratio=0.75, cap1=64, cap_rows=256, null=(), counts=None):
    hold = {k: np.full(8192, 7, dt) for k, dt in OUT}
    if counts is not None:
        hold["counts"] = counts
    hold["cand"] = cand

    def a(k):
        v = hold[k] if k in hold else t.get(k)
        return None if (k in null or v is None) else lib.ptr(v)
    return lib.load().orbl_loop_sim3_candidates(cur, len(cand) if n_cand is None else n_cand, a("cand"), len(t["kf_slot_off"]) - 1 if nkf is None else nkf,
                                                *[a(k) for k in KF], len(t["pt_bad"]) if npts is None else npts, *[a(k) for k in PT], a("level_sigma2"), n_levels,
                                                nnratio, 1, 20, cap1, cap_rows, *[a(k) for k, _ in OUT])


def test_symbols_are_exported_declared_and_bound(lib):
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "orbslam_hip.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in lib.SYMBOLS and "int %s(" % name in header, name
    decl = lib.parse_header(header)
    assert len(decl["orbl_loop_sim3_candidates"][1]) == 43 and len(decl["orbl_loop_sim3_candidates_device"][1]) == 50
    assert decl["orbl_loop_sim3_candidates"][1][24] is C.c_float and decl["orbl_loop_sim3_candidates_workspace"][1] == [C.c_int32, C.c_int32, C.c_void_p]
    from ceres_mono_orb_slam2_amd import loopclosing
    assert callable(loopclosing.sim3_candidates) and callable(loopclosing.sim3_candidates_device)


def test_every_argument_error_is_einval_before_device_work(lib, case):
    tab, cur, cand = case
    L = lib.load()
    nkf, npts = len(tab["kf_slot_off"]) - 1, len(tab["pt_bad"])
    two = np.concatenate([tab["fv_ent"][:1], tab["fv_ent"][:1]])
    cases = {
        "no candidate": lambda: _call(lib, tab, cur, cand, n_cand=0), "too many candidates": lambda: _call(lib, tab, cur, cand, n_cand=1025),
        "negative cap1": lambda: _call(lib, tab, cur, cand, cap1=-1), "cap1 beyond 32768": lambda: _call(lib, tab, cur, cand, cap1=32769),
        "negative cap_rows": lambda: _call(lib, tab, cur, cand, cap_rows=-1), "cap_rows beyond 32768 n_cand": lambda: _call(lib, tab, cur, cand, cap_rows=4 * 32768 + 1),
        "nkf 0": lambda: _call(lib, tab, cur, cand, nkf=0), "negative npts": lambda: _call(lib, tab, cur, cand, npts=-1),
        "cur_kf too large": lambda: _call(lib, tab, nkf, cand), "cur_kf negative": lambda: _call(lib, tab, -1, cand),
        "no level": lambda: _call(lib, tab, cur, cand, n_levels=0), "too many levels": lambda: _call(lib, tab, cur, cand, n_levels=65),
        "nnratio 0": lambda: _call(lib, tab, cur, cand, nnratio=0.0),
        "a candidate too large": lambda: _call(lib, tab, cur, np.array([1, nkf], np.int32)), "a candidate negative": lambda: _call(lib, tab, cur, np.array([-1], np.int32)),
        "kf_slot_off not from 0": lambda: _call(lib, _changed(tab, "kf_slot_off", 0, 1), cur, cand),
        "kf_slot_off decreases": lambda: _call(lib, _changed(tab, "kf_slot_off", 2, 0), cur, cand),
        "kf_fv_off decreases": lambda: _call(lib, _changed(tab, "kf_fv_off", 2, 0), cur, cand),
        "fv_ent_off decreases": lambda: _call(lib, _changed(tab, "fv_ent_off", 3, 0), cur, cand),
        "obs_off decreases": lambda: _call(lib, _changed(tab, "obs_off", 3, -1), cur, cand),
        "a slot point too large": lambda: _call(lib, _changed(tab, "kf_slot_pt", 3, npts), cur, cand),
        "a slot point below -1": lambda: _call(lib, _changed(tab, "kf_slot_pt", 3, -2), cur, cand),
        "a level too large": lambda: _call(lib, _changed(tab, "kf_slot_level", 1, 8), cur, cand), "a level negative": lambda: _call(lib, _changed(tab, "kf_slot_level", 1, -1), cur, cand),
        "an observer too large": lambda: _call(lib, _changed(tab, "obs_kf", 2, nkf), cur, cand), "an observer negative": lambda: _call(lib, _changed(tab, "obs_kf", 2, -1), cur, cand),
        "an obs_slot outside its keyframe": lambda: _call(lib, _changed(tab, "obs_slot", 2, 100000), cur, cand),
        "an obs_slot negative": lambda: _call(lib, _changed(tab, "obs_slot", 2, -1), cur, cand),
        "fv_node not ascending": lambda: _call(lib, _changed(tab, "fv_node", 1, int(tab["fv_node"][0])), cur, cand),
        "an fv_ent outside its keyframe": lambda: _call(lib, _changed(tab, "fv_ent", 0, 100000), cur, cand), "an fv_ent negative": lambda: _call(lib, _changed(tab, "fv_ent", 0, -1), cur, cand),
        "a keypoint named twice": lambda: _call(lib, _changed(tab, "fv_ent", 1, int(two[0])), cur, cand),
    }
    for k in KF[1:] + PT + ("level_sigma2", "cand") + tuple(k for k, _ in OUT):
        cases["NULL " + k] = lambda k=k: _call(lib, tab, cur, cand, null=(k,))
    for what, call in cases.items():
        assert call() == EINVAL, what
        assert b"orbl_loop_sim3_candidates" in L.orbhip_last_error(), what
    # a capacity is not an argument error - but it is found before any device work when the current keyframe does not fit a row
    counts = np.full(2, 7, np.int32)
    assert _call(lib, tab, cur, cand, cap1=29, counts=counts) == ECAP and counts.tolist() == [0, 0] and b"30 slots" in L.orbhip_last_error()
    # the device form checks counts, NULLs and alignment on the host; no pointer below is dereferenced
    z, odd, four = C.c_void_p(256), C.c_void_p(258), C.c_void_p(260)
    ok = [0, 3, z, 4, z, z, z, 9, z, z, z, z, z, 5, z, z, 9, z, z, 6, z, z, 12, z, z, z, z, 8, 0.75, 1, 20, 64, 128] + [z] * 14 + [z, z, None]
    f = L.orbl_loop_sim3_candidates_device
    assert len(ok) == len(f.argtypes) == 50
    bad = [(1, 0), (1, 1025), (3, -1), (7, -1), (13, -1), (16, -1), (19, -1), (22, -1), (27, 0), (27, 65), (28, 0.0), (31, -1), (31, 32769), (32, -1), (32, 3 * 32768 + 1)]
    bad += [(i, None) for i in (2, 5, 6, 8, 9, 10, 11, 12, 14, 15, 17, 18, 20, 21, 23, 24, 25, 26, 48)] + [(i, None) for i in range(33, 47)]
    bad += [(2, odd), (12, odd), (15, odd), (33, odd), (46, odd), (47, odd), (5, four), (21, four), (39, four), (40, four), (48, four)]
    for at, value in bad:
        b = list(ok); b[at] = value
        assert f(*b) == EINVAL, at


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_call_without_gpu_is_enodev(lib, case):
    tab, cur, cand = case
    from ceres_mono_orb_slam2_amd import loopclosing
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()
    for call in (lambda: _call(lib, tab, cur, cand), lambda: _call(lib, tab, cur, cand, null=("kf_bad",)), lambda: _call(lib, tab, cur, cand, cap1=30, cap_rows=0)):
        assert call() == ENODEV and b"no HIP device" in L.orbhip_last_error()
    with pytest.raises(OrbHipError, match="no HIP device"):
        loopclosing.sim3_candidates(tab, cur, cand)


def test_workspace_arithmetic(lib):
    L = lib.load()
    n = C.c_size_t(7)

    def up(x):
        return (x + 255) // 256 * 256
    for nc, cap1 in ((1, 0), (1, 1), (7, 333), (16, 2000), (1024, 32768)):
        assert L.orbl_loop_sim3_candidates_workspace(nc, cap1, C.byref(n)) == 0
        assert n.value == up(128 * nc) + up(nc * cap1) + 2 * up(4 * nc * cap1) + up(4 * (nc + 1))
    for nc, cap1 in ((0, 1), (1025, 1), (1, -1), (1, 32769)):
        assert L.orbl_loop_sim3_candidates_workspace(nc, cap1, C.byref(n)) == EINVAL
    assert L.orbl_loop_sim3_candidates_workspace(1, 1, None) == EINVAL
