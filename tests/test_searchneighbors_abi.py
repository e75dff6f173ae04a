"""CPU checks of the SearchInNeighbors entry points (include/orbslam_hip.h: orbl_fuse_targets*, orbl_fuse_rows*, orbl_fuse_candidates*,
orbl_update_map_points_on_tables*): the symbols are exported and listed, every argument error is ORBHIP_EINVAL before any device work, a
valid call without a GPU is ORBHIP_ENODEV (no CPU fallback), and the workspace sizes are the documented host arithmetic."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import searchneighborscases as sc  # noqa: E402

EINVAL, ENODEV = -1, -2
NAMES = [e + s for e in ("orbl_fuse_targets", "orbl_fuse_rows", "orbl_fuse_candidates", "orbl_update_map_points_on_tables") for s in ("", "_device", "_workspace")]
ROW_KF = ("kf_Tcw", "kf_center", "kf_K4", "kf_bounds", "kf_slot_off", "kf_slot_uv", "kf_slot_level", "kf_slot_desc")
ROW_PT = ("X", "pt_normal", "pt_min_dist", "pt_max_dist", "pt_desc", "scale_factors", "inv_level_sigma2")
ROW_OUT = ("op_kind", "op_pt", "op_arg", "op_kf", "op_slot", "best_idx", "best_dist", "q_uv", "q_level")
UPD_KF = ("kf_bad", "kf_center", "kf_slot_off", "kf_slot_pt", "kf_slot_level", "kf_slot_desc")
UPD_PT = ("pt_bad", "X", "pt_ref_kf", "obs_off", "obs_kf", "obs_slot", "scale_factors")
UPD_IO = ("pt_desc", "pt_normal", "pt_min_dist", "pt_max_dist")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def tab():
    t = sc.make(sc.SEEDS[0])["tab"]
    return {k: (None if v is None else np.ascontiguousarray(v)) for k, v in t.items()}


def _changed(t, key, at, value):
    q = dict(t); q[key] = t[key].copy(); q[key].reshape(-1)[at] = value
    return q


def _targets(lib, t, cur_kf=0, nkf=None, nn=20, nn2=5, cap=120, null=()):
    hold = dict(stamp=np.array(t["kf_fuse_target"]), tgt=np.zeros(256, np.int32), counts=np.zeros(2, np.int32))

    def a(k):
        v = hold[k] if k in hold else t.get(k)
        return None if (k in null or v is None) else lib.ptr(v)
    return lib.load().orbl_fuse_targets(cur_kf, 7, len(t["ord_off"]) - 1 if nkf is None else nkf, a("kf_bad"), a("ord_off"), a("ord_kf"), a("stamp"), nn, nn2, cap, a("tgt"),
                                        a("counts"))


def _rows(lib, t, kf=0, n=None, nkf=None, npts=None, n_levels=8, lsf=0.1823, th=3.0, null=(), pts=None):
    pts = np.arange(8, dtype=np.int32) if pts is None else pts
    hold = {k: np.zeros(64, np.float32 if k == "q_uv" else np.int32) for k in ROW_OUT}
    hold["pts"] = pts

    def a(k):
        v = hold[k] if k in hold else t.get(k)
        return None if (k in null or v is None) else lib.ptr(v)
    return lib.load().orbl_fuse_rows(kf, len(pts) if n is None else n, a("pts"), len(t["kf_slot_off"]) - 1 if nkf is None else nkf, *[a(k) for k in ROW_KF],
                                     len(t["pt_bad"]) if npts is None else npts, *[a(k) for k in ROW_PT], lsf, n_levels, th, *[a(k) for k in ROW_OUT])


def _cands(lib, t, tgt=(1, 2, 1), nkf=None, npts=None, cap=4096, null=(), n_tgt=None):
    hold = dict(tgt=np.array(tgt, np.int32), stamp=np.array(t["pt_fuse_cand"]), cand=np.zeros(4096, np.int32), counts=np.zeros(2, np.int32))

    def a(k):
        v = hold[k] if k in hold else t.get(k)
        return None if (k in null or v is None) else lib.ptr(v)
    return lib.load().orbl_fuse_candidates(len(tgt) if n_tgt is None else n_tgt, a("tgt"), len(t["kf_slot_off"]) - 1 if nkf is None else nkf, a("kf_slot_off"), a("kf_slot_pt"),
                                           len(t["pt_bad"]) if npts is None else npts, a("pt_bad"), a("stamp"), 9, cap, a("cand"), a("counts"))


def _update(lib, t, what=3, mask=True, mask_kf=0, nkf=None, npts=None, n_levels=8, null=()):
    n = len(t["pt_bad"])
    hold = {k: np.array(t[k]) for k in UPD_IO}
    hold.update(pt_mask=np.ones(n, np.uint8) if mask else None, best_obs=np.zeros(n, np.int32), nd_written=np.zeros(n, np.uint8))

    def a(k):
        v = hold[k] if k in hold else t.get(k)
        return None if (k in null or v is None) else lib.ptr(v)
    return lib.load().orbl_update_map_points_on_tables(what, a("pt_mask"), mask_kf, len(t["kf_slot_off"]) - 1 if nkf is None else nkf, *[a(k) for k in UPD_KF],
                                                       n if npts is None else npts, *[a(k) for k in UPD_PT], n_levels, *[a(k) for k in UPD_IO], a("best_obs"), a("nd_written"))


def test_symbols_are_exported_and_listed(lib):
    L = lib.load()
    for name in NAMES:
        assert hasattr(L, name) and name in lib.SYMBOLS, name
    from ceres_mono_orb_slam2_amd import localmapping
    for f in ("fuse_targets", "fuse_rows", "fuse_candidates", "update_map_points_on_tables", "search_in_neighbors_on_tables"):
        assert callable(getattr(localmapping, f)), f
    header = open(os.path.join(ROOT, "include", "orbslam_hip.h")).read()
    for name in NAMES:
        assert "int %s(" % name in header, name


def test_every_argument_error_is_einval_before_device_work(lib, tab):
    L = lib.load()
    nkf, npts = len(tab["kf_slot_off"]) - 1, len(tab["pt_bad"])
    e0 = int(tab["obs_off"][np.argmax(np.diff(tab["obs_off"]) > 0)])
    cases = {
        "targets: negative nkf": lambda: _targets(lib, tab, nkf=-1), "targets: cur_kf too large": lambda: _targets(lib, tab, cur_kf=nkf),
        "targets: cur_kf negative": lambda: _targets(lib, tab, cur_kf=-1), "targets: negative nn": lambda: _targets(lib, tab, nn=-1),
        "targets: negative nn2": lambda: _targets(lib, tab, nn2=-1), "targets: negative cap": lambda: _targets(lib, tab, cap=-1),
        "targets: ord_off not from 0": lambda: _targets(lib, _changed(tab, "ord_off", 0, 1)), "targets: ord_off decreases": lambda: _targets(lib, _changed(tab, "ord_off", 3, 0)),
        "targets: ord_kf too large": lambda: _targets(lib, _changed(tab, "ord_kf", 2, nkf)), "targets: ord_kf negative": lambda: _targets(lib, _changed(tab, "ord_kf", 2, -1)),
        "rows: negative n": lambda: _rows(lib, tab, n=-1), "rows: negative nkf": lambda: _rows(lib, tab, nkf=-1), "rows: negative npts": lambda: _rows(lib, tab, npts=-1),
        "rows: kf too large": lambda: _rows(lib, tab, kf=nkf), "rows: kf negative": lambda: _rows(lib, tab, kf=-1), "rows: no level": lambda: _rows(lib, tab, n_levels=0),
        "rows: too many levels": lambda: _rows(lib, tab, n_levels=65), "rows: log_scale_factor 0": lambda: _rows(lib, tab, lsf=0.0), "rows: th 0": lambda: _rows(lib, tab, th=0.0),
        "rows: kf_slot_off not from 0": lambda: _rows(lib, _changed(tab, "kf_slot_off", 0, 1)), "rows: kf_slot_off decreases": lambda: _rows(lib, _changed(tab, "kf_slot_off", 2, 0)),
        "rows: a point too large": lambda: _rows(lib, tab, pts=np.array([0, npts], np.int32)), "rows: a point below -1": lambda: _rows(lib, tab, pts=np.array([-2], np.int32)),
        "rows: a level too large": lambda: _rows(lib, _changed(tab, "kf_slot_level", 1, 8)), "rows: a level negative": lambda: _rows(lib, _changed(tab, "kf_slot_level", 1, -1)),
        "candidates: negative n_tgt": lambda: _cands(lib, tab, n_tgt=-1), "candidates: negative nkf": lambda: _cands(lib, tab, nkf=-1),
        "candidates: negative npts": lambda: _cands(lib, tab, npts=-1), "candidates: negative cap": lambda: _cands(lib, tab, cap=-1),
        "candidates: a target too large": lambda: _cands(lib, tab, tgt=(1, nkf)), "candidates: a target negative": lambda: _cands(lib, tab, tgt=(-1,)),
        "candidates: kf_slot_off decreases": lambda: _cands(lib, _changed(tab, "kf_slot_off", 2, 0)),
        "candidates: a slot point too large": lambda: _cands(lib, _changed(tab, "kf_slot_pt", 3, npts)), "candidates: a slot point below -1": lambda: _cands(lib, _changed(tab, "kf_slot_pt", 3, -2)),
        "update: what 0": lambda: _update(lib, tab, what=0), "update: what 4": lambda: _update(lib, tab, what=4), "update: negative nkf": lambda: _update(lib, tab, nkf=-1),
        "update: negative npts": lambda: _update(lib, tab, npts=-1), "update: mask_kf too large": lambda: _update(lib, tab, mask_kf=nkf), "update: mask_kf below -1": lambda: _update(lib, tab, mask_kf=-2),
        "update: nothing selects": lambda: _update(lib, tab, mask=False, mask_kf=-1), "update: no level": lambda: _update(lib, tab, n_levels=0),
        "update: kf_slot_off not from 0": lambda: _update(lib, _changed(tab, "kf_slot_off", 0, 1)), "update: obs_off decreases": lambda: _update(lib, _changed(tab, "obs_off", 5, -1)),
        "update: observer too large": lambda: _update(lib, _changed(tab, "obs_kf", e0, nkf)), "update: observer negative": lambda: _update(lib, _changed(tab, "obs_kf", e0, -1)),
        "update: obs_slot outside its keyframe": lambda: _update(lib, _changed(tab, "obs_slot", e0, 100000)), "update: obs_slot negative": lambda: _update(lib, _changed(tab, "obs_slot", e0, -1)),
        "update: a slot point too large": lambda: _update(lib, _changed(tab, "kf_slot_pt", 1, npts)), "update: pt_ref_kf too large": lambda: _update(lib, _changed(tab, "pt_ref_kf", 0, nkf)),
        "update: pt_ref_kf below -1": lambda: _update(lib, _changed(tab, "pt_ref_kf", 0, -2)), "update: a level too large": lambda: _update(lib, _changed(tab, "kf_slot_level", 1, 8)),
    }
    for k in ("ord_off", "ord_kf", "stamp", "tgt", "counts"):
        cases["targets: NULL " + k] = lambda k=k: _targets(lib, tab, null=(k,))
    for k in ROW_KF + ROW_PT + ROW_OUT[:5] + ("pts",):
        cases["rows: NULL " + k] = lambda k=k: _rows(lib, tab, null=(k,))
    for k in ("tgt", "kf_slot_off", "kf_slot_pt", "pt_bad", "stamp", "cand", "counts"):
        cases["candidates: NULL " + k] = lambda k=k: _cands(lib, tab, null=(k,))
    for k in UPD_KF[1:] + UPD_PT + UPD_IO:
        cases["update: NULL " + k] = lambda k=k: _update(lib, tab, null=(k,))
    for what, call in cases.items():
        assert call() == EINVAL, what
        assert b"orbl_" in L.orbhip_last_error(), what
    # the device forms check counts, NULLs and alignment on the host; no pointer below is dereferenced
    z, odd = C.c_void_p(256), C.c_void_p(258)
    ok = dict(orbl_fuse_targets_device=[0, 7, 4, z, 9, z, z, z, 20, 5, 120, z, z, z, None, None],
              orbl_fuse_rows_device=[z, 5, z, 4, z, z, z, z, z, 9, z, z, z, 6, z, z, z, z, z, z, z, 0.18, 8, 3.0, z, z, z, z, z, z, z, z, z, z, None, None],
              orbl_fuse_candidates_device=[3, z, 4, z, 9, z, 6, z, z, 9, 6, z, z, z, z, None],
              orbl_update_map_points_on_tables_device=[3, z, 0, 4, z, z, z, 9, z, z, z, 6, z, z, z, 12, z, z, z, z, 8, z, z, z, z, z, z, z, z, None])
    bad = dict(orbl_fuse_targets_device=[(2, -1), (4, -1), (8, -1), (9, -1), (10, -1), (5, None), (6, None), (7, None), (11, None), (12, None), (5, odd), (12, odd)],
               orbl_fuse_rows_device=[(1, -1), (3, -1), (9, -1), (13, -1), (22, 0), (22, 65), (21, 0.0), (23, 0.0), (0, None), (2, None), (4, None), (5, None), (6, None),
                                      (7, None), (8, None), (10, None), (11, None), (12, None), (14, None), (15, None), (16, None), (17, None), (18, None), (19, None),
                                      (20, None), (24, None), (25, None), (26, None), (27, None), (28, None), (0, odd), (12, odd), (18, odd), (4, C.c_void_p(260))],
               orbl_fuse_candidates_device=[(0, -1), (2, -1), (4, -1), (6, -1), (10, -1), (0, (1 << 24) + 1), (1, None), (3, None), (5, None), (7, None), (8, None), (11, None),
                                            (12, None), (14, None), (1, odd), (14, C.c_void_p(260))],
               orbl_update_map_points_on_tables_device=[(0, 0), (0, 4), (3, -1), (7, -1), (11, -1), (15, -1), (2, 4), (2, -2), (20, 0), (6, None), (8, None), (9, None),
                                                        (10, None), (12, None), (13, None), (14, None), (16, None), (17, None), (18, None), (19, None), (21, None),
                                                        (22, None), (23, None), (24, None), (28, None), (10, odd), (28, C.c_void_p(264))])
    for name, args in ok.items():
        f = getattr(L, name)
        assert len(args) == len(f.argtypes), name
        for at, value in bad[name]:
            b = list(args); b[at] = value
            assert f(*b) == EINVAL, (name, at)
    assert L.orbl_update_map_points_on_tables_device(*[None if i == 1 else (-1 if i == 2 else v) for i, v in enumerate(ok["orbl_update_map_points_on_tables_device"])]) == EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_call_without_gpu_is_enodev(lib, tab):
    from ceres_mono_orb_slam2_amd import localmapping
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()
    for call in (lambda: _targets(lib, tab), lambda: _targets(lib, tab, null=("kf_bad",)), lambda: _rows(lib, tab),
                 lambda: _rows(lib, tab, null=("best_idx", "best_dist", "q_uv", "q_level")), lambda: _cands(lib, tab), lambda: _update(lib, tab),
                 lambda: _update(lib, tab, what=1, mask_kf=-1, null=("kf_bad", "kf_center", "kf_slot_pt", "kf_slot_level", "X", "pt_ref_kf", "scale_factors", "pt_normal",
                                                                     "pt_min_dist", "pt_max_dist", "nd_written"))):
        assert call() == ENODEV and b"no HIP device" in L.orbhip_last_error()
    with pytest.raises(OrbHipError, match="no HIP device"):
        localmapping.fuse_rows(0, [0, 1], tab)
    with pytest.raises(OrbHipError, match="no HIP device"):
        localmapping.fuse_targets(0, 7, tab)


def test_workspace_arithmetic(lib):
    L = lib.load()
    n = C.c_size_t(7)

    def up(x):
        return (x + 255) // 256 * 256
    for v in (0, 1, 500):
        assert L.orbl_fuse_targets_workspace(v, C.byref(n)) == 0 and n.value == 0
        assert L.orbl_fuse_rows_workspace(v, C.byref(n)) == 0 and n.value == 0
    for n_tgt, npts in ((0, 0), (1, 1), (23, 341), (130, 100000)):
        assert L.orbl_fuse_candidates_workspace(n_tgt, npts, C.byref(n)) == 0 and n.value == up(8 * npts) + up(4 * (n_tgt + 1))
    for npts, nobs in ((0, 0), (1, 1), (341, 900), (100000, 600000)):
        assert L.orbl_update_map_points_on_tables_workspace(npts, nobs, C.byref(n)) == 0
        assert n.value == up(npts) + up(npts) + 2 * up(4 * npts) + up(npts) + up(8 * npts) + up(nobs) + up(32 * nobs) + up(32 + 20 * npts)
    assert L.orbl_fuse_targets_workspace(-1, C.byref(n)) == EINVAL and L.orbl_fuse_targets_workspace(1, None) == EINVAL
    assert L.orbl_fuse_rows_workspace(-1, C.byref(n)) == EINVAL and L.orbl_fuse_rows_workspace(1, None) == EINVAL
    assert L.orbl_fuse_candidates_workspace(-1, 0, C.byref(n)) == EINVAL and L.orbl_fuse_candidates_workspace(0, -1, C.byref(n)) == EINVAL
    assert L.orbl_fuse_candidates_workspace(1, 1, None) == EINVAL
    assert L.orbl_update_map_points_on_tables_workspace(-1, 0, C.byref(n)) == EINVAL and L.orbl_update_map_points_on_tables_workspace(0, -1, C.byref(n)) == EINVAL
    assert L.orbl_update_map_points_on_tables_workspace(1, 1, None) == EINVAL
