"""CPU checks of the map-correction entry points (include/orbslam_hip.h: orbl_correct_loop*, orbl_propagate_global_ba*): the symbols are
exported and listed, every argument error is ORBHIP_EINVAL before any device work, a valid call without a GPU is ORBHIP_ENODEV (no CPU
fallback), the workspace sizes are the documented host arithmetic, and the drop-in test program compiles and links."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import mapcorrectcases as mc  # noqa: E402

EINVAL, ENODEV = -1, -2
NAMES = ("orbl_correct_loop", "orbl_correct_loop_device", "orbl_correct_loop_workspace", "orbl_propagate_global_ba", "orbl_propagate_global_ba_device",
         "orbl_propagate_global_ba_workspace")
ML_IN = ("kf_Tcw", "kf_center", "conn_kf", "conn_rank", "Scw", "slot_off", "slot_pt", "X", "pt_bad", "pt_done", "obs_off", "obs_kf", "ref_kf", "ref_level", "scale_factors")
ML_OUT = ("corrected", "non_corrected", "pt_owner", "normal", "min_max", "nd_written", "counts")
GB_IN = ("kf_Tcw", "kf_gba_Tcw", "kf_in_gba", "kf_parent", "origin_kf", "kf_center", "X", "pt_bad", "pt_in_gba", "pt_gba_X", "pt_ref_kf")
GB_OUT = ("kf_bef_Tcw", "kf_reached", "pt_moved", "counts")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


def _loop(lib, pr, null=(), nkf=None, nconn=None, npts=None, n_levels=None):
    L = lib.load()
    v = {k: (None if pr[k] is None else np.array(pr[k])) for k in ML_IN}
    n, nc = pr["npts"], len(pr["conn_kf"])
    v.update(corrected=np.zeros((nc, 7)), non_corrected=np.zeros((nc, 7)), pt_owner=np.zeros(n, np.int32), normal=np.zeros((n, 3)), min_max=np.zeros((n, 2), np.float32),
             nd_written=np.zeros(n, np.uint8), counts=np.zeros(2, np.int32))
    if pr["obs_off"] is None:
        null = tuple(null) + ("normal", "min_max", "nd_written")

    def a(k):
        return None if (k in null or v[k] is None) else lib.ptr(v[k])
    return L.orbl_correct_loop(pr["nkf"] if nkf is None else nkf, a("kf_Tcw"), a("kf_center"), nc if nconn is None else nconn, a("conn_kf"), a("conn_rank"), a("Scw"),
                               a("slot_off"), a("slot_pt"), n if npts is None else npts, a("X"), a("pt_bad"), a("pt_done"), a("obs_off"), a("obs_kf"), a("ref_kf"),
                               a("ref_level"), a("scale_factors"), (8 if pr["obs_off"] is not None else 0) if n_levels is None else n_levels,
                               *[a(k) for k in ML_OUT])


def _gba(lib, pr, null=(), nkf=None, n_origin=None, npts=None):
    L = lib.load()
    v = {k: (None if pr[k] is None else np.array(pr[k])) for k in GB_IN}
    v.update(kf_bef_Tcw=np.zeros((pr["nkf"], 12)), kf_reached=np.zeros(pr["nkf"], np.uint8), pt_moved=np.zeros(pr["npts"], np.uint8), counts=np.zeros(4, np.int32))

    def a(k):
        return None if (k in null or v[k] is None) else lib.ptr(v[k])
    return L.orbl_propagate_global_ba(pr["nkf"] if nkf is None else nkf, a("kf_Tcw"), a("kf_gba_Tcw"), a("kf_in_gba"), a("kf_parent"),
                                      len(pr["origin_kf"]) if n_origin is None else n_origin, a("origin_kf"), a("kf_center"), pr["npts"] if npts is None else npts,
                                      a("X"), a("pt_bad"), a("pt_in_gba"), a("pt_gba_X"), a("pt_ref_kf"), *[a(k) for k in GB_OUT])


def _changed(pr, key, at, value):
    q = dict(pr); q[key] = np.array(pr[key]); q[key].reshape(-1)[at] = value
    return q


def test_symbols_are_exported_listed_and_declared(lib):
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "orbslam_hip.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in lib.SYMBOLS and ("int %s(" % name) in hdr
    from ceres_mono_orb_slam2_amd import loopclosing
    for f in ("correct_loop", "correct_loop_device", "propagate_global_ba", "propagate_global_ba_device"):
        assert callable(getattr(loopclosing, f))


def test_correct_loop_argument_errors_are_einval_before_device_work(lib):
    L = lib.load()
    pr = mc.make_loop(3, nconn=5, npts=60, max_slots=30)
    live = [p for p in range(pr["npts"]) if pr["obs_off"][p] < pr["obs_off"][p + 1] and not pr["pt_bad"][p]][0]
    ch = _changed
    cases = {
        "nkf 0": dict(pr=pr, nkf=0), "nconn 0": dict(pr=pr, nconn=0), "negative npts": dict(pr=pr, npts=-1),
        "n_levels 0": dict(pr=pr, n_levels=0), "n_levels 65": dict(pr=pr, n_levels=65),
        "slot_off not from 0": dict(pr=ch(pr, "slot_off", 0, 1)), "slot_off decreases": dict(pr=ch(pr, "slot_off", 2, 0)),
        "obs_off not from 0": dict(pr=ch(pr, "obs_off", 0, 1)), "obs_off decreases": dict(pr=ch(pr, "obs_off", 7, 0)),
        "connected keyframe too large": dict(pr=ch(pr, "conn_kf", 1, pr["nkf"])), "connected keyframe negative": dict(pr=ch(pr, "conn_kf", 0, -1)),
        "duplicate connected keyframe": dict(pr=ch(pr, "conn_kf", 3, pr["conn_kf"][1])),
        "rank too large": dict(pr=ch(pr, "conn_rank", 2, 5)), "rank negative": dict(pr=ch(pr, "conn_rank", 2, -1)), "rank repeats": dict(pr=ch(pr, "conn_rank", 2, pr["conn_rank"][3])),
        "slot point too large": dict(pr=ch(pr, "slot_pt", 7, pr["npts"])), "slot point below -1": dict(pr=ch(pr, "slot_pt", 0, -2)),
        "observer too large": dict(pr=ch(pr, "obs_kf", 3, pr["nkf"])), "observer negative": dict(pr=ch(pr, "obs_kf", -1, -1)),
        "reference keyframe too large": dict(pr=ch(pr, "ref_kf", live, pr["nkf"])), "reference keyframe negative": dict(pr=ch(pr, "ref_kf", live, -1)),
        "level too large": dict(pr=ch(pr, "ref_level", live, 8)), "level negative": dict(pr=ch(pr, "ref_level", live, -1)),
        "Scw NaN": dict(pr=ch(pr, "Scw", 5, np.nan)), "Scw inf": dict(pr=ch(pr, "Scw", 1, np.inf)), "Scw zero quaternion": dict(pr=dict(pr, Scw=np.array([0, 0, 0, 0, 1.0, 2, 3]))),
        "NULL kf_Tcw": dict(pr=pr, null=("kf_Tcw",)), "NULL conn_kf": dict(pr=pr, null=("conn_kf",)), "NULL Scw": dict(pr=pr, null=("Scw",)),
        "NULL slot_off": dict(pr=pr, null=("slot_off",)), "NULL slot_pt": dict(pr=pr, null=("slot_pt",)), "NULL X": dict(pr=pr, null=("X",)),
        "NULL corrected": dict(pr=pr, null=("corrected",)), "NULL non_corrected": dict(pr=pr, null=("non_corrected",)), "NULL pt_owner": dict(pr=pr, null=("pt_owner",)),
        "NULL counts": dict(pr=pr, null=("counts",)), "normal set without obs_off": dict(pr=pr, null=("obs_off",)), "normal set without obs_kf": dict(pr=pr, null=("obs_kf",)),
        "normal set without ref_kf": dict(pr=pr, null=("ref_kf",)), "normal set without scale_factors": dict(pr=pr, null=("scale_factors",)),
        "normal set without normal": dict(pr=pr, null=("normal",)), "normal set without nd_written": dict(pr=pr, null=("nd_written",)),
        "normals without kf_center": dict(pr=pr, null=("kf_center",)),
    }
    for what, kw in cases.items():
        assert _loop(lib, **kw) == EINVAL, what
        assert b"orbl_correct_loop" in L.orbhip_last_error(), what
    # the device form checks counts, NULLs and alignment on the host
    z = C.c_void_p(256)                                             # (never dereferenced: every call below fails its checks first)
    args = [4, z, z, 2, z, z, z, 5, z, z, 6, z, None, None, 9, z, z, z, z, z, 8, z, z, z, z, z, z, z, None, z, None]
    for at, value in ((0, 0), (3, 0), (7, -1), (10, -1), (14, -1), (20, 0), (20, 65), (1, None), (4, None), (6, None), (8, None), (9, None), (11, None), (21, None), (22, None),
                      (23, None), (27, None), (29, None), (15, None), (17, None), (19, None), (24, None), (26, None), (2, None), (1, C.c_void_p(260)), (11, C.c_void_p(252)),
                      (4, C.c_void_p(258)), (25, C.c_void_p(258)), (29, C.c_void_p(260)), (28, C.c_void_p(257))):
        b = list(args); b[at] = value
        assert L.orbl_correct_loop_device(*b) == EINVAL, at


def test_propagate_global_ba_argument_errors_are_einval_before_device_work(lib):
    L = lib.load()
    pr = mc.make_gba(4, 12, npts=40)
    live = [p for p in range(pr["npts"]) if not pr["pt_bad"][p] and not pr["pt_in_gba"][p]][0]
    child = int(np.nonzero(pr["kf_parent"] >= 0)[0][0])
    ch = _changed
    cases = {
        "negative nkf": dict(pr=pr, nkf=-1), "negative n_origin": dict(pr=pr, n_origin=-1), "negative npts": dict(pr=pr, npts=-1),
        "origin too large": dict(pr=ch(pr, "origin_kf", 0, 12)), "origin negative": dict(pr=ch(pr, "origin_kf", 1, -1)),
        "parent too large": dict(pr=ch(pr, "kf_parent", child, 12)), "parent below -1": dict(pr=ch(pr, "kf_parent", child, -2)), "parent is itself": dict(pr=ch(pr, "kf_parent", child, child)),
        "reference keyframe too large": dict(pr=ch(pr, "pt_ref_kf", live, 12)), "reference keyframe negative": dict(pr=ch(pr, "pt_ref_kf", live, -1)),
        "NULL kf_Tcw": dict(pr=pr, null=("kf_Tcw",)), "NULL kf_gba_Tcw": dict(pr=pr, null=("kf_gba_Tcw",)), "NULL kf_in_gba": dict(pr=pr, null=("kf_in_gba",)),
        "NULL kf_parent": dict(pr=pr, null=("kf_parent",)), "NULL origin_kf": dict(pr=pr, null=("origin_kf",)), "NULL X": dict(pr=pr, null=("X",)),
        "NULL pt_ref_kf": dict(pr=pr, null=("pt_ref_kf",)), "NULL kf_bef_Tcw": dict(pr=pr, null=("kf_bef_Tcw",)), "NULL kf_reached": dict(pr=pr, null=("kf_reached",)),
        "NULL pt_moved": dict(pr=pr, null=("pt_moved",)), "NULL counts": dict(pr=pr, null=("counts",)),
        "pt_in_gba without pt_gba_X": dict(pr=pr, null=("pt_gba_X",)), "pt_gba_X without pt_in_gba": dict(pr=pr, null=("pt_in_gba",)),
    }
    for what, kw in cases.items():
        assert _gba(lib, **kw) == EINVAL, what
        assert b"orbl_propagate_global_ba" in L.orbhip_last_error(), what
    z = C.c_void_p(256)
    args = [4, z, z, z, z, 1, z, None, 6, z, None, z, z, z, z, z, z, z, None, z, None]
    for at, value in ((0, -1), (5, -1), (8, -1), (1, None), (2, None), (3, None), (4, None), (6, None), (9, None), (13, None), (14, None), (15, None), (16, None), (17, None),
                      (19, None), (11, None), (12, None), (1, C.c_void_p(260)), (14, C.c_void_p(260)), (4, C.c_void_p(258)), (17, C.c_void_p(258)), (18, C.c_void_p(257))):
        b = list(args); b[at] = value
        assert L.orbl_propagate_global_ba_device(*b) == EINVAL, at


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_calls_without_gpu_are_enodev(lib):
    from ceres_mono_orb_slam2_amd import loopclosing
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()
    pr = mc.make_loop(3, nconn=5, npts=60, max_slots=30)
    assert _loop(lib, pr) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _loop(lib, pr, null=("conn_rank", "pt_bad", "pt_done", "obs_off", "obs_kf", "ref_kf", "ref_level", "scale_factors", "normal", "min_max", "nd_written", "kf_center")) == ENODEV
    with pytest.raises(OrbHipError, match="no HIP device"):
        loopclosing.correct_loop(pr["kf_Tcw"], pr["conn_kf"], pr["Scw"], pr["slot_off"], pr["slot_pt"], pr["X"])
    pg = mc.make_gba(4, 12, npts=40)
    assert _gba(lib, pg) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _gba(lib, pg, null=("kf_center", "pt_bad", "pt_in_gba", "pt_gba_X")) == ENODEV
    with pytest.raises(OrbHipError, match="no HIP device"):
        loopclosing.propagate_global_ba(pg["kf_Tcw"], pg["kf_gba_Tcw"], pg["kf_in_gba"], pg["kf_parent"], pg["origin_kf"], pg["X"], pg["pt_ref_kf"])


def test_workspace_arithmetic(lib):
    L = lib.load()
    n = C.c_size_t(0)

    def up(x):
        return (x + 255) // 256 * 256
    for nkf, nconn, npts in ((1, 1, 0), (8, 3, 257), (500, 40, 100000), (1100, 65, 3000)):
        assert L.orbl_correct_loop_workspace(nkf, nconn, npts, C.byref(n)) == 0
        assert n.value == up(4 * nconn) + up(npts) + up(4 * nkf) + up(8 * npts) + up(4 * nconn) + up(56 * nconn) + up(96 * nconn) + up(24 * nconn)
        assert L.orbl_propagate_global_ba_workspace(nkf, npts, C.byref(n)) == 0 and n.value == max(up(nkf), 256)
    assert L.orbl_propagate_global_ba_workspace(0, 0, C.byref(n)) == 0 and n.value == 256
    for bad in ((-1, 1, 1), (1, -1, 1), (1, 1, -1)):
        assert L.orbl_correct_loop_workspace(*bad, C.byref(n)) == EINVAL
    assert L.orbl_correct_loop_workspace(1, 1, 1, None) == EINVAL
    assert L.orbl_propagate_global_ba_workspace(-1, 0, C.byref(n)) == EINVAL and L.orbl_propagate_global_ba_workspace(0, -1, C.byref(n)) == EINVAL
    assert L.orbl_propagate_global_ba_workspace(1, 1, None) == EINVAL


def test_dropin_test_program_compiles_and_links(lib, tmp_path):
    exe = tmp_path / "test_mapcorrect_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_mapcorrect_dropin.cpp"), "-o", str(exe), lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    assert exe.exists()
