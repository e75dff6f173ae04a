"""CPU checks of the LocalBundleAdjustment-on-the-tables entry points (include/orbslam_hip.h: orbl_local_ba_assemble*, orbl_local_ba_apply*):
the symbols are exported and listed, every argument error is ORBHIP_EINVAL before any device work, a valid call without a GPU is
ORBHIP_ENODEV (no CPU fallback), the workspace sizes are the documented host arithmetic, and the drop-in test program compiles and links."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import localbacases as lc  # noqa: E402
from tests import nplocalba as npl  # noqa: E402

EINVAL, ENODEV = -1, -2
NAMES = ("orbl_local_ba_assemble", "orbl_local_ba_assemble_device", "orbl_local_ba_assemble_workspace", "orbl_local_ba_apply", "orbl_local_ba_apply_device",
         "orbl_local_ba_apply_workspace")
LA_IN = ("nbr_kf", "kf_id", "kf_bad", "kf_rank", "kf_Tcw", "kf_K4", "kf_slot_off", "kf_slot_pt", "X", "pt_bad", "pt_rank", "obs_off", "obs_kf", "obs_uv", "obs_level",
         "inv_level_sigma2")
LA_OUT = (("counts", np.int32, 4), ("cam_kf", np.int32, 1), ("K4", np.float64, 4), ("poses7", np.float64, 7), ("cam_fixed", np.uint8, 1), ("cam_local", np.uint8, 1),
          ("lpt_pt", np.int32, 1), ("pts3", np.float64, 3), ("lobs_cam", np.int32, 1), ("lobs_pt", np.int32, 1), ("lobs_uv", np.float64, 2), ("lobs_inv_sigma2", np.float32, 1),
          ("lobs_src", np.int32, 1), ("kf_role", np.uint8, 1), ("pt_local", np.uint8, 1))
AP_IN = ("cam_kf", "cam_local", "poses7", "lpt_pt", "pts3", "lobs_src", "obs_erase", "kf_Tcw", "kf_center", "kf_slot_off", "kf_slot_pt", "X", "pt_bad", "pt_nobs", "pt_ref_kf",
         "obs_off", "obs_kf", "obs_slot", "obs_level", "kf_level0", "scale_factors")
AP_OUT = ("obs_erased", "normal", "min_max", "nd_written", "counts")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def world():
    m = lc.make_map(11, 14, 120, half=3)
    asm = npl.assemble(m)
    poses7, pts3, erase = lc.solver_result(12, m, asm)
    ap = dict(m)
    ap.update(cam_kf=asm["cam_kf"], cam_local=asm["cam_local"], poses7=poses7, lpt_pt=asm["lpt_pt"], pts3=pts3, lobs_src=asm["lobs_src"], obs_erase=erase)
    return m, ap


def _assemble(lib, m, null=(), cur=None, nkf=None, npts=None, n_nbr=None, n_levels=8, caps=None):
    L = lib.load()
    v = {k: (None if m[k] is None else np.array(m[k])) for k in LA_IN}
    n = max(m["nkf"], m["npts"], len(m["obs_kf"]), 4)
    v.update({k: np.zeros(w * n, dt) for k, dt, w in LA_OUT})

    def a(k):
        return None if (k in null or v[k] is None) else lib.ptr(v[k])
    cap = (n, n, n) if caps is None else caps
    return L.orbl_local_ba_assemble(m["cur_kf"] if cur is None else cur, len(m["nbr_kf"]) if n_nbr is None else n_nbr, a("nbr_kf"), m["nkf"] if nkf is None else nkf,
                                    *[a(k) for k in LA_IN[1:8]], m["npts"] if npts is None else npts, *[a(k) for k in LA_IN[8:]], n_levels, *cap,
                                    *[a(k) for k, _, _ in LA_OUT])


def _apply(lib, p, null=(), ncam=None, npl_=None, nol=None, nkf=None, npts=None, n_levels=8):
    L = lib.load()
    v = {k: (None if p[k] is None else np.array(p[k])) for k in AP_IN}
    v.update(obs_erased=np.zeros(len(p["obs_kf"]), np.uint8), normal=np.zeros((p["npts"], 3)), min_max=np.zeros((p["npts"], 2), np.float32), nd_written=np.zeros(p["npts"], np.uint8),
             counts=np.zeros(4, np.int32))

    def a(k):
        return None if (k in null or v[k] is None) else lib.ptr(v[k])
    return L.orbl_local_ba_apply(len(p["cam_kf"]) if ncam is None else ncam, a("cam_kf"), a("cam_local"), a("poses7"), len(p["lpt_pt"]) if npl_ is None else npl_, a("lpt_pt"),
                                 a("pts3"), len(p["lobs_src"]) if nol is None else nol, a("lobs_src"), a("obs_erase"), p["nkf"] if nkf is None else nkf,
                                 *[a(k) for k in AP_IN[7:11]], p["npts"] if npts is None else npts, *[a(k) for k in AP_IN[11:]], n_levels, *[a(k) for k in AP_OUT])


def _changed(pr, key, at, value):
    q = dict(pr); q[key] = np.array(pr[key]); q[key].reshape(-1)[at] = value
    return q


def test_symbols_are_exported_listed_and_declared(lib):
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "orbslam_hip.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in lib.SYMBOLS and ("int %s(" % name) in hdr
    from ceres_mono_orb_slam2_amd import localmapping
    for f in ("local_ba_assemble", "local_ba_assemble_device", "local_ba_apply", "local_ba_apply_device", "local_bundle_adjustment_on_tables"):
        assert callable(getattr(localmapping, f))


def test_assemble_argument_errors_are_einval_before_device_work(lib, world):
    L = lib.load()
    m, _ = world
    ch = _changed
    nkf, npts = m["nkf"], m["npts"]
    cases = {
        "nkf 0": dict(m=m, nkf=0), "negative npts": dict(m=m, npts=-1), "negative n_nbr": dict(m=m, n_nbr=-1), "cur_kf too large": dict(m=m, cur=nkf),
        "cur_kf negative": dict(m=m, cur=-1), "n_levels 0": dict(m=m, n_levels=0), "n_levels 65": dict(m=m, n_levels=65), "negative capacity": dict(m=m, caps=(4, -1, 4)),
        "kf_slot_off not from 0": dict(m=ch(m, "kf_slot_off", 0, 1)), "kf_slot_off decreases": dict(m=ch(m, "kf_slot_off", 2, 0)),
        "obs_off not from 0": dict(m=ch(m, "obs_off", 0, 1)), "obs_off decreases": dict(m=ch(m, "obs_off", 7, 0)),
        "neighbour too large": dict(m=ch(m, "nbr_kf", 1, nkf)), "neighbour negative": dict(m=ch(m, "nbr_kf", 0, -1)),
        "slot point too large": dict(m=ch(m, "kf_slot_pt", 7, npts)), "slot point below -1": dict(m=ch(m, "kf_slot_pt", 0, -2)),
        "observer too large": dict(m=ch(m, "obs_kf", 3, nkf)), "observer negative": dict(m=ch(m, "obs_kf", -1, -1)),
        "level too large": dict(m=ch(m, "obs_level", 5, 8)), "level negative": dict(m=ch(m, "obs_level", 5, -1)),
        "kf_rank too large": dict(m=ch(m, "kf_rank", 2, nkf)), "kf_rank repeats": dict(m=ch(m, "kf_rank", 2, m["kf_rank"][3])),
        "pt_rank negative": dict(m=ch(m, "pt_rank", 2, -1)), "pt_rank repeats": dict(m=ch(m, "pt_rank", 2, m["pt_rank"][3])),
    }
    for k in ("nbr_kf", "kf_id", "kf_Tcw", "kf_K4", "kf_slot_off", "kf_slot_pt", "X", "obs_off", "obs_kf", "obs_uv", "obs_level", "inv_level_sigma2") + tuple(k for k, _, _ in LA_OUT):
        cases["NULL " + k] = dict(m=m, null=(k,))
    for what, kw in cases.items():
        assert _assemble(lib, **kw) == EINVAL, what
        assert b"orbl_local_ba_assemble" in L.orbhip_last_error(), what
    # the device form checks counts, NULLs and alignment on the host
    z = C.c_void_p(256)                                             # (never dereferenced: every call below fails its checks first)
    args = [1, 2, z, 4, z, None, None, z, z, 9, z, z, 6, z, None, None, 12, z, z, z, z, z, 8, 4, 6, 12] + [z] * 15 + [None, z, None]
    assert len(args) == len(L.orbl_local_ba_assemble_device.argtypes)
    for at, value in ((0, 4), (0, -1), (1, -1), (3, 0), (9, -1), (12, -1), (16, -1), (22, 0), (22, 65), (23, -1), (24, -1), (25, -1), (2, None), (4, None), (7, None), (8, None),
                      (10, None), (11, None), (13, None), (17, None), (18, None), (19, None), (20, None), (21, None), (26, None), (27, None), (28, None), (29, None), (30, None),
                      (31, None), (32, None), (33, None), (34, None), (35, None), (36, None), (37, None), (38, None), (39, None), (40, None), (42, None),
                      (7, C.c_void_p(260)), (13, C.c_void_p(252)), (29, C.c_void_p(260)), (4, C.c_void_p(258)), (19, C.c_void_p(258)), (37, C.c_void_p(258)),
                      (42, C.c_void_p(260)), (41, C.c_void_p(257))):
        b = list(args); b[at] = value
        assert L.orbl_local_ba_assemble_device(*b) == EINVAL, at


def test_apply_argument_errors_are_einval_before_device_work(lib, world):
    L = lib.load()
    _, p = world
    ch = _changed
    nkf, npts, nobs = p["nkf"], p["npts"], len(p["obs_kf"])
    loc = int(np.nonzero(p["cam_local"])[0][0])
    live = next(int(j) for j in p["lpt_pt"] if p["obs_off"][j] < p["obs_off"][j + 1])
    e = 3
    width = int(p["kf_slot_off"][p["obs_kf"][e] + 1] - p["kf_slot_off"][p["obs_kf"][e]])
    cases = {
        "negative ncam": dict(p=p, ncam=-1), "negative npts_local": dict(p=p, npl_=-1), "negative nobs_local": dict(p=p, nol=-1), "negative nkf": dict(p=p, nkf=-1),
        "negative npts": dict(p=p, npts=-1), "n_levels 0": dict(p=p, n_levels=0), "n_levels 65": dict(p=p, n_levels=65),
        "kf_slot_off not from 0": dict(p=ch(p, "kf_slot_off", 0, 1)), "obs_off decreases": dict(p=ch(p, "obs_off", 7, 0)),
        "camera keyframe too large": dict(p=ch(p, "cam_kf", 1, nkf)), "camera keyframe negative": dict(p=ch(p, "cam_kf", 0, -1)),
        "local point too large": dict(p=ch(p, "lpt_pt", 2, npts)), "local point negative": dict(p=ch(p, "lpt_pt", 0, -1)),
        "row source too large": dict(p=ch(p, "lobs_src", 2, nobs)), "row source negative": dict(p=ch(p, "lobs_src", 0, -1)),
        "observer too large": dict(p=ch(p, "obs_kf", 3, nkf)), "observer negative": dict(p=ch(p, "obs_kf", -1, -1)),
        "slot past the keyframe's": dict(p=ch(p, "obs_slot", e, width)), "slot negative": dict(p=ch(p, "obs_slot", e, -1)),
        "level too large": dict(p=ch(p, "obs_level", 5, 8)), "level negative": dict(p=ch(p, "obs_level", 5, -1)), "kf_level0 too large": dict(p=ch(p, "kf_level0", 1, 8)),
        "reference keyframe too large": dict(p=ch(p, "pt_ref_kf", live, nkf)), "reference keyframe negative": dict(p=ch(p, "pt_ref_kf", live, -1)),
        "pose NaN": dict(p=ch(p, "poses7", 7 * loc + 1, np.nan)), "pose inf": dict(p=ch(p, "poses7", 7 * loc + 4, np.inf)),
        "pose zero quaternion": dict(p=ch(p, "poses7", slice(7 * loc + 3, 7 * loc + 7), 0.0)),
        "normal set without normal": dict(p=p, null=("normal",)), "normal set without min_max": dict(p=p, null=("min_max",)),
        "normal set without nd_written": dict(p=p, null=("nd_written",)), "normal set without scale_factors": dict(p=p, null=("scale_factors",)),
        "normals without kf_center": dict(p=p, null=("kf_center",)), "normals without obs_level": dict(p=p, null=("obs_level",)),
    }
    for k in ("cam_kf", "cam_local", "poses7", "lpt_pt", "pts3", "lobs_src", "obs_erase", "kf_Tcw", "kf_slot_off", "kf_slot_pt", "X", "pt_bad", "pt_nobs", "pt_ref_kf", "obs_off",
              "obs_kf", "obs_slot", "obs_erased", "counts"):
        cases["NULL " + k] = dict(p=p, null=(k,))
    for what, kw in cases.items():
        assert _apply(lib, **kw) == EINVAL, what
        assert b"orbl_local_ba_apply" in L.orbhip_last_error(), what
    z = C.c_void_p(256)
    args = [3, z, z, z, 5, z, z, 7, z, z, 4, z, z, 9, z, z, 6, z, z, z, z, 12, z, z, z, z, None, z, 8, z, z, z, z, z, None, z, None]
    assert len(args) == len(L.orbl_local_ba_apply_device.argtypes)
    for at, value in ((0, -1), (4, -1), (7, -1), (10, -1), (13, -1), (16, -1), (21, -1), (28, 0), (28, 65), (1, None), (2, None), (3, None), (5, None), (6, None), (8, None), (9, None),
                      (11, None), (14, None), (15, None), (17, None), (18, None), (19, None), (20, None), (22, None), (23, None), (24, None), (29, None), (33, None), (35, None),
                      (30, None), (31, None), (32, None), (27, None), (12, None), (25, None), (3, C.c_void_p(260)), (17, C.c_void_p(252)), (30, C.c_void_p(260)),
                      (1, C.c_void_p(258)), (24, C.c_void_p(258)), (31, C.c_void_p(258)), (35, C.c_void_p(260)), (34, C.c_void_p(257))):
        b = list(args); b[at] = value
        assert L.orbl_local_ba_apply_device(*b) == EINVAL, at


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_calls_without_gpu_are_enodev(lib, world):
    from ceres_mono_orb_slam2_amd import localmapping
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()
    m, p = world
    assert _assemble(lib, m) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _assemble(lib, m, null=("kf_bad", "kf_rank", "pt_bad", "pt_rank")) == ENODEV
    assert _apply(lib, p) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _apply(lib, p, null=("kf_level0",)) == ENODEV
    assert _apply(lib, p, null=("normal", "min_max", "nd_written", "scale_factors", "kf_center", "obs_level", "kf_level0")) == ENODEV
    with pytest.raises(OrbHipError, match="no HIP device"):
        localmapping.local_ba_assemble(m["cur_kf"], m["nbr_kf"], m)
    with pytest.raises(OrbHipError, match="no HIP device"):
        localmapping.local_ba_apply(p, p["poses7"], p["pts3"], p["obs_erase"], p)
    with pytest.raises(OrbHipError, match="no HIP device"):
        localmapping.local_bundle_adjustment_on_tables(m["cur_kf"], m["nbr_kf"], m)
    for hm in [v[0] for v in lc.hand_assemble_cases().values()]:
        assert _assemble(lib, hm) == ENODEV


def test_workspace_arithmetic(lib):
    L = lib.load()
    n = C.c_size_t(0)

    def up(x):
        return (x + 255) // 256 * 256
    for nkf, npts, nobs in ((1, 0, 0), (8, 257, 1000), (500, 100000, 600001), (1100, 3000, 7)):
        assert L.orbl_local_ba_assemble_workspace(nkf, npts, C.byref(n)) == 0
        assert n.value == 3 * up(4 * nkf) + up(4 * npts) + up(nkf) + up(8 * nkf) + up(8 * ((nkf + 255) // 256 + 1)) + up(8 * npts) + up(8 * ((npts + 255) // 256 + 1)) + 256
        assert L.orbl_local_ba_apply_workspace(nobs, C.byref(n)) == 0 and n.value == max(up(4 * nobs), 256)
    for bad in ((-1, 1), (1, -1)):
        assert L.orbl_local_ba_assemble_workspace(*bad, C.byref(n)) == EINVAL
    assert L.orbl_local_ba_assemble_workspace(1, 1, None) == EINVAL
    assert L.orbl_local_ba_apply_workspace(-1, C.byref(n)) == EINVAL and L.orbl_local_ba_apply_workspace(1, None) == EINVAL


def test_dropin_test_program_compiles_and_links(lib, tmp_path):
    exe = tmp_path / "test_localba_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_localba_dropin.cpp"), "-o", str(exe), lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    assert exe.exists()
