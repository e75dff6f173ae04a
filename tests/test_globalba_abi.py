"""CPU checks of the GlobalBundleAdjustment-on-the-tables entry points (include/orbslam_hip.h: orbl_global_ba_assemble*,
orbl_global_ba_apply*): the symbols are exported and listed, every argument error is ORBHIP_EINVAL before any device work, a valid call
without a GPU is ORBHIP_ENODEV (no CPU fallback), the workspace sizes are the documented host arithmetic, and the drop-in test program
compiles and links."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import globalbacases as gc  # noqa: E402
from tests import npglobalba as npg  # noqa: E402

EINVAL, ENODEV = -1, -2
NAMES = ("orbl_global_ba_assemble", "orbl_global_ba_assemble_device", "orbl_global_ba_assemble_workspace", "orbl_global_ba_apply", "orbl_global_ba_apply_device",
         "orbl_global_ba_apply_workspace")
GA_KF = ("kf_id", "kf_bad", "kf_Tcw", "kf_K4")
GA_PT = ("X", "pt_bad", "obs_off", "obs_kf", "obs_uv", "obs_level", "inv_level_sigma2")
GA_OUT = (("counts", np.int32, 3), ("cam_kf", np.int32, 1), ("kf_cam", np.int32, 1), ("K4", np.float64, 4), ("poses7", np.float64, 7), ("cam_fixed", np.uint8, 1),
          ("gpt_pt", np.int32, 1), ("pt_idx", np.int32, 1), ("pts3", np.float64, 3), ("gobs_cam", np.int32, 1), ("gobs_pt", np.int32, 1), ("gobs_uv", np.float64, 2),
          ("gobs_weight", np.float64, 1), ("gobs_robust", np.uint8, 1), ("gobs_src", np.int32, 1))
GP_ND_IN = ("pt_ref_kf", "obs_off", "obs_kf", "ref_level", "scale_factors")
GP_ND_OUT = ("normal", "min_max", "nd_written")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def world():
    m = gc.make_map(5, 12, 80)
    asm = npg.assemble(m)
    p7, p3 = gc.solver_result(6, asm)
    ap = dict(m)
    ap.update(cam_kf=asm["cam_kf"], gpt_pt=asm["gpt_pt"], poses7=p7, pts3=p3)
    return m, ap


def _assemble(lib, m, null=(), n_ba_kf=None, n_ba_pt=None, nkf=None, npts=None, n_levels=8, caps=(64, 256, 2048)):
    L = lib.load()
    v = {k: (None if m[k] is None else np.array(m[k])) for k in ("ba_kf", "ba_pt") + GA_KF + GA_PT}
    v.update({k: np.zeros(w * 2048, dt) for k, dt, w in GA_OUT})

    def a(k):
        return None if (k in null or v[k] is None) else lib.ptr(v[k])
    nbk = (m["nkf"] if (m["ba_kf"] is None or "ba_kf" in null) else len(m["ba_kf"])) if n_ba_kf is None else n_ba_kf
    nbp = (m["npts"] if (m["ba_pt"] is None or "ba_pt" in null) else len(m["ba_pt"])) if n_ba_pt is None else n_ba_pt
    return L.orbl_global_ba_assemble(nbk, a("ba_kf"), nbp, a("ba_pt"), m["nkf"] if nkf is None else nkf, *[a(k) for k in GA_KF], m["npts"] if npts is None else npts,
                                     *[a(k) for k in GA_PT], n_levels, 1, *caps, *[a(k) for k, _, _ in GA_OUT])


def _apply(lib, p, null=(), stage=0, ncam=None, npts_ba=None, nkf=None, npts=None, n_levels=8):
    L = lib.load()
    keys = ("cam_kf", "poses7", "gpt_pt", "pts3", "kf_bad", "kf_Tcw", "kf_center", "X", "pt_bad") + GP_ND_IN
    v = {k: (None if p[k] is None else np.array(p[k])) for k in keys}
    n, nk = p["npts"], p["nkf"]
    v.update(normal=np.zeros((n, 3)), min_max=np.zeros((n, 2), np.float32), nd_written=np.zeros(n, np.uint8), counts=np.zeros(3, np.int32), kf_gba_Tcw=np.zeros((nk, 12)),
             kf_in_gba=np.zeros(nk, np.uint8), pt_gba_X=np.zeros((n, 3)), pt_in_gba=np.zeros(n, np.uint8))

    def a(k):
        return None if (k in null or v[k] is None) else lib.ptr(v[k])
    return L.orbl_global_ba_apply(len(p["cam_kf"]) if ncam is None else ncam, a("cam_kf"), a("poses7"), len(p["gpt_pt"]) if npts_ba is None else npts_ba, a("gpt_pt"), a("pts3"),
                                  stage, nk if nkf is None else nkf, a("kf_bad"), a("kf_Tcw"), a("kf_center"), n if npts is None else npts, a("X"), a("pt_bad"), a("kf_gba_Tcw"),
                                  a("kf_in_gba"), a("pt_gba_X"), a("pt_in_gba"), *[a(k) for k in GP_ND_IN], n_levels, *[a(k) for k in GP_ND_OUT], a("counts"))


def _changed(pr, key, at, value):
    q = dict(pr); q[key] = np.array(pr[key]); q[key].reshape(-1)[at] = value
    return q


def test_symbols_are_exported_listed_and_declared(lib):
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "orbslam_hip.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in lib.SYMBOLS and ("int %s(" % name) in hdr
    from ceres_mono_orb_slam2_amd import loopclosing
    for f in ("global_ba_assemble", "global_ba_assemble_device", "global_ba_apply", "global_ba_apply_device", "global_bundle_adjustment_on_tables"):
        assert callable(getattr(loopclosing, f))


def test_assemble_argument_errors_are_einval_before_device_work(lib, world):
    L = lib.load()
    m, _ = world
    ch = _changed
    nkf, npts = m["nkf"], m["npts"]
    cases = {
        "negative n_ba_kf": dict(m=m, n_ba_kf=-1), "negative n_ba_pt": dict(m=m, n_ba_pt=-1), "negative nkf": dict(m=m, nkf=-1), "negative npts": dict(m=m, npts=-1),
        "n_levels 0": dict(m=m, n_levels=0), "n_levels 65": dict(m=m, n_levels=65), "negative cap_cam": dict(m=m, caps=(-1, 4, 4)), "negative cap_pts": dict(m=m, caps=(4, -1, 4)),
        "negative cap_obs": dict(m=m, caps=(4, 4, -1)), "NULL ba_kf with another count": dict(m=m, null=("ba_kf",), n_ba_kf=nkf - 1),
        "NULL ba_pt with another count": dict(m=m, null=("ba_pt",), n_ba_pt=npts + 1),
        "ba_kf too large": dict(m=ch(m, "ba_kf", 1, nkf)), "ba_kf negative": dict(m=ch(m, "ba_kf", 0, -1)),
        "ba_pt too large": dict(m=ch(m, "ba_pt", 1, npts)), "ba_pt negative": dict(m=ch(m, "ba_pt", 0, -1)), "ba_pt repeats": dict(m=ch(m, "ba_pt", 3, m["ba_pt"][9])),
        "obs_off not from 0": dict(m=ch(m, "obs_off", 0, 1)), "obs_off decreases": dict(m=ch(m, "obs_off", npts, 0)),
        "observer too large": dict(m=ch(m, "obs_kf", 3, nkf)), "observer negative": dict(m=ch(m, "obs_kf", -1, -1)),
        "level too large": dict(m=ch(m, "obs_level", 2, 8)), "level negative": dict(m=ch(m, "obs_level", 5, -1)),
    }
    for k in ("kf_id", "kf_Tcw", "kf_K4", "X", "obs_off", "obs_kf", "obs_uv", "obs_level", "inv_level_sigma2") + tuple(k for k, _, _ in GA_OUT):
        cases["NULL " + k] = dict(m=m, null=(k,))
    for what, kw in cases.items():
        assert _assemble(lib, **kw) == EINVAL, what
        assert b"orbl_global_ba_assemble" in L.orbhip_last_error(), what
    # a keyframe may repeat in ba_kf; the nullable inputs left out pass the checks (0 with a GPU, ORBHIP_ENODEV without)
    assert _assemble(lib, ch(m, "ba_kf", 3, m["ba_kf"][4])) in (0, ENODEV)
    for null in (("kf_bad",), ("pt_bad",), ("ba_kf",), ("ba_pt",), ("ba_kf", "ba_pt", "kf_bad", "pt_bad")):
        assert _assemble(lib, m, null=null) in (0, ENODEV), null
    assert _assemble(lib, m, null=("ba_kf", "ba_pt"), n_ba_kf=0, n_ba_pt=0) in (0, ENODEV)
    # the device form checks counts, NULLs and alignment on the host
    z = C.c_void_p(256)                                             # (never dereferenced: every call below fails its checks first)
    args = [5, z, 7, z, 6, z, None, z, z, 9, z, None, 20, z, z, z, z, z, 8, 1, 6, 9, 20] + [z] * 15 + [None, z, None]
    assert len(args) == len(L.orbl_global_ba_assemble_device.argtypes)
    for at, value in ((0, -1), (2, -1), (4, -1), (9, -1), (12, -1), (18, 0), (18, 65), (20, -1), (21, -1), (22, -1), (1, None), (3, None), (5, None), (7, None), (8, None),
                      (10, None), (13, None), (14, None), (15, None), (16, None), (17, None)) + tuple((i, None) for i in range(23, 38)) + (
                      (39, None), (7, C.c_void_p(260)), (10, C.c_void_p(252)), (26, C.c_void_p(260)), (34, C.c_void_p(260)), (39, C.c_void_p(260)), (1, C.c_void_p(258)),
                      (14, C.c_void_p(258)), (24, C.c_void_p(258)), (38, C.c_void_p(258))):
        b = list(args); b[at] = value
        assert L.orbl_global_ba_assemble_device(*b) == EINVAL, at


def test_apply_argument_errors_are_einval_before_device_work(lib, world):
    L = lib.load()
    _, p = world
    ch = _changed
    nkf, npts = p["nkf"], p["npts"]
    seen = next(int(q) for q in p["gpt_pt"] if not p["pt_bad"][q] and p["obs_off"][q] < p["obs_off"][q + 1])
    cases = {
        "negative ncam": dict(p=p, ncam=-1), "negative npts_ba": dict(p=p, npts_ba=-1), "negative nkf": dict(p=p, nkf=-1), "negative npts": dict(p=p, npts=-1),
        "stage 2": dict(p=p, stage=2), "stage -1": dict(p=p, stage=-1), "n_levels 0": dict(p=p, n_levels=0), "n_levels 65": dict(p=p, n_levels=65),
        "camera keyframe too large": dict(p=ch(p, "cam_kf", 1, nkf)), "camera keyframe negative": dict(p=ch(p, "cam_kf", 0, -1)),
        "camera keyframe twice": dict(p=ch(p, "cam_kf", 0, p["cam_kf"][1])), "problem point too large": dict(p=ch(p, "gpt_pt", 1, npts)),
        "problem point negative": dict(p=ch(p, "gpt_pt", 0, -1)), "problem point twice": dict(p=ch(p, "gpt_pt", 0, p["gpt_pt"][1])),
        "pose NaN": dict(p=ch(p, "poses7", 8, np.nan)), "pose inf": dict(p=ch(p, "poses7", 3, np.inf)), "zero quaternion": dict(p=ch(p, "poses7", slice(3, 7), 0.0)),
        "pose NaN in stage 1": dict(p=ch(p, "poses7", 8, np.nan), stage=1),
        "reference keyframe too large": dict(p=ch(p, "pt_ref_kf", seen, nkf)), "reference keyframe below -1": dict(p=ch(p, "pt_ref_kf", seen, -2)),
        "obs_off not from 0": dict(p=ch(p, "obs_off", 0, 1)), "obs_off decreases": dict(p=ch(p, "obs_off", npts, 0)),
        "observer too large": dict(p=ch(p, "obs_kf", 3, nkf)), "observer negative": dict(p=ch(p, "obs_kf", -1, -1)),
        "level too large": dict(p=ch(p, "ref_level", seen, 8)), "level negative": dict(p=ch(p, "ref_level", seen, -1)),
        "normals without kf_center": dict(p=p, null=("kf_center",)),
    }
    for k in GP_ND_IN + GP_ND_OUT:
        cases["normal set without " + k] = dict(p=p, null=(k,))
    for k in ("cam_kf", "poses7", "gpt_pt", "pts3", "kf_Tcw", "X", "counts"):
        cases["NULL " + k] = dict(p=p, null=(k,))
    for k in ("kf_gba_Tcw", "kf_in_gba", "pt_gba_X", "pt_in_gba"):
        cases["stage 1 NULL " + k] = dict(p=p, null=(k,), stage=1)
    for what, kw in cases.items():
        assert _apply(lib, **kw) == EINVAL, what
        assert b"orbl_global_ba_apply" in L.orbhip_last_error(), what
    # the nullable inputs left out pass the checks (0 with a GPU, ORBHIP_ENODEV without)
    nd = GP_ND_IN + GP_ND_OUT
    for null, stage in ((("kf_bad",), 0), (("pt_bad",), 0), (nd, 0), (nd + ("kf_center",), 0), (nd + ("kf_center", "kf_bad", "pt_bad"), 0), (("kf_Tcw", "kf_center", "X") + nd, 1),
                        (("kf_gba_Tcw", "kf_in_gba", "pt_gba_X", "pt_in_gba"), 0)):
        assert _apply(lib, p, null=null, stage=stage) in (0, ENODEV), (null, stage)
    z = C.c_void_p(256)
    args = [3, z, z, 4, z, z, 0, 5, None, z, z, 6, z, None, None, None, None, None, z, 9, z, z, z, z, 8, z, z, z, z, None, z, None]
    assert len(args) == len(L.orbl_global_ba_apply_device.argtypes)
    for at, value in ((0, -1), (3, -1), (6, 2), (7, -1), (11, -1), (19, -1), (24, 0), (24, 65), (1, None), (2, None), (4, None), (5, None), (9, None), (12, None), (28, None),
                      (30, None), (10, None), (18, None), (20, None), (21, None), (22, None), (23, None), (25, None), (26, None), (27, None), (2, C.c_void_p(260)),
                      (12, C.c_void_p(252)), (25, C.c_void_p(260)), (30, C.c_void_p(260)), (1, C.c_void_p(258)), (18, C.c_void_p(258)), (26, C.c_void_p(258)),
                      (29, C.c_void_p(258))):
        b = list(args); b[at] = value
        assert L.orbl_global_ba_apply_device(*b) == EINVAL, at
    s1 = [3, z, z, 4, z, z, 1, 5, None, None, None, 6, None, None, z, z, z, z, None, 0, None, None, None, None, 0, None, None, None, z, None, z, None]
    for at in (14, 15, 16, 17):
        b = list(s1); b[at] = None
        assert L.orbl_global_ba_apply_device(*b) == EINVAL, at
    b = list(s1); b[14] = C.c_void_p(260)
    assert L.orbl_global_ba_apply_device(*b) == EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_calls_without_gpu_are_enodev(lib, world):
    from ceres_mono_orb_slam2_amd import loopclosing
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()
    m, p = world
    assert _assemble(lib, m) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _assemble(lib, m, null=("ba_kf", "ba_pt", "kf_bad", "pt_bad")) == ENODEV
    for stage in (0, 1):
        assert _apply(lib, p, stage=stage) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _apply(lib, p, null=GP_ND_IN + GP_ND_OUT + ("kf_center",)) == ENODEV
    for hm, _, _ in gc.hand_assemble_cases().values():
        assert _assemble(lib, hm) == ENODEV
    with pytest.raises(OrbHipError, match="no HIP device"):
        loopclosing.global_ba_assemble(m, ba_kf=m["ba_kf"], ba_pt=m["ba_pt"])
    for stage in (0, 1):
        with pytest.raises(OrbHipError, match="no HIP device"):
            loopclosing.global_ba_apply(p["cam_kf"], p["gpt_pt"], p["poses7"], p["pts3"], p, stage=stage)
    with pytest.raises(OrbHipError, match="no HIP device"):
        loopclosing.global_bundle_adjustment_on_tables(m, ba_kf=m["ba_kf"], ba_pt=m["ba_pt"])


def test_workspace_arithmetic(lib):
    L = lib.load()
    n = C.c_size_t(0)

    def up(x):
        return (x + 255) // 256 * 256
    for nkf, npts, nbk, nbp in ((1, 0, 1, 0), (8, 60, 10, 54), (500, 100000, 500, 100000), (3, 70000, 5, 63000), (0, 0, 0, 0), (300, 3000, 242, 2700)):
        assert L.orbl_global_ba_assemble_workspace(nkf, npts, nbk, nbp, C.byref(n)) == 0
        assert n.value == up(4 * nkf) + up(4 * npts) + up(8 * nbk) + up(4 * nbk) + up(16) + up(8 * nbp) + up(8 * ((nbp + 255) // 256 + 1))
        assert L.orbl_global_ba_apply_workspace(nkf, npts, C.byref(n)) == 0 and n.value == max(up(4 * nkf) + up(4 * npts), 256)
    for bad in ((-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1)):
        assert L.orbl_global_ba_assemble_workspace(*bad, C.byref(n)) == EINVAL
    assert L.orbl_global_ba_assemble_workspace(1, 1, 1, 1, None) == EINVAL
    for bad in ((-1, 1), (1, -1)):
        assert L.orbl_global_ba_apply_workspace(*bad, C.byref(n)) == EINVAL
    assert L.orbl_global_ba_apply_workspace(1, 1, None) == EINVAL


def test_dropin_test_program_compiles_and_links(lib, tmp_path):
    """with it the explicit instantiation of FrameOpsT over mock::Types, a data model without the members the new entries read"""
    import subprocess
    exe = tmp_path / "test_globalba_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_globalba_dropin.cpp"), "-o", str(exe), lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    assert exe.exists()
