"""CPU checks of the keyframe culling entry points (include/orbslam_hip.h: orbl_keyframe_culling*): the symbols are exported and
listed, every argument error is ORBHIP_EINVAL before any device work, a valid call without a GPU is ORBHIP_ENODEV (no CPU
fallback), the workspace size is the documented host arithmetic, and the drop-in test program compiles and links."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import cullingcases as cc  # noqa: E402

EINVAL, ENODEV = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


def _call(lib, pr, th_obs=3, ratio=0.9, ncand=None, nkf=None, npts=None, null=()):
    L = lib.load()
    ncand = len(pr["cand_kf"]) if ncand is None else ncand
    nobs = len(pr["obs_kf"])
    out = dict(culled=np.zeros(max(ncand, 1), np.uint8), n_redundant=np.zeros(max(ncand, 1), np.int32), n_map_points=np.zeros(max(ncand, 1), np.int32),
               pt_bad_out=np.zeros(pr["npts"], np.uint8), pt_nobs_out=np.zeros(pr["npts"], np.int32), obs_erased=np.zeros(nobs, np.uint8))

    def a(k):
        v = out[k] if k in out else pr[k]
        return None if (k in null or v is None) else lib.ptr(v)
    return L.orbl_keyframe_culling(ncand, a("cand_kf"), a("cand_flags"), a("slot_off"), a("slot_pt"), a("slot_level"), pr["nkf"] if nkf is None else nkf,
                                   pr["npts"] if npts is None else npts, a("obs_off"), a("obs_kf"), a("obs_level"), a("pt_bad"), a("pt_nobs"), th_obs, ratio,
                                   a("culled"), a("n_redundant"), a("n_map_points"), a("pt_bad_out"), a("pt_nobs_out"), a("obs_erased"))


def test_symbols_are_exported_and_listed(lib):
    L = lib.load()
    for name in ("orbl_keyframe_culling", "orbl_keyframe_culling_device", "orbl_keyframe_culling_workspace"):
        assert hasattr(L, name) and name in lib.SYMBOLS
    from ceres_mono_orb_slam2_amd import localmapping
    assert callable(localmapping.keyframe_culling) and callable(localmapping.keyframe_culling_device)


def test_every_argument_error_is_einval_before_device_work(lib):
    L = lib.load()
    pr = cc.make(1, **cc.CONFIGS["tiny"][0])

    def changed(key, at, value):
        q = dict(pr); q[key] = pr[key].copy(); q[key][at] = value
        return q
    cases = {
        "negative ncand": dict(pr=pr, ncand=-1), "negative nkf": dict(pr=pr, nkf=-1), "negative npts": dict(pr=pr, npts=-1),
        "slot_off not from 0": dict(pr=changed("slot_off", 0, 1)), "slot_off decreases": dict(pr=changed("slot_off", 2, 0)),
        "obs_off not from 0": dict(pr=changed("obs_off", 0, 2)), "obs_off decreases": dict(pr=changed("obs_off", 5, 0)),
        "candidate keyframe too large": dict(pr=changed("cand_kf", 1, pr["nkf"])), "candidate keyframe negative": dict(pr=changed("cand_kf", 0, -1)),
        "slot point too large": dict(pr=changed("slot_pt", 7, pr["npts"])), "slot point negative": dict(pr=changed("slot_pt", 0, -1)),
        "observer too large": dict(pr=changed("obs_kf", 3, pr["nkf"])), "observer negative": dict(pr=changed("obs_kf", -1, -2)),
        "slot level negative": dict(pr=changed("slot_level", 4, -1)), "observation level negative": dict(pr=changed("obs_level", 9, -1)),
        "th_obs 0": dict(pr=pr, th_obs=0), "th_obs negative": dict(pr=pr, th_obs=-3),
        "ratio nan": dict(pr=pr, ratio=float("nan")), "ratio inf": dict(pr=pr, ratio=float("inf")), "ratio -inf": dict(pr=pr, ratio=float("-inf")),
        "NULL cand_kf": dict(pr=pr, null=("cand_kf",)), "NULL slot_off": dict(pr=pr, null=("slot_off",)), "NULL slot_pt": dict(pr=pr, null=("slot_pt",)),
        "NULL obs_off": dict(pr=pr, null=("obs_off",)), "NULL obs_level": dict(pr=pr, null=("obs_level",)), "NULL culled": dict(pr=pr, null=("culled",)),
        "NULL n_redundant": dict(pr=pr, null=("n_redundant",)),
    }
    for what, kw in cases.items():
        assert _call(lib, **kw) == EINVAL, what
        assert b"orbl_keyframe_culling" in L.orbhip_last_error(), what
    # the device form checks counts, NULLs and alignment on the host
    z = C.c_void_p(256)                                             # (never dereferenced: every call below fails its checks first)
    args = [2, z, None, 5, z, z, z, 4, 6, 9, z, z, z, None, None, 3, 0.9, z, z, z, None, None, None, None, z, None]
    for at, value in ((0, -1), (3, -1), (7, -1), (8, -1), (9, -1), (15, 0), (16, float("nan")), (24, None), (1, None), (4, None), (5, None), (10, None), (11, None),
                      (17, None), (19, None), (1, C.c_void_p(258)), (18, C.c_void_p(257)), (24, C.c_void_p(259))):
        b = list(args); b[at] = value
        assert L.orbl_keyframe_culling_device(*b) == EINVAL, at


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_call_without_gpu_is_enodev(lib):
    from ceres_mono_orb_slam2_amd import localmapping
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()
    pr = cc.make(1, **cc.CONFIGS["tiny"][0])
    assert _call(lib, pr) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _call(lib, pr, null=("cand_flags", "pt_bad_out", "pt_nobs_out", "obs_erased")) == ENODEV
    with pytest.raises(OrbHipError, match="no HIP device"):
        localmapping.keyframe_culling(pr["cand_kf"], pr["cand_flags"], pr["slot_off"], pr["slot_pt"], pr["slot_level"], pr["nkf"], pr["obs_off"], pr["obs_kf"],
                                      pr["obs_level"])


def test_workspace_arithmetic(lib):
    L = lib.load()
    n = C.c_size_t(0)

    def up(x):
        return (4 * x + 255) // 256 * 256
    for ncand, nslots, npts, nobs in ((0, 0, 0, 0), (1, 1, 1, 1), (3, 64, 64, 65), (100, 50000, 10000, 50000), (7, 129, 1000, 3)):
        assert L.orbl_keyframe_culling_workspace(ncand, nslots, npts, nobs, C.byref(n)) == 0
        assert n.value == max(4 * up(nslots) + 2 * up(nobs) + 3 * up(npts), 256)
    for bad in ((-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1)):
        assert L.orbl_keyframe_culling_workspace(*bad, C.byref(n)) == EINVAL
    assert L.orbl_keyframe_culling_workspace(1, 1, 1, 1, None) == EINVAL


def test_dropin_test_program_compiles_and_links(lib, tmp_path):
    exe = tmp_path / "test_culling_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_culling_dropin.cpp"), "-o", str(exe), lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    assert exe.exists()
    # the call site as the reference spells it, in the `#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES` branch of the drop-in header
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_culling_reference_types.cpp")])
