"""CPU checks of the UpdateLocalMap entry points (include/orbslam_hip.h: orbt_update_local_keyframes, orbt_update_local_points,
orbt_update_local_map_device, orbt_update_local_map_workspace, orbt_track_local_map_device): the symbols are exported and listed,
every argument error is ORBHIP_EINVAL before any device work, a valid call without a GPU is ORBHIP_ENODEV (no CPU fallback), the
workspace size is the documented host arithmetic, and the drop-in test program compiles and links."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import localmapcases as lc  # noqa: E402

EINVAL, ENODEV = -1, -2
NAMES = ("orbt_update_local_keyframes", "orbt_update_local_points", "orbt_update_local_map_device", "orbt_update_local_map_workspace", "orbt_track_local_map_device")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


def _keyframes(lib, pr, null=(), cap_kf=None, **count):
    """orbt_update_local_keyframes on problem pr; count: n_kp / npts / nkf / n_prev overrides"""
    L = lib.load()
    nkf, npts, n_kp = len(pr["kf_bad"]), len(pr["pt_bad"]), len(pr["frame_pt"])
    out = dict(frame_pt_out=np.zeros(max(n_kp, 1), np.int32), local_kf=np.zeros(max(nkf, 1), np.int32), votes=np.zeros(max(nkf, 1), np.int32))
    n, ref, st = C.c_int(0), C.c_int(0), C.c_int(0)

    def a(k):
        v = out[k] if k in out else pr[k]
        return None if (k in null or v is None) else lib.ptr(v)
    return L.orbt_update_local_keyframes(count.get("n_kp", n_kp), a("frame_pt"), count.get("npts", npts), a("pt_bad"), a("obs_off"), a("obs_kf"), count.get("nkf", nkf),
                                         a("kf_bad"), a("kf_rank"), a("kf_parent"), a("cov_off"), a("cov_kf"), a("child_off"), a("child_kf"),
                                         count.get("n_prev", len(pr["prev_local_kf"])), a("prev_local_kf"), nkf if cap_kf is None else cap_kf, a("frame_pt_out"), a("local_kf"),
                                         None if "n_local_kf" in null else C.byref(n), None if "ref_kf" in null else C.byref(ref), None if "status" in null else C.byref(st),
                                         a("votes"))


def _points(lib, pr, null=(), cap_pt=None, **count):
    """orbt_update_local_points over ALL keyframes of pr as the local list"""
    L = lib.load()
    nkf, npts, n_kp = len(pr["kf_bad"]), len(pr["pt_bad"]), len(pr["frame_pt"])
    cap = npts if cap_pt is None else cap_pt
    out = dict(local_pt=np.zeros(max(cap, 1), np.int32), mp_Xw=np.zeros(3 * max(cap, 1)), mp_normal=np.zeros(3 * max(cap, 1)), mp_min_dist=np.zeros(max(cap, 1), np.float32),
               mp_max_dist=np.zeros(max(cap, 1), np.float32), mp_desc=np.zeros(32 * max(cap, 1), np.uint8), mp_state=np.zeros(max(cap, 1), np.uint8),
               slot_Xw=np.zeros(3 * max(n_kp, 1)), slot_state=np.zeros(max(n_kp, 1), np.uint8))
    n = C.c_int(0)

    def a(k):
        v = out[k] if k in out else pr[k]
        return None if (k in null or v is None) else lib.ptr(v)
    return L.orbt_update_local_points(count.get("n_local_kf", nkf), a("kf_slot_off"), a("kf_slot_pt"), count.get("npts", npts), a("pt_bad"), a("pt_nobs"), a("pt_Xw"), a("pt_normal"),
                                      a("pt_min_dist"), a("pt_max_dist"), a("pt_desc"), count.get("n_kp", n_kp), a("frame_pt"), count.get("n_seen", len(pr["seen_pt"])), a("seen_pt"),
                                      cap, a("local_pt"), None if "n_local_pt" in null else C.byref(n), a("mp_Xw"), a("mp_normal"), a("mp_min_dist"), a("mp_max_dist"),
                                      a("mp_desc"), a("mp_state"), a("slot_Xw"), a("slot_state"))


def _problem():
    pr = lc.make(1, **lc.CONFIGS["tiny"][0])
    assert len(pr["seen_pt"]) and len(pr["prev_local_kf"]) and (pr["frame_pt"] >= 0).any()
    return pr


def _changed(pr, key, at, value):
    q = dict(pr); q[key] = pr[key].copy(); q[key][at] = value
    return q


def test_symbols_are_exported_and_listed(lib):
    L = lib.load()
    for name in NAMES:
        assert hasattr(L, name) and name in lib.SYMBOLS
    from ceres_mono_orb_slam2_amd import tracking
    for f in ("update_local_keyframes", "update_local_points", "update_local_map_device", "track_local_map_device"):
        assert callable(getattr(tracking, f))


def test_every_argument_error_of_the_host_calls_is_einval_before_device_work(lib):
    L = lib.load()
    pr = _problem()
    nkf, npts = len(pr["kf_bad"]), len(pr["pt_bad"])
    eleven = dict(pr); eleven["cov_off"] = np.array([0, 11] + [11] * (nkf - 1), np.int32); eleven["cov_kf"] = np.zeros(11, np.int32)
    twice = _changed(pr, "kf_rank", 0, int(pr["kf_rank"][1]))
    cases = {
        "negative n_kp": dict(pr=pr, n_kp=-1), "negative npts": dict(pr=pr, npts=-1), "negative nkf": dict(pr=pr, nkf=-1), "negative n_prev": dict(pr=pr, n_prev=-1),
        "negative cap_kf": dict(pr=pr, cap_kf=-1), "n_prev above nkf": dict(pr=pr, n_prev=nkf + 1),
        "obs_off not from 0": dict(pr=_changed(pr, "obs_off", 0, 1)), "obs_off decreases": dict(pr=_changed(pr, "obs_off", 5, -1)),
        "cov_off not from 0": dict(pr=_changed(pr, "cov_off", 0, 2)), "cov_off decreases": dict(pr=_changed(pr, "cov_off", 2, 0)),
        "child_off not from 0": dict(pr=_changed(pr, "child_off", 0, 1)), "child_off decreases": dict(pr=_changed(pr, "child_off", nkf, 0)),
        "observer too large": dict(pr=_changed(pr, "obs_kf", 3, nkf)), "observer negative": dict(pr=_changed(pr, "obs_kf", -1, -1)),
        "neighbour too large": dict(pr=_changed(pr, "cov_kf", 0, nkf)), "child negative": dict(pr=_changed(pr, "child_kf", 0, -2)),
        "parent too large": dict(pr=_changed(pr, "kf_parent", 2, nkf)), "parent below -1": dict(pr=_changed(pr, "kf_parent", 2, -2)),
        "frame point too large": dict(pr=_changed(pr, "frame_pt", 0, npts)), "frame point below -1": dict(pr=_changed(pr, "frame_pt", 1, -2)),
        "previous keyframe too large": dict(pr=_changed(pr, "prev_local_kf", 0, nkf)), "previous keyframe negative": dict(pr=_changed(pr, "prev_local_kf", 1, -1)),
        "rank out of range": dict(pr=_changed(pr, "kf_rank", 0, nkf)), "rank negative": dict(pr=_changed(pr, "kf_rank", 0, -1)), "rank twice": dict(pr=twice),
        "eleven neighbours": dict(pr=eleven),
        "NULL frame_pt": dict(pr=pr, null=("frame_pt",)), "NULL frame_pt_out": dict(pr=pr, null=("frame_pt_out",)), "NULL pt_bad": dict(pr=pr, null=("pt_bad",)),
        "NULL obs_off": dict(pr=pr, null=("obs_off",)), "NULL obs_kf": dict(pr=pr, null=("obs_kf",)), "NULL kf_bad": dict(pr=pr, null=("kf_bad",)),
        "NULL kf_parent": dict(pr=pr, null=("kf_parent",)), "NULL cov_off": dict(pr=pr, null=("cov_off",)), "NULL cov_kf": dict(pr=pr, null=("cov_kf",)),
        "NULL child_off": dict(pr=pr, null=("child_off",)), "NULL child_kf": dict(pr=pr, null=("child_kf",)), "NULL prev_local_kf": dict(pr=pr, null=("prev_local_kf",)),
        "NULL local_kf": dict(pr=pr, null=("local_kf",)), "NULL n_local_kf": dict(pr=pr, null=("n_local_kf",)), "NULL ref_kf": dict(pr=pr, null=("ref_kf",)),
        "NULL status": dict(pr=pr, null=("status",)),
    }
    for what, kw in cases.items():
        assert _keyframes(lib, **kw) == EINVAL, what
        assert b"orbt_update_local" in L.orbhip_last_error(), what
    cases = {
        "negative n_local_kf": dict(pr=pr, n_local_kf=-1), "negative npts": dict(pr=pr, npts=-1), "negative n_kp": dict(pr=pr, n_kp=-1), "negative n_seen": dict(pr=pr, n_seen=-1),
        "negative cap_pt": dict(pr=pr, cap_pt=-1),
        "slot_off not from 0": dict(pr=_changed(pr, "kf_slot_off", 0, 1)), "slot_off decreases": dict(pr=_changed(pr, "kf_slot_off", 3, 0)),
        "slot point too large": dict(pr=_changed(pr, "kf_slot_pt", 4, npts)), "slot point below -1": dict(pr=_changed(pr, "kf_slot_pt", 4, -2)),
        "frame point too large": dict(pr=_changed(pr, "frame_pt", 0, npts)), "seen point too large": dict(pr=_changed(pr, "seen_pt", 0, npts)),
        "seen point negative": dict(pr=_changed(pr, "seen_pt", 0, -1)),
        "NULL kf_slot_off": dict(pr=pr, null=("kf_slot_off",)), "NULL kf_slot_pt": dict(pr=pr, null=("kf_slot_pt",)), "NULL pt_bad": dict(pr=pr, null=("pt_bad",)),
        "NULL frame_pt": dict(pr=pr, null=("frame_pt",)), "NULL seen_pt": dict(pr=pr, null=("seen_pt",)), "NULL local_pt": dict(pr=pr, null=("local_pt",)),
        "NULL n_local_pt": dict(pr=pr, null=("n_local_pt",)), "NULL pt_nobs with packed outputs": dict(pr=pr, null=("pt_nobs",)),
        "NULL pt_desc with packed outputs": dict(pr=pr, null=("pt_desc",)), "packed outputs in part (no mp_state)": dict(pr=pr, null=("mp_state",)),
        "packed outputs in part (only slot_Xw missing)": dict(pr=pr, null=("slot_Xw",)),
    }
    for what, kw in cases.items():
        assert _points(lib, **kw) == EINVAL, what
        assert b"orbt_update_local" in L.orbhip_last_error(), what


def _device_args():
    """a call whose every check passes (the pointers are never dereferenced: without a GPU the first launch fails, with one the tests
    below only send calls that fail their checks first)"""
    z = C.c_void_p(4096)
    #        0  1  2  3  4  5  6  7  8  9  10 11 12 13 14 15 16 17 18 19 20 21 22 23 24 25 26 27 28 29 30 31 32  33
    return [4, z, 2, z, 3, z, 9, z, z, 20, z, z, z, z, z, z, z, 5, z, z, z, 7, z, z, 4, z, z, 30, z, z, 30, 5, 9] + [z] * 15 + [None]


def test_device_form_checks_counts_nulls_and_alignment_on_the_host(lib):
    L = lib.load()
    args = _device_args()
    assert len(args) == 49
    bad = [(i, -1) for i in (0, 2, 4, 6, 9, 17, 21, 24, 27, 30, 31, 32)]                                  # the twelve counts
    bad += [(4, 6)]                                                                                    # n_prev > nkf
    bad += [(i, None) for i in (1, 3, 5, 7, 10, 11, 18, 20, 22, 23, 25, 26, 28, 29, 34, 35, 36, 47)]    # arrays that are needed, counts, workspace
    bad += [(i, None) for i in (8, 12, 13, 14, 15, 16)]                                                # point records with the packed outputs given
    bad += [(i, None) for i in range(38, 46)]                                                          # the packed outputs in part
    bad += [(i, C.c_void_p(4098)) for i in (1, 3, 5, 8, 10, 11, 14, 15, 19, 20, 22, 23, 25, 26, 28, 29, 33, 34, 35, 36, 37, 40, 41, 46)]     # 32-bit arrays
    bad += [(i, C.c_void_p(4104)) for i in (12, 13, 16, 38, 39, 42, 44, 47)]                            # 16-byte records and the workspace
    for at, value in bad:
        b = list(args); b[at] = value
        assert L.orbt_update_local_map_device(*b) == EINVAL, at
        assert b"orbt_update_local_map_device" in L.orbhip_last_error(), at
    # the device form of TrackLocalMap: NULL, counts and alignment come first, whatever frame is resident
    z = C.c_void_p(4096)
    t = [z, z, z, z, 0.18, z, z, z, z, z, z, 5, z, z, 7, 1.0, 0.8, None, z, z, z, z, z]
    for at, value, code in ((0, None, EINVAL), (5, None, EINVAL), (10, None, EINVAL), (12, None, EINVAL), (13, None, EINVAL), (18, None, EINVAL), (22, None, EINVAL),
                            (11, -1, -4), (11, 16385, -4), (5, C.c_void_p(4100), EINVAL), (7, C.c_void_p(4098), EINVAL), (9, C.c_void_p(4104), EINVAL),
                            (12, C.c_void_p(4100), EINVAL)):
        b = list(t); b[at] = value
        assert L.orbt_track_local_map_device(*b) == code, at


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_calls_without_gpu_are_enodev(lib):
    from ceres_mono_orb_slam2_amd import tracking
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()
    pr = _problem()
    assert _keyframes(lib, pr) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _keyframes(lib, pr, null=("votes", "kf_rank")) == ENODEV
    assert _points(lib, pr) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _points(lib, pr, null=("mp_Xw", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_desc", "mp_state", "slot_Xw", "slot_state", "pt_nobs", "pt_Xw")) == ENODEV
    assert L.orbt_update_local_map_device(*_device_args()) == ENODEV
    with pytest.raises(OrbHipError, match="no HIP device"):
        tracking.update_local_keyframes(pr["frame_pt"], pr["pt_bad"], pr["obs_off"], pr["obs_kf"], pr["kf_bad"], pr["kf_rank"], pr["kf_parent"], pr["cov_off"], pr["cov_kf"],
                                        pr["child_off"], pr["child_kf"], pr["prev_local_kf"])
    with pytest.raises(OrbHipError, match="no HIP device"):
        tracking.update_local_points(pr["kf_slot_off"], pr["kf_slot_pt"], pr["pt_bad"], pr["pt_nobs"], pr["pt_Xw"], pr["pt_normal"], pr["pt_min_dist"], pr["pt_max_dist"],
                                     pr["pt_desc"], pr["frame_pt"], pr["seen_pt"], len(pr["pt_bad"]))


def test_workspace_arithmetic(lib):
    L = lib.load()
    n = C.c_size_t(0)

    def up(x):
        return (x + 255) // 256 * 256
    for nkf, npts, slots in ((0, 0, 0), (1, 1, 1), (63, 64, 256), (64, 1000, 257), (5000, 200000, 160000), (7, 129, 3)):
        assert L.orbt_update_local_map_workspace(nkf, npts, slots, C.byref(n)) == 0
        assert n.value == 4 * up(4 * nkf) + up(4 * nkf + 4) + 2 * up(4 * npts) + up(4 * max(1, (slots + 255) // 256)) + up(8)
    for bad in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert L.orbt_update_local_map_workspace(*bad, C.byref(n)) == EINVAL
    assert L.orbt_update_local_map_workspace(1, 1, 1, None) == EINVAL


def test_dropin_test_program_compiles_and_links(lib, tmp_path):
    exe = tmp_path / "test_local_map_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_local_map_dropin.cpp"), "-o", str(exe), lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    assert exe.exists()
    # the call sites as the reference spells them, in the `#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES` branch of the drop-in header
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_local_map_reference_types.cpp")])
