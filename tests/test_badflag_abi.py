"""CPU checks of the SetBadFlag entry points (include/orbslam_hip.h: orbl_set_bad_keyframes*): the symbols are exported and listed, every
argument error is ORBHIP_EINVAL before any device work, a valid call without a GPU is ORBHIP_ENODEV (no CPU fallback), the workspace
size is the documented host arithmetic, and the drop-in test program compiles and links."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import badflagcases as bc  # noqa: E402

EINVAL, ENODEV = -1, -2
KF = ("kf_bad", "kf_parent", "kf_rank", "kf_Tcw", "child_off", "child_kf", "conn_off", "conn_kf", "conn_w", "ord_off", "ord_kf", "ord_w")
PT = ("kf_slot_off", "kf_slot_pt", "pt_bad", "pt_nobs", "pt_ref_kf", "obs_off", "obs_kf", "obs_slot", "obs_erased")
OUT = ("tgt_status", "tgt_Tcp", "oconn_off", "oconn_kf", "oconn_w", "oord_off", "oord_kf", "oord_w", "ochild_off", "ochild_kf", "counts")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


def _call(lib, pr, ntgt=None, nkf=None, npts=None, null=(), caps=(4096, 4096)):
    L = lib.load()
    ntgt = len(pr["tgt_kf"]) if ntgt is None else ntgt
    hold = {k: np.zeros(4097, np.float64 if k == "tgt_Tcp" else np.int32) for k in OUT}
    hold["obs_erased"] = np.zeros(len(pr["obs_kf"]), np.uint8)
    hold.update({k: np.array(pr[k]) for k in ("kf_bad", "kf_parent", "kf_slot_pt", "pt_bad", "pt_nobs", "pt_ref_kf")})      # (in/out: copies)

    def a(k):
        v = hold[k] if k in hold else pr[k]
        return None if (k in null or v is None) else lib.ptr(v)
    return L.orbl_set_bad_keyframes(ntgt, a("tgt_kf"), a("tgt_flags"), a("tgt_mask"), pr["nkf"] if nkf is None else nkf, *[a(k) for k in KF],
                                    pr["npts"] if npts is None else npts, *[a(k) for k in PT], *caps, *[a(k) for k in OUT])


def _problem():
    return bc.make(1, nkf=12, ntgt=5)


def test_symbols_are_exported_and_listed(lib):
    L = lib.load()
    for name in ("orbl_set_bad_keyframes", "orbl_set_bad_keyframes_device", "orbl_set_bad_keyframes_workspace"):
        assert hasattr(L, name) and name in lib.SYMBOLS
    from ceres_mono_orb_slam2_amd import localmapping
    assert callable(localmapping.set_bad_keyframes) and callable(localmapping.set_bad_keyframes_device)


def test_every_argument_error_is_einval_before_device_work(lib):
    L = lib.load()
    pr = _problem()
    nkf = pr["nkf"]
    t0 = int(pr["tgt_kf"][0])
    assert pr["kf_rank"] is not None and pr["conn_off"][1] >= 2 and list(pr["tgt_flags"][:3]) == [0, 0, 0] and list(pr["tgt_mask"][:3]) == [1, 1, 1]
    row = next(k for k in range(nkf) if pr["child_off"][k + 1] - pr["child_off"][k] >= 2)           # a child row with two entries
    c0 = int(pr["child_off"][row])
    e0 = int(pr["obs_off"][3])                                        # the first observation of point 3

    def changed(key, at, value):
        q = dict(pr); q[key] = pr[key].copy(); q[key][at] = value
        return q
    cases = {
        "negative ntgt": dict(pr=pr, ntgt=-1), "negative nkf": dict(pr=pr, nkf=-1), "negative npts": dict(pr=pr, npts=-1),
        "negative cap_ord": dict(pr=pr, caps=(-1, 4096)), "negative cap_child": dict(pr=pr, caps=(4096, -1)),
        "child_off not from 0": dict(pr=changed("child_off", 0, 1)), "child_off decreases": dict(pr=changed("child_off", 3, -1)),
        "conn_off not from 0": dict(pr=changed("conn_off", 0, 1)), "conn_off decreases": dict(pr=changed("conn_off", 3, 0)),
        "ord_off not from 0": dict(pr=changed("ord_off", 0, 1)), "ord_off decreases": dict(pr=changed("ord_off", 3, -1)),
        "kf_slot_off not from 0": dict(pr=changed("kf_slot_off", 0, 1)), "kf_slot_off decreases": dict(pr=changed("kf_slot_off", 3, 0)),
        "obs_off not from 0": dict(pr=changed("obs_off", 0, 2)), "obs_off decreases": dict(pr=changed("obs_off", 5, 0)),
        "target too large": dict(pr=changed("tgt_kf", 1, nkf)), "target negative": dict(pr=changed("tgt_kf", 0, -1)),
        "duplicate target": dict(pr=changed("tgt_kf", 3, pr["tgt_kf"][1])),
        "target already bad": dict(pr=changed("kf_bad", t0, 1)),
        "target without parent": dict(pr=changed("kf_parent", t0, -1)), "target its own parent": dict(pr=changed("kf_parent", t0, t0)),
        "parent too large": dict(pr=changed("kf_parent", 5, nkf)), "parent below -1": dict(pr=changed("kf_parent", 5, -2)),
        "child too large": dict(pr=changed("child_kf", 0, nkf)), "child negative": dict(pr=changed("child_kf", 0, -1)),
        "child row names itself": dict(pr=changed("child_kf", c0, row)), "child row names a keyframe twice": dict(pr=changed("child_kf", c0 + 1, pr["child_kf"][c0])),
        "table keyframe too large": dict(pr=changed("conn_kf", 4, nkf)), "table keyframe negative": dict(pr=changed("conn_kf", 4, -1)),
        "table row names itself": dict(pr=changed("conn_kf", 0, 0)), "table row names a keyframe twice": dict(pr=changed("conn_kf", 1, pr["conn_kf"][0])),
        "list keyframe too large": dict(pr=changed("ord_kf", 2, nkf)), "list keyframe negative": dict(pr=changed("ord_kf", 2, -1)),
        "rank out of range": dict(pr=changed("kf_rank", 2, nkf)), "rank repeats": dict(pr=changed("kf_rank", 2, pr["kf_rank"][3])),
        "slot point too large": dict(pr=changed("kf_slot_pt", 7, pr["npts"])), "slot point below -1": dict(pr=changed("kf_slot_pt", 0, -2)),
        "reference keyframe too large": dict(pr=changed("pt_ref_kf", 1, nkf)),
        "observer too large": dict(pr=changed("obs_kf", 3, nkf)), "observer negative": dict(pr=changed("obs_kf", -1, -2)),
        "obs_slot negative": dict(pr=changed("obs_slot", e0, -1)), "obs_slot outside its keyframe": dict(pr=changed("obs_slot", e0, 100000)),
        "NULL tgt_kf": dict(pr=pr, null=("tgt_kf",)), "NULL kf_bad": dict(pr=pr, null=("kf_bad",)), "NULL kf_parent": dict(pr=pr, null=("kf_parent",)),
        "NULL kf_Tcw": dict(pr=pr, null=("kf_Tcw",)), "NULL child_off": dict(pr=pr, null=("child_off",)), "NULL child_kf": dict(pr=pr, null=("child_kf",)),
        "NULL conn_off": dict(pr=pr, null=("conn_off",)), "NULL conn_w": dict(pr=pr, null=("conn_w",)), "NULL ord_off": dict(pr=pr, null=("ord_off",)),
        "NULL ord_kf": dict(pr=pr, null=("ord_kf",)), "NULL tgt_status": dict(pr=pr, null=("tgt_status",)), "NULL tgt_Tcp": dict(pr=pr, null=("tgt_Tcp",)),
        "NULL counts": dict(pr=pr, null=("counts",)), "NULL oconn_off": dict(pr=pr, null=("oconn_off",)), "NULL oconn_kf": dict(pr=pr, null=("oconn_kf",)),
        "NULL oord_off": dict(pr=pr, null=("oord_off",)), "NULL oord_w": dict(pr=pr, null=("oord_w",)), "NULL ochild_off": dict(pr=pr, null=("ochild_off",)),
        "NULL ochild_kf": dict(pr=pr, null=("ochild_kf",)),
    }
    for k in PT:                                                     # part of the point set without the rest
        cases["point set without " + k] = dict(pr=pr, null=(k,))
    cases["point set: obs_off alone"] = dict(pr=pr, null=tuple(k for k in PT if k != "obs_off"))
    for what, kw in cases.items():
        assert _call(lib, **kw) == EINVAL, what
        assert b"orbl_set_bad_keyframes" in L.orbhip_last_error(), what
    # the device form checks counts, NULLs and alignment on the host
    z = C.c_void_p(256)                                             # (never dereferenced: every call below fails its checks first)
    args = [2, z, None, None, 4, z, z, None, z, 3, z, z, 5, z, z, z, 5, z, z, z, 6, 9, z, z, z, z, z, 12, z, z, z, z, 9, 9] + [z] * 11 + [None, z, None]
    assert len(args) == len(L.orbl_set_bad_keyframes_device.argtypes)
    for at, value in ((0, -1), (4, -1), (9, -1), (12, -1), (16, -1), (20, -1), (21, -1), (27, -1), (32, -1), (33, -1), (46, None), (1, None), (5, None), (6, None),
                      (8, None), (10, None), (11, None), (13, None), (14, None), (15, None), (17, None), (18, None), (19, None), (23, None), (24, None), (25, None),
                      (26, None), (28, None), (29, None), (30, None), (31, None), (34, None), (35, None), (36, None), (37, None), (38, None), (39, None), (40, None),
                      (41, None), (42, None), (43, None), (44, None), (1, C.c_void_p(258)), (8, C.c_void_p(260)), (35, C.c_void_p(260)), (40, C.c_void_p(257)),
                      (46, C.c_void_p(258))):
        b = list(args); b[at] = value
        assert L.orbl_set_bad_keyframes_device(*b) == EINVAL, at
    # without kf_slot_off no other point table may be given
    b = list(args); b[22] = None
    assert L.orbl_set_bad_keyframes_device(*b) == EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_call_without_gpu_is_enodev(lib):
    from ceres_mono_orb_slam2_amd import localmapping
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()
    pr = _problem()
    assert _call(lib, pr) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _call(lib, pr, null=("tgt_flags", "tgt_mask", "kf_rank") + PT, npts=0) == ENODEV
    with pytest.raises(OrbHipError, match="no HIP device"):
        localmapping.set_bad_keyframes(pr["tgt_kf"], pr, tgt_flags=pr["tgt_flags"], tgt_mask=pr["tgt_mask"])


def test_workspace_arithmetic(lib):
    L = lib.load()
    n = C.c_size_t(0)

    def up(x):
        return (x + 255) // 256 * 256
    for ntgt, nkf, nchild, nconn, nobs in ((0, 0, 0, 0, 0), (1, 1, 0, 0, 1), (3, 64, 63, 100, 0), (5, 500, 499, 9000, 400000), (257, 257, 300, 66000, 7)):
        assert L.orbl_set_bad_keyframes_workspace(ntgt, nkf, nchild, nconn, nobs, C.byref(n)) == 0
        adds = ntgt * nkf
        want = (4 * up(4 * nkf) + up(4 * nconn) + up(4) + up(nchild) + up(nobs) + up(4 * nkf) + up(4 * ntgt) + 2 * up(4 * adds) + up(adds) + 2 * up(4 * nkf) +
                up(12 * nkf) + up(4 * (nchild + adds)))
        assert n.value == want
    for bad in ((-1, 0, 0, 0, 0), (0, -1, 0, 0, 0), (0, 0, -1, 0, 0), (0, 0, 0, -1, 0), (0, 0, 0, 0, -1)):
        assert L.orbl_set_bad_keyframes_workspace(*bad, C.byref(n)) == EINVAL
    assert L.orbl_set_bad_keyframes_workspace(1, 1, 1, 1, 1, None) == EINVAL


def test_dropin_test_program_compiles_and_links(lib, tmp_path):
    exe = tmp_path / "test_badflag_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_badflag_dropin.cpp"), "-o", str(exe), lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    assert exe.exists()
