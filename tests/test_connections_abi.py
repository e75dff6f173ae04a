"""CPU checks of the UpdateConnections entry points (include/orbslam_hip.h: orbl_update_connections*): the symbols are exported and
listed, every argument error is ORBHIP_EINVAL before any device work, a valid call without a GPU is ORBHIP_ENODEV (no CPU fallback),
the workspace size is the documented host arithmetic, and the drop-in test program compiles and links."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import connectioncases as cc  # noqa: E402

EINVAL, ENODEV = -1, -2
OUT = ("tgt_status", "tgt_parent", "aff_kf", "oconn_off", "oconn_kf", "oconn_w", "oord_off", "oord_kf", "oord_w", "link_off", "link_kf", "counts")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


def _call(lib, pr, th=None, ntgt=None, nkf=None, npts=None, null=(), caps=None):
    L = lib.load()
    ntgt = len(pr["tgt_kf"]) if ntgt is None else ntgt
    cap = 4096
    caps = (cap, cap, cap, cap) if caps is None else caps
    out = {k: np.zeros(cap + 1, np.int32) for k in OUT}

    def a(k):
        v = out[k] if k in out else pr[k]
        return None if (k in null or v is None) else lib.ptr(v)
    return L.orbl_update_connections(ntgt, a("tgt_kf"), a("tgt_flags"), a("slot_off"), a("slot_pt"), pr["nkf"] if nkf is None else nkf,
                                     pr["npts"] if npts is None else npts, a("obs_off"), a("obs_kf"), a("pt_bad"), a("kf_rank"), a("conn_off"), a("conn_kf"),
                                     a("conn_w"), a("prev_off"), a("prev_kf"), pr["th"] if th is None else th, *caps, *[a(k) for k in OUT])


def _problem():
    return cc.make(1, nkf=12, ntgt=5)


def test_symbols_are_exported_and_listed(lib):
    L = lib.load()
    for name in ("orbl_update_connections", "orbl_update_connections_device", "orbl_update_connections_workspace"):
        assert hasattr(L, name) and name in lib.SYMBOLS
    from ceres_mono_orb_slam2_amd import localmapping
    assert callable(localmapping.update_connections) and callable(localmapping.update_connections_device)


def test_every_argument_error_is_einval_before_device_work(lib):
    L = lib.load()
    pr = _problem()
    assert pr["kf_rank"] is not None and pr["prev_off"] is not None and len(pr["conn_kf"]) > 8 and pr["conn_off"][1] >= 2

    def changed(key, at, value):
        q = dict(pr); q[key] = pr[key].copy(); q[key][at] = value
        return q
    twice = changed("conn_kf", 1, pr["conn_kf"][0])                 # (row 0 has at least two entries)
    cases = {
        "negative ntgt": dict(pr=pr, ntgt=-1), "negative nkf": dict(pr=pr, nkf=-1), "negative npts": dict(pr=pr, npts=-1),
        "negative capacity": dict(pr=pr, caps=(4096, -1, 4096, 4096)),
        "slot_off not from 0": dict(pr=changed("slot_off", 0, 1)), "slot_off decreases": dict(pr=changed("slot_off", 2, 0)),
        "obs_off not from 0": dict(pr=changed("obs_off", 0, 2)), "obs_off decreases": dict(pr=changed("obs_off", 5, 0)),
        "conn_off not from 0": dict(pr=changed("conn_off", 0, 1)), "conn_off decreases": dict(pr=changed("conn_off", 3, 0)),
        "prev_off not from 0": dict(pr=changed("prev_off", 0, 1)), "prev_off decreases": dict(pr=changed("prev_off", 2, -1)),
        "target too large": dict(pr=changed("tgt_kf", 1, pr["nkf"])), "target negative": dict(pr=changed("tgt_kf", 0, -1)),
        "duplicate target": dict(pr=changed("tgt_kf", 3, pr["tgt_kf"][1])),
        "slot point too large": dict(pr=changed("slot_pt", 7, pr["npts"])), "slot point below -1": dict(pr=changed("slot_pt", 0, -2)),
        "observer too large": dict(pr=changed("obs_kf", 3, pr["nkf"])), "observer negative": dict(pr=changed("obs_kf", -1, -2)),
        "table keyframe too large": dict(pr=changed("conn_kf", 4, pr["nkf"])), "table keyframe negative": dict(pr=changed("conn_kf", 4, -1)),
        "table row names itself": dict(pr=changed("conn_kf", 0, 0)), "table row names a keyframe twice": dict(pr=twice),
        "previous neighbour too large": dict(pr=changed("prev_kf", 0, pr["nkf"])),
        "rank out of range": dict(pr=changed("kf_rank", 2, pr["nkf"])), "rank repeats": dict(pr=changed("kf_rank", 2, pr["kf_rank"][3])),
        "th 0": dict(pr=pr, th=0), "th negative": dict(pr=pr, th=-15),
        "NULL tgt_kf": dict(pr=pr, null=("tgt_kf",)), "NULL slot_off": dict(pr=pr, null=("slot_off",)), "NULL slot_pt": dict(pr=pr, null=("slot_pt",)),
        "NULL obs_off": dict(pr=pr, null=("obs_off",)), "NULL obs_kf": dict(pr=pr, null=("obs_kf",)), "NULL conn_off": dict(pr=pr, null=("conn_off",)),
        "NULL conn_w": dict(pr=pr, null=("conn_w",)), "NULL tgt_status": dict(pr=pr, null=("tgt_status",)), "NULL counts": dict(pr=pr, null=("counts",)),
        "NULL aff_kf": dict(pr=pr, null=("aff_kf",)), "NULL oconn_off": dict(pr=pr, null=("oconn_off",)), "NULL oord_w": dict(pr=pr, null=("oord_w",)),
        "prev_off without prev_kf": dict(pr=pr, null=("prev_kf",)), "prev_kf without prev_off": dict(pr=pr, null=("prev_off",)),
        "links without prev": dict(pr=pr, null=("prev_off", "prev_kf")), "link_kf without link_off": dict(pr=pr, null=("link_off",)),
    }
    for what, kw in cases.items():
        assert _call(lib, **kw) == EINVAL, what
        assert b"orbl_update_connections" in L.orbhip_last_error(), what
    # the device form checks counts, NULLs and alignment on the host
    z = C.c_void_p(256)                                             # (never dereferenced: every call below fails its checks first)
    args = [2, z, None, 5, z, z, 4, 6, 9, z, z, None, None, 3, z, z, z, 1, z, z, 15, 4, 9, 9, 9] + [z] * 12 + [None, z, None]
    for at, value in ((0, -1), (3, -1), (6, -1), (7, -1), (8, -1), (13, -1), (17, -1), (20, 0), (21, -1), (24, -1), (38, None), (1, None), (4, None), (5, None),
                      (9, None), (10, None), (14, None), (15, None), (16, None), (18, None), (19, None), (25, None), (27, None), (28, None), (31, None), (33, None),
                      (36, None), (1, C.c_void_p(258)), (30, C.c_void_p(257)), (38, C.c_void_p(260))):
        b = list(args); b[at] = value
        assert L.orbl_update_connections_device(*b) == EINVAL, at
    # a link output needs the previous lists
    b = list(args); b[17] = 0; b[18] = None; b[19] = None
    assert L.orbl_update_connections_device(*b) == EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_call_without_gpu_is_enodev(lib):
    from ceres_mono_orb_slam2_amd import localmapping
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()
    pr = _problem()
    assert _call(lib, pr) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _call(lib, pr, null=("tgt_flags", "pt_bad", "kf_rank", "prev_off", "prev_kf", "link_off", "link_kf")) == ENODEV
    with pytest.raises(OrbHipError, match="no HIP device"):
        localmapping.update_connections(pr["tgt_kf"], pr["slot_off"], pr["slot_pt"], pr["nkf"], pr["obs_off"], pr["obs_kf"], pr["conn_off"], pr["conn_kf"], pr["conn_w"])


def test_workspace_arithmetic(lib):
    L = lib.load()
    n = C.c_size_t(0)

    def up(x):
        return (x + 255) // 256 * 256
    for ntgt, nkf, npts, nslots, nconn in ((0, 0, 0, 0, 0), (1, 1, 1, 1, 0), (3, 64, 64, 65, 100), (60, 500, 24000, 120000, 9000), (257, 257, 7, 129, 66000)):
        assert L.orbl_update_connections_workspace(ntgt, nkf, npts, nslots, nconn, C.byref(n)) == 0
        cells = ntgt * nkf
        ent = nconn + 2 * cells
        want = 2 * up(4 * cells) + up(cells) + 2 * up(4 * nkf) + up(24 * ntgt) + up(28 * nkf) + up(4 * ent) + up(8 * ent) + up(4 * cells)
        assert n.value == max(want, 256)
        assert L.orbl_update_connections_workspace(ntgt, nkf, npts + 5, nslots + 9, nconn, C.byref(n)) == 0 and n.value == max(want, 256)
    for bad in ((-1, 0, 0, 0, 0), (0, -1, 0, 0, 0), (0, 0, -1, 0, 0), (0, 0, 0, -1, 0), (0, 0, 0, 0, -1)):
        assert L.orbl_update_connections_workspace(*bad, C.byref(n)) == EINVAL
    assert L.orbl_update_connections_workspace(1, 1, 1, 1, 1, None) == EINVAL


def test_dropin_test_program_compiles_and_links(lib, tmp_path):
    exe = tmp_path / "test_connections_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_connections_dropin.cpp"), "-o", str(exe), lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    assert exe.exists()
