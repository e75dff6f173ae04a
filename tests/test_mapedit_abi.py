"""CPU checks of the map-edit entry points (include/orbslam_hip.h: orbl_apply_map_edits*): the symbols are exported and listed, every argument
error is ORBHIP_EINVAL before any device work, a valid call without a GPU is ORBHIP_ENODEV (no CPU fallback), and the workspace size is
the documented host arithmetic."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import mapeditcases as mc  # noqa: E402

EINVAL, ENODEV = -1, -2
IN1 = ("kf_slot_off", "kf_rank", "kf_slot_pt", "kf_slot_level", "kf_slot_uv")
IN2 = ("pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced", "obs_off", "obs_kf", "obs_slot", "obs_dead")
OUT = ("op_status", "op_found", "pt_touched", "oobs_off", "oobs_kf", "oobs_slot", "oobs_src", "oobs_level", "oobs_uv", "counts")
INOUT = ("kf_slot_pt", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


def _call(lib, pr, nops=None, nkf=None, npts=None, null=(), cap=4096):
    L = lib.load()
    hold = {k: np.zeros(8194, np.float32 if k == "oobs_uv" else np.uint8 if k == "pt_touched" else np.int32) for k in OUT}
    hold.update({k: np.array(pr[k]) for k in INOUT if pr.get(k) is not None})          # (in/out: copies)

    def a(k):
        v = hold[k] if k in hold else pr.get(k)
        return None if (k in null or v is None) else lib.ptr(v)
    return L.orbl_apply_map_edits(len(pr["op_kind"]) if nops is None else nops, *[a(k) for k in mc.OP_KEYS], pr["nkf"] if nkf is None else nkf, *[a(k) for k in IN1],
                                  pr["npts"] if npts is None else npts, *[a(k) for k in IN2], cap, *[a(k) for k in OUT])


def _problem():
    pr = mc.make(1, nkf=8, npts=60, nops=40)
    return dict(pr, obs_dead=np.zeros(len(pr["obs_kf"]), np.uint8))


def test_symbols_are_exported_and_listed(lib):
    L = lib.load()
    for name in ("orbl_apply_map_edits", "orbl_apply_map_edits_device", "orbl_apply_map_edits_workspace"):
        assert hasattr(L, name) and name in lib.SYMBOLS
    from ceres_mono_orb_slam2_amd import localmapping
    assert callable(localmapping.apply_map_edits) and callable(localmapping.apply_map_edits_device)
    assert localmapping.MapEditResult.__slots__


def test_every_argument_error_is_einval_before_device_work(lib):
    L = lib.load()
    pr = _problem()
    nkf, npts = pr["nkf"], pr["npts"]
    kinds = list(pr["op_kind"])
    i_add, i_rep, i_fuse, i_found = kinds.index(mc.ADD), kinds.index(mc.REPLACE), kinds.index(mc.FUSE), kinds.index(mc.REPLACE_FOUND)
    p2 = next(p for p in range(npts) if pr["obs_off"][p + 1] - pr["obs_off"][p] >= 2)          # a point with two observations
    e0 = int(pr["obs_off"][p2])
    per_kf = int(pr["kf_slot_off"][1])

    def changed(key, at, value):
        q = dict(pr); q[key] = pr[key].copy(); q[key][at] = value
        return q
    cases = {
        "negative nops": dict(pr=pr, nops=-1), "negative nkf": dict(pr=pr, nkf=-1), "negative npts": dict(pr=pr, npts=-1), "negative cap_obs": dict(pr=pr, cap=-1),
        "kf_slot_off not from 0": dict(pr=changed("kf_slot_off", 0, 1)), "kf_slot_off decreases": dict(pr=changed("kf_slot_off", 3, 0)),
        "obs_off not from 0": dict(pr=changed("obs_off", 0, 2)), "obs_off decreases": dict(pr=changed("obs_off", 5, 0)),
        "rank out of range": dict(pr=changed("kf_rank", 2, nkf)), "rank repeats": dict(pr=changed("kf_rank", 2, pr["kf_rank"][3])),
        "slot point too large": dict(pr=changed("kf_slot_pt", per_kf - 1, npts)), "slot point below -1": dict(pr=changed("kf_slot_pt", per_kf - 1, -2)),
        "observer too large": dict(pr=changed("obs_kf", e0, nkf)), "observer negative": dict(pr=changed("obs_kf", e0, -1)),
        "obs_slot negative": dict(pr=changed("obs_slot", e0, -1)), "obs_slot outside its keyframe": dict(pr=changed("obs_slot", e0, per_kf)),
        "a list names a keyframe twice": dict(pr=changed("obs_kf", e0 + 1, pr["obs_kf"][e0])),
        "an observation's slot does not hold its point": dict(pr=changed("kf_slot_pt", int(pr["kf_slot_off"][pr["obs_kf"][e0]] + pr["obs_slot"][e0]), -1)),
        "pt_replaced too large": dict(pr=changed("pt_replaced", 0, npts)),
        "kind too large": dict(pr=changed("op_kind", 0, 7)), "kind negative": dict(pr=changed("op_kind", 0, -1)),
        "op_pt too large": dict(pr=changed("op_pt", i_add, npts)), "op_pt negative": dict(pr=changed("op_pt", i_fuse, -1)),
        "op_kf too large": dict(pr=changed("op_kf", i_add, nkf)), "op_kf negative": dict(pr=changed("op_kf", i_fuse, -1)),
        "op_slot outside its keyframe": dict(pr=changed("op_slot", i_add, per_kf)), "op_slot negative": dict(pr=changed("op_slot", i_fuse, -1)),
        "REPLACE onto no point": dict(pr=changed("op_arg", i_rep, npts)), "REPLACE onto a negative point": dict(pr=changed("op_arg", i_rep, -1)),
        "REPLACE_FOUND names itself": dict(pr=changed("op_arg", i_found, i_found)), "REPLACE_FOUND names a later op": dict(pr=changed("op_arg", i_found, i_found + 1)),
        "REPLACE_FOUND names a negative op": dict(pr=changed("op_arg", i_found, -1)), "REPLACE_FOUND names no FIND_OR_ADD": dict(pr=changed("op_arg", i_found, i_add)),
        "half a pair: pt_found": dict(pr=pr, null=("pt_found",)), "half a pair: pt_visible": dict(pr=pr, null=("pt_visible",)),
        "half a pair: kf_slot_level": dict(pr=pr, null=("kf_slot_level",)), "half a pair: kf_slot_uv": dict(pr=pr, null=("kf_slot_uv",)),
        "NULL oobs_level with the pair": dict(pr=pr, null=("oobs_level",)), "NULL oobs_uv with the pair": dict(pr=pr, null=("oobs_uv",)),
    }
    for k in mc.OP_KEYS + ("kf_slot_off", "kf_slot_pt", "pt_bad", "pt_nobs", "obs_off", "obs_kf", "obs_slot", "op_status", "op_found", "pt_touched", "oobs_off",
                           "oobs_kf", "oobs_slot", "counts"):
        cases["NULL " + k] = dict(pr=pr, null=(k,))
    assert i_add < i_found and kinds[i_add] != mc.FIND_OR_ADD
    for what, kw in cases.items():
        assert _call(lib, **kw) == EINVAL, what
        assert b"orbl_apply_map_edits" in L.orbhip_last_error(), what
    # the device form checks counts, NULLs and alignment on the host
    z = C.c_void_p(256)                                             # (never dereferenced: every call below fails its checks first)
    args = [3, z, z, z, z, z, 4, z, None, 9, z, z, z, 6, z, z, z, z, None, 12, z, z, z, None, 16, z, z, z, z, z, z, None, z, z, z, None, z, None]
    assert len(args) == len(L.orbl_apply_map_edits_device.argtypes)
    for at, value in ((0, -1), (6, -1), (9, -1), (13, -1), (19, -1), (24, -1), (1, None), (2, None), (3, None), (4, None), (5, None), (7, None), (10, None), (11, None),
                      (12, None), (14, None), (15, None), (16, None), (17, None), (20, None), (21, None), (22, None), (25, None), (26, None), (27, None), (28, None),
                      (29, None), (30, None), (32, None), (33, None), (34, None), (36, None), (1, C.c_void_p(258)), (15, C.c_void_p(257)), (33, C.c_void_p(258)),
                      (36, C.c_void_p(258))):
        b = list(args); b[at] = value
        assert L.orbl_apply_map_edits_device(*b) == EINVAL, at


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_call_without_gpu_is_enodev(lib):
    from ceres_mono_orb_slam2_amd import localmapping
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()
    pr = _problem()
    assert _call(lib, pr) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _call(lib, pr, null=("kf_rank", "kf_slot_level", "kf_slot_uv", "pt_found", "pt_visible", "pt_replaced", "obs_dead", "oobs_src", "oobs_level", "oobs_uv")) == ENODEV
    assert _call(lib, pr, nops=0, null=mc.OP_KEYS + ("op_status", "op_found")) == ENODEV          # (the pure rebuild)
    with pytest.raises(OrbHipError, match="no HIP device"):
        localmapping.apply_map_edits({k: pr[k] for k in mc.OP_KEYS}, pr)


def test_workspace_arithmetic(lib):
    L = lib.load()
    n = C.c_size_t(0)

    def up(x):
        return (x + 255) // 256 * 256
    for nops, nkf, npts, nslots, nobs in ((0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (40, 8, 60, 448, 270), (4500, 500, 100000, 400000, 600000), (1025, 80, 257, 9, 7)):
        assert L.orbl_apply_map_edits_workspace(nops, nkf, npts, nslots, nobs, C.byref(n)) == 0
        ents, blocks = nobs + nops, (npts + 255) // 256
        want = (2 * up(npts) + up(4 * nkf) + up(8) + up(4 * npts) + up(4 * ents) + up(nobs) + 2 * up(4 * npts) + up(4 * (blocks + 1)) + up(4 * ents))
        assert n.value == want
    for bad in ((-1, 0, 0, 0, 0), (0, -1, 0, 0, 0), (0, 0, -1, 0, 0), (0, 0, 0, -1, 0), (0, 0, 0, 0, -1)):
        assert L.orbl_apply_map_edits_workspace(*bad, C.byref(n)) == EINVAL
    assert L.orbl_apply_map_edits_workspace(1, 1, 1, 1, 1, None) == EINVAL
