"""CPU checks of the OptimizeEssentialGraph-on-the-tables entry points (include/orbslam_hip.h: orbl_essential_graph_assemble*,
orbl_essential_graph_apply*): the symbols are exported and listed, every argument error is ORBHIP_EINVAL before any device work, a valid
call without a GPU is ORBHIP_ENODEV (no CPU fallback), the workspace sizes are the documented host arithmetic, and the drop-in test program
compiles and links."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import essgraphcases as ec  # noqa: E402
from tests import npessgraph as npe  # noqa: E402

EINVAL, ENODEV = -1, -2
NAMES = ("orbl_essential_graph_assemble", "orbl_essential_graph_assemble_device", "orbl_essential_graph_assemble_workspace", "orbl_essential_graph_apply",
         "orbl_essential_graph_apply_device", "orbl_essential_graph_apply_workspace")
EG_IN = ("kf_id", "kf_bad", "kf_rank", "kf_Tcw", "kf_parent", "child_off", "child_kf", "loop_off", "loop_kf", "conn_off", "conn_kf", "conn_w", "ord_off", "ord_kf", "ord_w")
EG_GROUP = ("conn_group_kf", "corrected", "non_corrected")
EG_LINK = ("tgt_kf", "link_off", "link_kf")
EG_OUT = (("counts", np.int32, 4), ("vtx_kf", np.int32, 1), ("kf_vtx", np.int32, 1), ("lie7", np.float64, 7), ("vtx_fixed", np.uint8, 1), ("edge_j", np.int32, 1),
          ("edge_i", np.int32, 1), ("edge_Sji", np.float64, 7), ("edge_kind", np.uint8, 1))
EA_IN = ("X", "pt_bad", "pt_done", "pt_corr_ref", "pt_ref_kf", "obs_off", "obs_kf", "ref_level", "scale_factors")
EA_OUT = ("normal", "min_max", "nd_written", "pt_moved", "counts")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def world():
    m = ec.seeded_map(3, 30, 80, n_group=5)
    kb = np.array(m["kf_bad"])
    kb[next(k for k in range(30) if k not in m["conn_group_kf"] and k != m["loop"])] = 1         # (at least one bad keyframe)
    m = ec.without(m, kf_bad=kb)
    asm = npe.assemble(m)
    ap = dict(m)
    ap.update(vtx_kf=asm["vtx_kf"], lie_orig=asm["lie7"], lie_opt=ec.solver_result(4, asm["lie7"]))
    return m, ap


def _assemble(lib, m, null=(), nkf=None, nconn=None, ntgt=None, loop=None, cur=None, min_weight=100, caps=(64, 1024)):
    L = lib.load()
    v = {k: (None if m[k] is None else np.array(m[k])) for k in EG_IN + EG_GROUP + EG_LINK}
    v.update({k: np.zeros(w * 1024, dt) for k, dt, w in EG_OUT})

    def a(k):
        return None if (k in null or v[k] is None) else lib.ptr(v[k])
    return L.orbl_essential_graph_assemble(m["nkf"] if nkf is None else nkf, *[a(k) for k in EG_IN], len(m["conn_group_kf"]) if nconn is None else nconn, *[a(k) for k in EG_GROUP],
                                           len(m["tgt_kf"]) if ntgt is None else ntgt, *[a(k) for k in EG_LINK], m["loop"] if loop is None else loop, m["cur"] if cur is None else cur,
                                           min_weight, *caps, *[a(k) for k, _, _ in EG_OUT])


def _apply(lib, p, null=(), n_vtx=None, nkf=None, npts=None, n_levels=8):
    L = lib.load()
    keys = ("vtx_kf", "lie_orig", "lie_opt", "kf_Tcw", "kf_center") + EA_IN
    v = {k: (None if p[k] is None else np.array(p[k])) for k in keys}
    n = p["npts"]
    v.update(normal=np.zeros((n, 3)), min_max=np.zeros((n, 2), np.float32), nd_written=np.zeros(n, np.uint8), pt_moved=np.zeros(n, np.uint8), counts=np.zeros(2, np.int32))

    def a(k):
        return None if (k in null or v[k] is None) else lib.ptr(v[k])
    return L.orbl_essential_graph_apply(len(p["vtx_kf"]) if n_vtx is None else n_vtx, a("vtx_kf"), a("lie_orig"), a("lie_opt"), p["nkf"] if nkf is None else nkf, a("kf_Tcw"),
                                        a("kf_center"), n if npts is None else npts, *[a(k) for k in EA_IN], n_levels, *[a(k) for k in EA_OUT])


def _changed(pr, key, at, value):
    q = dict(pr); q[key] = np.array(pr[key]); q[key].reshape(-1)[at] = value
    return q


def test_symbols_are_exported_listed_and_declared(lib):
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "orbslam_hip.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in lib.SYMBOLS and ("int %s(" % name) in hdr
    from ceres_mono_orb_slam2_amd import loopclosing
    for f in ("essential_graph_assemble", "essential_graph_assemble_device", "essential_graph_apply", "essential_graph_apply_device", "optimize_essential_graph_on_tables"):
        assert callable(getattr(loopclosing, f))


def test_assemble_argument_errors_are_einval_before_device_work(lib, world):
    L = lib.load()
    m, _ = world
    ch = _changed
    nkf = m["nkf"]
    good = np.nonzero(m["kf_bad"] == 0)[0]
    cases = {
        "nkf 0": dict(m=m, nkf=0), "negative nconn": dict(m=m, nconn=-1), "negative ntgt": dict(m=m, ntgt=-1), "loop_kf too large": dict(m=m, loop=nkf),
        "loop_kf negative": dict(m=m, loop=-1), "cur_kf too large": dict(m=m, cur=nkf), "cur_kf negative": dict(m=m, cur=-1), "min_weight 0": dict(m=m, min_weight=0),
        "negative cap_vtx": dict(m=m, caps=(-1, 4)), "negative cap_edges": dict(m=m, caps=(4, -1)),
        "kf_rank too large": dict(m=ch(m, "kf_rank", 2, nkf)), "kf_rank repeats": dict(m=ch(m, "kf_rank", 2, m["kf_rank"][3])),
        "parent too large": dict(m=ch(m, "kf_parent", 4, nkf)), "parent below -1": dict(m=ch(m, "kf_parent", 4, -2)),
        "group member twice": dict(m=ch(m, "conn_group_kf", 0, m["conn_group_kf"][1])), "group member too large": dict(m=ch(m, "conn_group_kf", 0, nkf)),
        "target twice": dict(m=ch(m, "tgt_kf", 0, m["tgt_kf"][1])), "target negative": dict(m=ch(m, "tgt_kf", 0, -1)),
        "corrected NaN": dict(m=ch(m, "corrected", 9, np.nan)), "corrected inf": dict(m=ch(m, "corrected", 4, np.inf)),
        "corrected zero quaternion": dict(m=ch(m, "corrected", slice(7, 11), 0.0)), "non_corrected NaN": dict(m=ch(m, "non_corrected", 1, np.nan)),
        "non_corrected zero quaternion": dict(m=ch(m, "non_corrected", slice(0, 4), 0.0)),
        "kf_id repeats among the good": dict(m=ch(m, "kf_id", good[0], m["kf_id"][good[1]])),
    }
    for off, arr in (("child_off", "child_kf"), ("loop_off", "loop_kf"), ("conn_off", "conn_kf"), ("ord_off", "ord_kf"), ("link_off", "link_kf")):
        cases[off + " not from 0"] = dict(m=ch(m, off, 0, 1))
        cases[off + " decreases"] = dict(m=ch(m, off, len(m[off]) - 1, -1))
        cases[arr + " too large"] = dict(m=ch(m, arr, 0, nkf))
        cases[arr + " negative"] = dict(m=ch(m, arr, len(m[arr]) - 1, -1))
    for k in ("kf_id", "kf_Tcw", "kf_parent", "child_off", "child_kf", "loop_off", "loop_kf", "conn_off", "conn_kf", "conn_w", "ord_off", "ord_kf", "ord_w", "conn_group_kf",
              "corrected", "non_corrected", "tgt_kf", "link_off", "link_kf") + tuple(k for k, _, _ in EG_OUT):
        cases["NULL " + k] = dict(m=m, null=(k,))
    for what, kw in cases.items():
        assert _assemble(lib, **kw) == EINVAL, what
        assert b"orbl_essential_graph_assemble" in L.orbhip_last_error(), what
    # a bad keyframe may repeat an id
    bad = np.nonzero(m["kf_bad"])[0]
    assert len(bad) and _assemble(lib, ch(m, "kf_id", bad[0], m["kf_id"][good[0]])) in (0, ENODEV)
    # the nullable inputs left out pass the checks (0 with a GPU, ORBHIP_ENODEV without)
    assert _assemble(lib, m, null=("kf_bad", "kf_rank")) in (0, ENODEV)
    assert _assemble(lib, m, null=EG_GROUP, nconn=0) in (0, ENODEV) and _assemble(lib, m, null=EG_LINK, ntgt=0) in (0, ENODEV)
    assert _assemble(lib, m, null=("kf_bad", "kf_rank") + EG_GROUP + EG_LINK, nconn=0, ntgt=0) in (0, ENODEV)
    # the device form checks counts, NULLs and alignment on the host
    z = C.c_void_p(256)                                             # (never dereferenced: every call below fails its checks first)
    args = [4, z, None, None, z, z, 3, z, z, 3, z, z, 5, z, z, z, 5, z, z, z, 2, z, z, z, 2, z, 3, z, z, 0, 3, 100, 4, 9] + [z] * 9 + [None, z, None]
    assert len(args) == len(L.orbl_essential_graph_assemble_device.argtypes)
    for at, value in ((0, 0), (6, -1), (9, -1), (12, -1), (16, -1), (20, -1), (24, -1), (26, -1), (29, 4), (29, -1), (30, 4), (30, -1), (31, 0), (32, -1), (33, -1),
                      (1, None), (4, None), (5, None), (7, None), (8, None), (10, None), (11, None), (13, None), (14, None), (15, None), (17, None), (18, None), (19, None),
                      (21, None), (22, None), (23, None), (25, None), (27, None), (28, None), (34, None), (35, None), (36, None), (37, None), (38, None), (39, None), (40, None),
                      (41, None), (42, None), (44, None), (4, C.c_void_p(260)), (22, C.c_void_p(252)), (37, C.c_void_p(260)), (41, C.c_void_p(260)), (1, C.c_void_p(258)),
                      (14, C.c_void_p(258)), (36, C.c_void_p(258)), (43, C.c_void_p(258)), (44, C.c_void_p(260))):
        b = list(args); b[at] = value
        assert L.orbl_essential_graph_assemble_device(*b) == EINVAL, at


def test_apply_argument_errors_are_einval_before_device_work(lib, world):
    L = lib.load()
    _, p = world
    ch = _changed
    nkf, npts = p["nkf"], p["npts"]
    alive = [i for i in range(npts) if not p["pt_bad"][i]]
    plain = next(i for i in alive if not p["pt_done"][i])
    done = next(i for i in alive if p["pt_done"][i])
    seen = next(i for i in alive if p["obs_off"][i] < p["obs_off"][i + 1])
    cases = {
        "negative n_vtx": dict(p=p, n_vtx=-1), "negative nkf": dict(p=p, nkf=-1), "negative npts": dict(p=p, npts=-1), "n_levels 0": dict(p=p, n_levels=0),
        "n_levels 65": dict(p=p, n_levels=65), "vertex keyframe too large": dict(p=ch(p, "vtx_kf", 1, nkf)), "vertex keyframe negative": dict(p=ch(p, "vtx_kf", 0, -1)),
        "vertex keyframe twice": dict(p=ch(p, "vtx_kf", 0, p["vtx_kf"][1])), "lie_opt NaN": dict(p=ch(p, "lie_opt", 8, np.nan)), "lie_orig inf": dict(p=ch(p, "lie_orig", 3, np.inf)),
        "reference keyframe too large": dict(p=ch(p, "pt_ref_kf", plain, nkf)), "reference keyframe below -1": dict(p=ch(p, "pt_ref_kf", plain, -2)),
        "corrected reference too large": dict(p=ch(p, "pt_corr_ref", done, nkf)), "corrected reference below -1": dict(p=ch(p, "pt_corr_ref", done, -2)),
        "obs_off not from 0": dict(p=ch(p, "obs_off", 0, 1)), "obs_off decreases": dict(p=ch(p, "obs_off", npts, 0)),
        "observer too large": dict(p=ch(p, "obs_kf", 3, nkf)), "observer negative": dict(p=ch(p, "obs_kf", -1, -1)),
        "level too large": dict(p=ch(p, "ref_level", seen, 8)), "level negative": dict(p=ch(p, "ref_level", seen, -1)),
        "pt_done without pt_corr_ref": dict(p=p, null=("pt_corr_ref",)), "normals without kf_center": dict(p=p, null=("kf_center",)),
    }
    for k in ("obs_off", "obs_kf", "ref_level", "scale_factors", "normal", "min_max", "nd_written"):
        cases["normal set without " + k] = dict(p=p, null=(k,))
    for k in ("vtx_kf", "lie_orig", "lie_opt", "kf_Tcw", "X", "pt_ref_kf", "pt_moved", "counts"):
        cases["NULL " + k] = dict(p=p, null=(k,))
    for what, kw in cases.items():
        assert _apply(lib, **kw) == EINVAL, what
        assert b"orbl_essential_graph_apply" in L.orbhip_last_error(), what
    # the nullable inputs left out pass the checks (0 with a GPU, ORBHIP_ENODEV without)
    for null in (("pt_done", "pt_corr_ref"), ("pt_bad",), ("pt_bad", "pt_done", "pt_corr_ref"), ("pt_corr_ref", "pt_done", "normal", "min_max", "nd_written", "scale_factors",
                                                                                                 "obs_off", "obs_kf", "ref_level", "kf_center")):
        assert _apply(lib, p, null=null) in (0, ENODEV), null
    z = C.c_void_p(256)
    args = [3, z, z, z, 4, z, z, 6, z, None, z, z, z, 9, z, z, z, z, 8, z, z, z, z, z, None, z, None]
    assert len(args) == len(L.orbl_essential_graph_apply_device.argtypes)
    for at, value in ((0, -1), (4, -1), (7, -1), (13, -1), (18, 0), (18, 65), (1, None), (2, None), (3, None), (5, None), (8, None), (12, None), (22, None), (23, None), (25, None),
                      (11, None), (6, None), (14, None), (15, None), (16, None), (17, None), (19, None), (20, None), (21, None), (2, C.c_void_p(260)), (8, C.c_void_p(252)),
                      (19, C.c_void_p(260)), (25, C.c_void_p(260)), (1, C.c_void_p(258)), (12, C.c_void_p(258)), (20, C.c_void_p(258)), (24, C.c_void_p(258))):
        b = list(args); b[at] = value
        assert L.orbl_essential_graph_apply_device(*b) == EINVAL, at


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_calls_without_gpu_are_enodev(lib, world):
    from ceres_mono_orb_slam2_amd import loopclosing
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()
    m, p = world
    assert _assemble(lib, m) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _assemble(lib, m, null=("kf_bad", "kf_rank")) == ENODEV
    assert _apply(lib, p) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert _apply(lib, p, null=("pt_bad",)) == ENODEV
    assert _apply(lib, p, null=("normal", "min_max", "nd_written", "scale_factors", "obs_off", "obs_kf", "ref_level", "kf_center")) == ENODEV
    for hm in [ec.hand_map()[0]] + list(ec.small_cases().values()):
        assert _assemble(lib, hm) == ENODEV
    with pytest.raises(OrbHipError, match="no HIP device"):
        loopclosing.essential_graph_assemble(m["loop"], m["cur"], m)
    with pytest.raises(OrbHipError, match="no HIP device"):
        loopclosing.essential_graph_apply(p["vtx_kf"], p["lie_orig"], p["lie_opt"], p)
    with pytest.raises(OrbHipError, match="no HIP device"):
        loopclosing.optimize_essential_graph_on_tables(m["loop"], m["cur"], m)


def test_workspace_arithmetic(lib):
    L = lib.load()
    n = C.c_size_t(0)

    def up(x):
        return (x + 255) // 256 * 256
    for nkf, n_vtx in ((1, 0), (8, 8), (500, 470), (1100, 7), (0, 0)):
        assert L.orbl_essential_graph_assemble_workspace(nkf, C.byref(n)) == 0
        assert n.value == 3 * up(4 * nkf) + 2 * up(8 * nkf) + 2 * up(8 * ((nkf + 255) // 256 + 1)) + 2 * up(56 * nkf)
        assert L.orbl_essential_graph_apply_workspace(nkf, n_vtx, C.byref(n)) == 0 and n.value == max(up(4 * nkf) + 2 * up(56 * n_vtx), 256)
    assert L.orbl_essential_graph_assemble_workspace(-1, C.byref(n)) == EINVAL and L.orbl_essential_graph_assemble_workspace(1, None) == EINVAL
    for bad in ((-1, 1), (1, -1)):
        assert L.orbl_essential_graph_apply_workspace(*bad, C.byref(n)) == EINVAL
    assert L.orbl_essential_graph_apply_workspace(1, 1, None) == EINVAL


def test_dropin_test_program_compiles_and_links(lib, tmp_path):
    """with it the explicit instantiation of FrameOpsT over mock::Types, a data model without the members the new entries read"""
    import subprocess
    exe = tmp_path / "test_essgraph_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_essgraph_dropin.cpp"), "-o", str(exe), lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    assert exe.exists()
