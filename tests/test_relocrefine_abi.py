"""CPU checks of orbt_relocalization_refine's boundary (include/orbslam_hip.h): the symbol is exported, declared and bound in Python; the
struct layouts match; every argument error is ORBHIP_EINVAL (ORBHIP_ECAP for a capacity) with a message that names the entry and the
array, before any device work - the context is never looked at; a valid call without a GPU is ORBHIP_ENODEV."""
import ctypes as C
import os

import numpy as np
import pytest

EINVAL, ENODEV, ECAP = -1, -2, -4
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


class _Fake:                                   # an extractor handle that must never be dereferenced
    _h = C.c_void_p(256)


def _cand(n=6, n_kp=8, pose=True):
    slot = np.full(n_kp, -1, np.int32); slot[:3] = [0, 2, 4][:n_kp] if n else -1
    return dict(pt=np.arange(n, dtype=np.int32) + 100, Xw=np.ones((n, 3)), desc=np.zeros((n, 32), np.uint8), min_dist=np.ones(n, F32), max_dist=np.full(n, 9, F32),
                angle=np.zeros(n, F32), Tcw=np.eye(4) if pose else None, slot_kf=slot if pose else None)


def _call(cands, **kw):
    from ceres_mono_orb_slam2_amd import tracking
    return tracking.relocalization_refine(_Fake, [500, 500, 320, 240], [0, 640, 0, 480], cands, kw.pop("log_scale", 0.1823), n_kp=kw.pop("n_kp", 8), **kw)


def test_symbol_is_exported_declared_and_bound(lib):
    L = lib.load()
    hdr = open(os.path.join(os.path.dirname(lib._HERE), "include", "orbslam_hip.h")).read()
    name = "orbt_relocalization_refine"
    assert hasattr(L, name) and name in lib.SYMBOLS and ("int %s(" % name) in hdr and getattr(L, name).argtypes is not None
    from ceres_mono_orb_slam2_amd import tracking
    assert callable(tracking.relocalization_refine)
    assert C.sizeof(tracking._RefineCand) == 72 and C.sizeof(tracking._RefineResult) == 104
    assert "#define ORBT_RR_MAX_CANDIDATES 64" in hdr and tracking.RR_MAX_CANDIDATES == 64
    for i, k in enumerate(("NO_POSE", "FEW_INLIERS", "MATCH_FIRST", "MATCH_SECOND", "MATCH_THIRD", "FAIL_WIDE", "FAIL_SECOND", "FAIL_NARROW", "FAIL_THIRD")):
        assert ("#define ORBT_RR_%s %d " % (k, i)) in hdr and getattr(tracking, "RR_" + k) == i
    assert "orbt_relocalization_refine" in hdr.split("int orbt_relocalization_search_by_bow(")[0].rsplit("/* ----", 1)[1]      # the first stage points at it


def test_argument_errors_name_the_entry_and_the_array(lib):
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()

    def refused(cands, what, code=EINVAL, **kw):
        with pytest.raises(OrbHipError) as e:
            _call(cands, **kw)
        assert ("code %d" % code) in str(e.value) and what in str(e.value), str(e.value)
    c = _cand(); c["slot_kf"][5] = 6
    refused([_cand(), c], "orbt_relocalization_refine: candidates[1].slot_kf[5] = 6 is out of range (-1 to 5)")
    c = _cand(); c["slot_kf"][1] = -2
    refused([c], "orbt_relocalization_refine: candidates[0].slot_kf[1] = -2 is out of range")
    c = _cand(); c["pt"][2] = -1
    refused([c], "orbt_relocalization_refine: candidates[0].slot_kf[1] = 2 names a feature without a map point")
    c = _cand(); c["pt"][3] = -5
    refused([_cand(pose=False), _cand(), c], "orbt_relocalization_refine: candidates[2].pt[3] = -5 is below -1")
    c = _cand(n=0); c["slot_kf"][7] = 0
    refused([c], "candidates[0].slot_kf[7] = 0 is out of range")
    c = _cand(); c["Tcw"] = np.eye(4); c["Tcw"][1, 3] = np.nan
    refused([c], "non-finite candidate pose")
    refused([_cand()], "bad log_scale_factor", log_scale=0.0)
    refused([_cand()], "bad log_scale_factor", log_scale=float("nan"))
    refused([_cand(n_kp=1)] * 65, "more than 64 candidates", code=ECAP, n_kp=1)
    refused([_cand(n_kp=4097)], "more than 4096 features per frame", code=ECAP, n_kp=4097)
    refused([_cand(n=4097)], "more than 4096 features per keyframe", code=ECAP)
    # NULL arguments, straight through ctypes
    first = C.c_int32(7)
    z = np.zeros(64, np.int32)
    assert L.orbt_relocalization_refine(None, lib.ptr(z), lib.ptr(z), 0.18, None, 0, 8, 1, 1, None, None, None, C.byref(first)) == EINVAL
    assert L.orbt_relocalization_refine(_Fake._h, None, lib.ptr(z), 0.18, None, 0, 8, 1, 1, None, None, None, C.byref(first)) == EINVAL
    assert L.orbt_relocalization_refine(_Fake._h, lib.ptr(z), lib.ptr(z), 0.18, None, 0, 8, 1, 1, None, None, None, None) == EINVAL
    assert L.orbt_relocalization_refine(_Fake._h, lib.ptr(z), lib.ptr(z), 0.18, None, 1, 8, 1, 1, None, None, None, C.byref(first)) == EINVAL
    assert L.orbt_relocalization_refine(_Fake._h, lib.ptr(z), lib.ptr(z), 0.18, None, -1, 8, 1, 1, None, None, None, C.byref(first)) == EINVAL
    assert b"NULL" in L.orbhip_last_error() and first.value == 7
    # no candidates: nothing to do, no device needed
    assert L.orbt_relocalization_refine(_Fake._h, lib.ptr(z), lib.ptr(z), 0.18, None, 0, 8, 1, 1, None, None, None, C.byref(first)) == 0 and first.value == -1


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_call_without_a_gpu_is_enodev(lib):
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    with pytest.raises(OrbHipError, match="no HIP device") as e:
        _call([_cand(), _cand(pose=False)])
    assert ("code %d" % ENODEV) in str(e.value)
