"""CPU checks of the lens-distortion entry points of the device-resident Tracking calls (include/orbslam_hip.h: orbt_image_bounds,
orbt_set_distortion, orbt_last_undistorted_keypoints): orbt_image_bounds - host arithmetic - equals, bit for bit, the min / max of the
oracle's undistorted corners for the reference's three distorted configurations (Frame::ComputeImageBounds, src/Frame.cc:357-385);
k1 == 0 alone decides "no distortion"; every argument error is ORBHIP_EINVAL; the symbols are exported, declared and bound in Python.
(ORBHIP_ECAP of orbt_last_undistorted_keypoints needs a resident frame, hence a GPU: tests/test_gpu_track_distortion.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

from tests.trackdist_cases import CAMERAS, oracle_bounds

EINVAL = -1
NAMES = ("orbt_image_bounds", "orbt_set_distortion", "orbt_last_undistorted_keypoints")
# a vectorised numpy restatement of the five iterations gave these bounds: a sanity range, not the expected bits
SANITY = {"TUM1": [10.80, 626.05, 14.67, 473.31], "EuRoC": [-135.80, 895.51, -92.88, 565.55]}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


def _bounds(lib, w, h, K4, dist):
    out = np.full(4, -7, np.float32)
    rc = lib.load().orbt_image_bounds(w, h, lib.ptr(K4), lib.ptr(dist), lib.ptr(out))
    return rc, out


def test_symbols_are_exported_and_declared(lib):
    L = lib.load()
    hdr = open(os.path.join(os.path.dirname(lib._HERE), "include", "orbslam_hip.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in lib.SYMBOLS and ("int %s(" % name) in hdr
        assert getattr(L, name).argtypes is not None
    from ceres_mono_orb_slam2_amd import tracking
    assert callable(tracking.image_bounds) and callable(tracking.set_distortion)
    assert "zero distortion" not in hdr


@pytest.mark.parametrize("name", ["TUM1", "TUM2", "EuRoC"])
def test_image_bounds_equal_the_oracles_undistorted_corners(lib, oracle, name):
    cam = CAMERAS[name]
    rc, got = _bounds(lib, cam["w"], cam["h"], cam["K4"], cam["dist"])
    want = oracle_bounds(oracle, cam)
    print(name, got.tolist(), want.tolist())
    assert rc == 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if name in SANITY:
        assert np.abs(got - np.array(SANITY[name])).max() < 0.01
    assert got[0] < got[1] and got[2] < got[3]
    from ceres_mono_orb_slam2_amd import tracking
    assert np.array_equal(tracking.image_bounds(cam["w"], cam["h"], cam["K4"], cam["dist"]).view(np.uint32), want.view(np.uint32))


def test_k1_alone_decides(lib):
    cam = CAMERAS["TUM1"]
    d = cam["dist"].copy(); d[0] = 0.0                                          # the other four stay non-zero (src/Frame.cc:358 tests k1 alone)
    rc, got = _bounds(lib, cam["w"], cam["h"], cam["K4"], d)
    assert rc == 0 and got.tolist() == [0.0, 640.0, 0.0, 480.0]
    rc, got = _bounds(lib, 1241, 376, CAMERAS["KITTI_k1"]["K4"], np.zeros(5, np.float32))
    assert rc == 0 and got.tolist() == [0.0, 1241.0, 0.0, 376.0]


def test_argument_errors_are_einval(lib):
    L = lib.load()
    cam = CAMERAS["TUM1"]
    K4, d, out = cam["K4"], cam["dist"], np.zeros(4, np.float32)
    p = lib.ptr
    assert L.orbt_image_bounds(640, 480, None, p(d), p(out)) == EINVAL
    assert L.orbt_image_bounds(640, 480, p(K4), None, p(out)) == EINVAL
    assert L.orbt_image_bounds(640, 480, p(K4), p(d), None) == EINVAL
    assert b"NULL" in L.orbhip_last_error()
    for w, h in ((0, 480), (-1, 480), (640, 0), (640, -5)):
        assert L.orbt_image_bounds(w, h, p(K4), p(d), p(out)) == EINVAL, (w, h)
    for k in range(5):
        for bad in (np.nan, np.inf, -np.inf):
            b = d.copy(); b[k] = bad
            assert L.orbt_image_bounds(640, 480, p(K4), p(b), p(out)) == EINVAL, (k, bad)
    bK = K4.copy(); bK[0] = np.nan
    assert L.orbt_image_bounds(640, 480, p(bK), p(d), p(out)) == EINVAL
    assert (out == 0).all()                                                     # nothing written by a refused call
    # orbt_set_distortion: NULL context; non-finite coefficients (checked before the context is looked at: the handle below is never
    # dereferenced)
    fake = C.c_void_p(256)
    assert L.orbt_set_distortion(None, p(d)) == EINVAL
    assert L.orbt_set_distortion(None, None) == EINVAL
    for k in range(5):
        for bad in (np.nan, np.inf):
            b = d.copy(); b[k] = bad
            assert L.orbt_set_distortion(fake, p(b)) == EINVAL, (k, bad)
    assert b"non-finite" in L.orbhip_last_error()
    assert L.orbt_set_distortion(fake, None) == 0                               # "none" for a context that never had any: nothing to do
    # orbt_last_undistorted_keypoints: NULL arguments, negative capacity, no resident frame on this thread
    xy = np.zeros((8, 2), np.float32); n = C.c_int(-3)
    assert L.orbt_last_undistorted_keypoints(None, p(xy), 8, C.byref(n)) == EINVAL
    assert L.orbt_last_undistorted_keypoints(fake, p(xy), 8, None) == EINVAL
    assert L.orbt_last_undistorted_keypoints(fake, None, 8, C.byref(n)) == EINVAL
    assert L.orbt_last_undistorted_keypoints(fake, p(xy), -1, C.byref(n)) == EINVAL
    assert L.orbt_last_undistorted_keypoints(fake, p(xy), 8, C.byref(n)) == EINVAL
    assert b"no frame" in L.orbhip_last_error() and n.value == -3
