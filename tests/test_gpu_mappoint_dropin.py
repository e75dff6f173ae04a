"""FrameOpsT::UpdateMapPoints (csrc/compat/orbslam_dropin.h) over the mock data model: tests/cpp/test_mappoint_dropin.cpp runs the
mock's host MapPoint::ComputeDistinctiveDescriptors on one copy of a map and the drop-in's single library call on another; every
descriptor_ must be byte-equal, and the normal / depth fields equal to a restatement of src/MapPoint.cc:335-378."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_update_map_points_dropin_matches_mock_host_method(tmp_path):
    from ceres_mono_orb_slam2_amd import _lib
    exe = tmp_path / "test_mappoint_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_mappoint_dropin.cpp"), "-o", str(exe), _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    ok, npts, changed, maxn = r.stdout.split()[-4:]
    assert ok == "OK" and int(changed) > 1000 and int(maxn) >= 8
