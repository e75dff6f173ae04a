"""FrameOpsT::AssembleGlobalBA, ApplyGlobalBA and GlobalBundleAdjustemnt (csrc/compat/orbslam_dropin.h) over the mock data model:
tests/cpp/test_globalba_dropin.cpp runs the flattening and the write-back of CeresOptimizerT::BundleAdjustment (src/CeresOptimizer.cc:59-176,
:190-224, cut at the solve) on one copy of a map of real std::map pointer containers, and the drop-in calls on another whose keyframes and
points lie in memory in the same shuffled order.  The problem arrays must be equal field for field and, after ONE synthetic solution is
written back through both with a few keyframes and points turned bad in between, the written members - poses, centres, positions, normals,
depth ranges, global_BA_Tcw_, global_BA_pose_ and both stamps - bit for bit, for n_loop_keyframe == 0 and != 0; the whole calls of the
drop-in and of CeresOptimizerT stamp the same keyframes and points, and a map without keyframes is left alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_global_ba_dropins_leave_the_map_as_the_host_loops_do(tmp_path):
    from ceres_mono_orb_slam2_amd import _lib
    exe = tmp_path / "test_globalba_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_globalba_dropin.cpp"), "-o", str(exe), _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    h = subprocess.run([str(exe), "host"], capture_output=True, text=True, timeout=60)
    # (the host loops alone on this map: 35 cameras, 1373 points, 4853 rows; 31 poses and 1248 points written after the keyframes and
    # points that turned bad)
    assert h.returncode == 0 and h.stdout.split() == ["HOST", "35", "1373", "4853", "31", "1248"], h.stdout[-2000:] + h.stderr[-1000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    assert r.stdout.split()[-6:] == ["OK", "35", "1373", "4853", "31", "1248"]
