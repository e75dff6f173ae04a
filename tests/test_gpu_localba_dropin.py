"""FrameOpsT::AssembleLocalBA, ApplyLocalBA and LocalBundleAdjustment (csrc/compat/orbslam_dropin.h) over the mock data model:
tests/cpp/test_localba_dropin.cpp runs the reference-shaped loops of src/CeresOptimizer.cc:346-406, :423-506 and :573-598 on one copy of a map
of real std::map pointer containers, and the drop-in calls on another whose keyframes and points lie in memory in the same shuffled order.
The assembled problem must be equal field for field and, after a synthetic solver result is written back, the complete state - poses,
centres, slots, positions, normals, depth ranges, observations, Observations(), reference keyframes, bad flags - bit for bit; the stop flag
leaves a map untouched, a whole call leaves it consistent and reports the points it turned bad, a bad point caught in a slot does not
stop the call, an inconsistent map is refused with -1."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_local_ba_dropins_leave_the_map_as_the_host_loops_do(tmp_path):
    from ceres_mono_orb_slam2_amd import _lib
    exe = tmp_path / "test_localba_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_localba_dropin.cpp"), "-o", str(exe), _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    h = subprocess.run([str(exe), "host"], capture_output=True, text=True, timeout=60)
    # (the host loops alone on this map: 27 cameras, 622 local points, 2588 rows, 529 of them erased by the synthetic result, 115 points
    # turned bad by those erases)
    assert h.returncode == 0 and h.stdout.split() == ["HOST", "27", "622", "2588", "529", "115"], h.stdout[-2000:] + h.stderr[-1000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    assert r.stdout.split()[-6:] == ["OK", "27", "622", "2588", "529", "115"]
