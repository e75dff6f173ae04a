"""FrameOpsT::RelocalizationRefine (csrc/compat/orbslam_dropin.h) over the mock data model: tests/cpp/test_reloc_refine_dropin.cpp extracts a
frame on the device, runs a host loop of the reference's shape over the existing drop-ins (CeresOptimizer::PoseOptimization,
ORBmatcher::SearchByProjection(Frame&, KeyFrame*, ...), break at the first match) and then the drop-in's one library call on the same
frame; Tcw_, map_points_, is_outliers_ and the returned index must be identical, with the match in the middle of a round and without one."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_relocalization_refine_dropin_equals_the_host_loop(tmp_path):
    from ceres_mono_orb_slam2_amd import _lib
    exe = tmp_path / "test_reloc_refine_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_reloc_refine_dropin.cpp"), "-o", str(exe), _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    ok, rounds, first1, first2, filled, refined = r.stdout.split()[-6:]
    # round 1: candidates 0 and 2 fail, 1 has no pose, 3 is matched behind its second solve (4 would match at once: never refined by the
    # host loop); round 2: nobody matches, all four are refined
    assert ok == "OK" and int(rounds) == 2 and int(first1) == 3 and int(first2) == -1 and int(filled) >= 50 and int(refined) == 3 + 4
