"""FrameOpsT::UpdateLocalKeyFrames / UpdateLocalPoints (csrc/compat/orbslam_dropin.h) over the mock data model:
tests/cpp/test_local_map_dropin.cpp runs host loops of the reference's shape (a real std::map<KeyFrame*, int>, the real
std::set<KeyFrame*> of GetChilds(): pointer order is the real thing) and the drop-in's two library calls on the same map; the lists,
reference_keyframe_, the frame's slots and every track_reference_for_frame_ must be identical."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_update_local_map_dropin_equals_the_host_loops(tmp_path):
    from ceres_mono_orb_slam2_amd import _lib
    exe = tmp_path / "test_local_map_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_local_map_dropin.cpp"), "-o", str(exe), _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    ok, frames, n_kf, n_pt, no_votes, over80, parent_breaks = r.stdout.split()[-7:]
    # every path of the keyframe walk is taken by some frame of the program
    assert ok == "OK" and int(frames) == 8 and int(n_kf) > 100 and int(n_pt) > 1000 and int(no_votes) >= 1 and int(over80) >= 1 and int(parent_breaks) >= 1
