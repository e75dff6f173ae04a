"""FrameOpsT::SetBadFlags (csrc/compat/orbslam_dropin.h) over the mock data model: tests/cpp/test_badflag_dropin.cpp runs the mock's
reference-shaped KeyFrame::SetBadFlag on the targets one after the other on one copy of a 60-keyframe map, and the drop-in's single
library call on another whose keyframes lie in memory in the same shuffled order; the whole map state - maps, ordered lists, parents,
children, flags, Tcp to the bit, slots, observations, reference keyframes, and what was erased from the map and the database - must be
identical afterwards, and a keyframe listed twice is refused with the map untouched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_set_bad_flags_dropin_leaves_the_map_as_the_host_loop_does(tmp_path):
    from ceres_mono_orb_slam2_amd import _lib
    exe = tmp_path / "test_badflag_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_badflag_dropin.cpp"), "-o", str(exe), _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    h = subprocess.run([str(exe), "host"], capture_output=True, text=True, timeout=60)
    # (the host loop alone on this map: 7 of the 9 targets go - two have do_not_erase_ set -, 113 points turn bad, 6 keyframes get a new parent)
    assert h.returncode == 0 and h.stdout.split() == ["HOST", "7", "113", "6"], h.stdout[-2000:] + h.stderr[-1000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    assert r.stdout.split()[-4:] == ["OK", "7", "113", "6"]
