"""FrameOpsT::LoopSim3Candidates (csrc/compat/orbslam_dropin.h) over the mock data model: tests/cpp/test_loopsim3_dropin.cpp runs a
reference-shaped host loop - src/LoopClosing.cc:250-277 with SearchByBoW(KeyFrame*, KeyFrame*) and Sim3Solver's constructor over real
pointers and std::map observations - and the one drop-in call on the same scene; the match vectors, the discard flags and the packed rows
must be equal, the doubles bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_loop_sim3_candidates_dropin_equals_the_host_loop(tmp_path):
    from ceres_mono_orb_slam2_amd import _lib
    exe = tmp_path / "test_loopsim3_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_loopsim3_dropin.cpp"), "-o", str(exe), _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    h = subprocess.run([str(exe), "host"], capture_output=True, text=True, timeout=60)
    # (the host loop alone on this scene: 5 of 7 candidates kept - one is bad, one has fewer than 20 matches -, 3111 rows, 3586 matches)
    assert h.returncode == 0 and h.stdout.split() == ["HOST", "5", "3111", "3586"], h.stdout[-2000:] + h.stderr[-1000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    assert r.stdout.split()[-4:] == ["OK", "5", "3111", "3586"]
