"""FrameOpsT::AssembleEssentialGraph, ApplyEssentialGraph and OptimizeEssentialGraph (csrc/compat/orbslam_dropin.h) over the mock data model:
tests/cpp/test_essgraph_dropin.cpp runs CeresOptimizerT::OptimizeEssentialGraph - the host graph walk as it stands - on one copy of a map of
real std::set / std::map pointer containers, and the drop-in on another whose keyframes and points lie in memory in the same shuffled order.
The program defines ba_optimize_essential_graph itself: both callers hand it their problem, which must name the same vertices and the same
edges in the same order (tangents and Sji within 1e-12), and both get one synthetic result back, after which poses, centres and points agree
within 1e-12.  A data model without the members the entries read still instantiates FrameOpsT (an explicit instantiation in the program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_essential_graph_dropins_leave_the_map_as_the_host_walk_does(tmp_path):
    from ceres_mono_orb_slam2_amd import _lib
    exe = tmp_path / "test_essgraph_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_essgraph_dropin.cpp"), "-o", str(exe), _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    out = r.stdout.split()
    assert out[-5] == "OK" and int(out[-4]) > 45 and int(out[-3]) >= 90 and int(out[-2]) >= 3 and int(out[-1]) >= 300
