"""FrameOpsT::UpdateConnections (csrc/compat/orbslam_dropin.h) over the mock data model: tests/cpp/test_connections_dropin.cpp runs the
loop of LoopClosing.cc:551-573 with the mock's reference-shaped UpdateConnections / AddConnection on one copy of a map with stale
tables, and the drop-in's single library call on another whose keyframes lie in memory in the same shuffled order; every keyframe's
map, ordered lists, parent, children, first-connection flag and loop_connections must be identical afterwards."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_update_connections_dropin_leaves_the_graph_as_the_host_loop_does(tmp_path):
    from ceres_mono_orb_slam2_amd import _lib
    exe = tmp_path / "test_connections_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_connections_dropin.cpp"), "-o", str(exe), _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    h = subprocess.run([str(exe), "host"], capture_output=True, text=True, timeout=60)
    # (the host loop alone on this map: 38 of 40 keyframes written, 50 new links, 13 first connections)
    assert h.returncode == 0 and h.stdout.split() == ["HOST", "38", "50", "13"], h.stdout[-2000:] + h.stderr[-1000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    ok, written, links, parents = r.stdout.split()[-4:]
    assert ok == "OK" and int(written) == 38 and int(links) == 50 and int(parents) == 13
