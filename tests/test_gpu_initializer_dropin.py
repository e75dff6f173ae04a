"""InitializerT (csrc/compat/orbslam_initializer.h) over the mock data model: tests/cpp/test_initializer_dropin.cpp draws the sets
through a stand-in RNG, checks them against a restatement of src/Initializer.cc:88-101 on the same generator, and checks the
drop-in's outputs bit-identical to orbt_initialize on those sets."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def test_initializer_dropin_matches_library(tmp_path):
    from ceres_mono_orb_slam2_amd import _lib, synth
    exe = tmp_path / "test_initializer_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_initializer_dropin.cpp"), "-o", str(exe), _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    results = []
    for seed, kind, noise in ((10, "general", 0.0), (0, "planar", 0.0), (0, "sparse", 0.5)):
        s = synth.make_two_view(seed, kind, 400 if kind != "sparse" else 200, 0.0, noise)
        path = tmp_path / ("scene_%s.bin" % kind)
        with open(path, "wb") as f:
            f.write(np.array([len(s["kps1"]), len(s["kps2"]), 200], np.int32).tobytes())
            f.write(np.asarray(s["K4"], np.float32).tobytes())
            f.write(np.ascontiguousarray(s["kps1"], np.float32).tobytes()); f.write(np.ascontiguousarray(s["kps2"], np.float32).tobytes())
            f.write(np.ascontiguousarray(s["matches12"], np.int32).tobytes())
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
        ok, success, n, model = r.stdout.split()[-4:]
        assert ok == "OK"
        results.append((kind, int(success), int(model)))
    assert ("general", 1, 1) in results and ("planar", 1, 0) in results, results
    assert ("sparse", 0, 1) in results, results
