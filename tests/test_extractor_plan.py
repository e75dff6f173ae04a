"""The extractor's plan (csrc/orb_geometry.h) on the host alone: tests/cpp/test_extractor_plan.cpp plans every shape the GPU tests
and the bench use plus a sweep around them and asserts the preconditions the kernels rely on, under AddressSanitizer and
UndefinedBehaviorSanitizer.  A stand-alone program: no GPU, no HIP, nothing loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extractor_plan_preconditions_under_sanitizers(tmp_path):
    exe = tmp_path / "test_extractor_plan"
    # (the sanitizer runtimes are linked statically: the program then starts in whatever environment the test inherits)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "ceres_mono_orb_slam2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_extractor_plan.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plans checked" in r.stdout and not r.stderr, r.stdout + r.stderr
