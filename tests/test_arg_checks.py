"""The argument checks the host-pointer entry points share (csrc/orb_argcheck.h) on the host alone: tests/cpp/test_arg_checks.cpp
drives the CSR, index-range, "listed once" and permutation checks over their edge cases (no rows, empty rows, a decrease at either
end, a total of INT32_MAX, both bounds and one past each, the -1 exemption) and asserts acceptance or rejection and that a rejection
names the entry point and the array, under AddressSanitizer and UndefinedBehaviorSanitizer.  A stand-alone program: no GPU, no HIP,
nothing loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arg_checks_under_sanitizers(tmp_path):
    exe = tmp_path / "test_arg_checks"
    # (the sanitizer runtimes are linked statically: the program then starts in whatever environment the test inherits)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "ceres_mono_orb_slam2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_arg_checks.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "argument checks checked" in r.stdout and not r.stderr, r.stdout + r.stderr
