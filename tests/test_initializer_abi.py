"""CPU checks of the orbt_initialize* entry points: every argument check returns ORBHIP_EINVAL before any device work, valid
arguments fail loudly without a GPU, and the structs match the header."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


def _args(n1=20, n2=20, nm=12, it=4):
    rng = np.random.default_rng(0)
    a = dict(k1=rng.uniform(0, 500, (n1, 2)).astype(np.float32), k2=rng.uniform(0, 500, (n2, 2)).astype(np.float32),
             m=np.full(n1, -1, np.int32), K=np.array([700, 700, 600, 180], np.float32), sigma=1.0, it=it,
             sets=np.tile(np.arange(8, dtype=np.int32), (it, 1)), R=np.zeros(9), t=np.zeros(3), P=np.zeros((n1, 3)), tri=np.zeros(n1, np.uint8))
    a["m"][:nm] = np.arange(nm)
    a["n1"], a["n2"] = n1, n2
    return a


def _call(lib, a, **over):
    a = dict(a, **over)
    L = lib.load()
    p = lambda x: None if x is None else lib.ptr(x)            # noqa: E731
    rep = lib.InitReport()
    return L.orbt_initialize(p(a["k1"]), a["n1"], p(a["k2"]), a["n2"], p(a["m"]), p(a["K"]), float(a["sigma"]), a["it"], p(a["sets"]),
                             p(a["R"]), p(a["t"]), p(a["P"]), p(a["tri"]), C.byref(rep) if not a.get("norep") else None, None)


def test_struct_layouts(lib, tmp_path):
    """The ctypes mirrors against the C header itself: sizes and every field offset."""
    src = tmp_path / "sizes.c"
    rep = [f for f, _ in lib.InitReport._fields_]
    tr = [f for f, _ in lib.InitTrace._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbslam_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(orbt_init_report), sizeof(orbt_init_trace));\n' +
                   "".join('  printf("%%zu ", offsetof(orbt_init_report, %s));\n' % f for f in rep) + '  printf("\\n");\n' +
                   "".join('  printf("%%zu ", offsetof(orbt_init_trace, %s));\n' % f for f in tr) + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    assert [int(v) for v in lines[0].split()] == [C.sizeof(lib.InitReport), C.sizeof(lib.InitTrace)]
    assert [int(v) for v in lines[1].split()] == [getattr(lib.InitReport, f).offset for f in rep]
    assert [int(v) for v in lines[2].split()] == [getattr(lib.InitTrace, f).offset for f in tr]
    assert C.sizeof(lib.InitReport) == 104


def test_initializer_dropin_compiles_and_links(lib, tmp_path):
    """The reference-types branch of csrc/compat/orbslam_initializer.h compiles (-fsyntax-only, the reference's names bound to the
    mock data model), and the drop-in test program links against the library (it runs on the GPU box:
    tests/test_gpu_initializer_dropin.py)."""
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall"] + inc + [os.path.join(ROOT, "tests", "cpp", "test_initializer_reference_types.cpp")])
    exe = tmp_path / "test_initializer_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + inc + [os.path.join(ROOT, "tests", "cpp", "test_initializer_dropin.cpp"), "-o", str(exe),
                           lib.LIB_PATH, "-lpthread", "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    assert exe.exists()


def test_initialize_rejects_mismatched_sets(lib):
    from ceres_mono_orb_slam2_amd import initializer
    a = _args()
    with pytest.raises(ValueError, match="ransac_sets"):
        initializer.initialize(a["k1"], a["k2"], a["m"], a["K"], 1.0, 5, a["sets"])


@pytest.mark.parametrize("name,over", [
    ("negative n1", dict(n1=-1)), ("oversized n1", dict(n1=32769)), ("negative n2", dict(n2=-1)), ("oversized n2", dict(n2=32769)),
    ("zero iterations", dict(it=0)), ("too many iterations", dict(it=4097)),
    ("sigma zero", dict(sigma=0.0)), ("sigma negative", dict(sigma=-1.0)), ("sigma nan", dict(sigma=float("nan"))),
    ("null kps1", dict(k1=None)), ("null kps2", dict(k2=None)), ("null matches", dict(m=None)), ("null K", dict(K=None)),
    ("null sets", dict(sets=None)), ("null R", dict(R=None)), ("null t", dict(t=None)), ("null P3D", dict(P=None)),
    ("null triangulated", dict(tri=None)), ("null report", dict(norep=True)),
])
def test_einval_arguments(lib, name, over):
    assert _call(lib, _args(), **over) == -1, name
    assert b"orbt_initialize" in lib.load().orbhip_last_error()


def test_einval_data(lib):
    a = _args(nm=7)
    assert _call(lib, a) == -1 and b"fewer than 8" in lib.load().orbhip_last_error()
    a = _args(); a["m"][3] = 20                                 # == n2
    assert _call(lib, a) == -1
    a = _args(); a["m"][3] = -2
    assert _call(lib, a) == -1
    a = _args(); a["sets"][2, 5] = 12                           # == n_matches
    assert _call(lib, a) == -1
    a = _args(); a["sets"][0, 0] = -1
    assert _call(lib, a) == -1


def test_device_entry_and_workspace_check_counts(lib):
    L = lib.load()
    n = C.c_size_t(0)
    assert L.orbt_initialize_workspace(0, 10, 10, 200, C.byref(n)) == -1
    assert L.orbt_initialize_workspace(1, 10, 10, 0, C.byref(n)) == -1
    assert L.orbt_initialize_workspace(1, 40000, 10, 200, C.byref(n)) == -1
    assert L.orbt_initialize_workspace(2, 4000, 4000, 200, C.byref(n)) == 0 and n.value > 0
    vp = C.c_void_p(16)
    assert L.orbt_initialize_batch_device(1, vp, vp, 10, vp, vp, 10, vp, vp, 0.0, 200, vp, vp, vp, vp, vp, vp, vp, None) == -1
    assert L.orbt_initialize_batch_device(1, vp, vp, 10, vp, vp, 10, vp, vp, 1.0, 200, vp, vp, vp, vp, vp, vp, None, None) == -1
    assert L.orbt_initialize_batch_device(0, vp, vp, 10, vp, vp, 10, vp, vp, 1.0, 200, vp, vp, vp, vp, vp, vp, vp, None) == -1


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device error path cannot be exercised")
def test_valid_arguments_fail_loudly_without_gpu(lib):
    from ceres_mono_orb_slam2_amd import initializer
    a = _args()
    with pytest.raises(lib.OrbHipError, match="no HIP device"):
        initializer.initialize(a["k1"], a["k2"], a["m"], a["K"], 1.0, 4, a["sets"])
