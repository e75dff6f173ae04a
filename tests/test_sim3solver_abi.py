"""CPU checks of the orbt_sim3_* entry points: every argument check returns ORBHIP_EINVAL before any device work, valid arguments
fail loudly without a GPU, the structs match the header, and orbt_sim3_ransac_params is SetRansacParameters' arithmetic."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


def _args(n=30, ns=5):
    rng = np.random.default_rng(0)
    X = rng.uniform(-5, 5, (n, 3)) + np.array([0, 0, 12.0])
    return dict(x1=X.copy(), x2=X.copy(), e1=np.full(n, 9, np.float32), e2=np.full(n, 9, np.float32), n=n, K1=np.array([700, 700, 600, 180], np.float32),
                K2=np.array([700, 700, 600, 180], np.float32), fs=1, mi=20, sets=np.tile(np.arange(3, dtype=np.int32), (ns, 1)), ns=ns,
                bc=C.c_int32(0), bm=np.zeros(n, np.uint8), bR=np.eye(3), bt=np.zeros(3), bs=C.c_float(1.0), inl=np.zeros(n, np.uint8))


def _call(lib, a, **over):
    a = dict(a, **over)
    p = lambda x: None if x is None else lib.ptr(x)            # noqa: E731
    ref = lambda x: None if x is None else C.byref(x)          # noqa: E731
    res = lib.Sim3Result()
    return lib.load().orbt_sim3_iterate(p(a["x1"]), p(a["x2"]), p(a["e1"]), p(a["e2"]), a["n"], p(a["K1"]), p(a["K2"]), a["fs"], a["mi"], p(a["sets"]), a["ns"],
                                        ref(a["bc"]), p(a["bm"]), p(a["bR"]), p(a["bt"]), ref(a["bs"]), C.byref(res) if not a.get("nores") else None,
                                        p(a["inl"]), None)


def test_symbols_are_exported(lib):
    L = lib.load()
    for name in ("orbt_sim3_ransac_params", "orbt_sim3_iterate", "orbt_sim3_iterate_batch_device", "orbt_sim3_iterate_workspace"):
        assert name in lib.SYMBOLS and getattr(L, name)


def test_struct_layouts(lib, tmp_path):
    """The ctypes mirrors against the C header itself: sizes and every field offset; the status codes and limits."""
    src = tmp_path / "sizes.c"
    structs = (("orbt_sim3_params", lib.Sim3Params), ("orbt_sim3_result", lib.Sim3Result), ("orbt_sim3_trace", lib.Sim3Trace))
    body = '  printf("' + "%zu " * len(structs) + '\\n", ' + ", ".join("sizeof(%s)" % n for n, _ in structs) + ");\n"
    for name, cls in structs:
        body += "".join('  printf("%%zu ", offsetof(%s, %s));\n' % (name, f) for f, _ in cls._fields_) + '  printf("\\n");\n'
    body += '  printf("%d %d %d %d %d %d %d\\n", ORBT_SIM3_FOUND, ORBT_SIM3_NOT_FOUND, ORBT_SIM3_TOO_FEW, ORBT_SIM3_BAD_INPUT, ORBT_SIM3_MAX_N, ' \
            'ORBT_SIM3_MAX_ITERATIONS, ORBT_SIM3_MAX_CANDIDATES);\n'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbslam_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    assert [int(v) for v in lines[0].split()] == [C.sizeof(cls) for _, cls in structs]
    for k, (_, cls) in enumerate(structs):
        assert [int(v) for v in lines[1 + k].split()] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert C.sizeof(lib.Sim3Result) == 240 and C.sizeof(lib.Sim3Params) == 16
    from ceres_mono_orb_slam2_amd import sim3solver
    assert [int(v) for v in lines[4].split()] == [sim3solver.FOUND, sim3solver.NOT_FOUND, sim3solver.TOO_FEW, sim3solver.BAD_INPUT, 32768, 4096, 65535]


def test_sim3solver_dropin_compiles(lib):
    """The drop-in test program over the mock data model, and the ORBSLAM_DROPIN_REFERENCE_TYPES branch (ORB_SLAM2::Sim3Solver)."""
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp")]
    for src in ("test_sim3solver_dropin.cpp", "test_sim3solver_reference_types.cpp"):
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall"] + inc + [os.path.join(ROOT, "tests", "cpp", src)])


def test_iterate_argument_checks(lib):
    a = _args()
    bad = [dict(n=-1), dict(n=32769), dict(ns=-1), dict(ns=4097), dict(mi=2), dict(x1=None), dict(x2=None), dict(e1=None), dict(e2=None), dict(K1=None),
           dict(K2=None), dict(sets=None), dict(bc=None), dict(bm=None), dict(bR=None), dict(bt=None), dict(bs=None), dict(nores=True), dict(inl=None)]
    s = a["sets"].copy(); s[2, 1] = 30
    bad.append(dict(sets=s))
    s = a["sets"].copy(); s[0, 0] = -1
    bad.append(dict(sets=s))
    s = a["sets"].copy(); s[4, 2] = s[4, 0]
    bad.append(dict(sets=s))
    bad.append(dict(bc=C.c_int32(2)))                           # the mask holds no correspondence
    m = a["bm"].copy(); m[3] = 1
    bad.append(dict(bm=m))                                       # one in the mask, best_count 0
    bad.append(dict(bc=C.c_int32(-1)))
    for o in bad:
        assert _call(lib, a, **o) == EINVAL, o
        assert lib.load().orbhip_last_error()


def test_batch_and_workspace_argument_checks(lib):
    L = lib.load()
    nb = C.c_size_t(0)
    assert L.orbt_sim3_iterate_workspace(1, 100, 300, C.byref(nb)) == 0 and nb.value > 0
    small = nb.value
    assert L.orbt_sim3_iterate_workspace(16, 1600, 300, C.byref(nb)) == 0 and nb.value > small
    for a in ((0, 10, 35), (65536, 10, 35), (1, -1, 35), (1, 32769, 35), (1, 10, 0), (1, 10, 4097)):
        assert L.orbt_sim3_iterate_workspace(*a, C.byref(nb)) == EINVAL, a
    assert L.orbt_sim3_iterate_workspace(1, 10, 35, None) == EINVAL
    one = C.c_void_p(16)                                         # never dereferenced: the checks come first
    good = [1, one, one, one, one, one, 10, one, one, one, one, one, 35, one, one, one, one, one, one, one, one, one, None]
    assert len(good) == len(L.orbt_sim3_iterate_batch_device.argtypes)
    pointers = [k for k, v in enumerate(good) if v is one]
    assert len(pointers) == 19
    for k, v in ((0, 0), (0, 65536), (6, -1), (12, 0), (12, 5000)) + tuple((k, None) for k in pointers):
        args = list(good); args[k] = v
        assert L.orbt_sim3_iterate_batch_device(*args) == EINVAL, k


def test_valid_arguments_fail_loudly_without_a_gpu(lib):
    """No quiet fall-back: without a device the call fails with a device error (with one it runs)."""
    import torch
    rc = _call(lib, _args())
    if torch.cuda.is_available():
        assert rc == 0
        return
    assert rc != 0 and rc != EINVAL
    assert b"device" in lib.load().orbhip_last_error().lower()


def test_ransac_params(lib):
    import npsim3solver as ref
    L = lib.load()
    out = lib.Sim3Params()
    grid = [(N, mi, mx, p) for N in (0, 1, 3, 6, 19, 20, 21, 25, 40, 50, 64, 200, 1000, 32768) for mi in (0, 3, 6, 20, 50) for mx in (1, 35, 300)
            for p in (0.5, 0.99, 0.999)]
    seen_equal = seen_clamp = seen_few = seen_mid = 0
    for N, mi, mx, p in grid:
        assert L.orbt_sim3_ransac_params(N, p, mi, mx, C.byref(out)) == 0
        its = ref.ransac_params(N, p, mi, mx)
        assert (out.n, out.min_inliers, out.max_iterations) == (N, mi, its), (N, mi, mx, p)
        seen_equal += N == mi and N > 0
        seen_few += 0 < N < mi and its == 1
        seen_clamp += its == 300
        seen_mid += 1 < its < mx
    assert seen_equal and seen_clamp and seen_few and seen_mid
    # LoopClosing's call (src/LoopClosing.cc:271): 0.99, 20, 300
    assert L.orbt_sim3_ransac_params(40, 0.99, 20, 300, C.byref(out)) == 0 and out.max_iterations == 35
    assert L.orbt_sim3_ransac_params(20, 0.99, 20, 300, C.byref(out)) == 0 and out.max_iterations == 1
    assert L.orbt_sim3_ransac_params(12, 0.99, 20, 300, C.byref(out)) == 0 and out.max_iterations == 1
    for a in ((-1, 0.99, 20, 300), (32769, 0.99, 20, 300), (10, 1.0, 20, 300), (10, 0.0, 20, 300), (10, 0.99, -1, 300), (10, 0.99, 20, 0)):
        assert L.orbt_sim3_ransac_params(*a, C.byref(out)) == EINVAL, a
    assert L.orbt_sim3_ransac_params(10, 0.99, 20, 300, None) == EINVAL
