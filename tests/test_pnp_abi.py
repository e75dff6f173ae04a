"""CPU checks of the orbt_pnp_* entry points: every argument check returns ORBHIP_EINVAL before any device work, valid arguments
fail loudly without a GPU, the structs match the header, and orbt_pnp_ransac_params is SetRansacParameters' arithmetic."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    return dict(p3=rng.uniform(-5, 5, (n, 3)).astype(np.float32), p2=rng.uniform(0, 500, (n, 2)).astype(np.float32), e=np.full(n, 5.991, np.float32),
                n=n, K=np.array([700, 700, 600, 180], np.float32), mi=15, sets=np.tile(np.arange(4, dtype=np.int32), (ns, 1)), ns=ns,
                bc=C.c_int32(0), bm=np.zeros(n, np.uint8), bt=np.eye(4), inl=np.zeros(n, np.uint8))


def _call(lib, a, **over):
    a = dict(a, **over)
    p = lambda x: None if x is None else lib.ptr(x)            # noqa: E731
    res = lib.PnpResult()
    return lib.load().orbt_pnp_iterate(p(a["p3"]), p(a["p2"]), p(a["e"]), a["n"], p(a["K"]), a["mi"], p(a["sets"]), a["ns"],
                                       C.byref(a["bc"]) if a["bc"] is not None else None, p(a["bm"]), p(a["bt"]),
                                       C.byref(res) if not a.get("nores") else None, p(a["inl"]), None)


def test_struct_layouts(lib, tmp_path):
    """The ctypes mirrors against the C header itself: sizes and every field offset."""
    src = tmp_path / "sizes.c"
    structs = (("orbt_pnp_params", lib.PnpParams), ("orbt_pnp_result", lib.PnpResult), ("orbt_pnp_trace", lib.PnpTrace))
    body = '  printf("' + "%zu " * len(structs) + '\\n", ' + ", ".join("sizeof(%s)" % n for n, _ in structs) + ");\n"
    for name, cls in structs:
        body += "".join('  printf("%%zu ", offsetof(%s, %s));\n' % (name, f) for f, _ in cls._fields_) + '  printf("\\n");\n'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbslam_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    assert [int(v) for v in lines[0].split()] == [C.sizeof(cls) for _, cls in structs]
    for k, (_, cls) in enumerate(structs):
        assert [int(v) for v in lines[1 + k].split()] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert C.sizeof(lib.PnpResult) == 144 and C.sizeof(lib.PnpParams) == 16


def test_pnpsolver_dropin_compiles(lib):
    """The drop-in test program over the mock data model, and the ORBSLAM_DROPIN_REFERENCE_TYPES branch (ORB_SLAM2::PnPsolver)."""
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp")]
    for src in ("test_pnpsolver_dropin.cpp", "test_pnpsolver_reference_types.cpp"):
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall"] + inc + [os.path.join(ROOT, "tests", "cpp", src)])


def test_iterate_argument_checks(lib):
    a = _args()
    bad = [dict(n=-1), dict(n=32769), dict(ns=-1), dict(ns=4097), dict(mi=3), dict(p3=None), dict(p2=None), dict(e=None), dict(K=None),
           dict(sets=None), dict(bc=None), dict(bm=None), dict(bt=None), dict(nores=True), dict(inl=None)]
    s = a["sets"].copy(); s[2, 1] = 30
    bad.append(dict(sets=s))
    s = a["sets"].copy(); s[0, 0] = -1
    bad.append(dict(sets=s))
    s = a["sets"].copy(); s[4, 3] = s[4, 1]
    bad.append(dict(sets=s))
    bad.append(dict(bc=C.c_int32(2)))                           # the mask holds no point
    m = a["bm"].copy(); m[3] = 1
    bad.append(dict(bm=m))                                       # a point in the mask, best_count 0
    bad.append(dict(bc=C.c_int32(-1)))
    for o in bad:
        assert _call(lib, a, **o) == EINVAL, o
        assert lib.load().orbhip_last_error()


def test_batch_and_workspace_argument_checks(lib):
    L = lib.load()
    nb = C.c_size_t(0)
    assert L.orbt_pnp_iterate_workspace(1, 100, 35, C.byref(nb)) == 0 and nb.value > 0
    small = nb.value
    assert L.orbt_pnp_iterate_workspace(16, 1600, 35, C.byref(nb)) == 0 and nb.value > small
    for a in ((0, 10, 35), (65536, 10, 35), (1, -1, 35), (1, 32769, 35), (1, 10, 0), (1, 10, 4097)):
        assert L.orbt_pnp_iterate_workspace(*a, C.byref(nb)) == EINVAL, a
    assert L.orbt_pnp_iterate_workspace(1, 10, 35, None) == EINVAL
    one = C.c_void_p(16)                                         # never dereferenced: the checks come first
    good = [1, one, one, one, one, 10, one, one, one, 35, one, one, one, one, one, one, one, None]
    for k, v in ((0, 0), (5, -1), (9, 0), (9, 5000)) + tuple((k, None) for k in (1, 2, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16)):
        args = list(good); args[k] = v
        assert L.orbt_pnp_iterate_batch_device(*args) == EINVAL, k


def test_valid_arguments_fail_loudly_without_a_gpu(lib):
    """No quiet fall-back: without a device the call fails with a device error (with one it runs)."""
    import torch
    rc = _call(lib, _args())
    if torch.cuda.is_available():
        assert rc == 0
        return
    assert rc != 0 and rc != EINVAL
    assert b"device" in lib.load().orbhip_last_error().lower()


def _params_ref(N, p, min_inliers, max_its, min_set, eps):
    """src/PnPsolver.cc:130-153 with Python's own arithmetic (float32 where the reference has float)."""
    f = np.float32
    n_min = int(f(N) * f(eps))
    if n_min < min_inliers:
        n_min = min_inliers
    if n_min < min_set:
        n_min = min_set
    e = f(eps)
    if N > 0 and e < f(n_min) / f(N):
        e = f(n_min) / f(N)
    if n_min == N or N == 0:
        its = 1
    else:
        try:
            v = math.ceil(math.log(1 - p) / math.log(1 - float(e) ** 3))
        except (ValueError, ZeroDivisionError):                 # log of a negative number / of zero: the reference's int(NaN) ends at 1
            v = 1
        its = v
    return n_min, max(1, min(its, max_its)), e


def test_ransac_params(lib):
    L = lib.load()
    out = lib.PnpParams()
    grid = [(N, mi, mx, eps) for N in (0, 3, 4, 9, 10, 11, 19, 20, 21, 50, 200, 1999, 2000) for mi in (0, 4, 10, 50) for mx in (1, 35, 300)
            for eps in (0.05, 0.1, 0.4, 0.5, 0.9, 1.0)]
    seen_one = seen_clamp = seen_raise = seen_few = 0
    for N, mi, mx, eps in grid:
        assert L.orbt_pnp_ransac_params(N, 0.99, mi, mx, 4, eps, C.byref(out)) == 0
        n_min, its, e = _params_ref(N, 0.99, mi, mx, 4, eps)
        assert (out.n, out.min_inliers, out.max_iterations) == (N, n_min, its), (N, mi, mx, eps)
        assert np.float32(out.epsilon) == e or N == 0
        seen_one += n_min == N and its == 1
        seen_clamp += its == 300
        seen_raise += N > 0 and e > np.float32(eps)
        seen_few += 0 < N < n_min
    assert seen_one and seen_clamp and seen_raise and seen_few
    # Tracking's call (src/Tracking.cc:1030)
    assert L.orbt_pnp_ransac_params(200, 0.99, 10, 300, 4, 0.5, C.byref(out)) == 0
    assert (out.min_inliers, out.max_iterations) == (100, 35)
    for a in ((10, 0.99, 10, 300, 3, 0.5), (10, 0.99, 10, 300, 5, 0.5), (-1, 0.99, 10, 300, 4, 0.5), (10, 1.0, 10, 300, 4, 0.5), (10, 0.0, 10, 300, 4, 0.5),
              (10, 0.99, -1, 300, 4, 0.5), (10, 0.99, 10, 0, 4, 0.5), (10, 0.99, 10, 300, 4, 0.0), (10, 0.99, 10, 300, 4, 1.5)):
        assert L.orbt_pnp_ransac_params(*a, C.byref(out)) == EINVAL, a
    assert L.orbt_pnp_ransac_params(10, 0.99, 10, 300, 4, 0.5, None) == EINVAL
