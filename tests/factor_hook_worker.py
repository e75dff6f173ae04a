"""Child process of tests/test_gpu_diag_factor.py: loads the hook library and makes the calls one job file describes, so that a
call that hangs or faults ends a child under a timeout and not the test session.
    python factor_hook_worker.py LIB IN.npz OUT.npz
IN holds either  A [n, 32, 32], groups [g] (block counts: one hook call per group, its blocks factored back to back) and nw,
or  x [n] (the scalar maps)."""
import ctypes as C
import sys

import numpy as np


def main(lib, src, dst):
    L = C.CDLL(lib)
    L.ba_debug_factor_batch_nw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.ba_debug_factor_scalar_maps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
    job = np.load(src)
    if "x" in job.files:
        x = np.ascontiguousarray(job["x"], np.float64)
        w = np.zeros_like(x); y = np.zeros_like(x)
        rc = L.ba_debug_factor_scalar_maps(x.ctypes.data, w.ctypes.data, y.ctypes.data, len(x))
        assert rc == 0, rc
        np.savez(dst, w=w, y=y)
        return
    A = np.ascontiguousarray(job["A"], np.float64)
    nw = int(job["nw"])
    X = np.zeros_like(A); bad = np.full(len(A), -1, np.int32)
    at = 0
    for g in job["groups"].tolist():
        rc = L.ba_debug_factor_batch_nw(A[at:].ctypes.data, X[at:].ctypes.data, bad[at:].ctypes.data, g, nw)
        assert rc == 0, rc
        at += g
    assert at == len(A)
    np.savez(dst, X=X, bad=bad)


if __name__ == "__main__":
    main(*sys.argv[1:4])
