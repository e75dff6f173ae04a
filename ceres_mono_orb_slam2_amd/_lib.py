"""ctypes loader for the in-tree HIP C-ABI library (include/orbslam_hip.h), the ctypes mirrors of its structs, and the helpers every
wrapper module calls it with.  The signatures are read from the header at load: a new entry point is bound by declaring it there.

There is no CPU fallback: if the library is missing or a call fails the product raises.
"""
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORBHIP_LIB") or os.path.join(_HERE, "lib", "liborbslam_hip.so")   # (ORBHIP_LIB: a profiling / experiment build)


class BaProblem(C.Structure):                 # ba_problem
    _fields_ = [("K4", C.c_void_p), ("poses7", C.c_void_p), ("cam_fixed", C.c_void_p), ("ncam", C.c_int32),
                ("pts3", C.c_void_p), ("npts", C.c_int32), ("obs_cam", C.c_void_p), ("obs_pt", C.c_void_p),
                ("obs_uv", C.c_void_p), ("obs_weight", C.c_void_p), ("obs_robust", C.c_void_p), ("nobs", C.c_int32)]


class BaLocalProblem(C.Structure):            # ba_local_problem
    _fields_ = [("K4", C.c_void_p), ("poses7", C.c_void_p), ("cam_fixed", C.c_void_p), ("cam_local", C.c_void_p),
                ("ncam", C.c_int32), ("pts3", C.c_void_p), ("npts", C.c_int32), ("obs_cam", C.c_void_p),
                ("obs_pt", C.c_void_p), ("obs_uv", C.c_void_p), ("obs_inv_sigma2", C.c_void_p), ("nobs", C.c_int32),
                ("obs_erase", C.c_void_p)]


class OrbHipError(RuntimeError):
    pass


class InitReport(C.Structure):                # orbt_init_report
    _fields_ = [("model", C.c_int32), ("reason", C.c_int32), ("score_h", C.c_float), ("score_f", C.c_float), ("rh", C.c_float),
                ("best_h", C.c_int32), ("best_f", C.c_int32), ("n_matches", C.c_int32), ("n_inliers", C.c_int32), ("motion", C.c_int32),
                ("n_good", C.c_int32 * 8), ("parallax", C.c_float * 8)]


class InitTrace(C.Structure):                 # orbt_init_trace
    _fields_ = [("H21", C.c_void_p), ("H12", C.c_void_p), ("F21", C.c_void_p), ("score_h", C.c_void_p), ("score_f", C.c_void_p),
                ("motion_R", C.c_void_p), ("motion_t", C.c_void_p), ("inliers_h", C.c_void_p), ("inliers_f", C.c_void_p)]


class PnpParams(C.Structure):                 # orbt_pnp_params
    _fields_ = [("n", C.c_int32), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("epsilon", C.c_float)]


class PnpResult(C.Structure):                 # orbt_pnp_result
    _fields_ = [("status", C.c_int32), ("consumed", C.c_int32), ("n_inliers", C.c_int32), ("n_refits", C.c_int32), ("Tcw", C.c_double * 16)]


class PnpTrace(C.Structure):                  # orbt_pnp_trace
    _fields_ = [("R", C.c_void_p), ("t", C.c_void_p), ("approx", C.c_void_p), ("rep_error", C.c_void_p), ("count", C.c_void_p),
                ("refit_iteration", C.c_void_p), ("refit_R", C.c_void_p), ("refit_t", C.c_void_p), ("refit_count", C.c_void_p)]


class Sim3Params(C.Structure):                # orbt_sim3_params
    _fields_ = [("n", C.c_int32), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("reserved", C.c_int32)]


class Sim3Result(C.Structure):                # orbt_sim3_result
    _fields_ = [("status", C.c_int32), ("consumed", C.c_int32), ("n_inliers", C.c_int32), ("scale", C.c_float), ("T12", C.c_double * 16),
                ("R", C.c_double * 9), ("t", C.c_double * 3)]


class Sim3Trace(C.Structure):                 # orbt_sim3_trace
    _fields_ = [("R", C.c_void_p), ("t", C.c_void_p), ("scale", C.c_void_p), ("count", C.c_void_p), ("relgap", C.c_void_p)]


class DbQueryInfo(C.Structure):              # orbv_db_query_info
    _fields_ = [("max_common", C.c_int32), ("n_sharing", C.c_int32), ("n_scored", C.c_int32), ("n_kept", C.c_int32), ("n_cand", C.c_int32),
                ("status", C.c_int32), ("best_acc", C.c_float), ("min_common", C.c_int32)]


class DbTrace(C.Structure):                  # orbv_db_trace
    _fields_ = [("info", C.POINTER(DbQueryInfo)), ("kept_slot", C.c_void_p), ("kept_score", C.c_void_p), ("kept_acc", C.c_void_p),
                ("kept_best", C.c_void_p), ("kept_cap", C.c_int32), ("reserved", C.c_int32)]


class BaOptions(C.Structure):                 # ba_options
    _fields_ = [("max_iterations", C.c_int32), ("huber_delta", C.c_double), ("fix_points", C.c_int32),
                ("stop_flag", C.c_void_p)]


class BaSummary(C.Structure):                 # ba_summary
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("iterations", C.c_int32),
                ("successful_steps", C.c_int32), ("termination", C.c_int32), ("final_radius", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# ---- the signatures: include/orbslam_hip.h is their only statement -----------------------------------------------------------------
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "orbslam_hip.h")
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "long long": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}


def _struct_ptr(cls):
    """void* that also takes a `cls` object itself, by reference: the header gives the host out-parameter of a call and the device array
    of its batched form the same type, so the one ctypes type has to take a structure, byref() of one and a plain address"""
    def from_param(c, v):
        return C.byref(v) if isinstance(v, cls) else C.c_void_p.from_param(v)
    return type("LP_" + cls.__name__, (C.c_void_p,), {"from_param": classmethod(from_param)})


# the structs that call sites hand over as the object itself; a pointer to any other type is a plain void*
_STRUCTS = {name: _struct_ptr(cls) for name, cls in (
    ("ba_options", BaOptions), ("ba_summary", BaSummary), ("orbt_init_report", InitReport), ("orbt_init_trace", InitTrace), ("orbt_pnp_params", PnpParams),
    ("orbt_pnp_result", PnpResult), ("orbt_pnp_trace", PnpTrace), ("orbt_sim3_params", Sim3Params), ("orbt_sim3_result", Sim3Result),
    ("orbt_sim3_trace", Sim3Trace), ("orbv_db_query_info", DbQueryInfo), ("orbv_db_trace", DbTrace))}


def _declarations(text):
    """[(return type, name, [parameter, ...])] of every function a header declares at file scope"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s*"C"\s*\{', " ", text)
    text = re.sub(r"\{[^{}]*\}", " ", text)                     # (struct bodies)
    out = []
    for stmt in text.split(";"):
        if "(" not in stmt:
            continue
        m = re.fullmatch(r"[\s}]*(.*?)\b(\w+)\s*\(([^()]*)\)\s*", stmt, flags=re.S)
        if not m:
            raise OrbHipError("cannot parse the declaration %r" % " ".join(stmt.split()))
        params = [" ".join(a.split()) for a in m.group(3).split(",")]
        out.append((" ".join(m.group(1).split()), m.group(2), [] if params in ([""], ["void"]) else params))
    return out


def _ctype(decl, where, named=True):
    """the ctypes type of one parameter (named) or return type; `where` names the declaration in the error"""
    t, arrays = re.subn(r"\[[^\]]*\]", " ", decl)
    words = re.sub(r"\b(?:const|volatile|struct)\b|\*", " ", t).split()
    if named and len(words) > 1 and " ".join(words) not in _SCALARS:
        words = words[:-1]                                      # (the parameter's name)
    base, depth = " ".join(words), t.count("*") + arrays
    if depth == 0:
        if base == "void" and not named:
            return None
        if base not in _SCALARS:
            raise OrbHipError("%s: no ctypes type for %r" % (where, decl))
        return _SCALARS[base]
    if depth == 1 and base == "char" and "const" in decl:
        return C.c_char_p
    if depth == 1 and base in _STRUCTS:
        return _STRUCTS[base]
    return C.c_void_p


def parse_header(text):
    """{name: (restype, [argtype, ...])} of every function the header text declares, in its order"""
    return {name: (_ctype(ret, name, named=False), [_ctype(a, name) for a in params]) for ret, name, params in _declarations(text)}


with open(HEADER_PATH) as _f:
    _DECLS = _declarations(_f.read())
SYMBOLS = [name for _, name, _ in _DECLS]       # every symbol include/orbslam_hip.h declares (tests check that the library exports them all)

_lib = None


def load():
    """Load liborbslam_hip.so (built by __graft_entry__.build()) and give every function the header declares its argtypes and restype;
    raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OrbHipError("HIP library %s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)" % LIB_PATH)
    # PyTorch (device memory / streams / torch.distributed plumbing) bundles its own libamdhip64.so.7;
    # load it FIRST so this library binds to the same HIP runtime instead of a second copy from
    # /opt/rocm (two runtimes in one process cannot both own the GPU).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    for ret, name, params in _DECLS:
        f = getattr(L, name)
        f.restype, f.argtypes = _ctype(ret, name, named=False), [_ctype(a, name) for a in params]
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        msg = load().orbhip_last_error().decode("utf-8", "replace")
        raise OrbHipError("%s failed (code %d): %s" % (what or "HIP call", rc, msg))


# ---- what every wrapper needs around a call ------------------------------------------------------------------------------------------
def ptr(a, empty_null=False):
    """host numpy array or torch tensor -> void*; None -> NULL, and with empty_null an array without elements too"""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr()) if a.numel() or not empty_null else None
    return a.ctypes.data_as(C.c_void_p) if a.size or not empty_null else None


def ptr_nonempty(a):
    return ptr(a, empty_null=True)


def stream():
    """the current torch stream as a hipStream_t"""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(name, *counts, device, min_bytes=0, reuse=None):
    """The uint8 device tensor the `_device` entry of a family works in: `name`(*counts, &nbytes) states its size.  reuse: the caller's
    own tensor, taken instead of a new one when it is large enough."""
    import torch
    nbytes = C.c_size_t(0)
    check(getattr(load(), name)(*counts, C.byref(nbytes)), name)
    if reuse is None:
        return torch.empty(max(nbytes.value, min_bytes), dtype=torch.uint8, device=device)
    assert reuse.numel() >= nbytes.value
    return reuse


def carray(a, dtype):
    return np.ascontiguousarray(a, dtype)


def flat(a, dtype):
    """carray as one dimension; None stays None"""
    return None if a is None else np.ascontiguousarray(a, dtype).reshape(-1)
