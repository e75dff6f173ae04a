"""Sim3Solver (reference src/Sim3Solver.cc: Horn's closed-form Sim(3) inside RANSAC, the loop-closing pose) on the GPU
(include/orbslam_hip.h: orbt_sim3_*).  Thin ctypes layer: arrays in, arrays out."""
import ctypes as C

import numpy as np

from . import _lib

# result->status (ORBT_SIM3_*)
FOUND, NOT_FOUND, TOO_FEW, BAD_INPUT = 0, 1, 2, 3
STATUS = {FOUND: "found", NOT_FOUND: "not found (every given set used)", TOO_FEW: "too few correspondences", BAD_INPUT: "bad input"}
TRACE_KEYS = ("R", "t", "scale", "count", "relgap")


def ransac_params(n, probability=0.99, min_inliers=6, max_iterations=300):
    """SetRansacParameters' arithmetic (src/Sim3Solver.cc:120-145; the defaults are the header's, LoopClosing passes (0.99, 20, 300)).
    Returns dict n, min_inliers, max_iterations (the adjusted value)."""
    out = _lib.Sim3Params()
    _lib.check(_lib.load().orbt_sim3_ransac_params(int(n), float(probability), int(min_inliers), int(max_iterations), C.byref(out)),
               "orbt_sim3_ransac_params")
    return dict(n=out.n, min_inliers=out.min_inliers, max_iterations=out.max_iterations)


def max_errors(sigma2):
    """max_errors_1_ / _2_ (src/Sim3Solver.cc:93-94): the double product 9.210 * float sigma2 stored in a std::vector<size_t>, that is
    TRUNCATED to an integer; returned as float32 (the comparison of :379 converts it to float)."""
    return np.floor(9.210 * np.asarray(sigma2, np.float32).astype(np.float64)).astype(np.float32)


def draw_sets(n, iterations, randint=None):
    """The minimal sets of src/Sim3Solver.cc:169-182: per iteration 3 draws by swap-remove from the full index list
    (randint(0, len - 1) picks a slot, the slot takes the back entry, the back is popped).  randint(lo, hi) is inclusive on both
    ends, as DUtils::Random::RandomInt; the default is numpy's generator (seed 0)."""
    if randint is None:
        rng = np.random.default_rng(0)

        def randint(lo, hi):
            return int(rng.integers(lo, hi + 1))
    sets = np.zeros((iterations, 3), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(3):
            r = randint(0, len(avail) - 1)
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


class Sim3State:
    """n_best_inliers_ / is_best_inliers_ / best_rotation_ / best_translation_ / best_scale_ of one solver: what an `iterate` call
    reads and leaves behind."""

    def __init__(self, n):
        self.best_count = 0
        self.best_mask = np.zeros(int(n), np.uint8)
        self.best_R = np.eye(3)
        self.best_t = np.zeros(3)
        self.best_scale = np.float32(1.0)

    def copy(self):
        s = Sim3State(len(self.best_mask))
        s.best_count, s.best_mask, s.best_R, s.best_t, s.best_scale = self.best_count, self.best_mask.copy(), self.best_R.copy(), self.best_t.copy(), self.best_scale
        return s


def _result_dict(res):
    return dict(status=res.status, consumed=res.consumed, n_inliers=res.n_inliers, scale=np.float32(res.scale),
                T12=np.array(res.T12[:], np.float64).reshape(4, 4), R=np.array(res.R[:], np.float64).reshape(3, 3), t=np.array(res.t[:], np.float64))


def iterate(X1c, X2c, max_err1, max_err2, K1, K2, fix_scale, min_inliers, sets, state=None, trace=False):
    """orbt_sim3_iterate: one Sim3Solver::iterate call of one candidate.  X1c[n, 3], X2c[n, 3] float64 (camera frames), max_err1 / 2[n]
    = max_errors(sigma2) float32; K1, K2 = (fx, fy, cx, cy); sets[n_sets, 3] = every set the call may consume (n_sets =
    min(max_iterations - iterations so far, n_iterations)); state: a Sim3State, updated in place (None = a fresh one).
    Returns dict status, consumed, n_inliers, T12 (4, 4), R, t, scale (the state's best), inliers[n] bool, state and, with
    trace=True, R [n_sets, 3, 3], t [n_sets, 3], scale, count, relgap [n_sets] under the keys trace_R, trace_t, trace_scale, trace_count,
    trace_relgap."""
    L = _lib.load()
    X1 = np.ascontiguousarray(X1c, np.float64).reshape(-1, 3)
    X2 = np.ascontiguousarray(X2c, np.float64).reshape(-1, 3)
    E1 = np.ascontiguousarray(max_err1, np.float32).reshape(-1)
    E2 = np.ascontiguousarray(max_err2, np.float32).reshape(-1)
    k1 = np.ascontiguousarray(K1, np.float32).reshape(4)
    k2 = np.ascontiguousarray(K2, np.float32).reshape(4)
    n = len(X1)
    if len(X2) != n or len(E1) != n or len(E2) != n:
        raise ValueError("iterate: X1c, X2c, max_err1 and max_err2 must have the same number of rows")
    S = np.ascontiguousarray(sets, np.int32).reshape(-1, 3)
    ns = len(S)
    if state is None:
        state = Sim3State(n)
    if len(state.best_mask) != n or state.best_mask.dtype != np.uint8:
        raise ValueError("iterate: the state belongs to another correspondence count")
    bc = C.c_int32(int(state.best_count))
    bs = C.c_float(float(state.best_scale))
    bR = np.ascontiguousarray(state.best_R, np.float64).reshape(3, 3).copy()
    bt = np.ascontiguousarray(state.best_t, np.float64).reshape(3).copy()
    res = _lib.Sim3Result()
    inl = np.zeros(max(n, 1), np.uint8)
    o, tr = {}, None
    if trace:
        m = max(ns, 1)
        o.update(R=np.zeros((m, 3, 3)), t=np.zeros((m, 3)), scale=np.zeros(m), count=np.zeros(m, np.int32), relgap=np.zeros(m))
        tr = _lib.Sim3Trace(*[_lib.ptr(o[k]) for k in TRACE_KEYS])
    _lib.check(L.orbt_sim3_iterate(_lib.ptr(X1), _lib.ptr(X2), _lib.ptr(E1), _lib.ptr(E2), n, _lib.ptr(k1), _lib.ptr(k2), int(bool(fix_scale)),
                                   int(min_inliers), _lib.ptr(S), ns, C.byref(bc), _lib.ptr(state.best_mask), _lib.ptr(bR), _lib.ptr(bt), C.byref(bs),
                                   C.byref(res), _lib.ptr(inl), C.byref(tr) if tr is not None else None), "orbt_sim3_iterate")
    state.best_count = bc.value
    state.best_R, state.best_t, state.best_scale = bR, bt, np.float32(bs.value)
    o = {"trace_" + k: v[:ns] for k, v in o.items()}
    o.update(_result_dict(res))
    o["inliers"] = inl[:n].astype(bool)
    o["state"] = state
    return o


def iterate_batch_device(X1c, X2c, max_err1, max_err2, off, K1, K2, fix_scale, min_inliers, n_sets, sets, best_count, best_mask, best_R, best_t,
                         best_scale, result, inliers):
    """orbt_sim3_iterate_batch_device on torch CUDA tensors, enqueued on the current stream: X1c / X2c[n_total, 3] float64,
    max_err1 / 2[n_total] float32, off[n_candidates + 1] int32 (CSR), K1 / K2[n_candidates, 4] float32, fix_scale / min_inliers /
    n_sets[n_candidates] int32, sets[n_candidates, iterations, 3] int32, the state best_count[n_candidates] int32 / best_mask[n_total]
    uint8 / best_R[n_candidates, 3, 3] / best_t[n_candidates, 3] float64 / best_scale[n_candidates] float32 (in/out),
    result[n_candidates * sizeof(orbt_sim3_result)] uint8 and inliers[n_total] uint8 (out).  Returns the workspace tensor (keep it alive
    until the stream is synchronised)."""
    L = _lib.load()
    nc = off.numel() - 1
    iterations = sets.shape[1]
    ws = _lib.workspace("orbt_sim3_iterate_workspace", nc, X1c.shape[0], int(iterations), device=X1c.device, min_bytes=16)
    p = _lib.ptr
    _lib.check(L.orbt_sim3_iterate_batch_device(nc, p(X1c), p(X2c), p(max_err1), p(max_err2), p(off), X1c.shape[0], p(K1), p(K2), p(fix_scale),
                                                p(min_inliers), p(n_sets), int(iterations), p(sets), p(best_count), p(best_mask), p(best_R), p(best_t),
                                                p(best_scale), p(result), p(inliers), p(ws), _lib.stream()),
               "orbt_sim3_iterate_batch_device")
    return ws


def result_bytes(n_candidates):
    """Size in bytes of n_candidates orbt_sim3_result records."""
    return n_candidates * C.sizeof(_lib.Sim3Result)


def decode_results(buf):
    """bytes of orbt_sim3_result records (a host numpy uint8 array) -> list of result dicts."""
    b = np.ascontiguousarray(buf, np.uint8)
    sz = C.sizeof(_lib.Sim3Result)
    return [_result_dict(_lib.Sim3Result.from_buffer_copy(b[i * sz:(i + 1) * sz].tobytes())) for i in range(len(b) // sz)]


def upload_batch(cands, iterations=None):
    """The device tensors of iterate_batch_device for a list of candidate dicts (see iterate_batch), as a dict, plus `off` on the host."""
    import torch
    dev = torch.device("cuda")
    ns = [len(np.asarray(c["sets"]).reshape(-1, 3)) for c in cands]
    I = int(iterations) if iterations is not None else max(max(ns), 1)
    n = [len(np.asarray(c["X1c"]).reshape(-1, 3)) for c in cands]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    for c, k in zip(cands, n):
        c.setdefault("state", Sim3State(k))
    sets = np.zeros((len(cands), I, 3), np.int32)
    for i, c in enumerate(cands):
        sets[i, :ns[i]] = np.asarray(c["sets"], np.int32).reshape(-1, 3)

    def cat(key, dt, w):
        return np.concatenate([np.asarray(c[key], dt).reshape(-1, w) for c in cands])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    d = dict(X1c=up((cat("X1c", np.float64, 3))), X2c=up((cat("X2c", np.float64, 3))), max_err1=up((cat("max_err1", np.float32, 1).reshape(-1))),
             max_err2=up((cat("max_err2", np.float32, 1).reshape(-1))), off=up(off),
             K1=up(np.stack([np.asarray(c["K1"], np.float32).reshape(4) for c in cands])),
             K2=up(np.stack([np.asarray(c["K2"], np.float32).reshape(4) for c in cands])),
             fix_scale=up(np.array([int(bool(c["fix_scale"])) for c in cands], np.int32)),
             min_inliers=up(np.array([c["min_inliers"] for c in cands], np.int32)), n_sets=up(np.array(ns, np.int32)), sets=up(sets),
             best_count=up(np.array([c["state"].best_count for c in cands], np.int32)),
             best_mask=up((np.concatenate([c["state"].best_mask for c in cands]))),
             best_R=up(np.stack([np.asarray(c["state"].best_R, np.float64).reshape(3, 3) for c in cands])),
             best_t=up(np.stack([np.asarray(c["state"].best_t, np.float64).reshape(3) for c in cands])),
             best_scale=up(np.array([c["state"].best_scale for c in cands], np.float32)),
             result=torch.zeros(result_bytes(len(cands)), dtype=torch.uint8, device=dev),
             inliers=torch.zeros(max(int(off[-1]), 1), dtype=torch.uint8, device=dev))
    return d, off


def iterate_batch(cands, iterations=None):
    """One `iterate` of several candidates in one device call.  cands: list of dicts X1c, X2c, max_err1, max_err2, K1, K2, fix_scale,
    min_inliers, sets and optionally state (a Sim3State, updated in place).  Returns the list of result dicts `iterate` returns
    (without a trace)."""
    import torch
    d, off = upload_batch(cands, iterations)
    ws = iterate_batch_device(**d)
    torch.cuda.synchronize()
    del ws
    res = decode_results(d["result"].cpu().numpy())
    inl, bm, bc = d["inliers"].cpu().numpy(), d["best_mask"].cpu().numpy(), d["best_count"].cpu().numpy()
    bR, bt, bs = d["best_R"].cpu().numpy(), d["best_t"].cpu().numpy(), d["best_scale"].cpu().numpy()
    for i, (c, r) in enumerate(zip(cands, res)):
        a, b = int(off[i]), int(off[i + 1])
        r["inliers"] = inl[a:b].astype(bool)
        st = c["state"]
        if r["status"] != BAD_INPUT:
            st.best_count, st.best_mask, st.best_R, st.best_t, st.best_scale = int(bc[i]), bm[a:b].copy(), bR[i].copy(), bt[i].copy(), np.float32(bs[i])
        r["state"] = st
    return res
