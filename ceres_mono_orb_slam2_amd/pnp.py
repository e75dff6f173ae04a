"""PnPsolver (reference src/PnPsolver.cc: EPnP inside RANSAC, the relocalisation pose) on the GPU (include/orbslam_hip.h:
orbt_pnp_*).  Thin ctypes layer: arrays in, arrays out."""
import ctypes as C

import numpy as np

from . import _lib

# result->status (ORBT_PNP_*)
REFINED, EXHAUSTED_BEST, EXHAUSTED_NONE, TOO_FEW, BAD_INPUT = 0, 1, 2, 3, 4
STATUS = {REFINED: "refined", EXHAUSTED_BEST: "exhausted, best returned", EXHAUSTED_NONE: "exhausted, none", TOO_FEW: "too few points",
          BAD_INPUT: "bad input"}
TRACE_KEYS = ("R", "t", "approx", "rep_error", "count", "refit_iteration", "refit_R", "refit_t", "refit_count")


def ransac_params(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """SetRansacParameters' arithmetic (src/PnPsolver.cc:122-153; the defaults are the header's, Tracking passes
    (0.99, 10, 300, 4, 0.5)).  Returns dict n, min_inliers, max_iterations, epsilon (the adjusted values)."""
    out = _lib.PnpParams()
    _lib.check(_lib.load().orbt_pnp_ransac_params(int(n), float(probability), int(min_inliers), int(max_iterations), int(min_set), float(epsilon),
                                                  C.byref(out)), "orbt_pnp_ransac_params")
    return dict(n=out.n, min_inliers=out.min_inliers, max_iterations=out.max_iterations, epsilon=np.float32(out.epsilon))


def max_errors(sigma2, th2=5.991):
    """mvMaxError (src/PnPsolver.cc:155-157): float sigma2 * float th2."""
    return (np.asarray(sigma2, np.float32) * np.float32(th2)).astype(np.float32)


def draw_sets(n, iterations, randint=None):
    """The minimal sets of src/PnPsolver.cc:189-202: per iteration 4 draws by swap-remove from the full index list
    (randint(0, len - 1) picks a slot, the slot takes the back entry, the back is popped).  randint(lo, hi) is inclusive on both
    ends, as DUtils::Random::RandomInt; the default is numpy's generator (seed 0)."""
    if randint is None:
        rng = np.random.default_rng(0)

        def randint(lo, hi):
            return int(rng.integers(lo, hi + 1))
    sets = np.zeros((iterations, 4), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(4):
            r = randint(0, len(avail) - 1)
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


class PnPState:
    """mnBestInliers / mvbBestInliers / mBestTcw of one solver: what an `iterate` call reads and leaves behind."""

    def __init__(self, n):
        self.best_count = 0
        self.best_mask = np.zeros(int(n), np.uint8)
        self.best_Tcw = np.eye(4)

    def copy(self):
        s = PnPState(len(self.best_mask))
        s.best_count, s.best_mask, s.best_Tcw = self.best_count, self.best_mask.copy(), self.best_Tcw.copy()
        return s


def _result_dict(res):
    return dict(status=res.status, consumed=res.consumed, n_inliers=res.n_inliers, n_refits=res.n_refits,
                Tcw=np.array(res.Tcw[:], np.float64).reshape(4, 4))


def iterate(p3d, p2d, max_err, K4, min_inliers, sets, state=None, trace=False):
    """orbt_pnp_iterate: one PnPsolver::iterate call of one candidate.  p3d[n, 3], p2d[n, 2], max_err[n] float32; K4 = (fx, fy, cx,
    cy); min_inliers = ransac_params(...)["min_inliers"]; sets[n_sets, 4] = every set the call may consume (n_sets =
    max(max_iterations - iterations so far, nIterations)); state: a PnPState, updated in place (None = a fresh one).
    Returns dict status, consumed, n_inliers, n_refits, Tcw (4, 4), inliers[n] bool, state and, with trace=True, R [n_sets, 3, 3],
    t [n_sets, 3], approx, rep_error, count [n_sets], refit_iteration, refit_R, refit_t, refit_count [n_sets]."""
    L = _lib.load()
    P3 = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
    P2 = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
    E = np.ascontiguousarray(max_err, np.float32).reshape(-1)
    K = np.ascontiguousarray(K4, np.float32).reshape(4)
    n = len(P3)
    if len(P2) != n or len(E) != n:
        raise ValueError("iterate: p3d, p2d and max_err must have the same number of rows")
    S = np.ascontiguousarray(sets, np.int32).reshape(-1, 4)
    ns = len(S)
    if state is None:
        state = PnPState(n)
    if len(state.best_mask) != n or state.best_mask.dtype != np.uint8:
        raise ValueError("iterate: the state belongs to another point count")
    bc = C.c_int32(int(state.best_count))
    T = np.ascontiguousarray(state.best_Tcw, np.float64).reshape(4, 4).copy()
    res = _lib.PnpResult()
    inl = np.zeros(max(n, 1), np.uint8)
    o, tr = {}, None
    if trace:
        m = max(ns, 1)
        o.update(R=np.zeros((m, 3, 3)), t=np.zeros((m, 3)), approx=np.zeros(m, np.int32), rep_error=np.zeros(m), count=np.zeros(m, np.int32),
                 refit_iteration=np.zeros(m, np.int32), refit_R=np.zeros((m, 3, 3)), refit_t=np.zeros((m, 3)), refit_count=np.zeros(m, np.int32))
        tr = _lib.PnpTrace(*[_lib.ptr(o[k]) for k in TRACE_KEYS])
    _lib.check(L.orbt_pnp_iterate(_lib.ptr(P3), _lib.ptr(P2), _lib.ptr(E), n, _lib.ptr(K), int(min_inliers), _lib.ptr(S), ns, C.byref(bc),
                                  _lib.ptr(state.best_mask), _lib.ptr(T), C.byref(res), _lib.ptr(inl), C.byref(tr) if tr is not None else None),
               "orbt_pnp_iterate")
    state.best_count = bc.value
    state.best_Tcw = T
    o = {k: v[:ns] for k, v in o.items()}
    o.update(_result_dict(res))
    o["inliers"] = inl[:n].astype(bool)
    o["state"] = state
    return o


def iterate_batch_device(p3d, p2d, max_err, off, K4, min_inliers, n_sets, sets, best_count, best_mask, best_Tcw, result, inliers):
    """orbt_pnp_iterate_batch_device on torch CUDA tensors, enqueued on the current stream: p3d[n_total, 3], p2d[n_total, 2],
    max_err[n_total] float32, off[n_candidates + 1] int32 (CSR), K4[n_candidates, 4] float32, min_inliers / n_sets[n_candidates]
    int32, sets[n_candidates, iterations, 4] int32, the state best_count[n_candidates] int32 / best_mask[n_total] uint8 /
    best_Tcw[n_candidates, 4, 4] float64 (in/out), result[n_candidates * sizeof(orbt_pnp_result)] uint8 and inliers[n_total] uint8
    (out).  Returns the workspace tensor (keep it alive until the stream is synchronised)."""
    L = _lib.load()
    nc = off.numel() - 1
    iterations = sets.shape[1]
    ws = _lib.workspace("orbt_pnp_iterate_workspace", nc, p3d.shape[0], int(iterations), device=p3d.device, min_bytes=16)
    p = _lib.ptr
    _lib.check(L.orbt_pnp_iterate_batch_device(nc, p(p3d), p(p2d), p(max_err), p(off), p3d.shape[0], p(K4), p(min_inliers), p(n_sets), int(iterations),
                                               p(sets), p(best_count), p(best_mask), p(best_Tcw), p(result), p(inliers), p(ws),
                                               _lib.stream()), "orbt_pnp_iterate_batch_device")
    return ws


def result_bytes(n_candidates):
    """Size in bytes of n_candidates orbt_pnp_result records."""
    return n_candidates * C.sizeof(_lib.PnpResult)


def decode_results(buf):
    """bytes of orbt_pnp_result records (a host numpy uint8 array) -> list of result dicts."""
    b = np.ascontiguousarray(buf, np.uint8)
    sz = C.sizeof(_lib.PnpResult)
    return [_result_dict(_lib.PnpResult.from_buffer_copy(b[i * sz:(i + 1) * sz].tobytes())) for i in range(len(b) // sz)]


def iterate_batch(cands, iterations=None):
    """One `iterate` of several candidates in one device call.  cands: list of dicts p3d, p2d, max_err, K4, min_inliers, sets and
    optionally state (a PnPState, updated in place).  Returns the list of result dicts `iterate` returns (without a trace)."""
    import torch
    dev = torch.device("cuda")
    ns = [len(np.asarray(c["sets"]).reshape(-1, 4)) for c in cands]
    I = int(iterations) if iterations is not None else max(max(ns), 1)
    n = [len(np.asarray(c["p3d"]).reshape(-1, 3)) for c in cands]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    for c, k in zip(cands, n):
        c.setdefault("state", PnPState(k))
    sets = np.zeros((len(cands), I, 4), np.int32)
    for i, c in enumerate(cands):
        sets[i, :ns[i]] = np.asarray(c["sets"], np.int32).reshape(-1, 4)

    def cat(key, dt, w):
        return np.concatenate([np.asarray(c[key], dt).reshape(-1, w) for c in cands]) if cands else np.zeros((0, w), dt)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    d_p3, d_p2, d_e = up(cat("p3d", np.float32, 3)), up(cat("p2d", np.float32, 2)), up(cat("max_err", np.float32, 1).reshape(-1))
    d_bm = up(np.concatenate([c["state"].best_mask for c in cands]))
    d_bc = up(np.array([c["state"].best_count for c in cands], np.int32))
    d_bt = up(np.stack([np.asarray(c["state"].best_Tcw, np.float64).reshape(4, 4) for c in cands]))
    d_res = torch.zeros(result_bytes(len(cands)), dtype=torch.uint8, device=dev)
    d_inl = torch.zeros(max(int(off[-1]), 1), dtype=torch.uint8, device=dev)
    ws = iterate_batch_device(d_p3, d_p2, d_e, up(off), up(np.stack([np.asarray(c["K4"], np.float32).reshape(4) for c in cands])),
                              up(np.array([c["min_inliers"] for c in cands], np.int32)), up(np.array(ns, np.int32)), up(sets), d_bc, d_bm, d_bt,
                              d_res, d_inl)
    torch.cuda.synchronize()
    del ws
    res = decode_results(d_res.cpu().numpy())
    inl, bm, bc, bt = d_inl.cpu().numpy(), d_bm.cpu().numpy(), d_bc.cpu().numpy(), d_bt.cpu().numpy()
    for i, (c, r) in enumerate(zip(cands, res)):
        a, b = int(off[i]), int(off[i + 1])
        r["inliers"] = inl[a:b].astype(bool)
        st = c["state"]
        if r["status"] != BAD_INPUT:
            st.best_count, st.best_mask, st.best_Tcw = int(bc[i]), bm[a:b].copy(), bt[i].copy()
        r["state"] = st
    return res
