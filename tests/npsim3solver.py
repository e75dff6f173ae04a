"""Sim3Solver (reference src/Sim3Solver.cc) restated in numpy in the operation order of csrc/orb_sim3solver.inc: every sum in the
device's order, every float narrowing of the reference where the reference has it.  The device must equal this file: counts, masks,
statuses and `consumed` exactly, poses to rounding.  lapack=True takes the eigenvector of Horn's N from numpy.linalg.eig, the stand-in
for Eigen::EigenSolver; everything else is unchanged."""
import math

import numpy as np

FOUND, NOT_FOUND, TOO_FEW, BAD_INPUT = 0, 1, 2, 3
F = np.float32


def max_errors(sigma2):
    """(:93-94) 9.210 * float sigma2 in double, truncated by the std::vector<size_t> it is stored in."""
    return np.floor(9.210 * np.asarray(sigma2, np.float32).astype(np.float64)).astype(np.float32)


def ransac_params(n, probability, min_inliers, max_iterations):
    """(:131-142) with Python's own arithmetic; 1 where the reference's quotient is not a number."""
    if min_inliers == n or n == 0:
        its = 1
    else:
        eps = float(F(min_inliers) / F(n))
        try:
            its = math.ceil(math.log(1 - probability) / math.log(1 - eps ** 3))
        except (ValueError, ZeroDivisionError):
            its = 1
    return max(1, min(its, max_iterations))


def jacobi_sym4(A):
    """i_jacobi_sym4 (csrc/small_dense.h), line for line: returns (diagonal, V)."""
    A = [[float(A[i][j]) for j in range(4)] for i in range(4)]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    fro = 0.0
    for i in range(4):
        for j in range(4):
            fro += A[i][j] * A[i][j]
    tiny = 1e-18 * math.sqrt(fro) if math.isfinite(fro) else fro
    for sweep in range(30):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                if not (abs(apq) > tiny):
                    continue
                rotated = True
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                th2 = theta * theta
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(th2 + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                A[p][p] = A[p][p] - t * apq
                A[q][q] = A[q][q] + t * apq
                A[p][q] = 0.0
                A[q][p] = 0.0
                for r in range(4):
                    if r == p or r == q:
                        continue
                    arp, arq = A[r][p], A[r][q]
                    np_, nq_ = c * arp - s * arq, s * arp + c * arq
                    A[r][p] = np_; A[p][r] = np_; A[r][q] = nq_; A[q][r] = nq_
                for i in range(4):
                    vp, vq = V[i][p], V[i][q]
                    V[i][p] = c * vp - s * vq
                    V[i][q] = s * vp + c * vq
        if not rotated:
            break
    return [A[k][k] for k in range(4)], V


def horn_N(a, b):
    """Steps 1-3 of ComputeSim3 (:232-264): a[k], b[k] = point k of set 1 / set 2.  Returns N (4 x 4 list), O1, O2, Pr1, Pr2."""
    a = [[float(v) for v in r] for r in a]
    b = [[float(v) for v in r] for r in b]
    O1 = [((a[0][i] + a[1][i]) + a[2][i]) / 3.0 for i in range(3)]
    O2 = [((b[0][i] + b[1][i]) + b[2][i]) / 3.0 for i in range(3)]
    Pr1 = [[a[k][i] - O1[i] for i in range(3)] for k in range(3)]
    Pr2 = [[b[k][i] - O2[i] for i in range(3)] for k in range(3)]
    M = [[(Pr2[0][i] * Pr1[0][j] + Pr2[1][i] * Pr1[1][j]) + Pr2[2][i] * Pr1[2][j] for j in range(3)] for i in range(3)]
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = (M[0][0] + M[1][1]) + M[2][2]
    N[0][1] = M[1][2] - M[2][1]
    N[0][2] = M[2][0] - M[0][2]
    N[0][3] = M[0][1] - M[1][0]
    N[1][1] = (M[0][0] - M[1][1]) - M[2][2]
    N[1][2] = M[0][1] + M[1][0]
    N[1][3] = M[2][0] + M[0][2]
    N[2][2] = (-M[0][0] + M[1][1]) - M[2][2]
    N[2][3] = M[1][2] + M[2][1]
    N[3][3] = (-M[0][0] - M[1][1]) + M[2][2]
    for i in range(1, 4):
        for j in range(i):
            N[i][j] = N[j][i]
    return N, O1, O2, Pr1, Pr2


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def compute_sim3(a, b, fix_scale, lapack=False):
    """ComputeSim3 (:225-345).  Returns R (3 x 3), t (3), scale (np.float32), relgap."""
    N, O1, O2, Pr1, Pr2 = horn_N(a, b)
    if lapack:
        Nn = np.array(N)
        if not np.all(np.isfinite(Nn)):
            ev, V = [float("nan")] * 4, [[float("nan")] * 4 for _ in range(4)]
        else:
            w, v = np.linalg.eig(Nn)
            ev, V = [float(x) for x in w.real], v.real.tolist()
    else:
        ev, V = jacobi_sym4(N)
    mi, l3 = 0, ev[0]
    for k in range(1, 4):
        if ev[k] > l3:
            l3, mi = ev[k], k
    l2 = -1e300
    for k in range(4):
        if k != mi and ev[k] > l2:
            l2 = ev[k]
    relgap = _div(l3 - l2, l3)
    q = [V[i][mi] for i in range(4)]
    nq = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]) if all(math.isfinite(v) for v in q) else float("nan")
    w, x, y, z = (_div(v, nq) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = [1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)]
    s = F(1.0)
    if not fix_scale:
        P3 = [[(R[3 * i] * Pr2[k][0] + R[3 * i + 1] * Pr2[k][1]) + R[3 * i + 2] * Pr2[k][2] for i in range(3)] for k in range(3)]
        nom = den = 0.0
        for k in range(3):
            nom += (Pr1[k][0] * P3[k][0] + Pr1[k][1] * P3[k][1]) + Pr1[k][2] * P3[k][2]
        for i in range(3):
            for k in range(3):
                den += P3[k][i] * P3[k][i]
        with np.errstate(all="ignore"):
            s = F(_div(nom, den))
    sd = float(s)
    t = [O1[i] - (((sd * R[3 * i]) * O2[0] + (sd * R[3 * i + 1]) * O2[1]) + (sd * R[3 * i + 2]) * O2[2]) for i in range(3)]
    return np.array(R).reshape(3, 3), np.array(t), s, relgap


def to_image(Pc, K):
    """FromCameraToImage / Project's tail (:408-414, :429-434): invz float of a double quotient, x / y float of a double product,
    fx * x + cx in float, widened."""
    K = np.asarray(K, np.float32)
    with np.errstate(all="ignore"):
        invz = (1.0 / Pc[:, 2]).astype(F)
        x = (Pc[:, 0] * invz.astype(np.float64)).astype(F)
        y = (Pc[:, 1] * invz.astype(np.float64)).astype(F)
        return np.stack([(K[0] * x + K[2]).astype(np.float64), (K[1] * y + K[3]).astype(np.float64)], 1)


def errors(R, t, scale, X1, X2, K1, K2):
    """err1, err2 of CheckInliers (:367-377) under T12 = [s R | t] and T21 = [(1 / s) R^T | -(1 / s) R^T t]: float32[n] each."""
    X1 = np.asarray(X1, np.float64).reshape(-1, 3); X2 = np.asarray(X2, np.float64).reshape(-1, 3)
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        s = np.float64(F(scale))
        inv = np.float64(1.0) / s
        sR = s * R
        sRi = inv * R.T
        ti = np.array([-((sRi[i, 0] * t[0] + sRi[i, 1] * t[1]) + sRi[i, 2] * t[2]) for i in range(3)])
        p21 = np.stack([((sR[i, 0] * X2[:, 0] + sR[i, 1] * X2[:, 1]) + sR[i, 2] * X2[:, 2]) + t[i] for i in range(3)], 1)
        p12 = np.stack([((sRi[i, 0] * X1[:, 0] + sRi[i, 1] * X1[:, 1]) + sRi[i, 2] * X1[:, 2]) + ti[i] for i in range(3)], 1)
        im1, im2 = to_image(X1, K1), to_image(X2, K2)
        uv21, uv12 = to_image(p21, K1), to_image(p12, K2)
        d1 = im1 - uv21
        d2 = uv12 - im2
        e1 = (d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]).astype(F)
        e2 = (d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1]).astype(F)
        return e1, e2


def check_inliers(R, t, scale, X1, X2, me1, me2, K1, K2):
    """CheckInliers (:365-385): the mask (bool[n]).  me1 / me2 hold the TRUNCATED thresholds; a NaN error compares false."""
    e1, e2 = errors(R, t, scale, X1, X2, K1, K2)
    with np.errstate(all="ignore"):
        return (e1 < np.asarray(me1, F)) & (e2 < np.asarray(me2, F))


class State:
    def __init__(self, n):
        self.best_count = 0
        self.best_mask = np.zeros(int(n), np.uint8)
        self.best_R = np.eye(3)
        self.best_t = np.zeros(3)
        self.best_scale = F(1.0)


def walk(counts, best_count, min_inliers):
    """The sequential rule of iterate (:164-207) over the counts of the given sets: returns (status, consumed, best_it, best_count) -
    best_it = the last set that replaced the best (-1: none)."""
    best, best_it = int(best_count), -1
    for it, k in enumerate(counts):
        if k >= best:
            best, best_it = int(k), it
            if k > min_inliers:
                return FOUND, it + 1, best_it, best
    return NOT_FOUND, len(counts), best_it, best


def iterate(X1, X2, me1, me2, K1, K2, fix_scale, min_inliers, sets, state=None, lapack=False):
    """One Sim3Solver::iterate over the given sets, as orbt_sim3_iterate defines it.  Returns a dict like the library's, with the
    per-set hypotheses under trace_R, trace_t, trace_scale, trace_count, trace_relgap (all sets, also those after `consumed`)."""
    X1 = np.asarray(X1, np.float64).reshape(-1, 3); X2 = np.asarray(X2, np.float64).reshape(-1, 3)
    n = len(X1)
    sets = np.asarray(sets, np.int32).reshape(-1, 3)
    if state is None:
        state = State(n)
    out = dict(status=TOO_FEW, consumed=0, n_inliers=0, T12=np.eye(4), inliers=np.zeros(n, bool), state=state)
    if n >= min_inliers:
        hyp = [compute_sim3(X1[s], X2[s], fix_scale, lapack) for s in sets]
        masks = [check_inliers(h[0], h[1], h[2], X1, X2, me1, me2, K1, K2) for h in hyp]
        counts = [int(m.sum()) for m in masks]
        status, consumed, best_it, best = walk(counts, state.best_count, min_inliers)
        if best_it >= 0:
            state.best_count, state.best_mask = best, masks[best_it].astype(np.uint8)
            state.best_R, state.best_t, state.best_scale = hyp[best_it][0], hyp[best_it][1], hyp[best_it][2]
        out.update(status=status, consumed=consumed, trace_R=np.array([h[0] for h in hyp]).reshape(-1, 3, 3), trace_t=np.array([h[1] for h in hyp]).reshape(-1, 3),
                   trace_scale=np.array([float(h[2]) for h in hyp]), trace_count=np.array(counts, np.int32), trace_relgap=np.array([h[3] for h in hyp]))
        if status == FOUND:
            T = np.eye(4)
            T[:3, :3] = np.float64(state.best_scale) * state.best_R
            T[:3, 3] = state.best_t
            out.update(n_inliers=best, T12=T, inliers=state.best_mask.astype(bool))
    out.update(R=state.best_R, t=state.best_t, scale=state.best_scale)
    return out
