"""mp reference of the small dense helpers (csrc/small_dense.h, null_vector4_dev of csrc/tri_math.h): singular triples by mpmath's
svd_r, the symmetric 4 x 4 by eigsy, the 3 x 3 inverse and determinant, the minimum-norm least-squares solution with d_lstsq's own
rank rule, the DLT triangulation of one match - and the metrics of tests/densecases.py, evaluated in mp on float64 outputs.  None of
the metrics depends on a vector the mathematics leaves free.  Nothing here imports the product package."""
import numpy as np
from mpmath import mp, mpf

DPS = 60


def M(a):
    """a float64 array (1-d: a column) -> mp.matrix, exactly"""
    a = np.asarray(a, np.float64)
    if a.ndim == 1:
        a = a[:, None]
    return mp.matrix([[mpf(float(v)) for v in row] for row in a])


def F(m):
    """mp.matrix -> float64 array"""
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def maxabs(m):
    return max([abs(v) for v in m] + [mpf(0)])


def svd(A):
    """A (m x n float64) -> (U m x k, S list descending, V n x k) in mp, k = min(m, n): A = U diag(S) V^T"""
    with mp.workdps(DPS):
        Am = M(A)
        if Am.rows >= Am.cols:
            U, S, Vt = mp.svd_r(Am)
            return U, [S[i] for i in range(len(S))], Vt.T
        U, S, Vt = mp.svd_r(Am.T)
        return Vt.T, [S[i] for i in range(len(S))], U


def right_vectors(A):
    """all n right singular vectors of A (m x n) with their values, descending, from the symmetric problem A^T A at twice the digits (for
    m < n the SVD has only m triples); returns (sigma list of n, V n x n)"""
    with mp.workdps(2 * DPS):
        Am = M(A)
        E, Q = mp.eigsy(Am.T * Am)
        n = Am.cols
        order = sorted(range(n), key=lambda i: -E[i])
        sig = [mp.sqrt(E[i]) if E[i] > 0 else mpf(0) for i in order]
        V = mp.matrix(n, n)
        for c, i in enumerate(order):
            for r in range(n):
                V[r, c] = Q[r, i]
        return sig, V


def eigsy4(N):
    """symmetric 4 x 4 -> (eigenvalues ascending, V columns) in mp"""
    with mp.workdps(DPS):
        E, Q = mp.eigsy(M(N))
        return [E[i] for i in range(4)], Q


def det3(A):
    with mp.workdps(DPS):
        return mp.det(M(A))


def inv3(A):
    with mp.workdps(DPS):
        return M(A) ** -1


def lstsq(A, b):
    """the minimum-norm solution of min |A x - b| over the singular values with sigma_j^2 > 1e-24 sigma_max^2 (d_lstsq's rule)"""
    with mp.workdps(DPS):
        U, S, V = svd(A)
        bm = M(b)
        x = mp.matrix(V.rows, 1)
        for j, s in enumerate(S):
            if not s * s > mpf("1e-24") * S[0] * S[0]:
                continue
            w = sum(U[i, j] * bm[i] for i in range(U.rows)) / s
            for k in range(V.rows):
                x[k] += V[k, j] * w
        return x, S


def dlt_matrix(T1, T2, xn1, xn2):
    """the 4 x 4 system of one match (tri_math.h:73-80) in mp; T = 3 x 4 row-major (12), xn = normalised (x, y)"""
    with mp.workdps(DPS):
        T1 = [mpf(float(v)) for v in np.asarray(T1).reshape(12)]; T2 = [mpf(float(v)) for v in np.asarray(T2).reshape(12)]
        x1 = [mpf(float(v)) for v in xn1]; x2 = [mpf(float(v)) for v in xn2]
        A = mp.matrix(4, 4)
        for j in range(4):
            A[0, j] = x1[0] * T1[8 + j] - T1[j]; A[1, j] = x1[1] * T1[8 + j] - T1[4 + j]
            A[2, j] = x2[0] * T2[8 + j] - T2[j]; A[3, j] = x2[1] * T2[8 + j] - T2[4 + j]
        return A


def dlt_point(T1, T2, xn1, xn2):
    """the triangulated point: the null vector of the DLT system, dehomogenised; also (sigma list) of the system"""
    with mp.workdps(DPS):
        A = dlt_matrix(T1, T2, xn1, xn2)
        U, S, Vt = mp.svd_r(A)
        x = [Vt[3, k] for k in range(4)]
        return [x[0] / x[3], x[1] / x[3], x[2] / x[3]], [S[i] for i in range(4)]


# ---------------------------------------------------------------- metrics (all return floats; inf for a non-finite output)
def _finite(*arrs):
    return all(np.all(np.isfinite(np.asarray(a, np.float64))) for a in arrs)


INF = float("inf")


def vec_dist(x, truth):
    """min(|x - x*|, |x + x*|) of unit vectors: the distance itself (sqrt(1 - cos^2) has a 1.5e-8 floor)"""
    if not _finite(x):
        return INF
    with mp.workdps(DPS):
        xm = M(x)
        a = mp.sqrt(sum((xm[i] - truth[i]) ** 2 for i in range(xm.rows)))
        b = mp.sqrt(sum((xm[i] + truth[i]) ** 2 for i in range(xm.rows)))
        return float(min(a, b))


def orth_err(V):
    """max |V^T V - I|"""
    if not _finite(V):
        return INF
    with mp.workdps(DPS):
        Vm = M(V)
        return float(maxabs(Vm.T * Vm - mp.eye(Vm.cols)))


def col_cosines(U, floor_norm):
    """largest |cos| between two columns of U whose norms are both above floor_norm (a null column has no direction)"""
    if not _finite(U):
        return INF
    with mp.workdps(DPS):
        Um = M(U)
        G = Um.T * Um
        worst = mpf(0)
        for p in range(Um.cols):
            for q in range(p + 1, Um.cols):
                if G[p, p] > floor_norm ** 2 and G[q, q] > floor_norm ** 2:
                    worst = max(worst, abs(G[p, q]) / mp.sqrt(G[p, p] * G[q, q]))
        return float(worst)


def svd3_metrics(A, U, S, V, truth_S):
    """values, reconstruction, the sign convention A v2 = S2 u2, orthogonality of U and of V; all relative to sigma0 (1 for A = 0)"""
    if not _finite(U, S, V):
        return dict(values=INF, recon=INF, sign=INF, orthU=INF, orthV=INF)
    with mp.workdps(DPS):
        Am, Um, Vm = M(A), M(U), M(V)
        s0 = truth_S[0] if truth_S[0] > 0 else mpf(1)
        Sm = [mpf(float(v)) for v in S]
        val = max(abs(Sm[i] - truth_S[i]) for i in range(3)) / s0
        rec = maxabs(Um * mp.diag(Sm) * Vm.T - Am) / s0
        r = Am * Vm[:, 2] - Sm[2] * Um[:, 2]
        sign = mp.sqrt(sum(v * v for v in r)) / s0
        return dict(values=float(val), recon=float(rec), sign=float(sign), orthU=orth_err(U), orthV=orth_err(V))


def jacobi_metrics(A, U, V, truth_sig):
    """the one-sided Jacobi's outputs: |A V - U| / sigma0, V^T V - I, the column norms of U against the singular values (sorted),
    the cosines between the columns of U that are not null (norm above 1e-13 sigma0)"""
    if not _finite(U, V):
        return dict(values=INF, av=INF, orthV=INF, cosU=INF)
    with mp.workdps(DPS):
        Am, Um, Vm = M(A), M(U), M(V)
        s0 = truth_sig[0] if truth_sig[0] > 0 else mpf(1)
        av = maxabs(Am * Vm - Um) / s0
        nrm = sorted([mp.sqrt(sum(Um[i, j] ** 2 for i in range(Um.rows))) for j in range(Um.cols)], reverse=True)
        ts = list(truth_sig) + [mpf(0)] * (len(nrm) - len(truth_sig))
        val = max(abs(a - b) for a, b in zip(nrm, ts)) / s0
        return dict(values=float(val), av=float(av), orthV=orth_err(V), cosU=col_cosines(U, mpf("1e-13") * s0))


def residual_excess(A, x, truth_sig_min, s0):
    """|A x| / sigma0 - sigma_min / sigma0 for a unit x: how far x is from attaining the minimum (>= 0 up to rounding)"""
    if not _finite(x):
        return INF
    with mp.workdps(DPS):
        r = M(A) * M(x)
        xn = mp.sqrt(sum(v * v for v in M(x)))
        return float(max(mpf(0), mp.sqrt(sum(v * v for v in r)) / xn / s0 - truth_sig_min / s0))


def projector_err(Vs, Vt):
    """max |P - P*|, P the orthogonal projector onto the span of the columns (both orthonormal to rounding)"""
    if not _finite(Vs):
        return INF
    with mp.workdps(DPS):
        A = M(Vs)
        return float(maxabs(A * A.T - Vt * Vt.T))


def sym4_metrics(N, lam, V, truth_lam):
    """eigenvalues with sign (sorted, relative to |lambda|max), |N V - V L| / |lambda|max, V^T V - I"""
    if not _finite(lam, V):
        return dict(values=INF, nv=INF, orthV=INF)
    with mp.workdps(DPS):
        Nm, Vm = M(N), M(V)
        L = [mpf(float(v)) for v in lam]
        lm = max(abs(v) for v in truth_lam)
        lm = lm if lm > 0 else mpf(1)
        val = max(abs(a - b) for a, b in zip(sorted(L), sorted(truth_lam))) / lm
        nv = maxabs(Nm * Vm - Vm * mp.diag(L)) / lm
        return dict(values=float(val), nv=float(nv), orthV=orth_err(V))


def rel_err(x, truth):
    """|x - x*| / |x*| (2-norms; max-abs of x - x* when x* = 0)"""
    if not _finite(x):
        return INF
    with mp.workdps(DPS):
        xm = M(np.asarray(x, np.float64).reshape(-1))
        t = [truth[i] for i in range(len(truth))]
        d = mp.sqrt(sum((xm[i] - t[i]) ** 2 for i in range(len(t))))
        n = mp.sqrt(sum(v * v for v in t))
        return float(d / n if n > 0 else d)
