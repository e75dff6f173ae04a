"""numpy restatement of PnPsolver (reference src/PnPsolver.cc: RANSAC :166-261, Refine :263-310, CheckInliers :313-345, EPnP's
compute_pose :380-957), written from the reference lines with the operation order of the device code
(ceres_mono_orb_slam2_amd/csrc/orb_pnp.inc, small_dense.h):
- a sum over the points of one compute_pose call is W strided partial sums (partial j adds points j, j + W, ... in order) combined
  by the fixed tree s = W/2 ... 1: p[j] += p[j + s]; W = 1 (plain index order) for a 4-point hypothesis, W = 256 for Refine;
- the eigenvectors of MtM, the small least-squares solves and every 3 x 3 SVD are the device's one-sided Jacobi (npinit.jacobi /
  svd3), batched over hypotheses; cvSVD's Ut rows 11..8 are the columns of the four smallest |A V_j|^2 in a stable descending sort;
- definitions (not measurements): a singular value at or below 1e-12 of the largest is zero in the least-squares solves
  (sigma^2 <= 1e-24 max sigma^2) and in the 3 x 3 pseudo-inverse; qr_solve's `eta == 0` early return is a step of zero;
- every narrowing of CheckInliers is explicit.
lapack=True replaces only the three dense primitives (symmetric eigenvectors, 3 x 3 SVD, least squares) with numpy.linalg: the
stand-in for the reference wherever a result does not depend on the null-space basis ("PnP RANSAC").
Nothing here imports the product package."""
import numpy as np

import npinit

f32, f64 = np.float32, np.float64
REFINED, EXHAUSTED_BEST, EXHAUSTED_NONE, TOO_FEW, BAD_INPUT = 0, 1, 2, 3, 4
REFINE_W = 256


# ---------------------------------------------------------------- SetRansacParameters (:122-153) and the draw (:189-202)
def ransac_params(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    eps = f32(epsilon)
    n_min = int(f32(n) * eps)
    n_min = max(n_min, int(min_inliers), int(min_set))
    its = 1
    if n > 0:
        if eps < f32(n_min) / f32(n):
            eps = f32(n_min) / f32(n)
        if n_min != n:
            with np.errstate(all="ignore"):
                v = np.ceil(np.log(f64(1.0) - f64(probability)) / np.log(f64(1.0) - np.power(f64(eps), 3)))
            its = 1 if not (v >= 1.0) else int(max_iterations) if v > max_iterations else int(v)
    its = max(1, min(its, int(max_iterations)))
    return dict(n=int(n), min_inliers=n_min, max_iterations=its, epsilon=eps)


def draw_sets(n, iterations, randint):
    sets = np.zeros((iterations, 4), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(4):
            r = randint(0, len(avail) - 1)
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


# ---------------------------------------------------------------- sums and dense primitives
def tree_sum(X, W):
    """X (B, n, K) -> (B, K): W strided partial sums, then the fixed binary tree."""
    X = np.asarray(X, f64)
    B, n, K = X.shape
    P = np.zeros((B, W, K))
    for r in range(0, n, W):
        ch = X[:, r:r + W]
        P[:, :ch.shape[1]] = P[:, :ch.shape[1]] + ch
    s = W // 2
    while s >= 1:
        P[:, :s] = P[:, :s] + P[:, s:2 * s]
        s //= 2
    return P[:, 0].copy()


def col_norm2(U):
    B, M, N = U.shape
    out = np.zeros((B, N))
    for i in range(M):
        out = out + U[:, i, :] * U[:, i, :]
    return out


def eig_smallest4(A, lapack=False):
    """A (B, 12, 12) symmetric -> v (B, 4, 12): v[:, i] = cvSVD's Ut row 11 - i (i = 0: the smallest eigenvalue)."""
    if lapack:
        w, E = np.linalg.eigh(A)
        return np.stack([E[:, :, i] for i in range(4)], 1)
    U, V = npinit.jacobi(A)
    nrm2 = col_norm2(U)
    order = np.argsort(-nrm2, axis=1, kind="stable")
    r = np.arange(len(A))
    return np.stack([V[r, :, order[:, 11 - i]] for i in range(4)], 1)


def svd3(A, lapack=False):
    """(B, 3, 3) -> U, S, V with the singular vectors as columns, S descending."""
    if lapack:
        U, S, Vt = np.linalg.svd(A)
        return U, S, np.swapaxes(Vt, 1, 2)
    return npinit.svd3(A)


def lstsq(A, b, lapack=False):
    """min |A x - b| for A (B, m, n), b (B, m): the minimum-norm solution over the singular values above 1e-12 of the largest."""
    if lapack:
        return np.stack([np.linalg.lstsq(A[i], b[i], rcond=1e-12)[0] for i in range(len(A))])
    U, V = npinit.jacobi(A)
    B, m, n = U.shape
    nrm2 = col_norm2(U)
    mx = np.zeros(B)
    for j in range(n):
        mx = np.where(nrm2[:, j] > mx, nrm2[:, j], mx)
    x = np.zeros((B, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            keep = nrm2[:, j] > 1e-24 * mx
            d = np.zeros(B)
            for i in range(m):
                d = d + U[:, i, j] * b[:, i]
            w = d / nrm2[:, j]
            x = np.where(keep[:, None], x + V[:, :, j] * w[:, None], x)
    return x


def pinv3(cc, lapack=False):
    U, S, V = svd3(cc, lapack)
    with np.errstate(all="ignore"):
        sinv = np.where(S > 1e-12 * S[:, :1], 1.0 / S, 0.0)
        ci = np.empty_like(cc)
        for r in range(3):
            for c in range(3):
                ci[:, r, c] = ((V[:, r, 0] * sinv[:, 0]) * U[:, c, 0] + (V[:, r, 1] * sinv[:, 1]) * U[:, c, 1]) + (V[:, r, 2] * sinv[:, 2]) * U[:, c, 2]
    return ci


def qr_solve(A, b):
    """(:865-957) for (B, 6, 4) systems; a singular column (eta == 0) makes the step zero."""
    A = np.array(A, f64, copy=True); b = np.array(b, f64, copy=True)
    B, nr, nc = A.shape
    A1 = np.zeros((B, nc)); A2 = np.zeros((B, nc))
    dead = np.zeros(B, bool)
    with np.errstate(all="ignore"):
        for k in range(nc):
            eta = np.abs(A[:, k, k])
            for i in range(k + 1, nr):                           # (:885-890) rows k .. nr - 2
                elt = np.abs(A[:, i - 1, k])
                eta = np.where(eta < elt, elt, eta)
            dead |= eta == 0
            inv_eta = 1.0 / eta
            s = np.zeros(B)
            for i in range(k, nr):
                A[:, i, k] = A[:, i, k] * inv_eta
                s = s + A[:, i, k] * A[:, i, k]
            sigma = np.sqrt(s)
            sigma = np.where(A[:, k, k] < 0, -sigma, sigma)
            A[:, k, k] = A[:, k, k] + sigma
            A1[:, k] = sigma * A[:, k, k]
            A2[:, k] = -eta * sigma
            for j in range(k + 1, nc):
                s2 = np.zeros(B)
                for i in range(k, nr):
                    s2 = s2 + A[:, i, k] * A[:, i, j]
                tau = s2 / A1[:, k]
                for i in range(k, nr):
                    A[:, i, j] = A[:, i, j] - tau * A[:, i, k]
        for j in range(nc):
            tau = np.zeros(B)
            for i in range(j, nr):
                tau = tau + A[:, i, j] * b[:, i]
            tau = tau / A1[:, j]
            for i in range(j, nr):
                b[:, i] = b[:, i] - tau * A[:, i, j]
        X = np.zeros((B, nc))
        X[:, nc - 1] = b[:, nc - 1] / A2[:, nc - 1]
        for i in range(nc - 2, -1, -1):
            s = np.zeros(B)
            for j in range(i + 1, nc):
                s = s + A[:, i, j] * X[:, j]
            X[:, i] = (b[:, i] - s) / A2[:, i]
    X[dead] = 0.0
    return X


def gauss_newton(L, rho, betas):
    """(:845-863, :817-843) L (B, 6, 10), rho (B, 6), betas (B, 4)."""
    be = np.array(betas, f64, copy=True)
    with np.errstate(all="ignore"):
        for _ in range(5):
            b0, b1, b2, b3 = (be[:, i:i + 1] for i in range(4))
            r = [L[:, :, i] for i in range(10)]
            A = np.stack([(((2 * r[0]) * b0 + r[1] * b1) + r[3] * b2) + r[6] * b3,
                          ((r[1] * b0 + (2 * r[2]) * b1) + r[4] * b2) + r[7] * b3,
                          ((r[3] * b0 + r[4] * b1) + (2 * r[5]) * b2) + r[8] * b3,
                          ((r[6] * b0 + r[7] * b1) + r[8] * b2) + (2 * r[9]) * b3], 2)
            s = (r[0] * b0) * b0
            for ri, x, y in ((1, b0, b1), (2, b1, b1), (3, b0, b2), (4, b1, b2), (5, b2, b2), (6, b0, b3), (7, b1, b3), (8, b2, b3), (9, b3, b3)):
                s = s + (r[ri] * x) * y
            be = be + qr_solve(A, rho - s)
    return be


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def betas_and_ccs(MtM, cws, lapack=False):
    """The dense middle of compute_pose: (B, 12, 12), (B, 4, 3) -> ccs3 (B, 3, 4, 3), betas (B, 3, 4)."""
    B = len(MtM)
    v = eig_smallest4(MtM, lapack).reshape(B, 4, 4, 3)           # v[b, i, control point, xyz]
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = np.stack([v[:, :, a] - v[:, :, b] for a, b in pairs], 2)    # (B, 4, 6, 3)
    L = np.empty((B, 6, 10))
    for col, (p, q) in enumerate(((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3))):
        d = dot3(dv[:, p], dv[:, q])
        L[:, :, col] = d if p == q else 2.0 * d
    rho = np.stack([dot3(cws[:, a] - cws[:, b], cws[:, a] - cws[:, b]) for a, b in pairs], 1)
    betas = np.zeros((B, 3, 4))
    with np.errstate(all="ignore"):
        x = lstsq(L[:, :, [0, 1, 3, 6]], rho, lapack)            # find_betas_approx_1 (:672-699)
        neg = x[:, 0] < 0
        b0 = np.sqrt(np.where(neg, -x[:, 0], x[:, 0]))
        sg = np.where(neg, -1.0, 1.0)
        betas[:, 0, 0] = b0
        for k in (1, 2, 3):
            betas[:, 0, k] = (sg * x[:, k]) / b0
        for a, cols in ((1, [0, 1, 2]), (2, [0, 1, 2, 3, 4])):   # find_betas_approx_2 / _3 (:704-763)
            x = lstsq(L[:, :, cols], rho, lapack)
            neg = x[:, 0] < 0
            b0 = np.sqrt(np.where(neg, -x[:, 0], x[:, 0]))
            b1 = np.where(neg, np.where(x[:, 2] < 0, np.sqrt(-x[:, 2]), 0.0), np.where(x[:, 2] > 0, np.sqrt(x[:, 2]), 0.0))
            b0 = np.where(x[:, 1] < 0, -b0, b0)
            betas[:, a, 0] = b0; betas[:, a, 1] = b1
            if a == 2:
                betas[:, a, 2] = x[:, 3] / b0
        ccs3 = np.zeros((B, 3, 4, 3))
        for a in range(3):
            betas[:, a] = gauss_newton(L, rho, betas[:, a])
            s = np.zeros((B, 4, 3))
            for i in range(4):
                s = s + betas[:, a, i][:, None, None] * v[:, i]
            ccs3[:, a] = s
    return ccs3, betas


def compute_pose(pw, uv, K4, W=1, lapack=False):
    """compute_pose (:482-530) for B problems of n points each: pw (B, n, 3), uv (B, n, 2) float64 (the float32 inputs widened).
    Returns R (B, 3, 3), t (B, 3), N (B,) in 1..3, err (B,), errs (B, 3)."""
    pw = np.asarray(pw, f64); uv = np.asarray(uv, f64)
    B, n, _ = pw.shape
    dn = f64(n)
    fu, fv, uc, vc = (f64(f32(k)) for k in K4)
    with np.errstate(all="ignore"):
        c0 = tree_sum(pw, W) / dn                                # choose_control_points (:380-414)
        d = pw - c0[:, None]
        d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
        c6 = tree_sum(np.stack([d0 * d0, d0 * d1, d0 * d2, d1 * d1, d1 * d2, d2 * d2], 2), W)
        cov = c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(B, 3, 3)
        _, dc, Vc = svd3(cov, lapack)
        cws = np.empty((B, 4, 3))
        cws[:, 0] = c0
        for i in range(1, 4):
            k = np.sqrt(dc[:, i - 1] / dn)
            cws[:, i] = c0 + k[:, None] * Vc[:, :, i - 1]
        cc = np.empty((B, 3, 3))                                 # compute_barycentric_coordinates (:416-439)
        for i in range(3):
            for j in range(1, 4):
                cc[:, i, j - 1] = cws[:, j, i] - cws[:, 0, i]
        ci = pinv3(cc, lapack)
        al = np.empty((B, n, 4))
        for j in range(3):
            al[..., 1 + j] = (ci[:, j, 0][:, None] * d0 + ci[:, j, 1][:, None] * d1) + ci[:, j, 2][:, None] * d2
        al[..., 0] = ((1.0 - al[..., 1]) - al[..., 2]) - al[..., 3]
        u, v = uv[..., 0], uv[..., 1]
        M1 = np.zeros((B, n, 12)); M2 = np.zeros((B, n, 12))     # fill_M (:441-456)
        for k in range(4):
            M1[..., 3 * k] = al[..., k] * fu; M1[..., 3 * k + 2] = al[..., k] * (uc - u)
            M2[..., 3 * k + 1] = al[..., k] * fv; M2[..., 3 * k + 2] = al[..., k] * (vc - v)
        T = M1[..., :, None] * M1[..., None, :] + M2[..., :, None] * M2[..., None, :]
        MtM = tree_sum(T.reshape(B, n, 144), W).reshape(B, 12, 12)
        ccs3, _ = betas_and_ccs(MtM, cws, lapack)
        Rs = np.empty((B, 3, 3, 3)); ts = np.empty((B, 3, 3)); errs = np.empty((B, 3))
        a_0 = al[:, 0]
        for ap in range(3):                                      # compute_R_and_t (:656-667)
            ccs = ccs3[:, ap].copy()
            z0 = ((a_0[:, 0] * ccs[:, 0, 2] + a_0[:, 1] * ccs[:, 1, 2]) + a_0[:, 2] * ccs[:, 2, 2]) + a_0[:, 3] * ccs[:, 3, 2]
            ccs = np.where((z0 < 0.0)[:, None, None], -ccs, ccs)
            pc = ((al[..., 0:1] * ccs[:, None, 0] + al[..., 1:2] * ccs[:, None, 1]) + al[..., 2:3] * ccs[:, None, 2]) + al[..., 3:4] * ccs[:, None, 3]
            pc0 = tree_sum(pc, W) / dn
            dj = pc - pc0[:, None]
            abt = tree_sum((dj[..., :, None] * d[..., None, :]).reshape(B, n, 9), W).reshape(B, 3, 3)
            U, _, V = svd3(abt, lapack)
            R = np.empty((B, 3, 3))
            for i in range(3):
                for j in range(3):
                    R[:, i, j] = (U[:, i, 0] * V[:, j, 0] + U[:, i, 1] * V[:, j, 1]) + U[:, i, 2] * V[:, j, 2]
            det = (((((R[:, 0, 0] * R[:, 1, 1]) * R[:, 2, 2] + (R[:, 0, 1] * R[:, 1, 2]) * R[:, 2, 0]) + (R[:, 0, 2] * R[:, 1, 0]) * R[:, 2, 1]) -
                    (R[:, 0, 2] * R[:, 1, 1]) * R[:, 2, 0]) - (R[:, 0, 1] * R[:, 1, 0]) * R[:, 2, 2]) - (R[:, 0, 0] * R[:, 1, 2]) * R[:, 2, 1]
            R[:, 2] = np.where((det < 0)[:, None], -R[:, 2], R[:, 2])
            t = np.stack([pc0[:, i] - dot3(R[:, i], c0) for i in range(3)], 1)
            Xc = dot3(R[:, None, 0], pw) + t[:, None, 0]; Yc = dot3(R[:, None, 1], pw) + t[:, None, 1]
            inv_Zc = 1.0 / (dot3(R[:, None, 2], pw) + t[:, None, 2])
            ue = uc + (fu * Xc) * inv_Zc; ve = vc + (fv * Yc) * inv_Zc
            e = np.sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve))
            errs[:, ap] = tree_sum(e[..., None], W)[:, 0] / dn
            Rs[:, ap] = R; ts[:, ap] = t
        N = np.ones(B, np.int64)                                 # (:523-525)
        N = np.where(errs[:, 1] < errs[:, 0], 2, N)
        r = np.arange(B)
        N = np.where(errs[:, 2] < errs[r, N - 1], 3, N)
    return Rs[r, N - 1], ts[r, N - 1], N, errs[r, N - 1], errs


# ---------------------------------------------------------------- CheckInliers (:313-345)
def check_inliers(R, t, K4, p3d, p2d, max_err, xc_double=False):
    """mask (n,) bool.  xc_double=True computes Xc, Yc, invZc in double (NOT the reference: the test of the promotions uses it)."""
    R = np.asarray(R, f64).reshape(3, 3); t = np.asarray(t, f64).reshape(3)
    fu, fv, uc, vc = (f64(f32(k)) for k in K4)
    P = np.asarray(p3d, f32).reshape(-1, 3).astype(f64); q = np.asarray(p2d, f32).reshape(-1, 2)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        Xc = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0]
        Yc = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1]
        iZ = 1.0 / (((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2])
        if not xc_double:
            Xc, Yc, iZ = Xc.astype(f32).astype(f64), Yc.astype(f32).astype(f64), iZ.astype(f32).astype(f64)
        ue = uc + (fu * Xc) * iZ
        ve = vc + (fv * Yc) * iZ
        dx = (q[:, 0].astype(f64) - ue).astype(f32)
        dy = (q[:, 1].astype(f64) - ve).astype(f32)
        e2 = dx * dx + dy * dy
        return e2 < np.asarray(max_err, f32).reshape(-1)


# ---------------------------------------------------------------- the selection rules of one iterate call
def run_selection(n_sets, min_inliers, best_count, count_of, on_record, refit):
    """The device's walk over one call's iterations, equal to the sequential rule of :183-260: count_of(it) -> CheckInliers' count,
    on_record(it) stores hypothesis it as the best state, refit() -> Refine's count on the CURRENT best mask.  Refine depends only on
    that mask, so it is called once per distinct mask.  Returns (status, consumed, best_count, n_refits)."""
    refit_known = False
    n_refits = 0
    for it in range(n_sets):
        cnt = count_of(it)
        if cnt < min_inliers:
            continue
        if cnt > best_count:
            best_count = cnt
            on_record(it)
            refit_known = False
        if refit_known:
            continue
        rc = refit()
        n_refits += 1
        refit_known = True
        if rc > min_inliers:
            return REFINED, it + 1, best_count, n_refits
    return (EXHAUSTED_BEST if best_count >= min_inliers else EXHAUSTED_NONE), n_sets, best_count, n_refits


class State:
    def __init__(self, n):
        self.best_count = 0
        self.best_mask = np.zeros(int(n), np.uint8)
        self.best_Tcw = np.eye(4)

    def copy(self):
        s = State(len(self.best_mask))
        s.best_count, s.best_mask, s.best_Tcw = self.best_count, self.best_mask.copy(), self.best_Tcw.copy()
        return s


def Tcw_of(R, t):
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T


def hypotheses(p3d, p2d, K4, sets, lapack=False):
    P = np.asarray(p3d, f32).reshape(-1, 3).astype(f64); q = np.asarray(p2d, f32).reshape(-1, 2).astype(f64)
    S = np.asarray(sets, np.int64).reshape(-1, 4)
    if len(S) == 0:
        return np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 3))
    return compute_pose(P[S], q[S], K4, 1, lapack)


def iterate(p3d, p2d, max_err, K4, min_inliers, sets, state=None, lapack=False):
    """One PnPsolver::iterate call given every set it may consume.  Returns dict status, consumed, n_inliers, n_refits, Tcw,
    inliers, state (updated in place) and the trace: R, t, approx, rep_error, errs, count per CONSUMED iteration, refits = list
    of (iteration, R, t, count)."""
    P3 = np.asarray(p3d, f32).reshape(-1, 3); P2 = np.asarray(p2d, f32).reshape(-1, 2); E = np.asarray(max_err, f32).reshape(-1)
    n = len(P3)
    S = np.asarray(sets, np.int64).reshape(-1, 4)
    if state is None:
        state = State(n)
    out = dict(state=state, refits=[])
    if n < min_inliers:                                          # (:174-178)
        out.update(status=TOO_FEW, consumed=0, n_inliers=0, n_refits=0, Tcw=np.eye(4), inliers=np.zeros(n, bool))
        return out
    R, t, N, err, errs = hypotheses(P3, P2, K4, S, lapack)
    masks = [check_inliers(R[i], t[i], K4, P3, P2, E) for i in range(len(S))]
    counts = [int(m.sum()) for m in masks]
    last = {}

    def on_record(it):
        state.best_count, state.best_mask, state.best_Tcw = counts[it], masks[it].astype(np.uint8), Tcw_of(R[it], t[it])

    def refit():
        idx = np.nonzero(state.best_mask)[0]
        Rr, tr, _, _, _ = compute_pose(P3[idx].astype(f64)[None], P2[idx].astype(f64)[None], K4, REFINE_W, lapack)
        m = check_inliers(Rr[0], tr[0], K4, P3, P2, E)
        last.update(R=Rr[0], t=tr[0], mask=m)
        return int(m.sum())

    def refit_logged():
        c = refit()
        out["refits"].append((cur[0], last["R"], last["t"], c))
        return c

    cur = [0]

    def count_of(it):
        cur[0] = it
        return counts[it]
    status, consumed, bc, n_refits = run_selection(len(S), min_inliers, state.best_count, count_of, on_record, refit_logged)
    out.update(status=status, consumed=consumed, n_refits=n_refits, R=R[:consumed], t=t[:consumed], approx=N[:consumed], rep_error=err[:consumed],
               errs=errs[:consumed], count=np.array(counts[:consumed], np.int32))
    if status == REFINED:
        out.update(Tcw=Tcw_of(last["R"], last["t"]), inliers=last["mask"], n_inliers=int(last["mask"].sum()))
    elif status == EXHAUSTED_BEST:
        out.update(Tcw=state.best_Tcw.copy(), inliers=state.best_mask.astype(bool), n_inliers=state.best_count)
    else:
        out.update(Tcw=np.eye(4), inliers=np.zeros(n, bool), n_inliers=0)
    return out


# ---------------------------------------------------------------- the reference's class, line by line, on scripted estimators
class RefSolver:
    """PnPsolver::iterate (:166-261) and Refine (:263-310) with the estimators injected: hypothesis(k) -> (count, mask, pose) for the
    k-th iteration since construction, refine(mask) -> (count, mask, pose).  The test of the selection rules compares the
    library-style driver (sets supplied per call, run_selection, advance by `consumed`) with this."""

    def __init__(self, N, min_inliers, max_its, key_point_indices, n_matches, hypothesis, refine):
        self.N, self.min_inl, self.max_its = N, min_inliers, max_its
        self.kpi, self.n_matches = list(key_point_indices), n_matches
        self.hypothesis, self.refine = hypothesis, refine
        self.mnIterations = 0
        self.best_count, self.best_mask, self.best_pose = 0, [False] * N, None

    def scatter(self, mask):
        v = [False] * self.n_matches
        for i in range(self.N):
            if mask[i]:
                v[self.kpi[i]] = True
        return v

    def iterate(self, nIterations):
        """-> (pose or "I" for identity, bNoMore, vbInliers, nInliers)"""
        if self.N < self.min_inl:
            return "I", True, [], 0
        cur = 0
        while self.mnIterations < self.max_its or cur < nIterations:
            cur += 1
            k = self.mnIterations
            self.mnIterations += 1
            cnt, mask, pose = self.hypothesis(k)
            if cnt >= self.min_inl:
                if cnt > self.best_count:
                    self.best_mask, self.best_count, self.best_pose = list(mask), cnt, pose
                rc, rmask, rpose = self.refine(self.best_mask)
                if rc > self.min_inl:
                    return rpose, False, self.scatter(rmask), rc
        if self.mnIterations >= self.max_its:
            if self.best_count >= self.min_inl:
                return self.best_pose, True, self.scatter(self.best_mask), self.best_count
            return "I", True, [], 0
        return "I", False, [], 0


class LibDriver:
    """What a caller of the library does around one solver (the drop-in's bookkeeping): it owns mnIterations, supplies
    max(max_its - mnIterations, nIterations) sets per iterate call (:183's OR), advances by `consumed`, and derives bNoMore and the
    identity returns from the status.  Same injected estimators and return value as RefSolver."""

    def __init__(self, N, min_inliers, max_its, key_point_indices, n_matches, hypothesis, refine):
        self.ref = RefSolver(N, min_inliers, max_its, key_point_indices, n_matches, hypothesis, refine)   # (for scatter and the fields)
        self.N, self.min_inl, self.max_its = N, min_inliers, max_its
        self.hypothesis, self.refine = hypothesis, refine
        self.mnIterations = 0
        self.best_count, self.best_mask, self.best_pose = 0, [False] * N, None

    def iterate(self, nIterations):
        if self.N < self.min_inl:                                # TOO_FEW
            return "I", True, [], 0
        n_sets = max(self.max_its - self.mnIterations, nIterations)
        base = self.mnIterations
        hyp, last = {}, {}

        def count_of(it):
            hyp[it] = self.hypothesis(base + it)
            return hyp[it][0]

        def on_record(it):
            self.best_count, self.best_mask, self.best_pose = hyp[it][0], list(hyp[it][1]), hyp[it][2]

        def refit():
            last["r"] = self.refine(self.best_mask)
            return last["r"][0]
        status, consumed, _, _ = run_selection(n_sets, self.min_inl, self.best_count, count_of, on_record, refit)
        self.mnIterations += consumed
        if status == REFINED:
            rc, rmask, rpose = last["r"]
            return rpose, False, self.ref.scatter(rmask), rc
        if status == EXHAUSTED_BEST:
            return self.best_pose, True, self.ref.scatter(self.best_mask), self.best_count
        return "I", True, [], 0
