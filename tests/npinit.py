"""numpy restatement of Initializer::Initialize (reference src/Initializer.cc:54-889, monocular), written from the reference lines
with the operation order of the device code (ceres_mono_orb_slam2_amd/csrc/orb_init.inc):
- float sums run sequentially (np.add.accumulate in float32; np.sum would sum pairwise);
- every narrowing is explicit (f32(...) of a float64 value, f64(...) of a float32 one);
- the null vectors and SVDs are the device's one-sided Jacobi (null_vector4_dev's operation order), batched over hypotheses;
- where the reference's result depends on Eigen (JacobiSVD rounding and sign conventions, the 3 x 3 inverse formula, the summation
  order of 3-term products) this file follows the device, not Eigen: DESIGN.md section 2, "Two-view initialisation".
Every function takes and returns numpy arrays; nothing here imports the product package."""
import numpy as np

f32, f64 = np.float32, np.float64
TH_COS = 0.99998

OK, BAD_INPUT, NO_MODEL = 0, 1, 2
H_DEGENERATE, H_AMBIGUOUS, H_PARALLAX, H_FEW = 3, 4, 5, 6
F_FEW, F_AMBIGUOUS, F_PARALLAX = 7, 8, 9


def fsum_seq(a, axis=-1):
    """float32 sum in index order (the reference's `score += ...` loop)."""
    a = np.asarray(a, f32)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis), f32) if a.ndim > 1 else f32(0)
    return np.take(np.add.accumulate(a, axis=axis, dtype=f32), -1, axis=axis)


# ---------------------------------------------------------------- linear algebra (device operation order)
def jacobi(A, return_sweeps=False, tol=1e-15, null_rule=True):
    """One-sided Jacobi on the columns of A (B, M, N): returns (U = A V, V), the sweep / pair / row order of null_vector4_dev.
    Defaults: orb_init.inc's i_jacobi (a pair is orthogonal at |cos| <= 1e-15; a column below 1e-14 ||A||_F is not rotated again).
    tol=1e-16, null_rule=False: tri_math.h's null_vector4_dev.  return_sweeps: also the sweeps each system ran (the last one,
    without a rotation, included)."""
    U = np.array(A, f64, copy=True)
    B, M, N = U.shape
    V = np.broadcast_to(np.eye(N), (B, N, N)).copy()
    active = np.ones(B, bool)
    fro = np.zeros(B)
    for i in range(M):
        for j in range(N):
            fro = fro + U[:, i, j] * U[:, i, j]
    tiny = 1e-28 * fro if null_rule else np.full(B, -1.0)      # a column below 1e-14 ||A||_F is null: not rotated again
    sweeps = np.zeros(B, np.int64)
    with np.errstate(all="ignore"):
        for _ in range(60):
            rotated = np.zeros(B, bool)
            for p in range(N - 1):
                for q in range(p + 1, N):
                    alpha = np.zeros(B); beta = np.zeros(B); gamma = np.zeros(B)
                    for i in range(M):
                        up, uq = U[:, i, p], U[:, i, q]
                        alpha = alpha + up * up; beta = beta + uq * uq; gamma = gamma + up * uq
                    skip = (gamma == 0.0) | (np.abs(gamma) <= tol * np.sqrt(alpha * beta)) | (alpha <= tiny) | (beta <= tiny)
                    rot = active & ~skip
                    if not rot.any():
                        continue
                    zeta = (beta - alpha) / (2.0 * gamma)
                    t = np.where(zeta >= 0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    s = c * t
                    c_, s_ = c[:, None], s[:, None]
                    up, uq = U[:, :, p].copy(), U[:, :, q].copy()
                    r = rot[:, None]
                    U[:, :, p] = np.where(r, c_ * up - s_ * uq, up); U[:, :, q] = np.where(r, s_ * up + c_ * uq, uq)
                    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p] = np.where(r, c_ * vp - s_ * vq, vp); V[:, :, q] = np.where(r, s_ * vp + c_ * vq, vq)
                    rotated |= rot
            sweeps += active
            active &= rotated
            if not active.any():
                break
    return (U, V, sweeps) if return_sweeps else (U, V)


def min_col(U):
    """index of the column of least norm, first on ties (sequential sums)."""
    B, M, N = U.shape
    best = np.zeros(B, np.int64); bn = np.full(B, 1e300)
    for j in range(N):
        nrm = np.zeros(B)
        for i in range(M):
            nrm = nrm + U[:, i, j] * U[:, i, j]
        take = nrm < bn
        bn = np.where(take, nrm, bn); best = np.where(take, j, best)
    return best


def null_vector(A, **jacobi_rule):
    """(B, M, N) -> (B, N): the right singular vector of the smallest singular value."""
    U, V = jacobi(A, **jacobi_rule)
    c = min_col(U)
    return V[np.arange(len(V)), :, c]


def mm3(A, B):
    A = np.asarray(A, f64); B = np.asarray(B, f64)
    C = np.empty(np.broadcast_shapes(A.shape, B.shape))
    for i in range(3):
        for j in range(3):
            C[..., i, j] = (A[..., i, 0] * B[..., 0, j] + A[..., i, 1] * B[..., 1, j]) + A[..., i, 2] * B[..., 2, j]
    return C


def mv3(A, x):
    return np.stack([(A[..., i, 0] * x[..., 0] + A[..., i, 1] * x[..., 1]) + A[..., i, 2] * x[..., 2] for i in range(3)], -1)


def det3(a):
    a = np.asarray(a, f64).reshape(a.shape[:-2] + (9,))
    return (a[..., 0] * (a[..., 4] * a[..., 8] - a[..., 5] * a[..., 7]) + a[..., 1] * (a[..., 5] * a[..., 6] - a[..., 3] * a[..., 8])) + \
        a[..., 2] * (a[..., 3] * a[..., 7] - a[..., 4] * a[..., 6])


def inv3(a):
    a = np.asarray(a, f64)
    s = a.shape
    a = a.reshape(s[:-2] + (9,))
    m = np.stack([a[..., 4] * a[..., 8] - a[..., 5] * a[..., 7], a[..., 2] * a[..., 7] - a[..., 1] * a[..., 8], a[..., 1] * a[..., 5] - a[..., 2] * a[..., 4],
                  a[..., 5] * a[..., 6] - a[..., 3] * a[..., 8], a[..., 0] * a[..., 8] - a[..., 2] * a[..., 6], a[..., 2] * a[..., 3] - a[..., 0] * a[..., 5],
                  a[..., 3] * a[..., 7] - a[..., 4] * a[..., 6], a[..., 1] * a[..., 6] - a[..., 0] * a[..., 7], a[..., 0] * a[..., 4] - a[..., 1] * a[..., 3]], -1)
    det = (a[..., 0] * m[..., 0] + a[..., 1] * m[..., 3]) + a[..., 2] * m[..., 6]
    with np.errstate(all="ignore"):
        return (m / det[..., None]).reshape(s)


def svd3(A):
    """A (B, 3, 3) = U diag(S) V^T: S descending (stable), U's third column u0 x u1, v2 signed so that A v2 = S2 u2."""
    A = np.asarray(A, f64).reshape(-1, 3, 3)
    Bm, W = jacobi(A)
    nb = len(A)
    nrm = np.zeros((nb, 3))
    for j in range(3):
        s = np.zeros(nb)
        for i in range(3):
            s = s + Bm[:, i, j] * Bm[:, i, j]
        nrm[:, j] = np.sqrt(s)
    o = np.tile(np.arange(3), (nb, 1))
    r = np.arange(nb)
    for a_, b_ in ((0, 1), (1, 2), (0, 1)):
        sw = nrm[r, o[:, b_]] > nrm[r, o[:, a_]]
        oa, ob = o[:, a_].copy(), o[:, b_].copy()
        o[:, a_] = np.where(sw, ob, oa); o[:, b_] = np.where(sw, oa, ob)
    S = np.stack([nrm[r, o[:, k]] for k in range(3)], 1)
    col = lambda M, k: M[r, :, o[:, k]]                                    # noqa: E731  (B, 3)
    with np.errstate(all="ignore"):
        u0 = col(Bm, 0) / S[:, 0:1]; u1 = col(Bm, 1) / S[:, 1:2]
        # rank <= 1 to working precision: column 1 supplies no left vector; u1 = u0's complement along the axis least aligned with u0
        low = ~(S[:, 1] > 2e-14 * S[:, 0])
        e0 = np.zeros((nb, 3)); e0[:, 0] = 1.0
        u0 = np.where((low & ~(S[:, 0] > 0.0))[:, None], e0, u0)
        a = np.abs(u0)
        k = np.where((a[:, 0] <= a[:, 1]) & (a[:, 0] <= a[:, 2]), 0, np.where(a[:, 1] <= a[:, 2], 1, 2))
        w = np.eye(3)[k] - u0[r, k][:, None] * u0
        wn = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        u1 = np.where(low[:, None], w / wn[:, None], u1)
    b2 = col(Bm, 2)
    u2 = np.stack([u0[:, 1] * u1[:, 2] - u0[:, 2] * u1[:, 1], u0[:, 2] * u1[:, 0] - u0[:, 0] * u1[:, 2], u0[:, 0] * u1[:, 1] - u0[:, 1] * u1[:, 0]], 1)
    d2 = (b2[:, 0] * u2[:, 0] + b2[:, 1] * u2[:, 1]) + b2[:, 2] * u2[:, 2]
    # d2 == 0 exactly (a zero third column) leaves the sign free: V is made proper like U (det V = the parity of the sort)
    sg = np.where(d2 < 0, -1.0, np.where(d2 > 0, 1.0, np.where((o[:, 1] - o[:, 0] + 3) % 3 == 1, 1.0, -1.0)))
    U = np.stack([u0, u1, u2], 2)
    V = np.stack([col(W, 0), col(W, 1), sg[:, None] * col(W, 2)], 2)
    return U, S, V


# ---------------------------------------------------------------- the steps of Initialize
def match_list(matches12):
    """(:60-72) positions -> (i1, i2), ascending i1."""
    m = np.asarray(matches12, np.int64)
    i1 = np.nonzero(m >= 0)[0]
    return i1, m[i1]


def normalize(kps):
    """(:714-755) Normalize over ALL keypoints: float sums in index order; sX = float(1.0 / meanDevX); T in double."""
    k = np.asarray(kps, f32).reshape(-1, 2)
    n = f32(len(k))
    st = []
    pn = np.empty_like(k)
    for c in range(2):
        x = k[:, c]
        mean = f32(fsum_seq(x) / n)
        d = x - mean
        dev = f32(fsum_seq(np.abs(d)) / n)
        s = f32(1.0 / f64(dev))
        pn[:, c] = d * s
        st.append((mean, s))
    (mx, sx), (my, sy) = st
    T = np.array([[f64(sx), 0, f64(-mx * sx)], [0, f64(sy), f64(-my * sy)], [0, 0, 1.0]])
    return pn, T


def hypotheses(kps1, kps2, matches12, sets):
    """(:135-225) every iteration's H21, H12 (:167-169) and F21 (:213-215), as the scoring consumes them."""
    pn1, T1 = normalize(kps1)
    pn2, T2 = normalize(kps2)
    i1, i2 = match_list(matches12)
    sets = np.asarray(sets, np.int64).reshape(-1, 8)
    u1 = pn1[i1[sets], 0]; v1 = pn1[i1[sets], 1]; u2 = pn2[i2[sets], 0]; v2 = pn2[i2[sets], 1]      # (it, 8) float32
    B = len(sets)
    Ah = np.zeros((B, 16, 9)); Af = np.zeros((B, 8, 9))
    for j in range(8):                                          # (:234-253, :270-285): float products stored in double
        a, b, c, d = u1[:, j], v1[:, j], u2[:, j], v2[:, j]
        Ah[:, 2 * j, 0] = -a; Ah[:, 2 * j, 1] = -b; Ah[:, 2 * j, 2] = -1.0
        Ah[:, 2 * j, 6] = a * c; Ah[:, 2 * j, 7] = b * c; Ah[:, 2 * j, 8] = c
        Ah[:, 2 * j + 1, 3] = -a; Ah[:, 2 * j + 1, 4] = -b; Ah[:, 2 * j + 1, 5] = -1.0
        Ah[:, 2 * j + 1, 6] = a * d; Ah[:, 2 * j + 1, 7] = b * d; Ah[:, 2 * j + 1, 8] = d
        Af[:, j] = np.stack([c * a, c * b, c, d * a, d * b, d, a, b, np.ones_like(a)], 1)
    Hn = null_vector(Ah).reshape(B, 3, 3)                       # row-major: Map<Matrix3d>(V.col(8)).transpose()
    H21 = mm3(mm3(inv3(T2), Hn), T1)
    H12 = inv3(H21)
    Fpre = null_vector(Af).reshape(B, 3, 3)
    U, S, V = svd3(Fpre)                                        # (:293-301) rank 2
    Sz = np.stack([S[:, 0], S[:, 1], np.zeros(B)], 1)
    W = U * Sz[:, None, :]
    Fn = np.empty((B, 3, 3))
    for i in range(3):
        for j in range(3):
            Fn[:, i, j] = (W[:, i, 0] * V[:, j, 0] + W[:, i, 1] * V[:, j, 1]) + W[:, i, 2] * V[:, j, 2]
    F21 = mm3(mm3(np.swapaxes(T2, -1, -2), Fn), T1)
    return H21, H12, F21


def _pts(kps1, kps2, matches12):
    k1 = np.asarray(kps1, f32).reshape(-1, 2); k2 = np.asarray(kps2, f32).reshape(-1, 2)
    i1, i2 = match_list(matches12)
    return k1[i1, 0], k1[i1, 1], k2[i2, 0], k2[i2, 1]


def homography_terms(H21, H12, kps1, kps2, matches12, sigma=1.0):
    """(:306-376) per hypothesis (leading axis) and match: the two score terms and the inlier bit."""
    u1, v1, u2, v2 = _pts(kps1, kps2, matches12)
    du1, dv1, du2, dv2 = (f64(x) for x in (u1, v1, u2, v2))
    H21 = np.asarray(H21, f64).reshape(-1, 3, 3); H12 = np.asarray(H12, f64).reshape(-1, 3, 3)
    inv_s2 = f32(1.0 / f64(f32(sigma) * f32(sigma)))
    th = f32(5.991)
    h = lambda M, i, a, b: (M[:, i, 0, None] * a + M[:, i, 1, None] * b) + M[:, i, 2, None]   # noqa: E731
    with np.errstate(all="ignore"):
        z = h(H12, 2, du2, dv2)
        u2in1 = (h(H12, 0, du2, dv2) / z).astype(f32); v2in1 = (h(H12, 1, du2, dv2) / z).astype(f32)
        chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * inv_s2
        z = h(H21, 2, du1, dv1)
        u1in2 = (h(H21, 0, du1, dv1) / z).astype(f32); v1in2 = (h(H21, 1, du1, dv1) / z).astype(f32)
        chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * inv_s2
        ta = np.where(chi1 > th, f32(0), th - chi1); tb = np.where(chi2 > th, f32(0), th - chi2)
    return ta, tb, ~(chi1 > th) & ~(chi2 > th)


def fundamental_terms(F21, kps1, kps2, matches12, sigma=1.0):
    """(:378-444)"""
    u1, v1, u2, v2 = _pts(kps1, kps2, matches12)
    du1, dv1, du2, dv2 = (f64(x) for x in (u1, v1, u2, v2))
    F = np.asarray(F21, f64).reshape(-1, 3, 3)
    inv_s2 = f32(1.0 / f64(f32(sigma) * f32(sigma)))
    th, ths = f32(3.841), f32(5.991)
    with np.errstate(all="ignore"):
        l2 = [(F[:, i, 0, None] * du1 + F[:, i, 1, None] * dv1) + F[:, i, 2, None] for i in range(3)]
        num2 = ((du2 * l2[0] + dv2 * l2[1]) + l2[2]).astype(f32)
        chi1 = (f64(num2 * num2) / (l2[0] * l2[0] + l2[1] * l2[1])).astype(f32) * inv_s2
        l1 = [(du2 * F[:, 0, j, None] + dv2 * F[:, 1, j, None]) + F[:, 2, j, None] for j in range(3)]
        num1 = ((l1[0] * du1 + l1[1] * dv1) + l1[2]).astype(f32)
        chi2 = (f64(num1 * num1) / (l1[0] * l1[0] + l1[1] * l1[1])).astype(f32) * inv_s2
        ta = np.where(chi1 > th, f32(0), ths - chi1); tb = np.where(chi2 > th, f32(0), ths - chi2)
    return ta, tb, ~(chi1 > th) & ~(chi2 > th)


def score_terms(ta, tb):
    """the float sum in match order, the two terms of a match interleaved."""
    B, N = ta.shape
    return fsum_seq(np.stack([ta, tb], 2).reshape(B, 2 * N), axis=1) if N else np.zeros(B, f32)


def check_homography(H21, H12, kps1, kps2, matches12, sigma=1.0):
    ta, tb, inl = homography_terms(H21, H12, kps1, kps2, matches12, sigma)
    return score_terms(ta, tb), inl


def check_fundamental(F21, kps1, kps2, matches12, sigma=1.0):
    ta, tb, inl = fundamental_terms(F21, kps1, kps2, matches12, sigma)
    return score_terms(ta, tb), inl


def best_of(scores):
    """(:173-177) `currentScore > score` from score = 0: (best score, its index or -1)."""
    best, bi = f32(0), -1
    for i, s in enumerate(np.asarray(scores, f32)):
        if s > best:
            best, bi = s, i
    return best, bi


def K3(K4):
    fx, fy, cx, cy = (f64(v) for v in np.asarray(K4, f32))
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def motions_h(H21, K4):
    """(:556-651) -> (ok, R[8], t[8]); ok = False: d1 / d2 or d2 / d3 below 1.00001 (:573)."""
    K = K3(K4)
    A = mm3(mm3(inv3(K), np.asarray(H21, f64)), K)
    U, S, V = svd3(A)
    U, S, V = U[0], S[0], V[0]
    s = f32(det3(U) * det3(V))
    d1, d2, d3 = f32(S[0]), f32(S[1]), f32(S[2])
    with np.errstate(all="ignore"):
        if f64(d1 / d2) < 1.00001 or f64(d2 / d3) < 1.00001:
            return False, None, None
        aux1 = np.sqrt(f32((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)))
        aux3 = np.sqrt(f32((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3)))
        x1 = [aux1, aux1, -aux1, -aux1]; x3 = [aux3, -aux3, aux3, -aux3]
        aux_st = f32(np.sqrt(f32((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))) / ((d1 + d3) * d2))
        cth = f32((d2 * d2 + d1 * d3) / ((d1 + d3) * d2))
        st = [aux_st, -aux_st, -aux_st, aux_st]
        aux_sp = f32(np.sqrt(f32((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))) / ((d1 - d3) * d2))
        cph = f32((d1 * d3 - d2 * d2) / ((d1 - d3) * d2))
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        sU = f64(s) * U
        Vt = V.T.copy()
        Rs, ts = [], []
        for m in range(8):
            i = m & 3
            Rp = np.eye(3)
            if m < 4:
                Rp[0, 0] = cth; Rp[0, 2] = f64(-st[i]); Rp[2, 0] = st[i]; Rp[2, 2] = cth
                f = f64(d1 - d3)
                tp = np.array([f64(x1[i]) * f, 0.0 * f, f64(-x3[i]) * f])
            else:
                Rp[0, 0] = cph; Rp[0, 2] = sp[i]; Rp[1, 1] = -1; Rp[2, 0] = sp[i]; Rp[2, 2] = f64(-cph)
                f = f64(d1 + d3)
                tp = np.array([f64(x1[i]) * f, 0.0 * f, f64(x3[i]) * f])
            Rs.append(mm3(mm3(sU, Rp), Vt))
            t = mv3(U, tp)
            nt = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
            ts.append(t / nt)
    return True, np.array(Rs), np.array(ts)


def motions_f(F21, K4):
    """(:457-463, :866-889) E21 = K^T F21 K, DecomposeE: (R1, t), (R2, t), (R1, -t), (R2, -t)."""
    K = K3(K4)
    E = mm3(mm3(K.T.copy(), np.asarray(F21, f64)), K)
    U, S, V = svd3(E)
    U, V = U[0], V[0]
    Vt = V.T.copy()
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    R1 = mm3(mm3(U, W), Vt); R2 = mm3(mm3(U, W.T.copy()), Vt)
    t = U[:, 2].copy()
    nt = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    t = t / nt
    if det3(R1) < 0:
        R1 = -R1
    if det3(R2) < 0:
        R2 = -R2
    return np.array([R1, R2, R1, R2]), np.array([t, t, -t, -t])


def check_rt(R, t, kps1, kps2, matches12, inliers, K4, sigma=1.0):
    """(:757-864) for one motion: dict n_good, good[N], tri[N], P[N, 3] (valid where good), cos[N], parallax (float32 degrees).
    N = the match list; inliers[N] the model's winner mask.  sorted_cos[min(50, nGood - 1)] with NaN ordered after every number."""
    R = np.asarray(R, f64); t = np.asarray(t, f64)
    K = K3(K4)
    fx, fy, cx, cy = (f32(v) for v in np.asarray(K4, f32))
    x1p, y1p, x2p, y2p = _pts(kps1, kps2, matches12)
    N = len(x1p)
    inl = np.asarray(inliers, bool).reshape(N)
    P1 = np.zeros((3, 4)); P1[:, :3] = K
    Rt = np.zeros((3, 4)); Rt[:, :3] = R; Rt[:, 3] = t
    P2 = np.empty((3, 4))
    for i in range(3):
        for j in range(4):
            P2[i, j] = (K[i, 0] * Rt[0, j] + K[i, 1] * Rt[1, j]) + K[i, 2] * Rt[2, j]
    O2 = np.array([((-R[0, i]) * t[0] + (-R[1, i]) * t[1]) + (-R[2, i]) * t[2] for i in range(3)])
    idx = np.nonzero(inl)[0]
    a, b, c, d = (f64(v[idx]) for v in (x1p, y1p, x2p, y2p))
    A = np.empty((len(idx), 4, 4))
    for j in range(4):                                          # (:697-712)
        A[:, 0, j] = a * P1[2, j] - P1[0, j]; A[:, 1, j] = b * P1[2, j] - P1[1, j]
        A[:, 2, j] = c * P2[2, j] - P2[0, j]; A[:, 3, j] = d * P2[2, j] - P2[1, j]
    good = np.zeros(N, bool); tri = np.zeros(N, bool); P = np.full((N, 3), np.nan); cosv = np.full(N, np.nan, f32)
    if len(idx):
        X4 = null_vector(A, tol=1e-16, null_rule=False)            # null_vector4_dev (tri_math.h)
        with np.errstate(all="ignore"):
            p = X4[:, :3] / X4[:, 3:4]
            fin = np.isfinite(p).all(1)
            p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
            dist1 = np.sqrt((p0 * p0 + p1 * p1) + p2 * p2).astype(f32)
            n2 = p - O2
            dist2 = np.sqrt((n2[:, 0] * n2[:, 0] + n2[:, 1] * n2[:, 1]) + n2[:, 2] * n2[:, 2]).astype(f32)
            cs = (((p0 * n2[:, 0] + p1 * n2[:, 1]) + p2 * n2[:, 2]) / f64(dist1 * dist2)).astype(f32)
            lowpar = f64(cs) < TH_COS
            g1 = ~((p2 <= 0) & lowpar)
            q = np.stack([((R[i, 0] * p0 + R[i, 1] * p1) + R[i, 2] * p2) + t[i] for i in range(3)], 1)
            g2 = ~((q[:, 2] <= 0) & lowpar)
            iz1 = (1.0 / p2).astype(f32)
            im1x = (f64(fx) * p0 * f64(iz1) + f64(cx)).astype(f32); im1y = (f64(fy) * p1 * f64(iz1) + f64(cy)).astype(f32)
            xa, ya, xb, yb = x1p[idx], y1p[idx], x2p[idx], y2p[idx]
            e1 = (im1x - xa) * (im1x - xa) + (im1y - ya) * (im1y - ya)
            iz2 = (1.0 / q[:, 2]).astype(f32)
            im2x = (f64(fx) * q[:, 0] * f64(iz2) + f64(cx)).astype(f32); im2y = (f64(fy) * q[:, 1] * f64(iz2) + f64(cy)).astype(f32)
            e2 = (im2x - xb) * (im2x - xb) + (im2y - yb) * (im2y - yb)
            th2 = f32(4.0 * f64(f32(sigma) * f32(sigma)))
            ok = fin & g1 & g2 & ~(e1 > th2) & ~(e2 > th2)
        good[idx] = ok; tri[idx] = ok & lowpar
        P[idx[ok]] = p[ok]; cosv[idx[ok]] = cs[ok]
    ng = int(good.sum())
    return dict(n_good=ng, good=good, tri=tri, P=P, cos=cosv, parallax=parallax_of(cosv[good]))


def parallax_of(cos_good):
    """(:855-861) acos(sorted_cos[min(50, nGood - 1)]) * 180 / pi in float, 0 without good points.  NaN sorts after every number."""
    c = np.asarray(cos_good, f32)
    if len(c) == 0:
        return f32(0)
    cval = np.sort(c)[min(50, len(c) - 1)]                      # (np.sort puts NaN last)
    with np.errstate(all="ignore"):
        return f32(f64(np.arccos(f32(cval)) * f32(180)) / np.pi)


def decide_h(n_good, parallax, N, min_parallax=1.0, min_triangulated=50):
    """(:653-693) -> (motion or -1, reason)."""
    best, second, bi, bpar = 0, 0, -1, f32(-1)
    for i in range(8):
        if n_good[i] > best:
            second, best, bi, bpar = best, n_good[i], i, parallax[i]
        elif n_good[i] > second:
            second = n_good[i]
    if not second < 0.75 * best:
        return -1, H_AMBIGUOUS
    if not bpar >= f32(min_parallax):
        return -1, H_PARALLAX
    if not (best > min_triangulated and best > 0.9 * N):
        return -1, H_FEW
    return bi, OK


def decide_f(n_good, parallax, N, min_parallax=1.0, min_triangulated=50):
    """(:484-538) -> (motion or -1, reason); the first motion with nGood == maxGood decides, no fall-through."""
    g = list(n_good[:4])
    mx = max(g)
    nmin = max(int(0.9 * N), min_triangulated)
    nsim = sum(1 for v in g if v > 0.7 * mx)
    if mx < nmin:
        return -1, F_FEW
    if nsim > 1:
        return -1, F_AMBIGUOUS
    k = g.index(mx)
    return (k, OK) if parallax[k] > f32(min_parallax) else (-1, F_PARALLAX)


def initialize(kps1, kps2, matches12, K4, sigma=1.0, iterations=200, ransac_sets=None, hyp=None):
    """The whole of Initialize; returns the dict orbt_initialize's Python wrapper returns (success, R21, t21, P3D with NaN on the
    rows not written, triangulated, report fields) plus the intermediates: H21, H12, F21, score_h, score_f, inliers_h, inliers_f,
    motion_R, motion_t, rt (per-motion check_rt dicts).  hyp = (H21, H12, F21) replaces the hypotheses (the trace's)."""
    k1 = np.asarray(kps1, f32).reshape(-1, 2)
    m12 = np.asarray(matches12, np.int64)
    n1 = len(k1)
    sets = np.asarray(ransac_sets, np.int64).reshape(-1, 8)
    H21, H12, F21 = hyp if hyp is not None else hypotheses(kps1, kps2, matches12, sets)
    sh, inl_h_all = check_homography(H21, H12, kps1, kps2, matches12, sigma)
    sf, inl_f_all = check_fundamental(F21, kps1, kps2, matches12, sigma)
    SH, bh = best_of(sh)
    SF, bf = best_of(sf)
    nm = int((m12 >= 0).sum())
    inl_h = inl_h_all[bh] if bh >= 0 else np.zeros(nm, bool)
    inl_f = inl_f_all[bf] if bf >= 0 else np.zeros(nm, bool)
    with np.errstate(all="ignore"):
        RH = f32(SH / (SH + SF))
    model = 0 if f64(RH) > 0.40 else 1
    out = dict(H21=H21, H12=H12, F21=F21, score_h=sh, score_f=sf, inliers_h=inl_h, inliers_f=inl_f, model=model, rh=RH, score_h_best=SH,
               score_f_best=SF, best_h=bh, best_f=bf, n_matches=nm, n_inliers=int((inl_h if model == 0 else inl_f).sum()), motion=-1,
               n_good=np.zeros(8, np.int32), parallax=np.zeros(8, f32), motion_R=np.zeros((8, 3, 3)), motion_t=np.zeros((8, 3)), rt=[],
               success=False, R21=None, t21=None, P3D=np.full((n1, 3), np.nan), triangulated=None)
    out["score_h"], out["score_f"] = sh, sf
    best = bh if model == 0 else bf
    if best < 0:
        out["reason"] = NO_MODEL
        return out
    if model == 0:
        ok, Rs, ts = motions_h(H21[bh], K4)
        if not ok:
            out["reason"] = H_DEGENERATE
            return out
    else:
        Rs, ts = motions_f(F21[bf], K4)
    inl = inl_h if model == 0 else inl_f
    out["motion_R"][:len(Rs)] = Rs; out["motion_t"][:len(ts)] = ts
    rts = [check_rt(Rs[m], ts[m], kps1, kps2, matches12, inl, K4, sigma) for m in range(len(Rs))]
    out["rt"] = rts
    for m, r in enumerate(rts):
        out["n_good"][m] = r["n_good"]; out["parallax"][m] = r["parallax"]
    N = int(inl.sum())
    win, reason = (decide_h if model == 0 else decide_f)(out["n_good"], out["parallax"], N)
    out["reason"], out["motion"] = reason, win
    if win >= 0:
        i1, _ = match_list(matches12)
        r = rts[win]
        out["success"] = True
        out["R21"], out["t21"] = Rs[win], ts[win]
        out["P3D"][i1[r["good"]]] = r["P"][r["good"]]
        tri = np.zeros(n1, bool)
        tri[i1[r["tri"]]] = True
        out["triangulated"] = tri
    return out


def draw_ransac_sets_ref(n_matches, iterations, randint):
    """(:88-101) a second, loop-for-loop statement of the swap-remove draw (for cross-checking the package's)."""
    all_idx = list(range(n_matches))
    sets = [[0] * 8 for _ in range(iterations)]
    for it in range(iterations):
        avail = list(all_idx)
        for j in range(8):
            randi = randint(0, len(avail) - 1)
            sets[it][j] = avail[randi]
            avail[randi] = avail[len(avail) - 1]
            avail.pop()
    return np.array(sets, np.int32).reshape(iterations, 8)
