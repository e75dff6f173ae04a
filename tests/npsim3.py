"""A high-precision reference of the Sim(3) arithmetic of csrc/sim3_math.h, in mpmath at 50 digits, that does NOT restate the header's
closed forms: W is its power series, exp / log come from mp.sin / mp.cos / mp.atan2 and a linear solve, the group operations are 4x4
matrix algebra, Adj and ad are conjugation and commutators of hat matrices.  Only two things are restated, because they are the
reference's own definitions and not approximations of anything: the truncated series I + ad/2 + ad^2/12 of the essential-graph
Jacobian, and CheckOutlier's matrix-to-quaternion on the SCALED matrix.

Conventions (Sophus): tangent = [upsilon(3), omega(3), sigma]; storage qt7 = [qx, qy, qz, qw, tx, ty, tz] with |q|^2 = scale; a group
element is the 4x4 matrix [[s R, t], [0, 1]].  Every function takes float64 values (or mp values) exactly into mp.  Test infrastructure
only."""
import numpy as np
from mpmath import mp, mpf

DPS = 50
DBL_MIN = 2.2250738585072014e-308


def _v(a):
    return [mpf(float(x)) if not isinstance(x, mpf) else x for x in (a.reshape(-1) if isinstance(a, np.ndarray) else a)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _skew(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def mp_W_coeffs(theta2, sigma):
    """(C, A, B) with W = C I + A Om + B Om^2, from the power series itself: (sigma I + Om)^k = a_k I + b_k Om + c_k Om^2 with
    a' = sigma a, b' = sigma b + a - theta^2 c, c' = sigma c + b  (Om^3 = -theta^2 Om, exactly); each divided by (k + 1)! and summed until
    the terms are below 10^-(dps + 10) of the sums."""
    with mp.workdps(mp.dps + 15):
        a, b, c = mpf(1), mpf(0), mpf(0)
        C, A, B = mpf(0), mpf(0), mpf(0)
        fact = mpf(1)
        tiny = mpf(10) ** (-(mp.dps))
        k = 0
        while True:
            fact *= (k + 1)
            ta, tb, tc = a / fact, b / fact, c / fact
            C += ta; A += tb; B += tc
            if k > 3 and abs(ta) <= tiny * abs(C) and abs(tb) <= tiny * max(abs(A), tiny) and abs(tc) <= tiny * max(abs(B), tiny) and \
                    (k + 2) > 2 * (abs(sigma) + mp.sqrt(theta2)):
                break
            a, b, c = sigma * a, sigma * b + a - theta2 * c, sigma * c + b
            k += 1
            assert k < 2000
        return +C, +A, +B


def mp_W(omega, sigma):
    """W = sum_k (sigma I + [omega]x)^k / (k + 1)!  as a 3x3 mp matrix"""
    with mp.workdps(DPS):
        om = _v(omega); sg = _v([sigma])[0]
        C, A, B = mp_W_coeffs(om[0] ** 2 + om[1] ** 2 + om[2] ** 2, sg)
        Om = _skew(om)
        return C * mp.eye(3) + A * Om + B * (Om * Om)


def mp_W_matrix_series(omega, sigma):
    """the same series summed on the 3x3 matrices themselves (slow; the CPU test pins mp_W to it)"""
    with mp.workdps(DPS + 15):
        om = _v(omega); sg = _v([sigma])[0]
        M = sg * mp.eye(3) + _skew(om)
        P = mp.eye(3); W = mp.zeros(3); fact = mpf(1)
        bound = abs(sg) + mp.sqrt(om[0] ** 2 + om[1] ** 2 + om[2] ** 2)
        for k in range(2000):
            fact *= (k + 1)
            T = P / fact
            W += T
            if k > 3 and (k + 2) > 2 * bound and max(abs(x) for x in T) < mpf(10) ** (-(DPS + 10)):
                break
            P = P * M
        return W


def mat_of(S):
    """qt7 (or an mp 4x4 already) -> the 4x4 matrix [[s R, t], [0, 1]]; s R is quadratic in the scaled quaternion"""
    if isinstance(S, mp.matrix):
        return S
    with mp.workdps(DPS):
        x, y, z, w, tx, ty, tz = _v(S)
        return mp.matrix([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y), tx],
                          [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x), ty],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z, tz],
                          [0, 0, 0, 1]])


def _unit_quat_of_R(R):
    """rotation matrix -> unit quaternion (x, y, z, w), by the largest of the four squared components"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    d = [1 + 2 * R[0, 0] - tr, 1 + 2 * R[1, 1] - tr, 1 + 2 * R[2, 2] - tr, 1 + tr]           # 4 x^2, 4 y^2, 4 z^2, 4 w^2
    i = max(range(4), key=lambda k: d[k])
    r = mp.sqrt(d[i])
    if i == 3:
        q = [(R[2, 1] - R[1, 2]) / (2 * r), (R[0, 2] - R[2, 0]) / (2 * r), (R[1, 0] - R[0, 1]) / (2 * r), r / 2]
    else:
        j, k = (i + 1) % 3, (i + 2) % 3
        q = [0, 0, 0, (R[k, j] - R[j, k]) / (2 * r)]
        q[i] = r / 2; q[j] = (R[j, i] + R[i, j]) / (2 * r); q[k] = (R[k, i] + R[i, k]) / (2 * r)
    return q


def qt_of(S):
    """the scaled quaternion and translation of a group element: a qt7 is taken as it is (its sign kept), a matrix is decomposed"""
    with mp.workdps(DPS):
        if not isinstance(S, mp.matrix):
            return _v(S)
        s = mp.cbrt(mp.det(S[0:3, 0:3]))
        q = _unit_quat_of_R(S[0:3, 0:3] / s)
        r = mp.sqrt(s)
        return [r * c for c in q] + [S[0, 3], S[1, 3], S[2, 3]]


def mp_exp_qt(a):
    """tangent -> qt7 in mp: the unit quaternion from sin / cos of the half angle (its sign is cos(theta / 2)'s, as Sophus has it),
    |q|^2 = e^sigma, t = W upsilon"""
    with mp.workdps(DPS):
        a = _v(a)
        up, om, sg = a[0:3], a[3:6], a[6]
        t2 = om[0] ** 2 + om[1] ** 2 + om[2] ** 2
        th = mp.sqrt(t2)
        if th < mpf("1e-30"):
            fi = mpf(1) / 2 - t2 / 48; fr = 1 - t2 / 8
        else:
            fi = mp.sin(th / 2) / th; fr = mp.cos(th / 2)
        rs = mp.exp(sg / 2)
        C, A, B = mp_W_coeffs(t2, sg)
        c1 = _cross(om, up); c2 = _cross(om, c1)
        t = [C * up[i] + A * c1[i] + B * c2[i] for i in range(3)]
        return [rs * fi * om[0], rs * fi * om[1], rs * fi * om[2], rs * fr] + t


def mp_exp(a):
    return mat_of(mp_exp_qt(a))


def mp_log(S):
    """group element (qt7 or 4x4) -> tangent: sigma = log |q|^2; the canonical rotation vector, |theta| <= pi, from atan2 (a quaternion
    with w == 0 exactly keeps its own axis); upsilon = W^-1 t by a linear solve"""
    with mp.workdps(DPS):
        q = qt_of(S)
        n2q = q[0] ** 2 + q[1] ** 2 + q[2] ** 2 + q[3] ** 2
        sg = mp.log(n2q)
        r = mp.sqrt(n2q)
        u = [c / r for c in q[:4]]
        if u[3] < 0:
            u = [-c for c in u]
        n = mp.sqrt(u[0] ** 2 + u[1] ** 2 + u[2] ** 2)
        if n < mpf("1e-40"):
            f = 2 / u[3]
        else:
            f = 2 * mp.atan2(n, u[3]) / n
        om = [f * u[0], f * u[1], f * u[2]]
        C, A, B = mp_W_coeffs(om[0] ** 2 + om[1] ** 2 + om[2] ** 2, sg)
        Om = _skew(om)
        W = C * mp.eye(3) + A * Om + B * (Om * Om)
        up = mp.lu_solve(W, mp.matrix(q[4:7]))
        return [up[0], up[1], up[2]] + om + [sg]


def mp_mul(A, B):
    with mp.workdps(DPS):
        return mat_of(A) * mat_of(B)


def mp_inverse(S):
    with mp.workdps(DPS):
        return mp.inverse(mat_of(S))


def mp_act(S, p):
    with mp.workdps(DPS):
        M = mat_of(S); p = _v(p)
        return [M[i, 0] * p[0] + M[i, 1] * p[1] + M[i, 2] * p[2] + M[i, 3] for i in range(3)]


def mp_to_pose34(S):
    """Sim3 -> SE3 as the loop-closing write-backs do it: [R | t / s], 12 values row-major"""
    with mp.workdps(DPS):
        M = mat_of(S)
        s = mp.cbrt(mp.det(M[0:3, 0:3]))
        return [M[i, j] / s for i in range(3) for j in range(4)]


def mp_hat(xi):
    xi = _v(xi)
    H = mp.zeros(4)
    H[0:3, 0:3] = _skew(xi[3:6]) + xi[6] * mp.eye(3)
    for i in range(3):
        H[i, 3] = xi[i]
    return H


def mp_vee(H):
    return [H[0, 3], H[1, 3], H[2, 3], (H[2, 1] - H[1, 2]) / 2, (H[0, 2] - H[2, 0]) / 2, (H[1, 0] - H[0, 1]) / 2, (H[0, 0] + H[1, 1] + H[2, 2]) / 3]


def _unit(k):
    return [mpf(1) if i == k else mpf(0) for i in range(7)]


def mp_adj(S):
    """Adj by conjugation: column k = vee(M hat(e_k) M^-1); 7x7 mp matrix"""
    with mp.workdps(DPS):
        M = mat_of(S); Mi = mp.inverse(M)
        A = mp.zeros(7)
        for k in range(7):
            c = mp_vee(M * mp_hat(_unit(k)) * Mi)
            for i in range(7):
                A[i, k] = c[i]
        return A


def mp_ad(xi):
    """ad by commutators: column k = vee([hat(xi), hat(e_k)])"""
    with mp.workdps(DPS):
        X = mp_hat(xi)
        A = mp.zeros(7)
        for k in range(7):
            E = mp_hat(_unit(k))
            c = mp_vee(X * E - E * X)
            for i in range(7):
                A[i, k] = c[i]
        return A


def mp_plus(x, d):
    """Sim3Parameterization::Plus: log(exp(x) exp(d)), d[6] clamped at -20"""
    with mp.workdps(DPS):
        d = _v(d)
        d[6] = max(d[6], mpf(-20))
        return mp_log(mp_exp(x) * mp_exp(d))


def mp_graph_edge(lie_j, lie_i, Sji, jacobian=True):
    """r = log(Sji exp(lie_i) exp(lie_j)^-1) and J_i = (I + ad(r)/2 + ad(r)^2/12) Adj(exp(lie_j)): the truncation is the reference's own
    definition of its Jacobian and is kept.  Returns (r [7], J_i 7x7 mp matrix or None)."""
    with mp.workdps(DPS):
        Sj = mp_exp(lie_j)
        r = mp_log(mat_of(Sji) * mp_exp(lie_i) * mp.inverse(Sj))
        if not jacobian:
            return r, None
        ad = mp_ad(r)
        return r, (mp.eye(7) + ad / 2 + ad * ad / 12) * mp_adj(Sj)


def mp_term(K4, S, P, uv, w, huber):
    """Sim3ErrorTerm with the Huber corrector folded in.  S: the group element the point goes through (exp(x) or its inverse).
    r = sqrt(rho') w (proj(S P) - uv); column k of J = sqrt(rho') w d proj . (hat(e_k) [p; 1]), the derivative under exp(eps e_k) S;
    rho' = max(DBL_MIN, huber / sqrt(s)) past s = |r|^2 > huber^2.  Returns dict(r, J (2x7 lists), rho0, ratio = s / huber^2, linear)."""
    with mp.workdps(DPS):
        fx, fy, cx, cy = _v(K4)
        p = mp_act(S, P)
        u, v = _v(uv)
        w = _v([w])[0]; h = _v([huber])[0]
        r0 = w * (fx * p[0] / p[2] + cx - u); r1 = w * (fy * p[1] / p[2] + cy - v)
        s = r0 * r0 + r1 * r1
        b = h * h
        rho0, rho1 = s, mpf(1)
        lin = s > b
        if lin:
            rr = mp.sqrt(s)
            rho0 = 2 * h * rr - b
            rho1 = max(mpf(DBL_MIN), h / rr)
        sq = mp.sqrt(rho1)
        dp = [[fx / p[2], 0, -fx * p[0] / p[2] ** 2], [0, fy / p[2], -fy * p[1] / p[2] ** 2]]
        ph = mp.matrix([p[0], p[1], p[2], 1])
        J = [[None] * 7, [None] * 7]
        for k in range(7):
            g = mp_hat(_unit(k)) * ph
            for i in range(2):
                J[i][k] = sq * w * (dp[i][0] * g[0] + dp[i][1] * g[1] + dp[i][2] * g[2])
        return dict(r=[sq * r0, sq * r1], J=J, rho0=rho0, ratio=s / b, linear=bool(lin))


def mp_outlier_camera_point(S, P):
    """the camera point of CheckOutlier as the reference feeds it: Eigen::Quaterniond(s R) - the matrix-to-quaternion conversion on the
    SCALED matrix - and Eigen's unit-quaternion rotation formula with that (unnormalised) quaternion, plus t.  Returns (c [3], arm) with
    arm 3 for the trace > 0 branch and 0..2 for the diagonal element the other branch picks."""
    with mp.workdps(DPS):
        M = mat_of(S)
        Pm = _v(P)
        t = M[0, 0] + M[1, 1] + M[2, 2]
        q = [None] * 4
        if t > 0:
            arm = 3
            t = mp.sqrt(t + 1)
            q[3] = t / 2
            t = 1 / (2 * t)
            q[0] = (M[2, 1] - M[1, 2]) * t; q[1] = (M[0, 2] - M[2, 0]) * t; q[2] = (M[1, 0] - M[0, 1]) * t
        else:
            i = 0
            if M[1, 1] > M[0, 0]:
                i = 1
            if M[2, 2] > M[i, i]:
                i = 2
            arm = i
            j = (i + 1) % 3; k = (j + 1) % 3
            t = mp.sqrt(M[i, i] - M[j, j] - M[k, k] + 1)
            q[i] = t / 2
            t = 1 / (2 * t)
            q[3] = (M[k, j] - M[j, k]) * t; q[j] = (M[j, i] + M[i, j]) * t; q[k] = (M[k, i] + M[i, k]) * t
        uu = [2 * c for c in _cross(q[:3], Pm)]
        vv = _cross(q[:3], uu)
        return [Pm[i] + q[3] * uu[i] + vv[i] + M[i, 3] for i in range(3)], arm


def mp_check_outlier(K4, S, P, uv, inv_sigma, thres):
    """chi2 = |uv - proj(c)|^2 inv_sigma > thres at the camera point of mp_outlier_camera_point; inv_sigma is a float32.
    Returns (flag, chi2 / thres, arm)."""
    with mp.workdps(DPS):
        c, arm = mp_outlier_camera_point(S, P)
        fx, fy, cx, cy = _v(K4); u, v = _v(uv)
        eu = u - (fx * c[0] + cx * c[2]) / c[2]; ev = v - (fy * c[1] + cy * c[2]) / c[2]
        chi2 = (eu * eu + ev * ev) * mpf(float(np.float32(inv_sigma)))
        th = _v([thres])[0]
        return int(chi2 > th), chi2 / th, arm


def to_f64(a):
    """mp list / matrix -> float64 array, each value rounded once"""
    if isinstance(a, mp.matrix):
        return np.array([[float(a[i, j]) for j in range(a.cols)] for i in range(a.rows)])
    return np.array([float(x) for x in a])


def err(out, truth):
    """the issue's metric e = max |out - truth| / max(1, max |truth|), the difference taken in mp"""
    with mp.workdps(DPS):
        t = list(truth) if not isinstance(truth, mp.matrix) else [truth[i, j] for i in range(truth.rows) for j in range(truth.cols)]
        o = np.asarray(out, np.float64).reshape(-1)
        assert len(o) == len(t), (len(o), len(t))
        if not np.all(np.isfinite(o)):
            return float("inf")
        d = max(abs(mpf(float(a)) - b) for a, b in zip(o, t))
        return float(d / max(mpf(1), max(abs(b) for b in t)))
