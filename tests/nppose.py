"""Independent references for PoseOptimization (reference src/CeresOptimizer.cc:275-342; device k_pose_lm, csrc/ba_small_lm.inc).

No GPU and no oracle here, and nothing imports the product package.  Two references, written from the reference's lines:
  * mp_terms / mp_cost: the robust cost and the chi-square gate AT A GIVEN POSE in mpmath (50 digits by default).  Every input is
    converted exactly from its float64 / float32 value, so the only error left is the final rounding of the result to float64.
      - rotation: Eigen's q * v with the quaternion as given, NOT normalised:  v + w (2 qv x v) + qv x (2 qv x v);
      - projection: u = (fx p0 + cx p2) / p2, v = (fy p1 + cy p2) / p2 with p = q * X + t;
      - chi2 = inv_sigma2 (eu^2 + ev^2): what CheckOutlier compares with 5.991 (:227-241); it has no depth test;
      - s = inv_sigma2^2 (eu^2 + ev^2): the squared residual of the cost - the reference's "square-root information" is
        Identity * invSigma2 (:317-320), so the residual is invSigma2 * e;
      - cost = 1/2 sum rho(s), rho(s) = s for s <= 5.991, 2 sqrt(5.991) sqrt(s) - 5.991 above (ceres::HuberLoss(sqrt(5.991)), :296).
  * local_minimum: the local minimiser of the same cost in plain float64 numpy - a hand-written damped Gauss-Newton over the
    6-vector [dt, half-angle delta] applied with EigenQuaternionParameterization's Plus (q+ = [sin|d| / |d| d, cos|d|] (x) q), run
    until the cost stops moving in float64.  It shares no step control with the solver under test: the trust region of the solver
    (and its 1e-6 function tolerance) is what the optimality gap measures."""
import numpy as np
from mpmath import mp, mpf

TH2 = 5.991                                  # chi-square, 2 dof, 95 % (:296, :333)


# ---------------------------------------------------------------- mp: terms and cost at a pose
def mp_terms(K4, pose7, Xw, uv, inv_sigma2, dps=50):
    """-> (p2, chi2, s): three lists of mpf, one entry per observation."""
    K4 = np.asarray(K4); pose7 = np.asarray(pose7, np.float64); Xw = np.asarray(Xw, np.float64).reshape(-1, 3)
    uv = np.asarray(uv, np.float64).reshape(-1, 2); inv_sigma2 = np.asarray(inv_sigma2)
    depth, chi2, s = [], [], []
    with mp.workdps(dps):
        fx, fy, cx, cy = [mpf(float(k)) for k in K4]
        tx, ty, tz, qx, qy, qz, qw = [mpf(float(v)) for v in pose7]
        for i in range(len(Xw)):
            x, y, z = mpf(float(Xw[i, 0])), mpf(float(Xw[i, 1])), mpf(float(Xw[i, 2]))
            ax, ay, az = 2 * (qy * z - qz * y), 2 * (qz * x - qx * z), 2 * (qx * y - qy * x)          # 2 qv x v
            p0 = x + qw * ax + (qy * az - qz * ay) + tx
            p1 = y + qw * ay + (qz * ax - qx * az) + ty
            p2 = z + qw * az + (qx * ay - qy * ax) + tz
            eu = mpf(float(uv[i, 0])) - (fx * p0 + cx * p2) / p2
            ev = mpf(float(uv[i, 1])) - (fy * p1 + cy * p2) / p2
            w = mpf(float(inv_sigma2[i]))
            e2 = eu * eu + ev * ev
            depth.append(p2); chi2.append(w * e2); s.append(w * w * e2)
    return depth, chi2, s


def mp_cost(s_list, dps=50):
    """1/2 sum rho(s) as an mpf."""
    with mp.workdps(dps):
        b = mpf(TH2)                          # the double 5.991, exactly: the threshold the loss is built from
        d = mp.sqrt(b)
        tot = mpf(0)
        for s in s_list:
            tot += s if s <= b else 2 * d * mp.sqrt(s) - b
        return tot / 2


def mp_cost_at(K4, pose7, Xw, uv, inv_sigma2, dps=50):
    return mp_cost(mp_terms(K4, pose7, Xw, uv, inv_sigma2, dps)[2], dps)


def mp_flags(chi2, dps=50):
    """-> (flags uint8, band): chi2 > 5.991, and the smallest |chi2 / 5.991 - 1| over the observations (how close the nearest
    observation sits to the gate)."""
    with mp.workdps(dps):
        b = mpf(TH2)
        flags = np.array([1 if c > b else 0 for c in chi2], np.uint8)
        band = min((abs(c / b - 1) for c in chi2), default=mpf("inf"))
    return flags, float(band)


def rel_dev(value, ref, dps=50):
    """|value - ref| / |ref| of a float64 against an mpf, as a float."""
    with mp.workdps(dps):
        return float(abs(mpf(float(value)) - ref) / abs(ref))


# ---------------------------------------------------------------- float64: the same cost, and its local minimiser
def quat_plus(q, d):
    """EigenQuaternionParameterization::Plus: dq (x) q, dq = [sin|d| / |d| d, cos|d|], q = [x, y, z, w]."""
    q = np.asarray(q, np.float64); d = np.asarray(d, np.float64)
    n = np.sqrt(d @ d)
    if not n > 0.0:
        return q.copy()
    dx, dy, dz = np.sin(n) / n * d
    dw = np.cos(n)
    x, y, z, w = q
    return np.array([dw * x + dx * w + dy * z - dz * y,
                     dw * y - dx * z + dy * w + dz * x,
                     dw * z + dx * y - dy * x + dz * w,
                     dw * w - dx * x - dy * y - dz * z])


def pose_plus(pose7, step):
    pose7 = np.asarray(pose7, np.float64)
    return np.concatenate([pose7[:3] + step[:3], quat_plus(pose7[3:], step[3:])])


def _camera_points(pose7, Xw):
    qv, qw = pose7[3:6], pose7[6]
    a = 2.0 * np.cross(qv, Xw)
    RX = Xw + qw * a + np.cross(qv, a)
    return RX, RX + pose7[:3]


def cost(K4, pose7, Xw, uv, inv_sigma2):
    """The Huber cost in float64 numpy (pairwise sums)."""
    K4 = np.asarray(K4, np.float64); pose7 = np.asarray(pose7, np.float64); w = np.asarray(inv_sigma2, np.float64)
    _, p = _camera_points(pose7, np.asarray(Xw, np.float64))
    eu = uv[:, 0] - (K4[0] * p[:, 0] + K4[2] * p[:, 2]) / p[:, 2]
    ev = uv[:, 1] - (K4[1] * p[:, 1] + K4[3] * p[:, 2]) / p[:, 2]
    s = w * w * (eu * eu + ev * ev)
    rho = np.where(s <= TH2, s, 2.0 * np.sqrt(TH2) * np.sqrt(s) - TH2)
    return 0.5 * float(rho.sum())


def _normal_equations(K4, pose7, Xw, uv, w):
    """cost, gradient and the Gauss-Newton matrix with the loss' first derivative as weight (IRLS), at step 0 of pose7."""
    RX, p = _camera_points(pose7, Xw)
    iz = 1.0 / p[:, 2]
    e = np.stack([uv[:, 0] - (K4[0] * p[:, 0] + K4[2] * p[:, 2]) * iz, uv[:, 1] - (K4[1] * p[:, 1] + K4[3] * p[:, 2]) * iz], 1)
    n = len(Xw)
    Jpi = np.zeros((n, 2, 3))                                            # d pi / d p
    Jpi[:, 0, 0] = K4[0] * iz; Jpi[:, 0, 2] = -K4[0] * p[:, 0] * iz * iz
    Jpi[:, 1, 1] = K4[1] * iz; Jpi[:, 1, 2] = -K4[1] * p[:, 1] * iz * iz
    # d p / d delta = 2 delta x RX = -2 [RX]x delta  (a half-angle vector turns by 2 |delta|)
    S = np.zeros((n, 3, 3))
    S[:, 0, 1] = -RX[:, 2]; S[:, 0, 2] = RX[:, 1]; S[:, 1, 0] = RX[:, 2]; S[:, 1, 2] = -RX[:, 0]; S[:, 2, 0] = -RX[:, 1]; S[:, 2, 1] = RX[:, 0]
    J = -w[:, None, None] * np.concatenate([Jpi, -2.0 * (Jpi @ S)], 2)    # d (w e) / d [t, delta]
    r = w[:, None] * e
    s = (r * r).sum(1)
    big = s > TH2
    rho = np.where(big, 2.0 * np.sqrt(TH2) * np.sqrt(np.where(big, s, 1.0)) - TH2, s)
    rho1 = np.where(big, np.sqrt(TH2) / np.sqrt(np.where(big, s, 1.0)), 1.0)
    g = np.einsum("n,nij,ni->j", rho1, J, r)
    H = np.einsum("n,nij,nik->jk", rho1, J, J)
    return 0.5 * float(rho.sum()), g, H


def local_minimum(K4, pose7, Xw, uv, inv_sigma2, max_iterations=200):
    """Minimises cost() over the 6-vector [dt, half-angle delta], started at 0 (the given pose).  Damped Gauss-Newton: the damping
    grows until a step lowers the cost and shrinks after one that does; it ends when no damping up to 1e12 finds a lower cost, or
    the cost has not moved by more than one part in 1e15 over three accepted steps.
    -> (minimum cost, pose7 at the minimum, step [6] from the given pose composed over the iterations: dt exact, the half-angle
    part the sum of the steps - a first-order figure, for reporting only)."""
    K4 = np.asarray(K4, np.float64); x = np.asarray(pose7, np.float64).copy(); Xw = np.asarray(Xw, np.float64).reshape(-1, 3)
    uv = np.asarray(uv, np.float64).reshape(-1, 2); w = np.asarray(inv_sigma2, np.float64)
    total = np.zeros(6)
    lam = 1e-4
    still = 0
    c = cost(K4, x, Xw, uv, w)
    for _ in range(max_iterations):
        _, g, H = _normal_equations(K4, x, Xw, uv, w)
        if not np.any(g):
            break
        dH = np.maximum(np.diag(H), 1e-300)
        moved = False
        while lam <= 1e12:
            try:
                step = -np.linalg.solve(H + lam * np.diag(dH), g)
            except np.linalg.LinAlgError:
                lam *= 10.0
                continue
            xn = pose_plus(x, step)
            cn = cost(K4, xn, Xw, uv, w)
            if np.isfinite(cn) and cn < c:
                still = still + 1 if c - cn <= 1e-15 * c else 0
                x, c, total, moved = xn, cn, total + step, True
                lam = max(lam * 0.1, 1e-12)
                break
            lam *= 10.0
        if not moved or still >= 3:
            break
    return c, x, total
