"""Reference side of the 32 x 32 diagonal factor (diag_factor_invert_nw, csrc/ba_cholesky.inc): X = L^-1 with D = L L^T.

No GPU here.  Three independent computations of X and the inputs they are compared on:
  * mp_factor_inverse: Cholesky + inverse of the factor in mpmath (60 digits by default) - the truth the metrics are taken against;
  * lapack_factor_inverse: np.linalg.cholesky (dpotrf) + dtrtri in float64 - the BASELINE: what a float64 routine owes on a block;
  * restated_factor_inverse: the kernel's SCHEME in plain float64 (right-looking, square-root-free, multiplier = entry x (1 / d),
    forward substitution of the identity with the unit factor, rows scaled by 1 / sqrt(d)).  Not bit-exact to the kernel - the
    hardware reciprocal estimates cannot be reproduced on a CPU - it shows that a correct implementation of the scheme stays
    inside the acceptance cap.
Metrics (mp arithmetic on the float64 X):  residual = max |X D X^T - I|,  forward error = max |X - X_mp| / max |X_mp|.
Acceptance rule: per class, max over the class of the metric <= CAP x the same maximum for LAPACK, for both metrics.
Everything is read from the LOWER triangle of a block (what the kernel and dpotrf read)."""
import os
import subprocess

import mpmath
import numpy as np
import scipy.linalg.lapack as _lapack
from mpmath import libmp, mp, mpf

NB = 32
EPS = 2.0 ** -52
CAP = 4.0                                   # twice the largest class-maximum ratio two correct float64 algorithms showed against each other (1.9)
ACCURACY_CLASSES = ("W", "C2", "C6", "C10", "C13", "G", "J", "P")
NEVER_FLAGGED_CLASSES = ("W", "C2", "C6", "C10", "J", "P")
N_DELTAS = (-1e-8, -1e-12, -1e-15, 0.0, 1e-17, 1e-15, 1e-13, 1e-10)
N_THRESHOLD = 1e3 * NB * EPS                # |lambda_min| / lambda_max beyond which class N's flag is decided
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the hook library (compile only; loading it needs a GPU) ----------------------------------------------------------------------
def hook_build_command(target, defines=("-DORBHIP_TEST_HOOKS",)):
    """The product's compiler and flags (__graft_entry__) plus the define, on the two sources that hold the BA solver."""
    import __graft_entry__ as g
    srcs = [os.path.join(g.CSRC, f) for f in ("ba_solver.hip", "capi_common.hip")]
    return [g.HIPCC] + list(g.HIPFLAGS) + list(defines) + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", str(target)] + srcs


def build_hook_library(target, defines=("-DORBHIP_TEST_HOOKS",), timeout=900):
    subprocess.run(hook_build_command(target, defines), check=True, timeout=timeout)
    return str(target)


# ---- mp reference -------------------------------------------------------------------------------------------------------------
def _sym_lower(A):
    L = np.tril(np.asarray(A, np.float64))
    return np.ascontiguousarray(L + np.tril(L, -1).T)


def mp_factor_inverse(A, dps=60):
    """X = L^-1 (rows of mpf, lower triangle; zeros above) of the block's lower triangle; ValueError at a non-positive pivot."""
    n = A.shape[0]
    with mp.workdps(dps):
        a = [[mpf(float(A[i, j])) for j in range(i + 1)] for i in range(n)]
        L = [[mpf(0)] * n for _ in range(n)]
        for j in range(n):
            Lj = L[j]
            s = a[j][j]
            for k in range(j):
                s -= Lj[k] * Lj[k]
            if not s > 0:
                raise ValueError("non-positive pivot %d" % j)
            d = mp.sqrt(s)
            Lj[j] = d
            for i in range(j + 1, n):
                Li = L[i]
                t = a[i][j]
                for k in range(j):
                    t -= Li[k] * Lj[k]
                Li[j] = t / d
        X = [[mpf(0)] * n for _ in range(n)]
        for c in range(n):
            X[c][c] = 1 / L[c][c]
            for i in range(c + 1, n):
                Li = L[i]
                t = mpf(0)
                for k in range(c, i):
                    t -= Li[k] * X[k][c]
                X[i][c] = t / Li[i]
        return X


def mp_ldl_pivots(A, dps=60):
    """The pivots d_j of the square-root-free elimination in mp (it goes on through negative pivots and stops at an exact zero)."""
    n = A.shape[0]
    with mp.workdps(dps):
        a = [[mpf(float(A[max(i, j), min(i, j)])) for j in range(n)] for i in range(n)]
        piv = []
        for j in range(n):
            d = a[j][j]
            piv.append(d)
            if d == 0:
                break
            for i in range(j + 1, n):
                m = a[i][j] / d
                for k in range(j + 1, i + 1):
                    a[i][k] -= m * a[k][j]
        return piv


def mp_first_bad_pivot(A, dps=60):
    for j, d in enumerate(mp_ldl_pivots(A, dps)):
        if not d > 0:
            return j
    return None


def mp_spectrum(A, dps=50):
    """(lambda_min, lambda_max) of the symmetric matrix the lower triangle defines, in mp."""
    with mp.workdps(dps):
        ev = mp.eigsy(mp.matrix(_sym_lower(A).tolist()), eigvals_only=True)
        ev = [ev[i] for i in range(len(ev))]
        return min(ev), max(ev)


def residual(X, A, dps=60):
    """max |X A X^T - I| with the product formed in mp from the float64 X (any X: nothing assumes it is triangular)."""
    n = A.shape[0]
    X = np.asarray(X, np.float64)
    if not np.isfinite(X).all():
        return float("inf")
    with mp.workdps(dps):
        a = [[mpf(float(A[max(i, j), min(i, j)])) for j in range(n)] for i in range(n)]
        nz = [[k for k in range(n) if X[i, k] != 0.0] for i in range(n)]
        x = [[mpf(float(X[i, k])) for k in range(n)] for i in range(n)]
        worst = mpf(0)
        for i in range(n):
            xi = x[i]
            y = []                                              # row i of X A
            for k in range(n):
                s = mpf(0)
                for l in nz[i]:
                    s += xi[l] * a[l][k]
                y.append(s)
            for j in range(i + 1):                              # (X A X^T is symmetric)
                xj = x[j]
                s = mpf(-1 if i == j else 0)
                for k in nz[j]:
                    s += y[k] * xj[k]
                if abs(s) > worst:
                    worst = abs(s)
        return float(worst)


def forward_error(X, Xmp, dps=60):
    """max |X - X_mp| / max |X_mp| over the whole block (the entries above the diagonal count: X_mp is zero there)."""
    n = len(Xmp)
    X = np.asarray(X, np.float64)
    if not np.isfinite(X).all():
        return float("inf")
    with mp.workdps(dps):
        num = mpf(0)
        den = mpf(0)
        for i in range(n):
            for j in range(n):
                d = abs(mpf(float(X[i, j])) - Xmp[i][j])
                if d > num:
                    num = d
                if abs(Xmp[i][j]) > den:
                    den = abs(Xmp[i][j])
        return float(num / den)


def mp_to_float(Xmp):
    return np.array([[float(v) for v in row] for row in Xmp])


# ---- float64: the baseline and the restatement -----------------------------------------------------------------------------------
def lapack_factor_inverse(A):
    """dpotrf + dtrtri.  np.linalg.LinAlgError when dpotrf meets a non-positive pivot."""
    L = np.linalg.cholesky(_sym_lower(A))
    X, info = _lapack.dtrtri(L, lower=1)
    if info != 0:
        raise np.linalg.LinAlgError("dtrtri: %d" % info)
    return np.tril(X)


def restated_factor_inverse(A):
    """The kernel's scheme in plain float64 (see the module docstring).  Returns (X, bad): bad when a pivot is not positive and finite."""
    n = A.shape[0]
    a = _sym_lower(A)
    z = np.eye(n)
    d = np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n):
            d[j] = a[j, j]
            w = 1.0 / d[j]
            m = a[j + 1:, j] * w
            a[j + 1:, j + 1:] -= np.outer(m, a[j + 1:, j])
            z[j + 1:, :] -= np.outer(m, z[j, :])
        X = z * (1.0 / np.sqrt(d))[:, None]
    bad = not bool(np.all(np.isfinite(d) & (d > 0)))
    return np.tril(X), bad


# ---- references per block, cached for the session (mp work is the cost of these tests) ---------------------------------------
_REF = {}
_RES = {}


def reference(A):
    """{'Xmp', 'Xlapack', 'lapack_residual', 'lapack_forward'} of a block; Xmp is None when mp meets a non-positive pivot, the
    LAPACK entries are None when dpotrf fails."""
    key = A.tobytes()
    if key not in _REF:
        r = {"Xmp": None, "Xlapack": None, "lapack_residual": None, "lapack_forward": None}
        try:
            r["Xmp"] = mp_factor_inverse(A)
        except ValueError:
            pass
        try:
            r["Xlapack"] = lapack_factor_inverse(A)
            r["lapack_residual"] = cached_residual(r["Xlapack"], A)
            if r["Xmp"] is not None:
                r["lapack_forward"] = forward_error(r["Xlapack"], r["Xmp"])
        except np.linalg.LinAlgError:
            pass
        _REF[key] = r
    return _REF[key]


def cached_residual(X, A):
    key = (np.ascontiguousarray(X).tobytes(), A.tobytes())
    if key not in _RES:
        _RES[key] = residual(X, A)
    return _RES[key]


def class_errors(blocks, Xs):
    """(max residual, max forward error) over a class for the given inverses, and the same pair for LAPACK on the same blocks."""
    res = fwd = lres = lfwd = 0.0
    for A, X in zip(blocks, Xs):
        ref = reference(A)
        assert ref["Xmp"] is not None and ref["Xlapack"] is not None
        res = max(res, cached_residual(X, A))
        fwd = max(fwd, forward_error(X, ref["Xmp"]))
        lres = max(lres, ref["lapack_residual"])
        lfwd = max(lfwd, ref["lapack_forward"])
    return (res, fwd), (lres, lfwd)


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------
def _orth(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def _spectrum_block(rng, cond, n=NB):
    lam = cond ** (-np.arange(n) / max(n - 1, 1))
    q = _orth(rng, n)
    return _sym_lower((q * lam) @ q.T)


def _wishart(rng, sigma):
    M = rng.standard_normal((NB, 48))
    return _sym_lower(M @ M.T + sigma * np.eye(NB))


def _gen_W(rng, count=40):
    return [_wishart(rng, 0.5 if i % 2 == 0 else 1e-6) for i in range(count)]


def _gen_C(cond):
    def gen(rng, count=40):
        return [_spectrum_block(rng, cond) for _ in range(count)]
    return gen


def _gen_G(rng, count=40):
    out = []
    for _ in range(count):
        sc = 10.0 ** rng.uniform(-6, 6, NB)
        out.append(_sym_lower(_spectrum_block(rng, 1e3) * sc[:, None] * sc[None, :]))
    return out


def _gen_J(rng, count=40):
    out = []
    for _ in range(count):
        A = _spectrum_block(rng, 1e8)
        s = 1.0 / np.sqrt(np.diag(A))
        A = _sym_lower(A * s[:, None] * s[None, :])
        A[np.arange(NB), np.arange(NB)] = 1.0
        out.append(A)
    return out


def _gen_P(rng):
    out = []
    for k in range(1, NB):
        A = np.eye(NB)
        A[:k, :k] = _spectrum_block(rng, 1e4, k) * 10.0 ** rng.uniform(-2, 2)
        out.append(_sym_lower(A))
    return out


def _gen_D(rng):
    e_ramp = 2 * np.round(np.linspace(-250, 250, NB)).astype(int)
    e_alt = np.where(np.arange(NB) % 2 == 0, 500, -500)
    e_rand = 2 * rng.integers(-250, 251, NB)
    out = [np.eye(NB), np.diag(np.ldexp(1.0, e_ramp)), np.diag(np.ldexp(1.0, e_ramp[::-1])), np.diag(np.ldexp(1.0, e_alt)),
           np.diag(np.ldexp(1.0, e_rand)), np.diag(np.full(NB, 2.0 ** 500)), np.diag(np.full(NB, 2.0 ** -500)), np.diag(np.full(NB, 4.0)),
           np.diag(rng.uniform(0.5, 2.0, NB)), np.diag(10.0 ** rng.uniform(-100, 100, NB))]
    return [np.ascontiguousarray(a) for a in out]


def diagonal_expected(A):
    """The exact X of a diagonal block whose entries are even powers of two (None for any other block)."""
    d = np.diag(A)
    if np.count_nonzero(A - np.diag(d)) or not np.all(d > 0):
        return None
    m, e = np.frexp(d)                                          # d = m 2^e, m in [0.5, 1): a power of two has m = 0.5, d = 2^(e - 1)
    if not np.all(m == 0.5) or np.any((e - 1) % 2):
        return None
    return np.diag(np.ldexp(1.0, -((e - 1) // 2)))


def _gen_N(rng, nbase=3):
    out = []
    for _ in range(nbase):
        B = rng.standard_normal((NB, NB - 1))
        G = B @ B.T
        nrm2 = np.linalg.norm(B, 2) ** 2
        for delta in N_DELTAS:
            out.append(_sym_lower(G + delta * nrm2 * np.eye(NB)))
    return out


def _gen_S(rng):
    """Block p: a well-conditioned SPD block whose entry (p, p) is lowered until pivot p is -A(p, p) / 2 (the pivots before it stay)."""
    out = []
    for p in range(NB):
        A = _wishart(rng, 0.5)
        a = A.copy()
        for j in range(p):                                      # float64 elimination up to column p - 1: pivot p to ~1e-15 relative
            m = a[j + 1:, j] / a[j, j]
            a[j + 1:, j + 1:] -= np.outer(m, a[j + 1:, j])
        A[p, p] -= a[p, p] + 0.5 * A[p, p]
        out.append(A)
    return out


X_VALUES = (float("nan"), float("inf"), float("-inf"))
# (row, column): on the diagonal and below it, a column in every wave's range for NW = 2 ([0, 16), [16, 32)) and NW = 4 (eight columns
# each), the first and last column, and both sides of the boundaries
X_POSITIONS = ((0, 0), (1, 1), (9, 9), (17, 17), (25, 25), (31, 31), (15, 15), (16, 16),
               (6, 2), (13, 10), (22, 18), (31, 26), (31, 0), (31, 30), (16, 15), (8, 7), (24, 23))


def _gen_X(rng):
    out = []
    for v in X_VALUES:
        for (r, c) in X_POSITIONS:
            A = _wishart(rng, 0.5)
            A[r, c] = v
            A[c, r] = v
            out.append(A)
    return out


_GENERATORS = {"W": (101, _gen_W), "C2": (102, _gen_C(1e2)), "C6": (106, _gen_C(1e6)), "C10": (110, _gen_C(1e10)), "C13": (113, _gen_C(1e13)),
               "G": (120, _gen_G), "J": (130, _gen_J), "P": (140, _gen_P), "D": (150, _gen_D), "N": (160, _gen_N), "S": (170, _gen_S),
               "X": (180, _gen_X)}
CLASS_CONDITION = {"C2": 1e2, "C6": 1e6, "C10": 1e10, "C13": 1e13}
ALL_CLASSES = tuple(_GENERATORS)
_BLOCKS = {}


def blocks(cls):
    """The fixed list of blocks of a class (32 x 32 float64, C-contiguous, symmetric)."""
    if cls not in _BLOCKS:
        seed, gen = _GENERATORS[cls]
        _BLOCKS[cls] = [np.ascontiguousarray(a, dtype=np.float64) for a in gen(np.random.default_rng(seed))]
    return [a.copy() for a in _BLOCKS[cls]]


def back_to_back_sequence():
    """72 blocks across W, G, P and D, interleaved so that consecutive blocks differ wildly in scale."""
    W, G, P, D = blocks("W"), blocks("G"), blocks("P"), blocks("D")
    out = []
    for i in range(18):
        out += [W[i], D[i % len(D)], G[i], P[(5 * i) % len(P)]]
    return out


# ---- the scalar maps ------------------------------------------------------------------------------------------------------------
SCALAR_EMIN, SCALAR_EMAX = -1021, 1021


def scalar_inputs(seed=7, n_random=10 ** 6):
    """Log-uniform doubles over [2^-1021, 2^1021], every power of two in that range, its 8 neighbours on each side, and the
    mantissas of all ones; sorted, without repetitions."""
    rng = np.random.default_rng(seed)
    e = rng.integers(SCALAR_EMIN, SCALAR_EMAX, n_random)
    x = np.ldexp(1.0 + rng.random(n_random), e)                                       # uniform exponent, uniform mantissa
    p2 = np.ldexp(1.0, np.arange(SCALAR_EMIN, SCALAR_EMAX + 1))
    bits = p2.view(np.int64)
    nb = np.concatenate([(bits + k).view(np.float64) for k in range(-8, 9)])
    ones = np.ldexp(2.0 - 2.0 ** -52, np.arange(SCALAR_EMIN, SCALAR_EMAX))
    return np.unique(np.concatenate([x, p2, nb, ones]))


def recip_rn(x):
    """1 / x correctly rounded (round to nearest even), element-wise, through mpmath's integer arithmetic."""
    ff, div, tf, one = libmp.from_float, libmp.mpf_div, libmp.to_float, libmp.fone
    return np.array([tf(div(one, ff(float(v)), 53, "n")) for v in x])


def rsqrt_rn(x):
    """1 / sqrt(x) rounded to nearest from a 200-bit value (1 / sqrt(x) is a double only for x = 4^k and never a midpoint of two
    doubles, so an irrational value within 2^-200 of a midpoint is the only way this could differ from the correctly rounded one)."""
    ff, div, sq, tf, one = libmp.from_float, libmp.mpf_div, libmp.mpf_sqrt, libmp.to_float, libmp.fone
    return np.array([tf(div(one, sq(ff(float(v)), 200, "n"), 53, "n")) for v in x])


def ulp_distance(a, b):
    """Number of doubles between a and b, element-wise (positive finite values)."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    assert np.all(np.isfinite(a) & (a > 0)) and np.all(np.isfinite(b) & (b > 0))
    return np.abs(a.view(np.int64) - b.view(np.int64))
