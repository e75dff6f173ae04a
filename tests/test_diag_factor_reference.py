"""CPU side of the diagonal-factor tests (tests/npfactor.py): the mp reference is self-consistent, the seeded generators produce the
classes they claim, and the ACCEPTANCE RULE of tests/test_gpu_diag_factor.py - per class, max error <= 4 x LAPACK's - is met by a
plain float64 restatement of the kernel's scheme, i.e. the cap is one a correct implementation stays inside.

Restatement against LAPACK, class maxima, measured here (restated / LAPACK; mp reference at 60 digits):
    class     residual   forward error
    W           0.90        1.04
    C2          1.65        1.38
    C6          0.75        0.58
    C10         1.05        1.21
    C13         0.50        0.64
    G           1.18        0.69
    J           0.43        0.52
    P           0.30        0.43
"""
import numpy as np
import pytest
from mpmath import mp, mpf

from tests import npfactor as F

NB = F.NB


def _mp_residual_of_mp(Xmp, A, dps):
    with mp.workdps(dps):
        X = mp.matrix(Xmp)
        D = mp.matrix(F._sym_lower(A).tolist())
        R = X * D * X.T - mp.eye(NB)
        return max(abs(R[i, j]) for i in range(NB) for j in range(NB))


@pytest.mark.parametrize("cls", ["W", "C6", "G", "P"])
def test_mp_reference_is_self_consistent(cls):
    for A in F.blocks(cls)[:2]:
        X50, X100 = F.mp_factor_inverse(A, 50), F.mp_factor_inverse(A, 100)
        with mp.workdps(100):
            scale = max(abs(v) for row in X100 for v in row)
            diff = max(abs(X50[i][j] - X100[i][j]) for i in range(NB) for j in range(NB)) / scale
            assert diff < mpf("1e-40"), diff
            assert all(X100[i][j] == 0 for i in range(NB) for j in range(i + 1, NB))
        assert _mp_residual_of_mp(X100, A, 100) < mpf("1e-40")
        # the float64 metrics see the same thing: the rounded mp inverse is as good as float64 gets
        Xf = F.mp_to_float(X100)
        assert F.forward_error(Xf, X100) <= 2.0 ** -53
        piv = F.mp_ldl_pivots(A)
        with mp.workdps(60):                                     # the two mp eliminations agree: X(j, j) = 1 / sqrt(d_j)
            assert all(abs(X100[j][j] ** 2 * piv[j] - 1) < mpf("1e-40") for j in range(NB))


def test_generators_are_deterministic():
    first = {c: [a.tobytes() for a in F.blocks(c)] for c in F.ALL_CLASSES}
    F._BLOCKS.clear()
    for c in F.ALL_CLASSES:
        assert [a.tobytes() for a in F.blocks(c)] == first[c], c
    assert F.scalar_inputs().tobytes() == F.scalar_inputs().tobytes()
    s1, s2 = F.back_to_back_sequence(), F.back_to_back_sequence()
    assert len(s1) >= 64 and all(a.tobytes() == b.tobytes() for a, b in zip(s1, s2))


def test_class_sizes_and_shapes():
    for c in ("W", "C2", "C6", "C10", "C13", "G", "J"):
        assert len(F.blocks(c)) >= 40, c
    assert len(F.blocks("P")) == 31 and len(F.blocks("S")) == 32 and len(F.blocks("N")) == 3 * len(F.N_DELTAS)
    for c in F.ALL_CLASSES:
        for A in F.blocks(c):
            assert A.shape == (NB, NB) and A.dtype == np.float64 and A.flags.c_contiguous
            assert np.array_equal(A, A.T, equal_nan=True), c
            if c != "X":
                assert np.isfinite(A).all(), c


def _cond(A):
    ev = np.linalg.eigvalsh(A)                                   # absolute error ~ NB eps lambda_max: 7e-15 relative to lambda_max
    return ev[-1] / ev[0], ev


@pytest.mark.parametrize("cls", ["C2", "C6", "C10", "C13"])
def test_prescribed_condition_numbers(cls):
    target = F.CLASS_CONDITION[cls]
    for A in F.blocks(cls):
        c, ev = _cond(A)
        assert ev[0] > 0 and 0.5 * target < c < 2.0 * target, (cls, c)
    for A in F.blocks(cls)[:2]:                                  # and by the mp spectrum of the ROUNDED block
        lo, hi = F.mp_spectrum(A)
        assert lo > 0 and 0.8 * target < float(hi / lo) < 1.25 * target, (cls, float(hi / lo))


def test_wishart_graded_and_jacobi_classes():
    for i, A in enumerate(F.blocks("W")):
        c, ev = _cond(A)
        assert ev[0] >= (0.5 if i % 2 == 0 else 1e-6) * (1 - 1e-6)          # M M^T + sigma I
        assert c < 1e4                                                       # (32 x 48 factors: M M^T alone is well conditioned)
    for A in F.blocks("G"):
        d = np.diag(A)
        assert np.log10(d.max() / d.min()) > 14                              # +-6 decades on rows AND columns: 24 on the diagonal at most
        s = 1.0 / np.sqrt(d)
        c, ev = _cond(A * s[:, None] * s[None, :])                           # the grading taken out again
        assert ev[0] > 0 and 1e3 / NB < c < 1e3 * NB, c
    for A in F.blocks("J"):
        assert np.all(np.diag(A) == 1.0)
        c, ev = _cond(A)
        assert ev[0] > 0 and 1e7 < c < 1e9, c


def test_padded_and_diagonal_classes():
    for k, A in zip(range(1, NB), F.blocks("P")):
        assert np.array_equal(A[k:, k:], np.eye(NB - k)) and not A[k:, :k].any() and not A[:k, k:].any()
        assert np.linalg.eigvalsh(A[:k, :k])[0] > 0
        assert k == 1 or np.count_nonzero(np.tril(A[:k, :k], -1)) == k * (k - 1) // 2
    D = F.blocks("D")
    assert any(np.array_equal(A, np.eye(NB)) for A in D)
    exps = []
    for A in D:
        assert not (A - np.diag(np.diag(A))).any() and np.all(np.diag(A) > 0)
        E = F.diagonal_expected(A)
        if E is not None:
            assert np.array_equal(E @ A @ E, np.eye(NB))                     # exact: powers of two
            exps += list(np.frexp(np.diag(A))[1] - 1)
    assert min(exps) == -500 and max(exps) == 500 and all(e % 2 == 0 for e in exps)
    assert sum(F.diagonal_expected(A) is None for A in D) >= 2               # and diagonals that are not powers of two


def test_safely_positive_definite_classes():
    """The classes whose flag must stay clear: lambda_min > 1e3 x 32 eps lambda_max (eigvalsh's own error is 1e3 x smaller)."""
    for cls in F.NEVER_FLAGGED_CLASSES:
        for A in F.blocks(cls):
            ev = np.linalg.eigvalsh(A)
            assert ev[0] > 10 * F.N_THRESHOLD * ev[-1], (cls, ev[0] / ev[-1])
            assert F.reference(A)["Xmp"] is not None


def test_near_singular_ladder():
    blks = F.blocks("N")
    for i, A in enumerate(blks):
        delta = F.N_DELTAS[i % len(F.N_DELTAS)]
        lo, hi = F.mp_spectrum(A)
        assert abs(float(lo / hi) - delta) < 2e-14, (delta, float(lo / hi))    # rank 31 + delta |B|^2 I, rounded to float64
        ev = np.linalg.eigvalsh(A)
        assert ev[1] > 1e-6 * ev[-1]                                             # exactly one eigenvalue near the thresholds (7e-12)
    ratios = [float(lo / hi) for lo, hi in (F.mp_spectrum(A) for A in blks[:len(F.N_DELTAS)])]
    assert any(r < -F.N_THRESHOLD for r in ratios) and any(r > F.N_THRESHOLD for r in ratios) and any(abs(r) < F.N_THRESHOLD for r in ratios)


def test_forced_pivot_class_hits_every_position():
    for p, A in enumerate(F.blocks("S")):
        piv = F.mp_ldl_pivots(A)
        assert F.mp_first_bad_pivot(A) == p
        assert float(piv[p]) < -0.1 * np.abs(np.diag(A)).max() and all(d > 0 for d in piv[:p])      # clearly negative: -A(p, p) / 2 before the change
        with pytest.raises(np.linalg.LinAlgError):
            F.lapack_factor_inverse(A)
        assert F.restated_factor_inverse(A)[1]
        assert F.reference(A)["Xmp"] is None


def test_non_finite_class_positions():
    blks = F.blocks("X")
    assert len(blks) == len(F.X_VALUES) * len(F.X_POSITIONS)
    cols = [c for _, c in F.X_POSITIONS]
    for nw in (2, 4):
        cb = NB // nw
        for q in range(nw):
            assert any(r == c and q * cb <= c < (q + 1) * cb for r, c in F.X_POSITIONS), (nw, q)      # on the diagonal
            assert any(r > c and q * cb <= c < (q + 1) * cb for r, c in F.X_POSITIONS), (nw, q)       # and below it
    assert 0 in cols and NB - 1 in cols
    i = 0
    for v in F.X_VALUES:
        for (r, c) in F.X_POSITIONS:
            A = blks[i]; i += 1
            bad = ~np.isfinite(A)
            assert bad.sum() == (1 if r == c else 2) and bad[r, c] and bad[c, r]
            assert (np.isnan(A[r, c]) and np.isnan(v)) or A[r, c] == v
            assert F.restated_factor_inverse(A)[1]               # the scheme itself reports every one of them


# ---- the cap holds for the reference alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", F.ACCURACY_CLASSES)
def test_restated_scheme_meets_the_acceptance_rule(cls):
    blks = F.blocks(cls)
    Xs = []
    for A in blks:
        X, bad = F.restated_factor_inverse(A)
        assert not bad and not np.triu(X, 1).any()
        Xs.append(X)
    (res, fwd), (lres, lfwd) = F.class_errors(blks, Xs)
    print("%-4s restated / LAPACK: residual %.3e / %.3e = %.2f, forward %.3e / %.3e = %.2f" % (cls, res, lres, res / lres, fwd, lfwd, fwd / lfwd))
    assert lres > 0 and lfwd > 0
    assert res <= F.CAP * lres, (cls, res, lres)
    assert fwd <= F.CAP * lfwd, (cls, fwd, lfwd)


def test_metrics_see_a_degraded_multiplier():
    """A multiplier good to 2^-40 only (what a missing correction step of the reciprocal leaves) lands far beyond the cap on a
    well-conditioned class: the rule has teeth."""
    blks = F.blocks("C2")[:8]
    Xs = []
    for A in blks:
        n = NB
        a = F._sym_lower(A); z = np.eye(n); d = np.zeros(n)
        for j in range(n):
            d[j] = a[j, j]
            w = (1.0 / d[j]) * (1.0 + 2.0 ** -40)
            m = a[j + 1:, j] * w
            a[j + 1:, j + 1:] -= np.outer(m, a[j + 1:, j])
            z[j + 1:, :] -= np.outer(m, z[j, :])
        Xs.append(np.tril(z / np.sqrt(d)[:, None]))
    (res, fwd), (lres, lfwd) = F.class_errors(blks, Xs)
    assert res > 100 * F.CAP * lres and fwd > 100 * F.CAP * lfwd


# ---- the scalar references -----------------------------------------------------------------------------------------------------
def test_scalar_inputs_cover_what_they_claim():
    x = F.scalar_inputs()
    assert len(x) >= 10 ** 6 and np.all(np.diff(x) > 0)
    assert x[0] >= 2.0 ** -1022 and x[-1] <= 2.0 ** 1022
    p2 = np.ldexp(1.0, np.arange(F.SCALAR_EMIN, F.SCALAR_EMAX + 1))
    have = set(x.view(np.int64).tolist())
    bits = p2.view(np.int64)
    for k in range(-8, 9):
        assert set((bits + k).tolist()) <= have, k
    ones = np.ldexp(2.0 - 2.0 ** -52, np.arange(F.SCALAR_EMIN, F.SCALAR_EMAX))
    assert np.all((ones.view(np.int64) & ((1 << 52) - 1)) == (1 << 52) - 1) and set(ones.view(np.int64).tolist()) <= have
    e = np.frexp(x)[1]
    assert np.histogram(e, bins=16)[0].min() > 50000             # log-uniform: every sixteenth of the exponent range is populated


def test_scalar_references_are_correctly_rounded():
    x = F.scalar_inputs()
    sub = np.concatenate([x[::97], np.ldexp(1.0, np.arange(-1020, 1021, 2))])
    r = F.recip_rn(sub)
    assert np.array_equal(r, 1.0 / sub)                          # IEEE division IS the correctly rounded reciprocal
    y = F.rsqrt_rn(sub)
    assert F.ulp_distance(y, 1.0 / np.sqrt(sub)).max() <= 1      # two roundings against one
    with mp.workdps(80):                                         # against mpmath's own rounding on a few
        for v, yy in list(zip(sub, y))[::503]:
            assert float(1 / mp.sqrt(mpf(float(v)))) == yy
    p = np.ldexp(1.0, np.arange(-1020, 1021, 2))
    assert np.array_equal(F.rsqrt_rn(p), np.ldexp(1.0, -np.arange(-1020, 1021, 2) // 2))
    assert F.ulp_distance(np.array([1.0, 2.0]), np.array([1.0 + 2.0 ** -52, 2.0 - 2.0 ** -51])).tolist() == [1, 2]
