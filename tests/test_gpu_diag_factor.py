"""The 32 x 32 diagonal factor of every BA solve (diag_factor_invert_nw<NW>, csrc/ba_cholesky.inc: X = L^-1, D = L L^T) against a
high-precision reference, through the test hooks of a library built here with -DORBHIP_TEST_HOOKS (the product's compiler and flags).

What is asserted (tests/npfactor.py holds the mp reference, the LAPACK baseline, the metrics and the seeded inputs):
  * accuracy: per class, max residual |X D X^T - I| and max forward error are within CAP = 4 x LAPACK's on the same blocks, every NW;
  * the scalar maps: piv_recip's w and rsqrt_cubic within 1 ulp of the correctly rounded value, exact on powers of two;
  * structure: exact zeros above the diagonal, diagonal blocks give exactly diagonal X, NW = 1 / 2 / 4 and repeated runs give the same
    bytes and flags, different blocks factored back to back by one workgroup (k_chol_wg's case) give what they give one at a time;
  * flags: raised for a non-positive pivot at every position and for NaN / Inf, clear on safely positive definite blocks.
Every hook call runs in a child process under a timeout; after a timeout, an abort or a fault nothing more is started on the GPU.

MEASURED on an MI355X: MEASURED_RATIOS and MEASURED_ULP below (records; the caps asserted are the ones above, not these).

NaN entries: a flagged block's inverse is garbage by contract, and when the input itself holds a NaN or an Inf the garbage holds NaNs.
IEEE 754 leaves the sign and payload of a NaN result open, and which operand's NaN an fma passes on (the multiplier's arrives negated)
follows the operand order the compiler picked for each NW instantiation: on the MI355X the forms differ in the SIGN BIT of some NaN
entries of class X (first seen: NW = 2 against NW = 1, byte 519 of the class, 0x7f against 0xff).  The comparison between the forms
therefore asks for a NaN wherever the other form has a NaN and for identical bytes in every other entry; for a block whose flag is
clear (no NaN: asserted) that IS the byte comparison.  Runs of the SAME form are compared by their raw bytes, NaNs included."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import npfactor as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = F.NB
NWS = (1, 2, 4)
BUILD_TIMEOUT = 1200            # seconds; the build took 32 s cross-compiled
CALL_TIMEOUT = 180              # seconds per child process (a few hundred factors of microseconds each + the runtime's start)

# class: (residual ratio, forward-error ratio), kernel / LAPACK, class maxima, identical for NW = 1, 2, 4 (the forms agree bit for bit)
MEASURED_RATIOS = {"W": (0.77, 1.53), "C2": (2.04, 1.56), "C6": (0.50, 0.45), "C10": (0.88, 0.78), "C13": (0.51, 0.48), "G": (0.58, 0.51),
                   "J": (0.45, 0.43), "P": (0.22, 0.47)}
# maximum distance in ulps from the correctly rounded value over tests/npfactor.py::scalar_inputs (1 034 731 doubles)
# piv_recip's w: the correctly rounded reciprocal on every input; rsqrt_cubic: off by one ulp on 143 211 inputs (13.8 %), never by two
MEASURED_ULP = {"piv_recip_w": 0, "rsqrt_cubic": 1}
ULP_BOUND = {"piv_recip_w": 1, "rsqrt_cubic": 1}


class _Hook:
    """The hook library and the results of the calls made through it (cached: the tests share them)."""

    def __init__(self, lib, tmp):
        self.lib, self.tmp, self.dead, self.n, self.cache = lib, tmp, None, 0, {}

    def _child(self, **job):
        if self.dead:
            pytest.fail("not started: an earlier GPU call ended badly (%s)" % self.dead)
        self.n += 1
        src, dst = os.path.join(self.tmp, "job%d.npz" % self.n), os.path.join(self.tmp, "out%d.npz" % self.n)
        np.savez(src, **job)
        cmd = [sys.executable, os.path.join(ROOT, "tests", "factor_hook_worker.py"), self.lib, src, dst]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CALL_TIMEOUT)
        except subprocess.TimeoutExpired:
            self.dead = "timeout"
            pytest.fail("hook call timed out after %d s" % CALL_TIMEOUT)
        if r.returncode != 0:
            self.dead = "exit status %d" % r.returncode
            pytest.fail("hook call failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        out = np.load(dst)
        return {k: out[k] for k in out.files}

    def factor(self, key, blocks, groups, nw):
        """X [n, 32, 32] and flags [n]; one hook call per group of consecutive blocks.  key names the (cached) call."""
        key = (key, nw)
        if key not in self.cache:
            out = self._child(A=np.stack(blocks), groups=np.asarray(groups, np.int64), nw=np.int64(nw))
            assert np.all((out["bad"] == 0) | (out["bad"] == 1))
            self.cache[key] = (out["X"], out["bad"])
        return self.cache[key]

    def singles(self, cls, nw, run=0):
        """Every block of the class in a hook call of its own (one child process per NW and run makes the calls of ALL classes)."""
        sizes = [len(F.blocks(c)) for c in F.ALL_CLASSES]
        X, bad = self.factor(("single", run), [a for c in F.ALL_CLASSES for a in F.blocks(c)], [1] * sum(sizes), nw)
        at = sum(sizes[:F.ALL_CLASSES.index(cls)])
        return X[at:at + len(F.blocks(cls))], bad[at:at + len(F.blocks(cls))]

    def maps(self, x):
        if "maps" not in self.cache:
            out = self._child(x=x)
            self.cache["maps"] = (out["w"], out["y"])
        return self.cache["maps"]


@pytest.fixture(scope="module")
def hook(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("diag_factor_hook")
    lib = os.path.join(str(tmp), "liborbslam_hip_hooks.so")
    r = subprocess.run(F.hook_build_command(lib), capture_output=True, text=True, timeout=BUILD_TIMEOUT)
    assert r.returncode == 0, r.stderr[-4000:]
    return _Hook(lib, str(tmp))


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", F.ACCURACY_CLASSES)
def test_factor_is_as_accurate_as_lapack(hook, cls):
    blks = F.blocks(cls)
    for nw in NWS:
        X, bad = hook.singles(cls, nw)
        assert np.isfinite(X).all()
        (res, fwd), (lres, lfwd) = F.class_errors(blks, X)
        print("%-4s NW=%d kernel / LAPACK: residual %.3e / %.3e = %.2f, forward %.3e / %.3e = %.2f" % (cls, nw, res, lres, res / lres, fwd, lfwd, fwd / lfwd))
        assert lres > 0 and lfwd > 0
        assert res <= F.CAP * lres, (cls, nw, res, lres)
        assert fwd <= F.CAP * lfwd, (cls, nw, fwd, lfwd)


# ---- the scalar maps ------------------------------------------------------------------------------------------------------------
def test_scalar_maps_against_correctly_rounded_values(hook):
    """piv_recip and rsqrt_cubic as functions.  (Inside a wave's own block df_own_column spells piv_recip's three fmas out in line, in
    issue order; that copy is covered by the accuracy test above, not by this one.)"""
    x = F.scalar_inputs()
    w, y = hook.maps(x)
    assert np.all(np.isfinite(w) & (w > 0)) and np.all(np.isfinite(y) & (y > 0))
    dw = F.ulp_distance(w, F.recip_rn(x))
    dy = F.ulp_distance(y, F.rsqrt_rn(x))
    print("piv_recip w: max %d ulp (%d of %d off by one or more); rsqrt_cubic: max %d ulp (%d off by one or more)" %
          (dw.max(), np.count_nonzero(dw), len(x), dy.max(), np.count_nonzero(dy)))
    m, e = np.frexp(x)
    p2 = m == 0.5                                                # x = 2^(e - 1)
    assert np.count_nonzero(p2) == F.SCALAR_EMAX - F.SCALAR_EMIN + 1
    assert np.array_equal(w[p2], np.ldexp(1.0, -(e[p2] - 1)))    # w = 2^-e, exactly, for every power of two
    even = p2 & ((e - 1) % 2 == 0)
    assert np.array_equal(y[even], np.ldexp(1.0, -((e[even] - 1) // 2)))
    assert dw.max() <= ULP_BOUND["piv_recip_w"], x[np.argmax(dw)].hex()
    assert dy.max() <= ULP_BOUND["rsqrt_cubic"], x[np.argmax(dy)].hex()


# ---- exactness and structure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", F.ALL_CLASSES)
def test_forms_agree_and_upper_triangle_is_exactly_zero(hook, cls):
    X1, b1 = hook.singles(cls, 1)
    for nw in (2, 4):
        X, b = hook.singles(cls, nw)
        assert np.array_equal(b, b1), (cls, nw)
        nan = np.isnan(X1)                                       # (module docstring: the sign of a NaN is the compiler's choice)
        assert np.array_equal(np.isnan(X), nan), (cls, nw)
        assert not nan[b1 == 0].any()
        diff = np.flatnonzero(np.where(nan, 0.0, X).view(np.int64) != np.where(nan, 0.0, X1).view(np.int64))
        assert diff.size == 0, (cls, nw, diff.size, "first at block %d" % (diff[0] // (NB * NB)))
    iu = np.triu_indices(NB, 1)
    for i in np.flatnonzero(b1 == 0):                            # (a flagged block's inverse is garbage by contract)
        assert not X1[i][iu].any(), (cls, i)
        assert np.isfinite(X1[i]).all() and np.all(np.diag(X1[i]) > 0), (cls, i)


@pytest.mark.parametrize("cls", F.ALL_CLASSES)
def test_same_input_twice_gives_the_same_bytes(hook, cls):
    for nw in NWS:
        Xa, ba = hook.singles(cls, nw)
        Xb, bb = hook.singles(cls, nw, run=1)
        assert np.array_equal(ba, bb) and Xa.tobytes() == Xb.tobytes(), (cls, nw)


def test_diagonal_blocks_give_exactly_diagonal_inverses(hook):
    blks = F.blocks("D")
    for nw in NWS:
        X, bad = hook.singles("D", nw)
        assert not bad.any()
        exact = 0
        for A, Xi in zip(blks, X):
            assert not (Xi - np.diag(np.diag(Xi))).any()
            E = F.diagonal_expected(A)
            if E is not None:
                assert np.array_equal(Xi, E)
                exact += 1
            else:                                                # one rsqrt_cubic per entry
                assert F.ulp_distance(np.diag(Xi), F.rsqrt_rn(np.diag(A))).max() <= ULP_BOUND["rsqrt_cubic"]
        assert exact >= 8 and np.array_equal(X[0], np.eye(NB))


def test_back_to_back_factors_of_different_blocks(hook):
    """One workgroup factors 72 blocks of wildly different scale one after the other, the LDS counter base advancing by 32 per block
    and the LDS scratch of the previous block left in place - k_chol_wg's walk over the columns of a system."""
    seq = F.back_to_back_sequence()
    assert len(seq) >= 64
    for nw in NWS:
        Xb, bb = hook.factor("sequence-batch", seq, [len(seq)], nw)
        Xs, bs = hook.factor("sequence-single", seq, [1] * len(seq), nw)
        assert not bs.any() and np.array_equal(bb, bs)
        for i in range(len(seq)):
            assert Xb[i].tobytes() == Xs[i].tobytes(), (nw, i)
    # and in pieces of uneven length (the counter base restarts with every call)
    Xp, bp = hook.factor("sequence-pieces", seq, [1, 2, 3, 5, 8, 13, 21, len(seq) - 53], 4)
    assert Xp.tobytes() == hook.factor("sequence-single", seq, [1] * len(seq), 4)[0].tobytes() and not bp.any()


# ---- flags ------------------------------------------------------------------------------------------------------------------------
def test_flag_is_raised_for_a_non_positive_pivot_at_every_position(hook):
    for nw in NWS:
        X, bad = hook.singles("S", nw)
        assert len(bad) == NB and bad.all(), (nw, np.flatnonzero(bad == 0))


def test_flag_is_raised_for_nan_and_inf(hook):
    for nw in NWS:
        X, bad = hook.singles("X", nw)                           # (the call returned: a child that hangs fails in _child)
        assert len(bad) == len(F.X_VALUES) * len(F.X_POSITIONS) and bad.all(), (nw, np.flatnonzero(bad == 0))


@pytest.mark.parametrize("cls", F.NEVER_FLAGGED_CLASSES)
def test_flag_stays_clear_on_positive_definite_blocks(hook, cls):
    for nw in NWS:
        assert not hook.singles(cls, nw)[1].any(), (cls, nw)


def test_near_singular_ladder(hook):
    blks = F.blocks("N")
    ratios = []
    for A in blks:
        lo, hi = F.mp_spectrum(A)
        ratios.append(float(lo / hi))
    for nw in NWS:
        X, bad = hook.singles("N", nw)
        for i, A in enumerate(blks):
            if ratios[i] > F.N_THRESHOLD:
                assert not bad[i], (nw, i, ratios[i])
            if ratios[i] < -F.N_THRESHOLD:
                assert bad[i], (nw, i, ratios[i])
            if not bad[i]:
                assert np.isfinite(X[i]).all(), (nw, i)
                ref = F.reference(A)
                if ref["Xlapack"] is not None:
                    res = F.cached_residual(X[i], A)
                    if nw == 1:
                        print("N[%2d] lambda_min / lambda_max %+.1e: residual %.3e, LAPACK's %.3e" % (i, ratios[i], res, ref["lapack_residual"]))
                    assert res <= F.CAP * ref["lapack_residual"], (nw, i, res, ref["lapack_residual"])
