"""CPU side of the PoseOptimization tests: the references of tests/nppose.py and the CPU oracle pinned to each other on every
finite case of tests/posecases.py, and the oracle's behaviour on the whole table (what tests/test_gpu_pose_lm.py compares the device
with).  No GPU.

Measured here (mp at 50 digits; oracle = oracle/ba_oracle.cpp):
  oracle cost against mp_cost, largest relative deviation over the table:
      initial cost   4.19e-13  (exact_near: residuals of 1e-2 px cancel five digits of u; 3.7e-15 without that case)
      final cost     6.30e-14  (size_4: a 0.2 cost left of 21; 5.0e-15 without that case)
    the final cost of size_3, exact_near, exact_at_truth and the initial cost of exact_at_truth are rounding residue (no relative figure).
  oracle outlier flags against mp chi2 > 5.991 at the oracle's pose: identical on every case, nothing left out; the nearest observation
    sits at |chi2 / 5.991 - 1| = 1.5e-4 (size_2049).
  optimality gap of the oracle's pose, (float64 cost there - nppose.local_minimum) / cost:
      size_3 1.1e-18*  size_4 3.0e-10  size_63 7.1e-8  size_64 5.9e-8  size_65 2.3e-7  size_255 2.6e-9  size_256 9.2e-7  size_257 2.4e-9
      size_2047 9.1e-7  size_2048 5.0e-7  size_2049 8.0e-7  size_2304 9.2e-7  size_4100 3.1e-7  far_200 9.9e-8  far_2049 8.8e-7
      far_4100 3.8e-10  exact_near 4.4e-16*  exact_at_truth 1.9e-14*  zero_weights 0  half_zero_weights_2100 2.9e-7  behind_2100 6.5e-7
      all_outliers 1.2e-7      (* residue cases: relative to the initial cost / the rounding floor, posecases.gap)
    at most 9.2e-7,
    consistent with the 1e-6 function tolerance both solvers implement."""
import functools

import numpy as np
import pytest
from mpmath import mp, mpf

from tests import nppose
from tests import posecases as P


@functools.lru_cache(maxsize=None)
def _measure(name):
    """Everything the tests below need of one finite case, computed once."""
    p = P.make_case(name)
    n, pose, out, s = P.oracle_run(name)
    mp_i = P.mp_initial_cost(name)
    depth, chi2, sq = nppose.mp_terms(p["K4"], pose, p["Xw"], p["uv"], p["inv_sigma2"])
    mp_f = nppose.mp_cost(sq)
    flags, band = nppose.mp_flags(chi2)
    m = dict(mp_initial=mp_i, mp_final=mp_f, flags=flags, band=band, n_behind=sum(1 for z in depth if z <= 0),
             residue_initial=P.is_residue(name, mp_i, mp_i) and mp_i != 0, residue_final=P.is_residue(name, mp_f, mp_i) and mp_f != 0)
    m["dev_initial"] = None if m["residue_initial"] or mp_i == 0 else nppose.rel_dev(s["initial_cost"], mp_i)
    m["dev_final"] = None if m["residue_final"] or mp_f == 0 else nppose.rel_dev(s["final_cost"], mp_f)
    m["gap"] = P.gap(name, pose)
    return m


# ---------------------------------------------------------------- the references themselves
def test_mp_terms_by_hand():
    """fx = fy = 1, cx = cy = 0, identity pose, X = (0, 0, 1): u = v = 0.  Pixel (3, 4): e^2 = 25.
    w = 0.5: chi2 = 12.5, s = 6.25 > 5.991 -> rho = 2 sqrt(5.991) 2.5 - 5.991;  w = 0.25: chi2 = 6.25 (an outlier of the gate),
    s = 1.5625 <= 5.991 -> rho = s.  The gate weighs with inv_sigma2, the cost with its square."""
    K4 = np.array([1.0, 1.0, 0.0, 0.0]); pose = np.array([0, 0, 0, 0, 0, 0, 1.0])
    X = np.array([[0, 0, 1.0], [0, 0, 1.0]]); uv = np.array([[3.0, 4.0], [3.0, 4.0]]); w = np.array([0.5, 0.25], np.float32)
    depth, chi2, s = nppose.mp_terms(K4, pose, X, uv, w)
    assert [float(d) for d in depth] == [1.0, 1.0] and [float(c) for c in chi2] == [12.5, 6.25] and [float(v) for v in s] == [6.25, 1.5625]
    with mp.workdps(50):
        want = (2 * mp.sqrt(mpf(5.991)) * mpf(2.5) - mpf(5.991) + mpf(1.5625)) / 2
        assert abs(nppose.mp_cost(s) - want) < mpf("1e-45")
    assert list(nppose.mp_flags(chi2)[0]) == [1, 1]
    assert abs(nppose.cost(K4, pose, X, uv, w) - float(want)) <= 4e-16 * float(want)
    # the quaternion is used as given: a quarter turn about z DOUBLED, q = (0, 0, sqrt 2, sqrt 2), sends (1, 0, 0) to
    # v + w (2 qv x v) + qv x (2 qv x v) = (1, 0, 0) + (0, 4, 0) + (-4, 0, 0), not to (0, 1, 0)
    q = np.array([0, 0, np.sqrt(0.5), np.sqrt(0.5)]) * 2.0
    depth, _, _ = nppose.mp_terms(K4, np.concatenate([[0, 0, 5.0], q]), np.array([[1.0, 0, 0]]), np.array([[0.0, 0.0]]), np.ones(1, np.float32))
    RX, _ = nppose._camera_points(np.concatenate([[0, 0, 5.0], q]), np.array([[1.0, 0, 0]]))
    assert np.allclose(RX[0], [-3.0, 4.0, 0.0], atol=1e-15) and float(depth[0]) == 5.0


def test_mp_reference_is_self_consistent():
    p = P.make_case("size_257")
    a = nppose.mp_cost_at(p["K4"], p["pose0"], p["Xw"], p["uv"], p["inv_sigma2"], dps=50)
    b = nppose.mp_cost_at(p["K4"], p["pose0"], p["Xw"], p["uv"], p["inv_sigma2"], dps=100)
    with mp.workdps(100):
        assert abs(a - b) / b < mpf("1e-40")
    # the float64 cost the minimiser works on is the same function
    assert nppose.rel_dev(nppose.cost(p["K4"], p["pose0"], p["Xw"], p["uv"], p["inv_sigma2"]), a) < 1e-13


def test_local_minimum_recovers_a_known_minimiser():
    """Noise-free pixels: the minimiser is pose_gt, the minimum 0.  From 1 mm off, and from the near start of an ordinary case a
    second run from the first one's answer moves nothing."""
    p = P.make_case("exact_near")
    c, x, step = nppose.local_minimum(p["K4"], p["pose0"], p["Xw"], p["uv"], p["inv_sigma2"])
    assert np.abs(x - p["pose_gt"]).max() <= 1e-10 and c <= P.cost_floor(p)
    assert abs(step[0] + 1e-3) <= 1e-9
    p = P.make_case("size_255")
    c1, x1, _ = nppose.local_minimum(p["K4"], p["pose0"], p["Xw"], p["uv"], p["inv_sigma2"])
    c2, x2, _ = nppose.local_minimum(p["K4"], x1, p["Xw"], p["uv"], p["inv_sigma2"])
    assert c2 <= c1 and c1 - c2 <= 1e-13 * c1 and np.abs(x2 - x1).max() <= 1e-9
    # and a stationary point: the gradient is a rounding-sized fraction of its terms
    _, g, H = nppose._normal_equations(np.asarray(p["K4"], np.float64), x2, p["Xw"], p["uv"], p["inv_sigma2"].astype(np.float64))
    assert np.abs(np.linalg.solve(H, g)).max() <= 1e-9


# ---------------------------------------------------------------- the oracle on the table
@pytest.mark.parametrize("name", P.ALL_CASES)
def test_oracle_table(name):
    n, pose, out, s = P.oracle_run(name)
    assert (s["iterations"], s["successful_steps"], s["termination"]) == P.ORACLE_TABLE[name]
    p = P.make_case(name)
    if name in P.INF_CASES:
        assert pose.tobytes() == p["pose0"].tobytes() and not np.isfinite(s["initial_cost"])
    if name == "zero_weights":
        assert s["initial_cost"] == 0.0 and s["final_cost"] == 0.0 and n == len(out) and not out.any()
    if name == "all_outliers":
        assert n == 0 and out.all()
    if name in P.EXACT_CASES:
        assert np.abs(pose - p["pose_gt"]).max() <= P.RTOL_X
    assert n == len(out) - int(out.sum())


def test_table_covers_both_data_paths_and_rejected_steps():
    streaming = [c for c in P.ALL_CASES if P.is_streaming(c)]
    assert streaming == ["size_2049", "size_2304", "size_4100", "far_2049", "far_4100", "half_zero_weights_2100", "behind_2100", "inf_observation_2100"]
    assert P.n_obs("size_2048") == P.IN_REGISTERS_MAX
    for c in ("far_200", "far_2049", "far_4100"):                       # rejected steps on both paths
        it, ok, _ = P.ORACLE_TABLE[c]
        assert it - ok >= 7
    assert {P.ORACLE_TABLE[c][2] for c in P.ALL_CASES} == {1, 2, 3, 5}


@pytest.mark.parametrize("name", P.FINITE_CASES)
def test_oracle_costs_against_mp(name):
    m = _measure(name)
    s = P.oracle_run(name)[3]
    for key, cost, ref, bar in (("initial", s["initial_cost"], m["mp_initial"], P.ORACLE_DEV_INITIAL), ("final", s["final_cost"], m["mp_final"], P.ORACLE_DEV_FINAL)):
        dev = m["dev_" + key]
        print("%s %s cost %.17g  mp %s  deviation %s" % (name, key, cost, mp.nstr(ref, 20), dev))
        if ref == 0:
            assert cost == 0.0
        elif m["residue_" + key]:
            assert 0.0 <= cost <= P.residue_atol(name, m["mp_initial"])
        else:
            assert dev <= bar


def test_recorded_figures_are_the_measured_ones():
    """posecases.ORACLE_DEV_* (the GPU test's bar is 100 x them) are the maxima over the table, to two digits; the residue cases are
    the named ones."""
    ms = {c: _measure(c) for c in P.FINITE_CASES}
    dev_i = max(m["dev_initial"] for m in ms.values() if m["dev_initial"] is not None)
    dev_f = max(m["dev_final"] for m in ms.values() if m["dev_final"] is not None)
    print("largest deviation of the oracle from mp: initial %.3g, final %.3g" % (dev_i, dev_f))
    assert 0.5 * P.ORACLE_DEV_INITIAL <= dev_i <= P.ORACLE_DEV_INITIAL
    assert 0.5 * P.ORACLE_DEV_FINAL <= dev_f <= P.ORACLE_DEV_FINAL
    assert tuple(c for c in P.FINITE_CASES if ms[c]["residue_final"]) == P.RESIDUE_CASES
    assert tuple(c for c in P.FINITE_CASES if ms[c]["residue_initial"]) == P.RESIDUE_AT_START
    assert ms["behind_2100"]["n_behind"] == 200 and all(ms[c]["n_behind"] == 0 for c in P.FINITE_CASES if c != "behind_2100")


@pytest.mark.parametrize("name", P.FINITE_CASES)
def test_oracle_flags_against_mp_gate(name):
    """chi2 > 5.991 in mp at the oracle's pose, every observation (non-positive depth included: the gate has no depth test); none
    sits inside the 1e-9 band, so none is left out."""
    m = _measure(name)
    out = P.oracle_run(name)[2]
    print("%s nearest observation to the gate: %.3g" % (name, m["band"]))
    assert m["band"] > P.GATE_BAND
    assert np.array_equal(out, m["flags"])


@pytest.mark.parametrize("name", P.FINITE_CASES)
def test_oracle_optimality_gap_is_recorded(name):
    """No bound here: the GPU test compares its gap with this one.  The independent minimum is never above the oracle's cost."""
    m = _measure(name)
    print("%s optimality gap %.3g" % (name, m["gap"]))
    assert m["gap"] >= 0.0 and np.isfinite(m["gap"])
