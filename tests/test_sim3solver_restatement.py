"""CPU checks of tests/npsim3solver.py, the numpy restatement the GPU Sim3 RANSAC is compared with: it recovers the ground truth, its
two-sided Jacobi agrees with LAPACK to the eigenvector's conditioning, and it follows the reference's rules (the +- pairing of N's
eigenvalues, the truncated thresholds, the sequential walk)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import npsim3solver as ref  # noqa: E402
import sim3cases  # noqa: E402

# Ground truth on the noise-free scenes with outliers (sim3cases.NOISE_FREE), npsim3solver(lapack=True): the maximum over the cases of
# max |R - R_gt|, |t - t_gt|_inf / max(1, |t_gt|_inf) and |s - s_gt| / s_gt.  The restatement may be 10 x that: the margin covers a
# different but equally valid summation order inside the eigen-solver.  (The translation and scale errors are those of the FLOAT scale
# the reference keeps, 2^-24 relative, not of the estimator.)
GT_LAPACK_MAX_DR = 8.7e-14
GT_LAPACK_MAX_DT = 5.5e-7
GT_LAPACK_MAX_DS = 3.7e-8
# max over 4 200 hypotheses (14 scenes x 300 sets) of max |R_jacobi - R_lapack| * relgap, measured for the committed restatement:
# 2.284e-15 (largest |dR| 4.4e-12, smallest relgap 4.6e-5).  An eigenvector moves by eps / relgap under a backward error of eps, so
# the product is a small multiple of 2.2e-16 whatever the gap.  Asserted: 10 x the measured maximum.
JACOBI_LAPACK_MAX_PRODUCT = 2.284e-15


def _np_iter(a, **kw):
    return ref.iterate(*sim3cases.np_args(a), **kw)


@pytest.mark.parametrize("case", sim3cases.NOISE_FREE)
def test_recovers_ground_truth(case):
    a = sim3cases.build(case)
    s = a["scene"]
    r = _np_iter(a)
    assert r["status"] == ref.FOUND and r["n_inliers"] > sim3cases.MIN_INLIERS
    assert not (r["inliers"] & s["outlier"]).any()
    dR = np.abs(r["R"] - s["R"]).max()
    dt = np.abs(r["t"] - s["t"]).max() / max(1.0, np.abs(s["t"]).max())
    ds = abs(float(r["scale"]) - s["scale"]) / s["scale"]
    print("dR %.3e dt %.3e ds %.3e" % (dR, dt, ds))
    assert dR <= 10 * GT_LAPACK_MAX_DR and dt <= 10 * GT_LAPACK_MAX_DT and ds <= 10 * GT_LAPACK_MAX_DS


def test_jacobi_against_lapack_per_hypothesis():
    worst, worst_dr, min_gap, excluded, total = 0.0, 0.0, 1.0, 0, 0
    for case in sim3cases.MATRIX:
        if case[1] not in ("general", "planar") or case[2] < sim3cases.MIN_INLIERS:
            continue
        a = sim3cases.build(case, 300)
        for st in a["sets"]:
            Rj, tj, sj, gap = ref.compute_sim3(a["X1c"][st], a["X2c"][st], a["fix_scale"])
            Rl, tl, sl, _ = ref.compute_sim3(a["X1c"][st], a["X2c"][st], a["fix_scale"], lapack=True)
            total += 1
            if not np.isfinite(Rj).all() or not gap >= 1e-6:
                excluded += 1
                continue
            d = np.abs(Rj - Rl).max()
            worst, worst_dr, min_gap = max(worst, d * gap), max(worst_dr, d), min(min_gap, gap)
    print("max |dR| * relgap %.3e, max |dR| %.3e, min relgap %.3e, excluded %d of %d" % (worst, worst_dr, min_gap, excluded, total))
    assert total == 4200 and excluded <= total // 100           # general scenes stay under the GPU test's 1 % cap
    assert worst <= 10 * JACOBI_LAPACK_MAX_PRODUCT


def test_eigenvalues_of_N_come_in_pairs():
    """With three points both centred sets are coplanar, det M = 0, the characteristic polynomial of N is biquadratic: the spectrum
    is {-l3, -l2, l2, l3}.  That is why a one-sided Jacobi (singular values: |l| twice) cannot pick the eigenvector of +l3 and the
    library has a two-sided one.  Bound: 64 eps - eigvalsh's backward error is a few eps ||N||, and ||N||_2 = l3."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(3000):
        N = np.array(ref.horn_N(rng.normal(0, 5, (3, 3)), rng.normal(0, 5, (3, 3)))[0])
        ev = np.sort(np.linalg.eigvalsh(N))
        worst = max(worst, abs(ev[0] + ev[3]) / ev[3], abs(ev[1] + ev[2]) / ev[3])
    print("worst |l0 + l3| / l3: %.3e" % worst)
    assert worst <= 64 * 2.220446049250313e-16
    # and the two-sided Jacobi returns signed eigenvalues and their eigenvectors
    N = ref.horn_N(rng.normal(0, 5, (3, 3)), rng.normal(0, 5, (3, 3)))[0]
    ev, V = ref.jacobi_sym4(N)
    V = np.array(V)
    assert np.allclose(np.sort(ev), np.linalg.eigvalsh(np.array(N)), rtol=0, atol=1e-13 * max(np.abs(ev)))
    assert np.abs(np.array(N) @ V - V * np.array(ev)).max() <= 1e-13 * max(np.abs(ev))
    assert min(ev) < 0 < max(ev)


def test_jacobi_ties_and_non_finite_input():
    ev, V = ref.jacobi_sym4(np.zeros((4, 4)))
    assert ev == [0.0] * 4 and np.array_equal(np.array(V), np.eye(4))      # no rotation; the maximum is index 0
    R, t, s, gap = ref.compute_sim3(np.ones((3, 3)), np.ones((3, 3)), False)
    assert np.array_equal(R, np.eye(3)) and np.isnan(float(s)) and np.isnan(t).all()
    ev, V = ref.jacobi_sym4(np.full((4, 4), np.nan))                       # left alone, no endless loop
    assert np.isnan(ev).all()


def test_thresholds_are_truncated():
    """max_errors_ are std::vector<size_t>: 9.210 * sigma2 is truncated (9, 13, 19, 27, ...).  On this scene the untruncated
    thresholds would accept two more correspondences for the returned hypothesis."""
    lv = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
    assert ref.max_errors(lv).tolist()[:4] == [9.0, 13.0, 19.0, 27.0]
    assert ref.max_errors(lv).dtype == np.float32 and (ref.max_errors(lv) == np.floor(ref.max_errors(lv))).all()
    from ceres_mono_orb_slam2_amd import sim3solver
    assert np.array_equal(sim3solver.max_errors(lv), ref.max_errors(lv))
    a = sim3cases.build(sim3cases.MATRIX[2])
    s = a["scene"]
    r = _np_iter(a)
    assert r["status"] == ref.FOUND
    e1, e2 = ref.errors(r["R"], r["t"], r["scale"], a["X1c"], a["X2c"], a["K1"], a["K2"])
    u1 = (9.210 * s["sigma2_1"].astype(np.float64)).astype(np.float32)
    u2 = (9.210 * s["sigma2_2"].astype(np.float64)).astype(np.float32)
    truncated = (e1 < a["max_err1"]) & (e2 < a["max_err2"])
    untruncated = (e1 < u1) & (e2 < u2)
    assert np.array_equal(truncated, r["inliers"])
    assert int(untruncated.sum()) > int(truncated.sum())


# (counts of the given sets, incoming best_count, min_inliers) -> (status, consumed, set that last replaced the best, best_count)
WALK = [
    ("a count >= the best replaces it, ties go to the later set", [5, 7, 7, 3], 0, 20, (ref.NOT_FOUND, 4, 2, 7)),
    ("a count of 0 replaces a best of 0", [0, 0, 0], 0, 20, (ref.NOT_FOUND, 3, 2, 0)),
    ("the return needs strictly more than min_inliers", [20, 20, 21, 30], 0, 20, (ref.FOUND, 3, 2, 21)),
    ("exactly min_inliers never returns", [20, 20], 0, 20, (ref.NOT_FOUND, 2, 1, 20)),
    ("after a rejected success a later set has to reach the previous best", [25, 29, 30, 40], 30, 20, (ref.FOUND, 3, 2, 30)),
    ("above min_inliers but below the carried best: not returned", [25, 29, 22], 30, 20, (ref.NOT_FOUND, 3, -1, 30)),
    ("no sets (the caller is at the AND bound)", [], 12, 20, (ref.NOT_FOUND, 0, -1, 12)),
    ("the first set returns", [21], 0, 20, (ref.FOUND, 1, 0, 21)),
]


@pytest.mark.parametrize("what,counts,best,min_inl,expect", WALK, ids=[w[0] for w in WALK])
def test_walk_table(what, counts, best, min_inl, expect):
    assert ref.walk(counts, best, min_inl) == expect


def test_too_few_and_the_and_bound():
    a = sim3cases.build(sim3cases.MATRIX[12])                    # kind "few": n = 12 < 20
    st = ref.State(len(a["X1c"]))
    st.best_count = 0
    r = _np_iter(a, state=st)
    assert (r["status"], r["consumed"], r["n_inliers"]) == (ref.TOO_FEW, 0, 0)
    assert np.array_equal(r["T12"], np.eye(4)) and not r["inliers"].any() and st.best_count == 0 and np.array_equal(st.best_R, np.eye(3))
    # a caller that owns n_iterations_: chained iterate(5) calls, every pose rejected, end exactly at max_iterations
    a = sim3cases.build(sim3cases.MATRIX[10], 300)
    n = len(a["X1c"])
    max_its = ref.ransac_params(n, 0.99, sim3cases.MIN_INLIERS, 300)
    assert max_its == 35
    used, st = 0, ref.State(n)
    while used < max_its:
        k = min(max_its - used, 5)
        r = ref.iterate(a["X1c"], a["X2c"], a["max_err1"], a["max_err2"], a["K1"], a["K2"], a["fix_scale"], a["min_inliers"], a["sets"][used:used + k], state=st)
        assert 1 <= r["consumed"] <= k
        used += r["consumed"]
    assert used == max_its


def test_matrix_reaches_every_status():
    seen = {}
    for case in sim3cases.MATRIX:
        seen.setdefault(_np_iter(sim3cases.build(case))["status"], []).append(case[0])
    assert set(seen) == {ref.FOUND, ref.NOT_FOUND, ref.TOO_FEW}, seen
    assert len(seen[ref.FOUND]) >= 4 and len(seen[ref.NOT_FOUND]) >= 3 and len(seen[ref.TOO_FEW]) >= 2


def test_draw_sets_is_the_reference_draw():
    from ceres_mono_orb_slam2_amd import sim3solver
    script = iter([4, 0, 2, 0, 0, 0])
    s = sim3solver.draw_sets(5, 2, lambda lo, hi: next(script))
    # [0 1 2 3 4] slot 4 -> 4; [0 1 2 3] slot 0 -> 0, slot 0 takes the back: [3 1 2]; slot 2 -> 2
    assert s.tolist() == [[4, 0, 2], [0, 4, 3]]
