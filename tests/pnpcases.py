"""Seeded cases for the PnP RANSAC tests (tests/test_gpu_pnp.py, tests/test_pnp_restatement.py).  A case is a tuple
(seed, kind, n, outlier_frac, noise); make_case() returns the arrays a call takes, with Tracking's parameters
(SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), src/Tracking.cc:1030)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nppnp  # noqa: E402

TH2 = 5.991
TRACKING = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5)

# the end-to-end matrix: kind x outlier_frac x noise x N (N = 10 is the adjusted minimum itself: one iteration)
CASES = [(1000 + i, kind, n, of, noise)
         for i, (kind, n, of, noise) in enumerate((kind, n, of, noise) for kind in ("general", "planar") for n in (10, 20, 50, 200, 2000)
                                                  for of in (0.0, 0.3, 0.6) for noise in (0.0, 0.5, 1.0))]
CASES.append((2000, "few", 6, 0.0, 0.0))
# the hypothesis-level comparisons (300 sets each); test_pnp_restatement.py checks that nppnp against itself under a 1-ulp perturbation
# of the pixels changes the chosen approximation in at most 2 % of their hypotheses
HYP_CASES = [CASES[i] for i in (31, 40, 43, 85)]
# noise-free general scenes with 30 % outliers (the ground-truth test)
GT_CASES = [(3000 + i, "general", n, 0.3, 0.0) for i, n in enumerate((20, 50, 50, 200, 200, 2000))]
PLANAR_GT_CASES = [(3100 + i, "planar", n, 0.3, 0.0) for i, n in enumerate((50, 200, 2000))]
# exactly min_inliers true inliers among N = 2 min_inliers points: a hypothesis qualifies, its refit cannot exceed the minimum
REFIT_FAILS = (4003, "general", 40, 0.5, 0.0)
# A refit that fails FOLLOWED by one that succeeds inside one call needs a qualifying hypothesis whose refit stays at the minimum and
# a later, strictly larger record.  Searched with nppnp: seeds 7000-7399 x noise {0.7, 1.0} px on 41 points with 21 true inliers
# (min_inliers 20), 800 scenes: none.  The rule is covered by the table-driven test in test_pnp_restatement.py; the device by
# REFIT_FAILS and by the success from an incoming state (test_gpu_pnp.py).


def draw(seed, n, iterations):
    rng = np.random.default_rng(seed)
    return nppnp.draw_sets(n, iterations, lambda lo, hi: int(rng.integers(lo, hi + 1)))


def make_case(case, iterations=None):
    """-> dict p3d, p2d, max_err, K4, min_inliers, max_iterations, sets [max_iterations or `iterations`, 4], scene"""
    from ceres_mono_orb_slam2_amd import synth
    seed, kind, n, of, noise = case
    s = synth.make_reloc(seed, n, of, noise, kind)
    n = len(s["p3d"])
    pr = nppnp.ransac_params(n, **TRACKING)
    its = pr["max_iterations"] if iterations is None else iterations
    sets = draw(seed + 7, n, its) if n >= 4 else np.zeros((its, 4), np.int32)
    max_err = (s["sigma2"].astype(np.float32) * np.float32(TH2)).astype(np.float32)
    return dict(p3d=s["p3d"], p2d=s["p2d"], max_err=max_err, K4=s["K4"], min_inliers=pr["min_inliers"], max_iterations=pr["max_iterations"], sets=sets,
                scene=s)
