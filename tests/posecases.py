"""Seeded cases for the PoseOptimization tests (tests/test_pose_reference.py on the CPU, tests/test_gpu_pose_lm.py on the GPU), and
the figures the two share.  Every case is built from synth.make_pose_problem.

k_pose_lm (csrc/ba_small_lm.inc) keeps a frame's observations in registers up to 256 * 8 = 2048 of them and streams them from global
memory on every evaluation above that: is_streaming() names the cases that take the second path.  ORACLE_TABLE is what the CPU oracle
does on each case - (iterations, accepted steps, termination) - asserted by the CPU test so that the GPU test compares like with like:
  size_N                  near start (0.5 deg / 5 cm), sizes at the minimum, a wave, a workgroup and the switch between the two paths
  far_N                   the start 50 m off in every axis: rejected steps and retries from the kept state, on both paths
  exact_near              noise-free pixels, start 1 mm off: the minimiser is pose_gt, parameter-tolerance termination (2)
  exact_at_truth          the same started at pose_gt: one iteration, nothing accepted
  zero_weights            every weight 0: gradient termination at iteration 0 (1), cost 0, all inliers
  half_zero_weights_2100  every other weight 0, streaming
  behind_2100             200 points behind the camera (negative depth), streaming
  all_outliers            every pixel 30 - 50 px off
  inf_observation_N       one pixel coordinate +inf: a non-finite cost, five failed 6 x 6 factorisations, termination 5, no step"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import nppose  # noqa: E402

RTOL_COST, RTOL_X = 1e-9, 1e-7               # the project's bars (tests/test_gpu_ba.py)
GATE_BAND = 1e-9                             # an observation with |chi2 / 5.991 - 1| <= this may be left out of the flag comparison
IN_REGISTERS_MAX = 2048                      # 256 threads x POSE_R = 8 observations

SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2304, 4100)
FAR = (200, 2049, 4100)
INF_CASES = ("inf_observation_50", "inf_observation_2100")
FINITE_CASES = tuple(["size_%d" % n for n in SIZES] + ["far_%d" % n for n in FAR] +
                     ["exact_near", "exact_at_truth", "zero_weights", "half_zero_weights_2100", "behind_2100", "all_outliers"])
ALL_CASES = FINITE_CASES + INF_CASES
# final cost below RTOL_COST x initial cost: rounding residue of a zero-residual fit, no relative bar means anything (is_residue);
# exact_at_truth STARTS at the zero of a zero-residual fit, so its initial cost is residue as well
RESIDUE_CASES = ("size_3", "exact_near", "exact_at_truth")
RESIDUE_AT_START = ("exact_at_truth",)
EXACT_CASES = ("exact_near", "exact_at_truth")

# (iterations, accepted steps, termination) of the CPU oracle
ORACLE_TABLE = {
    "size_3": (4, 3, 2), "size_4": (4, 3, 3), "size_63": (3, 2, 3), "size_64": (3, 2, 3), "size_65": (4, 3, 3), "size_255": (4, 3, 3),
    "size_256": (3, 2, 3), "size_257": (4, 3, 3), "size_2047": (3, 2, 3), "size_2048": (3, 2, 3), "size_2049": (3, 2, 3),
    "size_2304": (3, 2, 3), "size_4100": (3, 2, 3),
    "far_200": (14, 7, 3), "far_2049": (15, 7, 3), "far_4100": (16, 8, 3),
    "exact_near": (3, 2, 2), "exact_at_truth": (1, 0, 2), "zero_weights": (0, 0, 1), "half_zero_weights_2100": (3, 2, 3),
    "behind_2100": (8, 7, 3), "all_outliers": (14, 13, 3),
    "inf_observation_50": (5, 0, 5), "inf_observation_2100": (5, 0, 5),
}

# Largest relative deviation of the oracle's initial / final cost from the mp cost over FINITE_CASES, to two digits
# (tests/test_pose_reference.py measures them and asserts that these are the figures: exact_near sets the first - residuals of 1e-2 px
# cancel five digits of u -, size_4 the second).  The GPU's bar against mp is 100 x the oracle's deviation: the kernel sums in a tree
# where the oracle sums in index order, and the residuals u_obs - u cancel three digits and more, so a few ulps per term differ
# legitimately; 100 x leaves both bars two orders and more inside RTOL_COST.
ORACLE_DEV_INITIAL = 4.2e-13
ORACLE_DEV_FINAL = 6.3e-14
MP_BAR_INITIAL = 100.0 * ORACLE_DEV_INITIAL
MP_BAR_FINAL = 100.0 * ORACLE_DEV_FINAL


def _freeze(p):
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def make_case(name):
    """-> dict K4, pose0, pose_gt, Xw, uv, inv_sigma2 (read-only arrays, shared between the tests)."""
    from ceres_mono_orb_slam2_amd import synth
    kind, _, arg = name.rpartition("_")
    if kind == "size":
        n = int(arg)
        p = synth.make_pose_problem(100 + n, n=n)
    elif kind == "far":
        n = int(arg)
        p = synth.make_pose_problem(900 + n, n=n)
        p["pose0"][:3] += 50.0
    elif name in EXACT_CASES:
        p = synth.make_pose_problem(7, n=300, outlier_frac=0.0)
        p["uv"] = synth.project(p["K4"], p["pose_gt"], p["Xw"])[0]
        p["pose0"] = p["pose_gt"].copy()
        if name == "exact_near":
            p["pose0"][0] += 1e-3
    elif name == "zero_weights":
        p = synth.make_pose_problem(13, n=100)
        p["inv_sigma2"][:] = 0
    elif name == "half_zero_weights_2100":
        p = synth.make_pose_problem(13, n=2100)
        p["inv_sigma2"][::2] = 0
    elif name == "behind_2100":
        p = synth.make_pose_problem(14, n=2100)
        p["Xw"][:200] = -p["Xw"][:200]
    elif name == "all_outliers":
        p = synth.make_pose_problem(10, n=200, outlier_frac=1.0)
    elif kind == "inf_observation":
        n = int(arg)
        p = synth.make_pose_problem(12, n=n)
        p["uv"][n - 1, 0] = np.inf
    else:
        raise KeyError(name)
    return _freeze({k: p[k] for k in ("K4", "pose0", "pose_gt", "Xw", "uv", "inv_sigma2")})


def args(p):
    return p["K4"], p["pose0"], p["Xw"], p["uv"], p["inv_sigma2"]


def cost_floor(p):
    """The cost that rounding alone produces: every pixel residual 16 ulps of its coordinate (the dozen roundings between X and
    u = (fx p0 + cx p2) / p2, each within an ulp of a quantity of u's size).  A cost below it is a sum of squared rounding errors -
    only its size means anything."""
    w = p["inv_sigma2"].astype(np.float64)
    ulp = 16.0 * np.spacing(np.abs(p["uv"]))
    return 0.5 * float((w * w * (ulp * ulp).sum(1)).sum())


def is_residue(name, cost, initial_cost):
    """A cost below RTOL_COST x the initial cost is the rounding residue of a zero-residual fit, one below cost_floor is rounding
    residue whatever the start was: no relative bar means anything there."""
    return float(cost) < max(RTOL_COST * float(initial_cost), cost_floor(make_case(name)))


def residue_atol(name, initial_cost):
    """The absolute bar that replaces a relative one on a residue cost."""
    return max(RTOL_COST * float(initial_cost), cost_floor(make_case(name)))


def n_obs(name):
    return len(make_case(name)["Xw"])


def is_streaming(name):
    return n_obs(name) > IN_REGISTERS_MAX


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The oracle's solve of the case: (n_inliers, pose7, outlier flags, summary)."""
    from oracle import pyoracle
    n, pose, out, s = pyoracle.pose_optimization(*args(make_case(name)))
    pose.setflags(write=False); out.setflags(write=False)
    return int(n), pose, out, s


@functools.lru_cache(maxsize=None)
def mp_initial_cost(name):
    """mp cost at pose0 (an mpf)."""
    p = make_case(name)
    return nppose.mp_cost_at(p["K4"], p["pose0"], p["Xw"], p["uv"], p["inv_sigma2"])


@functools.lru_cache(maxsize=None)
def minimum(name):
    """The independent local minimum next to the oracle's answer: nppose.local_minimum started at the oracle's returned pose."""
    p = make_case(name)
    c, x, _ = nppose.local_minimum(p["K4"], oracle_run(name)[1], p["Xw"], p["uv"], p["inv_sigma2"])
    return c, x


def gap(name, pose7):
    """Optimality gap of a returned pose: (float64 cost there - the independent minimum) / cost, the cost being the minimum.  Where
    the minimum is rounding residue (RESIDUE_CASES) the denominator is residue_atol / RTOL_COST - the initial cost, for a
    zero-residual fit - so that a bar of k x RTOL_COST on the gap is the absolute bar k x residue_atol the costs of these cases get
    everywhere else; 0 / 0 (zero_weights) is 0."""
    p = make_case(name)
    cmin = minimum(name)[0]
    num = nppose.cost(p["K4"], pose7, p["Xw"], p["uv"], p["inv_sigma2"]) - cmin
    mp_i = mp_initial_cost(name)
    den = residue_atol(name, mp_i) / RTOL_COST if is_residue(name, cmin, mp_i) else cmin
    return 0.0 if num == 0.0 else num / den
