"""csrc/small_dense.h and null_vector4_dev (csrc/tri_math.h) on the MI355X at rank, tie and scale edges, against the mp reference
tests/npdense.py on the case table of tests/densecases.py: once through the stand-alone probe tools/ubench/small_dense_probe.hip (every
instantiation the estimators use, one lane per case; the 12 x 12 also behind the LDS view of stride 16 that k_pnp_hyp uses), and once
through the library: frame.TriangulateMatches, initializer.initialize(trace=True) and pnp.iterate(trace=True).

The rule everywhere: per bucket, max e <= max(64 * 2.2e-16, 8 * E_ref[bucket]); E_ref is the figure of the numpy restatement (the device's
arithmetic restated line for line) against mp, committed in tests/golden/small_dense_ref_err.npz and reproduced, with its two conditions
(finite; <= 1e-13 in every gap-free metric), by tests/test_small_dense_reference.py, whose docstring lists the buckets above 1e-9 and why.
The outputs for 2^+-200 A are compared == with the exactly rescaled outputs for A.

Measured on the device (buckets; largest e and its bucket; the bucket nearest its bound; device to restatement):
  i_svd3              324  3.89e-9 (graded/k=8/vec/gap=1e-9, eps / gap)           rank2/noise/values 2.3e-15 of 1.84e-14          0
  i_inv3 / i_det3      13  10.6 (cond=1e12/x, the cofactor formula's own)         cond=1e4/x 2.78e-12 of 2.22e-11                 0
  i_jacobi<16,9>       63  2.81e-15 (collinear/orthV)                             general/orthV 2.63e-15 of 2.11e-14              0
  i_jacobi<8,9>        66  1.43e-13 (general/vec/gap=1e-5)                        general/values 1.24e-14 of 9.91e-14             0
  null_vector4_dev     20  1.34e-6 (diag/1-s3/s2=1e-10/vec/gap=1e-11)             diag/1-s3/s2=1e-2/vec 1.35e-14 of 1.08e-13      0
  d_jacobi 12 x 12     16  3.51e-13 (planar/proj/gap=1e-3)                        general/values 1.01e-14 of 8.11e-14             0
    the same figures behind DView{p, 1} and behind DView{p + lane, 16} in LDS: the two sections agree to the bit
  d_lstsq 6 x 3/4/5   3x8  2.55 / 2.02 / 4.18 (cond=1e10/b=out: cond^2 eps)       6 x 4 cond=1e2/b=out 4.85e-14 of 3.88e-13       0
  i_jacobi_sym4        85  4.07e-15 (horn/generic/vec/gap=1e-2)                   the same bucket, of 3.26e-14                    0
  The device-to-restatement difference is zero in every function: on these inputs the device's sqrt, division and products give the
  restatement's bits, so every figure above is E_ref itself, and the == scale checks hold on the device as they do on the CPU.
  TriangulateMatches: 5 buckets, largest 1.18e-15 (tri/cos=0.9995/X) of 1.41e-14; flags equal mp's gates on 249 matches, 8 (3.1 %) left out.
  initialize: 15 buckets, largest 2.88e-5 (init/F/general/repeat/resid, E_ref's own); nearest init/H/general/distinct/vec/gap=1e-1,
    4.13e-15 of 3.3e-14; sigma2 / sigma0 of the traced F at most 1.4e-19.
  pnp.iterate: planar 6.84e-5 of 5.47e-4 over 16 sets; see test_pnp_dense_middle_against_ground_truth for the general and collinear candidates.
Two things in i_svd3 had to change: a left vector for rank <= 1, and a proper V on an exactly null third column.

What bites where (one-line mutations of scratch copies of the headers, each once through the probe on the device):
  the sign sg of i_svd3 inverted - 48 buckets: recon and sign of every svd3 bucket with S2 > 0 (generic, negdet, graded, psd/full, tie2/0.3, ...);
  1e-24 turned into 1e-12 in d_lstsq - 9 buckets: cond=1e6 (b in and out) and cond=1e10/b=in of all three shapes;
  the rank rule of i_svd3 switched off (S1 > 0) - 6 buckets: orthU of rank1/outer and psd/collinear and their x2^+-200 copies;
  the parity term of the sign rule replaced by +1 - 3 buckets: rank2/zerocol/proper and its copies.
  Two mutations are caught by no bucket, and no truth can catch them: `nrm < bn` turned into `<=` in i_min_col only changes which of two
  columns of exactly equal norm is returned, and both attain the minimum (the choice is pinned by the device-to-restatement figure alone);
  the `alpha <= tiny` clause dropped from d_jacobi leaves `beta <= tiny` to skip the same pairs one sweep later: it is a stopping rule, the
  outputs on this table do not move, and the probe returns no sweep count (tests/test_initializer_restatement.py pins the sweeps of the
  restatement).
"""
import numpy as np
import pytest

from tests import densecases as C

pytestmark = pytest.mark.gpu

FUNCTIONS = dict(svd3="i_svd3", inv3="i_inv3 / i_det3", jach="i_jacobi<16,9> + i_min_col", jacf="i_jacobi<8,9> + i_min_col", null4="null_vector4_dev",
                 djac="d_jacobi 12 x 12, stride 1", djac16="d_jacobi 12 x 12, stride 16 in LDS", lstsq63="d_lstsq 6 x 3", lstsq64="d_lstsq 6 x 4",
                 lstsq65="d_lstsq 6 x 5", sym4="i_jacobi_sym4", tri="TriangulateMatches", init="initialize", pnp="pnp.iterate")


def _summary(what, m, E, d2r=None):
    for fn in sorted({b.split("/")[0] for b in m}):
        mine = {b: e for b, e in m.items() if b.split("/")[0] == fn}
        worst = max(mine, key=lambda b: mine[b] / C.bound(E, b))
        print("%s %s (%s): %d buckets, largest e %.3g (%s); nearest to its bound %s: %.3g of %.3g%s" % (
            what, fn, FUNCTIONS[fn], len(mine), max(mine.values()), max(mine, key=mine.get), worst, mine[worst], C.bound(E, worst),
            "" if d2r is None else "; device to restatement %.3g" % d2r[fn]))


def test_probe(tmp_path):
    exe = C.build_probe(tmp_path, C.PROBE_SRC)
    dev = C.run_probe(exe, tmp_path)
    E = C.load_golden()
    m = C.errors(dev)
    d2r = C.device_to_restatement(dev)
    _summary("probe", m, E, d2r)
    print("largest device-to-restatement difference: %.3g (%s)" % (max(d2r.values()), max(d2r, key=d2r.get)))
    print("d_jacobi behind stride 1 and behind stride 16 agree to the bit: %s" % np.array_equal(dev["djac"], dev["djac16"]))
    bad = C.scale_mismatches(dev)
    assert not bad, "outputs for 2^k A differ from the rescaled outputs for A: %s" % bad[:10]
    C.check(m, E, "small_dense.h / null_vector4_dev on the device")


def test_triangulate_matches_against_mp():
    """257 matches over the parallax ladder, cos 0.6 to 1 - 5e-7 (depths of 1 to 1e3 baselines): the accepted points against the mp DLT per
    rung, the accept flags == the gates evaluated in mp (matches with a gate quantity within 1e-4 of its threshold left out: at most 5 %)"""
    from ceres_mono_orb_slam2_amd import frame
    p = C.tri_problem()
    X, ok = frame.TriangulateMatches(p["T1"], p["T2"], p["K"], p["K"], p["kp1"], p["kp2"], p["ls"], p["sf"], p["ratio"])
    m, wrong, left = C.tri_errors(X, ok)
    E = C.load_golden()
    _summary("library", m, E)
    print("left out %.1f %%" % (100 * left))
    assert left <= 0.05
    assert not wrong, "accept flags differ from the gates in mp at matches %s" % wrong
    assert sorted(m) == sorted(b for b in E if b.startswith("tri/"))
    C.check(m, E, "TriangulateMatches against the mp DLT")


def test_initializer_hypotheses_against_mp():
    """65 iterations (one lane past a 64-lane block) on a general and a planar scene of 40 matches, hand-made sets with repeated positions:
    the traced H21 and F21, unit Frobenius norm and either sign, against the mp null vector carried through T2^-1 Hn T1 / T2^T Fn T1, per
    gap of the system; 'residual only' sets (F of a planar scene or of repeated points) by x2^T F x1 on their 8 points; sigma2 / sigma0 of
    every traced F within the bound of init/F/rank2"""
    from ceres_mono_orb_slam2_amd import initializer
    traces = []
    for p in C.init_problems():
        r = initializer.initialize(p["kps1"], p["kps2"], p["m12"], C.INIT_K4, sigma=1.0, iterations=C.INIT_ITERS, ransac_sets=p["sets"], trace=True)
        traces.append((r["H21"], r["F21"]))
    m = C.init_errors(traces)
    E = C.load_golden()
    _summary("library", m, E)
    assert sorted(m) == sorted(b for b in E if b.startswith("init/"))
    C.check(m, E, "the traced hypotheses of initialize")


def test_pnp_dense_middle_against_ground_truth():
    """17 sets (one past PNP_HYP_LANES) of 4 among 12 noise-free points.  A set is compared where its pose is a function of the problem:
    nppnp(lapack=True) recovers the ground truth to 1e-3 with LAPACK's basis of the null space of M^T M and with three rotations of it
    (densecases.pnp_nondegenerate).  Exactly planar candidate (z = 0): 16 of the 17 sets, R and t within 8 x nppnp(lapack=True)'s own
    figure, 6.8e-5 (minimal sets, float32 image points); the device reaches 6.8e-5.  Before i_svd3 made V proper on an exactly null
    third column, 7 of these sets came out 0.4 from the truth (a reflection 'repaired' by negating a row of R).  General candidate: four
    points in general position leave a null space of dimension 4 whose basis is free, the pose moves between 1e-7 and 1 with the basis
    under LAPACK itself, so no set qualifies; the poses are only required to be finite.  Collinear candidate: every traced pose is finite
    exactly where nppnp(lapack=True)'s is - before the rank rule of i_svd3 the device gave NaN - and a non-finite pose counts no inlier."""
    from ceres_mono_orb_slam2_amd import pnp
    poses, E = [], C.load_golden()
    for p, (Rl, tl) in zip(C.pnp_problems(), C.pnp_lapack()):
        n = len(p["p3d"])
        collinear = p["kind"] == "collinear"
        # max_err = 0: no point is ever an inlier, the walk consumes every set; the collinear candidate keeps real thresholds and one gross
        # outlier, so that no set reaches min_inliers = n either
        p2d = p["p2d"].copy(); max_err = np.zeros(n, np.float32)
        if collinear:
            p2d[n - 1] += 60.0; max_err[:] = 5.991
        d = pnp.iterate(p["p3d"], p2d, max_err, p["K4"], n, p["sets"], trace=True)
        assert d["consumed"] == C.PNP_SETS
        fin = C.pnp_finite(d["R"], d["t"])
        assert np.all(d["count"][~fin] == 0)
        if p["kind"] == "general":
            assert fin.all()
        if collinear:
            import nppnp
            Rl, tl, *_ = nppnp.hypotheses(p["p3d"], p2d, p["K4"], p["sets"], lapack=True)
            assert np.array_equal(fin, C.pnp_finite(Rl, tl)), (fin, C.pnp_finite(Rl, tl))
        poses.append((d["R"], d["t"]))
    m = C.pnp_errors(poses)
    _summary("library", m, E)
    assert sorted(m) == sorted(b for b in E if b.startswith("pnp/"))
    C.check(m, E, "the traced poses of pnp.iterate against the ground truth")
