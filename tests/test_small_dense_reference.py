"""CPU side of the small dense tests: the mp reference tests/npdense.py pinned by hand values and identities, the numpy restatements of
csrc/small_dense.h and null_vector4_dev (npinit.jacobi / svd3 / inv3 / null_vector, nppnp.lstsq, npsim3solver.jacobi_sym4 - the device's
arithmetic, line for line) measured against it on the case table of tests/densecases.py, and the conditions on the table.  No GPU.

E_ref[bucket] = the restatement's largest figure in the bucket (metrics: densecases' docstring), committed in
tests/golden/small_dense_ref_err.npz and reproduced here.  Two conditions keep the golden from absorbing a defect: every E_ref is finite,
and in the gap-free metrics (values, reconstruction and definitions, orthogonality, proper) E_ref <= 1e-13 in every bucket.  Before the
rank rule of i_svd3 the restatement broke both: svd3/rank1/exact, svd3/zero and svd3/psd/collinear (exact) gave NaN in orthU, recon and
sign; svd3/rank1/outer gave orthU up to 1 (u1 a normalised noise column); svd3/rank2/zerocol gave proper = 2 (V a reflection by the
parity of the sort) before the sign rule for an exactly null third column.

Measured here (mp at 60 digits): 874 cases of the helpers, 627 buckets of them (356 of those the x2^+-200 copies) and 22 of the library-level problems.
  Gap-free buckets: largest 1.24e-14 (jacf/general/values, 9 columns of norm up to 3 sigma0); svd3 and sym4 stay below 3.3e-15.
  Every x2^+-200 bucket equals its unscaled bucket, and the restatement's outputs for 2^k A are == the rescaled outputs for A.
  Buckets above 1e-9, and why:
    inv3/cond=1e8 (x, det 1.0e-6) and inv3/cond=1e12 (10.6, 2.3): the cofactor formula loses cond^2 eps relative to |x*|: the reference's own
      3 x 3 inverse (Eigen's) is the same formula; the callers invert T of Normalize, K and H21, whose condition numbers are below 1e4.
    lstsq6n/cond=1e6/b=out (2e-6 to 1.6e-5), cond=1e10/b=in (4e-7 to 8e-7) and cond=1e10/b=out (2 to 4.2): the problem's own conditioning, cond eps with b in
      the range and cond^2 eps with a residual; LAPACK's lstsq shows the same sizes.  cond=1e10 keeps sigma_min / sigma_max = 1e-10, a
      hundred times clear of the 1e-12 cut; every other bucket has no ratio between 1e-14 and 1e-9 (test_table_conditions).
    null4/diag/1-s3/s2=1e-10 (vec/gap=1e-11: 1.3e-6) and svd3/graded/k=8 (vec/gap=1e-9: 3.9e-9): eps / gap.
    init/F/general/repeat/resid (2.9e-5) and pnp/planar (6.8e-5; nppnp(lapack=True) on minimal sets of 4 points with float32 image points,
      which is what the reference's RANSAC fits): figures of the problem, not of the arithmetic; an F fitted to 7 distinct points and cut
      to rank 2 no longer passes through them.  pnp/general is 0: no minimal set in general position qualifies (pnp_nondegenerate).
  The vector buckets elsewhere follow eps / gap: jacf/general gap=1e-5 1.4e-13, djac/planar proj gap=1e-4 2e-13, everything at gap >= 1e-2
  below 6e-14.
"""
import numpy as np
import pytest
from mpmath import mp, mpf

from tests import densecases as C
from tests import npdense as D


# ---------------------------------------------------------------- npdense itself
def test_svd_by_hand():
    with mp.workdps(D.DPS):
        U, S, V = D.svd(np.array([[0.0, 2, 0], [0, 0, -3], [1, 0, 0]]))                 # a signed permutation: sigma = 3, 2, 1
        assert [float(s) for s in S] == [3.0, 2.0, 1.0]
        assert D.maxabs(U * mp.diag(S) * V.T - D.M([[0.0, 2, 0], [0, 0, -3], [1, 0, 0]])) < mpf("1e-55")
        A = np.outer([3.0, 4.0, 0.0], [1.0, 2.0, 2.0])                                   # rank 1: sigma0 = 5 * 3
        U, S, V = D.svd(A)
        assert abs(S[0] - 15) < mpf("1e-55") and S[1] < mpf("1e-50") and S[2] < mpf("1e-50")
        assert D.vec_dist(np.array([0.6, 0.8, 0.0]), U[:, 0]) < 1e-16 and D.vec_dist(-np.array([1.0, 2.0, 2.0]) / 3.0, V[:, 0]) < 1e-16
        # a wide system has its null vector in right_vectors; sigma agrees with svd on the leading triples
        rng = np.random.default_rng(1)
        B = rng.normal(size=(8, 9))
        sig, Vr = D.right_vectors(B)
        assert sig[8] < mpf("1e-50") and D.maxabs(D.M(B) * Vr[:, 8]) < mpf("1e-50")
        assert max(abs(a - b) for a, b in zip(sig, D.svd(B)[1])) < mpf("1e-50")


def test_eigsy_inverse_lstsq_dlt_by_hand():
    with mp.workdps(D.DPS):
        N = np.array([[2.0, 1, 0, 0], [1, 2, 0, 0], [0, 0, -1, 0], [0, 0, 0, 5]])
        E, Q = D.eigsy4(N)
        assert [float(e) for e in E] == [-1.0, 1.0, 3.0, 5.0] and abs(abs(Q[3, 3]) - 1) < mpf("1e-55")
        A = np.array([[2.0, 0, 1], [0, 4, 0], [0, 0, 8]])
        assert float(D.det3(A)) == 64.0 and D.maxabs(D.inv3(A) - D.M([[0.5, 0, -0.0625], [0, 0.25, 0], [0, 0, 0.125]])) < mpf("1e-55")
        # least squares: two equal columns -> the minimum-norm solution splits the weight; a residual component does not move x
        A = np.array([[1.0, 1, 0], [0, 0, 2], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]])
        x, S = D.lstsq(A, np.array([4.0, 6, 7, 0, 0, 0]))
        assert D.rel_err(np.array([2.0, 2.0, 3.0]), x) < 1e-50 and S[2] < mpf("1e-50")
        # the rank rule itself: sigma = 1, 1e-11 is kept, 1, 1e-13 is cut
        for s1, want in ((1e-11, 1e11), (1e-13, 0.0)):
            x, _ = D.lstsq(np.diag([1.0, s1, 1.0])[[0, 1, 2, 0, 0, 0]] * np.array([1, 1, 1, 0, 0, 0.0])[:, None], np.array([1.0, 1, 1, 0, 0, 0]))
            assert abs(float(x[1]) - want) <= 1e-4 * max(want, 1e-300) + 0.0
        # DLT: two cameras a baseline apart looking along z, a point at (0.5, 0, 4)
        T1 = np.hstack([np.eye(3), np.zeros((3, 1))]); T2 = np.hstack([np.eye(3), np.array([[-1.0], [0], [0]])])
        X, S = D.dlt_point(T1, T2, (0.125, 0.0), (-0.125, 0.0))
        assert max(abs(a - b) for a, b in zip(X, (0.5, 0, 4))) < mpf("1e-50") and S[3] < mpf("1e-50")


def test_metrics_by_hand():
    v = np.array([1.0, 0, 0]); t = mp.matrix([mpf(1), mpf("1e-12"), 0])
    assert abs(D.vec_dist(v, t) - 1e-12) < 1e-20 and abs(D.vec_dist(-v, t) - 1e-12) < 1e-20             # the distance itself, either sign
    assert D.vec_dist(np.array([np.nan, 0, 0]), t) == D.INF
    assert D.orth_err(np.eye(3)) == 0.0 and abs(D.orth_err(np.array([[1.0, 1e-8], [0, 1.0]])) - 1e-8) < 1e-15
    A = np.diag([3.0, 2.0, 1.0]); I = np.eye(3)
    m = D.svd3_metrics(A, I, np.array([3.0, 2.0, 1.0]), I, [mpf(3), mpf(2), mpf(1)])
    assert set(m.values()) == {0.0}
    m = D.svd3_metrics(A, I, np.array([3.0, 2.0, 1.0]), np.diag([1.0, 1.0, -1.0]), [mpf(3), mpf(2), mpf(1)])   # the sign convention
    assert abs(m["sign"] - 2.0 / 3.0) < 1e-15 and abs(m["recon"] - 2.0 / 3.0) < 1e-15 and m["orthV"] == 0.0
    assert abs(D.residual_excess(np.diag([2.0, 1.0]), np.array([0.0, 1.0]), mpf(1), mpf(2))) == 0.0
    assert abs(D.residual_excess(np.diag([2.0, 1.0]), np.array([1.0, 0.0]), mpf(1), mpf(2)) - 0.5) < 1e-15
    assert D.projector_err(np.eye(3)[:, [1, 0]], mp.matrix([[1, 0], [0, -1], [0, 0]])) == 0.0                    # the span, not the basis


# ---------------------------------------------------------------- the table
def test_table_conditions():
    cs = C.cases()
    assert 800 <= C.n_cases() <= 1500
    for name in C.ORDER:
        a = C.inputs(name)
        assert a.shape == (len(cs[name]), C.NIN[name])
    assert len(cs["djac16"]) == 17 and cs["djac16"] is cs["djac"]
    assert np.isnan(C.inputs("sym4")).any(1).sum() == 1 and all(np.all(np.isfinite(C.inputs(n))) for n in C.ORDER if n != "sym4")
    # i_svd3: every edge of the issue has its bucket, and each comes back times 2^+-200
    b = {c["bucket"] for c in cs["svd3"]}
    for k in ("generic", "negdet", "tie2/essential", "tie2/0.3", "tie3", "rank2/zerocol", "rank2/noise", "rank1/exact", "rank1/outer", "zero",
              "graded/k=2", "graded/k=4", "graded/k=6", "graded/k=8", "psd/full", "psd/planar", "psd/collinear"):
        assert {k, k + "/x2^+200", k + "/x2^-200"} <= b, k
    for c, t in zip(cs["svd3"], C.truth("svd3")):
        if c["bucket"] == "negdet":
            assert np.linalg.det(c["A"].reshape(3, 3)) < 0
        if c["bucket"].startswith("rank1") or c["bucket"].startswith("psd/collinear"):
            assert t["S"][1] <= mpf("1e-15") * t["S"][0]
    # d_lstsq: no singular value near the cut
    for n in (3, 4, 5):
        for c, t in zip(cs["lstsq6%d" % n], C.truth("lstsq6%d" % n)):
            lo = 0.99e-10 if c["bucket"].startswith("cond=1e10") else 1e-9
            assert all(not (1e-14 < float(s / t["S"][0]) < lo) for s in t["S"]), (c["bucket"], [float(s / t["S"][0]) for s in t["S"]])
            if c["bucket"].startswith("dependent"):
                assert float(t["S"][-1] / t["S"][0]) < 1e-14
    # the 'residual only' systems do have a null space of dimension >= 2 to the size of their float32 coordinates, the others a gap
    for name in ("jach", "jacf"):
        for c, t in zip(cs[name], C.truth(name)):
            if c["base"] is None:
                assert (float(t["gap"]) < 1e-5) == c["resid_only"], (name, c["bucket"], float(t["gap"]))
    # null_vector4_dev: the ladder's rungs and the near-ties
    b = {c["bucket"] for c in cs["null4"]}
    assert {"dlt/cos=%g" % c for c in C.COS_LADDER} <= b and {"diag/1-s3/s2=1e-2", "diag/1-s3/s2=1e-6", "diag/1-s3/s2=1e-10"} <= b
    # the 12 x 12: a null space of dimension 1 (general, n >= 6), and of 4 (near-orthographic: four values below 1e-4 of the fifth smallest)
    for c, t in zip(cs["djac"], C.truth("djac")):
        if c["bucket"] == "general" and c["n"] >= 6:
            assert t["sig"][11] < mpf("1e-13") * t["sig"][0] < t["sig"][10] * mpf("1e-3")
        if c["bucket"] == "ortho" and c["n"] >= 6:
            assert t["sig"][8] < mpf("1e-4") * t["sig"][7]
    # sym4: the ties are ties
    for c, t in zip(cs["sym4"], C.truth("sym4")):
        if c["bucket"] == "horn/collinear":
            assert float(t["gap"]) < 1e-12
        if c["bucket"] == "horn/generic":
            assert float(t["gap"]) > 1e-3


def test_triangulation_inputs_leave_out_few():
    """the gates in mp alone: at most 5 % of the 257 matches lie within 1e-4 of a threshold, both flags occur on every rung below the gate"""
    tr, p = C.tri_truth(), C.tri_problem()
    flags = [t[0] for t in tr]
    assert len(flags) == 257 and flags.count(None) <= 0.05 * 257, flags.count(None)
    for cos in C.TRI_COS:
        got = {f for f, r in zip(flags, p["rung"]) if r == "cos=%g" % cos}
        assert (got >= {0, 1}) if cos < 0.9998 else (got <= {0, None} and 0 in got), (cos, got)


# ---------------------------------------------------------------- the restatements against mp
@pytest.fixture(scope="module")
def measured():
    return C.measure_ref()


def test_restatement_reproduces_the_committed_table(measured):
    E = C.load_golden()
    lib = {b for b in E if b.split("/")[0] in ("tri", "init", "pnp")}
    assert sorted(set(E) - lib) == sorted(measured)
    bad = [(b, measured[b], E[b]) for b in measured if not (measured[b] <= 2 * E[b] + 1e-30 and E[b] <= 2 * measured[b] + 1e-30)]
    assert not bad, bad[:10]
    print("%d buckets, %d above 1e-9, largest gap-free %.3g" % (len(measured), sum(e > 1e-9 for e in measured.values()),
                                                                max(e for b, e in measured.items() if C.is_gapfree(b))))


def test_restatement_is_finite_and_capped_where_no_gap_excuses_it(measured):
    """the two conditions on E_ref: a NaN, a 0.88 or a 1e-5 in a gap-free metric is a defect, not a figure"""
    bad = ["%s: %.3g" % (b, e) for b, e in sorted(measured.items()) if not np.isfinite(e) or (C.is_gapfree(b) and not e <= C.GAPFREE_CAP)]
    assert not bad, "E_ref not finite, or above 1e-13 in a gap-free metric:\n  " + "\n  ".join(bad)


def test_buckets_above_1e_9_are_the_ones_the_docstring_names(measured):
    E = dict(C.load_golden())
    for b, e in E.items():
        if e > 1e-9:
            assert (b.startswith("inv3/cond=1e8") or b.startswith("inv3/cond=1e12") or (b.startswith("lstsq6") and ("cond=1e10" in b or "cond=1e6/b=out" in b))
                    or b.startswith("null4/diag/1-s3/s2=1e-10") or (b.startswith("svd3/graded/k=8") and "/vec/gap=1e-9" in b) or b == "init/F/general/repeat/resid"
                    or b == "pnp/planar/pose"), (b, e)


def test_scaling_by_a_power_of_two_is_exact_in_the_restatement():
    assert C.scale_mismatches(C.restate()) == []
    E = C.load_golden()
    for b in E:
        if "/x2^" in b:
            base = b.replace("/x2^+200", "").replace("/x2^-200", "")
            assert E[b] == E[base], b


def test_library_level_figures_reproduce():
    E = C.load_golden()
    m = C.library_ref()
    assert sorted(m) == sorted(b for b in E if b.split("/")[0] in ("tri", "init", "pnp"))
    bad = [(b, m[b], E[b]) for b in m if not (m[b] <= 2 * E[b] + 1e-30 and E[b] <= 2 * m[b] + 1e-30)]
    assert not bad, bad
    assert all(np.isfinite(v) for v in m.values())
    # the collinear candidate: nppnp(lapack=True) and the restatement of the device agree on which poses are finite
    import nppnp
    p = C.pnp_problems()[2]
    R, t, *_ = nppnp.hypotheses(p["p3d"], p["p2d"], p["K4"], p["sets"])
    assert np.array_equal(C.pnp_finite(R, t), C.pnp_finite(*C.pnp_lapack()[2]))


def test_probe_compiles(tmp_path):
    C.build_probe(tmp_path, C.PROBE_SRC)
