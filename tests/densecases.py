"""The case table of the small dense helpers (csrc/small_dense.h, null_vector4_dev of csrc/tri_math.h) and what is measured of them,
shared by tests/test_small_dense_reference.py (the numpy restatements against mp: E_ref, on the CPU) and tests/test_gpu_small_dense.py
(the device, through tools/ubench/small_dense_probe.hip and through the library).  Matrices are built as Q1 diag(sigma) Q2^T with seeded
orthogonal factors, or as the estimators build them (init_hyp's systems, fill_M's M^T M, the DLT of one match, Horn's N), so that the
structure of the truth is known; the truth itself is tests/npdense.py on the float64 matrix as built.

A case carries a bucket; every metric of the case goes to the bucket "<function>/<bucket>/<metric>".  Metrics (tests/npdense.py):
  gap-free: values, recon, sign, orthU, orthV, proper (i_svd3; proper = |det U det V - 1| where the third column is exactly null); values, av, orthV, cosU (the one-sided Jacobi outputs); values, nv, orthV (sym4)
  with a gap or a condition number in the name: vec/gap=1e-k (a singular vector whose sigma is separated by that much, relative to sigma0,
  as the distance min(|x - x*|, |x + x*|)), resid ("residual only" buckets: |A x| / sigma0 - sigma_min / sigma0), proj/gap=1e-k (the
  projector onto the four smallest columns of the 12 x 12), x (d_lstsq, i_inv3: |x - x*| / |x*|), det, nonfinite / returns (0 or inf).
Cases "<bucket>/x2^+200" are the same matrices times 2^+-200: their outputs are rescaled exactly and measured like the others, and
compared == with the outputs of the unscaled case (scale_mismatches).
The acceptance rule is sim3mathcases.check: per bucket max e <= max(64 * 2.2e-16, 8 * E_ref[bucket])."""
import functools
import os
import sys

import numpy as np
from mpmath import mp, mpf

from tests import npdense as D
from tests.sim3mathcases import ROOT, bound, build_probe, check, fold  # noqa: F401  (the rule and the helpers of the Sim(3) work)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))    # the restatements import one another by their plain names
import npinit  # noqa: E402
import nppnp  # noqa: E402
import npsim3solver  # noqa: E402

PROBE_SRC = os.path.join(ROOT, "tools", "ubench", "small_dense_probe.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "small_dense_ref_err.npz")
GAPFREE = ("values", "recon", "sign", "orthU", "orthV", "proper", "av", "cosU", "nv")
GAPFREE_CAP = 1e-13
SCALE_K = (200, -200)

ORDER = ("svd3", "inv3", "jach", "jacf", "null4", "djac", "djac16", "lstsq63", "lstsq64", "lstsq65", "sym4")
FID = {n: i for i, n in enumerate(ORDER)}
NIN = dict(svd3=9, inv3=9, jach=144, jacf=72, null4=16, djac=144, djac16=144, lstsq63=24, lstsq64=30, lstsq65=36, sym4=16)
NOUT = dict(svd3=21, inv3=10, jach=226, jacf=154, null4=4, djac=288, djac16=288, lstsq63=3, lstsq64=4, lstsq65=5, sym4=20)
SCALED_PART = dict(svd3=slice(9, 12), jach=slice(0, 144), jacf=slice(0, 72), sym4=slice(0, 4))      # the outputs that scale with A


def _orth(rng, n, det=None):
    Q, R = np.linalg.qr(rng.normal(size=(n, n)))
    Q = Q * np.sign(np.diag(R))
    if det is not None and np.linalg.det(Q) * det < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


def _qsq(rng, sig, m=None, det=None):
    """Q1 diag(sig) Q2^T, m x n"""
    n = len(sig); m = n if m is None else m
    Q1 = _orth(rng, m, det)[:, :n]; Q2 = _orth(rng, n, 1 if det is not None else None)
    return (Q1 * np.asarray(sig, np.float64)) @ Q2.T


def _case(A, bucket, sig=None, **kw):
    return dict(A=np.ascontiguousarray(A, np.float64), bucket=bucket, sig=None if sig is None else [float(s) for s in sig], base=None, k=0, **kw)


def _with_scales(cases):
    out = list(cases)
    for k in SCALE_K:
        for i, c in enumerate(cases):
            if c.get("noscale"):
                continue
            d = dict(c); d["A"] = np.ldexp(c["A"], k); d["bucket"] = "%s/x2^%+d" % (c["bucket"], k); d["base"] = i; d["k"] = k
            out.append(d)
    return out


def _gap_label(g):
    return "gap=1e%d" % int(np.floor(np.log10(float(g)) + 1e-9)) if g > 0 else "gap=0"


# ---------------------------------------------------------------- i_svd3
def _svd3_cases():
    rng = np.random.default_rng(101)
    c = []
    for sig in ((3, 2, 1), (10, 1, 0.1), (1.5, 1.2, 1.0), (7.3, 0.9, 0.02), (2, 1.9, 0.5), (100, 3, 0.7)):
        c.append(_case(_qsq(rng, sig, det=1), "generic", sig))
        c.append(_case(_qsq(rng, sig, det=-1), "negdet", sig))
    for _ in range(8):
        c.append(_case(_qsq(rng, (1, 1, 0)), "tie2/essential", (1, 1, 0)))
        c.append(_case(_qsq(rng, (1, 1, 0.3)), "tie2/0.3", (1, 1, 0.3)))
        c.append(_case(_orth(rng, 3, 1), "tie3", (1, 1, 1)))
        c.append(_case(_qsq(rng, (2, 1, 0)), "rank2/noise", (2, 1, 0)))
        c.append(_case(np.outer(rng.normal(size=3), rng.normal(size=3)), "rank1/outer", None, rank1=True))
    c.append(_case(np.eye(3), "tie3", (1, 1, 1))); c.append(_case(-np.eye(3), "tie3", (1, 1, 1))); c.append(_case(2.5 * np.eye(3)[[1, 2, 0]], "tie3", (2.5, 2.5, 2.5)))
    for p in ([0, 1, 2], [2, 0, 1], [1, 2, 0], [0, 2, 1], [2, 1, 0]):               # an exact zero column: (Q1 diag(sig)) P
        B = _orth(rng, 3) * np.array([2.0, 1.0, 0.0])
        c.append(_case(B[:, p], "rank2/zerocol", (2, 1, 0), proper=True))
    for A in (np.diag([2.0, 0, 0]), np.diag([0, 0, 3.0]), np.diag([0, -1.5, 0])):
        c.append(_case(A, "rank1/exact", None, rank1=True))
    for (i, j, v) in ((1, 2, 5.0), (2, 0, -4.0), (0, 1, 0.3)):
        A = np.zeros((3, 3)); A[i, j] = v
        c.append(_case(A, "rank1/exact", None, rank1=True))
    c.append(_case(np.zeros((3, 3)), "zero", (0, 0, 0)))
    for k in (2, 4, 6, 8):
        sig = (1.0, 10.0 ** -k, 10.0 ** (-2 * k))
        for _ in range(6):
            c.append(_case(_qsq(rng, sig), "graded/k=%d" % k, sig))
    for name, sig in (("psd/full", (3, 2, 1)), ("psd/planar", (2, 1, 0)), ("psd/collinear", (2, 0, 0))):
        for _ in range(6):
            Q = _orth(rng, 3)
            A = (Q * np.array(sig, np.float64)) @ Q.T
            c.append(_case((A + A.T) / 2, name, sig if name != "psd/collinear" else None, rank1=name == "psd/collinear"))
    # covariances of actual points, as EPnP forms them: planar z = 0 and collinear on an axis leave exact zeros
    P = rng.normal(size=(12, 3)); P[:, 2] = 0; d = P - P.mean(0)
    c.append(_case(d.T @ d, "psd/planar", None, proper=True))
    P = np.zeros((12, 3)); P[:, 0] = rng.normal(size=12); d = P - P.mean(0)
    c.append(_case(d.T @ d, "psd/collinear", None, rank1=True))
    return _with_scales(c)


# ---------------------------------------------------------------- i_inv3, i_det3
def _inv3_cases():
    rng = np.random.default_rng(102)
    c = []
    for lab, cond in (("1", 1.0), ("1e4", 1e4), ("1e8", 1e8), ("1e12", 1e12)):
        for _ in range(8):
            c.append(_case(rng.uniform(0.5, 3) * _qsq(rng, (1.0, cond ** -0.5, 1.0 / cond)), "cond=" + lab))
    for (mx, my, sx, sy) in ((320.5, 240.25, 1 / 85.0, 1 / 60.0), (512.0, 384.0, 0.01, 0.0125), (-3.0, 7.0, 2.0, 0.5)):
        sx, sy, mx, my = (np.float32(v) for v in (sx, sy, mx, my))
        c.append(_case(np.array([[sx, 0, np.float64(-mx * sx)], [0, sy, np.float64(-my * sy)], [0, 0, 1.0]], np.float64), "normalizeT"))
    for K4 in ((517.3, 516.5, 318.6, 255.3), (718.856, 718.856, 607.19, 185.22)):
        fx, fy, cx, cy = (np.float64(np.float32(v)) for v in K4)
        c.append(_case(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]), "K"))
    for A in (np.arange(1.0, 10.0).reshape(3, 3), np.zeros((3, 3)), np.diag([1.0, 1.0, 0.0]), np.array([[1.0, 2, 3], [2, 4, 6], [0, 1, 5]])):
        c.append(_case(A, "singular", singular=True))
    return c


# ---------------------------------------------------------------- the systems of init_hyp (orb_init.inc:195-202)
def _scene(rng, n, planar):
    """n matches of a two-view scene in normalised float32 coordinates (mean 0, mean absolute deviation 1 per axis and image)"""
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), (np.full(n, 6.0) if planar else rng.uniform(4, 9, n))], 1)
    if planar:
        X[:, 2] += 0.3 * X[:, 0] - 0.2 * X[:, 1]
    th = 0.15
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]]); t = np.array([-0.8, 0.05, 0.1])
    out = []
    for Xc in (X, X @ R.T + t):
        uv = 500.0 * Xc[:, :2] / Xc[:, 2:3] + np.array([320.0, 240.0])
        uv = uv.astype(np.float32)
        m = uv.mean(0); d = uv - m
        out.append((d / np.abs(d).mean(0)).astype(np.float32))
    return out[0], out[1]


def hyp_systems(p1, p2, sets):
    """(B, 16, 9) and (B, 8, 9): float products stored in double, as init_hyp stores them"""
    u1 = p1[sets, 0]; v1 = p1[sets, 1]; u2 = p2[sets, 0]; v2 = p2[sets, 1]
    B = len(sets)
    Ah = np.zeros((B, 16, 9)); Af = np.zeros((B, 8, 9))
    for j in range(8):
        a, b, c, d = u1[:, j], v1[:, j], u2[:, j], v2[:, j]
        Ah[:, 2 * j, 0] = -a; Ah[:, 2 * j, 1] = -b; Ah[:, 2 * j, 2] = -1.0
        Ah[:, 2 * j, 6] = a * c; Ah[:, 2 * j, 7] = b * c; Ah[:, 2 * j, 8] = c
        Ah[:, 2 * j + 1, 3] = -a; Ah[:, 2 * j + 1, 4] = -b; Ah[:, 2 * j + 1, 5] = -1.0
        Ah[:, 2 * j + 1, 6] = a * d; Ah[:, 2 * j + 1, 7] = b * d; Ah[:, 2 * j + 1, 8] = d
        Af[:, j] = np.stack([c * a, c * b, c, d * a, d * b, d, a, b, np.ones_like(a)], 1)
    return Ah, Af


def _collinear_scene(rng, n):
    s = np.linspace(-1.7, 1.9, n) + rng.uniform(-0.05, 0.05, n)
    p1 = np.stack([s, 0.4 * s + 0.1], 1).astype(np.float32)
    p2 = np.stack([0.9 * s + 0.2, -0.3 * s + 0.05], 1).astype(np.float32)
    return p1, p2


@functools.lru_cache(maxsize=None)
def _hyp_cases():
    rng = np.random.default_rng(103)
    H, F = [], []
    for kind, nset in (("general", 6), ("planar", 6), ("repeat", 4), ("collinear", 3)):
        p1, p2 = _collinear_scene(rng, 40) if kind == "collinear" else _scene(rng, 40, kind == "planar")
        sets = np.stack([rng.choice(40, 8, replace=False) for _ in range(nset)])
        if kind == "repeat":
            sets[:, 7] = sets[:, 2]; sets[2:, 6] = sets[2:, 0]                      # one point twice; two points twice
        Ah, Af = hyp_systems(p1, p2, sets)
        for a, f in zip(Ah, Af):
            H.append(_case(a, kind, resid_only=kind == "collinear"))
            F.append(_case(f, kind, resid_only=kind != "general"))
    return _with_scales(H), _with_scales(F)


# ---------------------------------------------------------------- null_vector4_dev
K_TRI = (458.654, 457.296, 367.215, 248.375)
COS_LADDER = (0.9, 0.99, 0.999, 0.9997, 0.99979)


def tri_geometry(cos, depth, rng):
    """two cameras a baseline b = 1 / depth apart and a point seen under a parallax angle of acos(cos), which puts it 0.5 / tan(angle / 2)
    baselines in front of them (`depth` only sets the scale of the scene): returns (T1, T2 (3 x 4), X)"""
    half = 0.5 * np.arccos(cos)
    b = 1.0 / depth
    z = 0.5 * b / np.tan(half)
    X = np.array([rng.uniform(-0.1, 0.1) * z, rng.uniform(-0.1, 0.1) * z, z])
    T1 = np.hstack([np.eye(3), np.array([[0.5 * b], [0], [0]])])
    th = rng.uniform(-0.02, 0.02)
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    T2 = np.hstack([R, R @ np.array([[-0.5 * b], [0], [0]])])
    return T1, T2, X


def project_px(T, X, K4):
    x = T[:, :3] @ X + T[:, 3]
    return np.array([K4[0] * x[0] / x[2] + K4[2], K4[1] * x[1] / x[2] + K4[3]]).astype(np.float32)


def xn_of(px, K4):
    """tri_math.h:57-60: float arithmetic, then widened"""
    K = np.asarray(K4, np.float32)
    return np.array([np.float64((px[0] - K[2]) * (np.float32(1.0) / K[0])), np.float64((px[1] - K[3]) * (np.float32(1.0) / K[1]))])


def dlt_f64(T1, T2, xn1, xn2):
    T1 = np.asarray(T1, np.float64).reshape(12); T2 = np.asarray(T2, np.float64).reshape(12)
    A = np.empty((4, 4))
    for j in range(4):
        A[0, j] = xn1[0] * T1[8 + j] - T1[j]; A[1, j] = xn1[1] * T1[8 + j] - T1[4 + j]
        A[2, j] = xn2[0] * T2[8 + j] - T2[j]; A[3, j] = xn2[1] * T2[8 + j] - T2[4 + j]
    return A


def _null4_cases():
    rng = np.random.default_rng(104)
    c = []
    for cos in COS_LADDER:
        for depth in (1.0, 30.0, 1e3):
            for _ in range(4):
                T1, T2, X = tri_geometry(cos, depth, rng)
                A = dlt_f64(T1, T2, xn_of(project_px(T1, X, K_TRI), K_TRI), xn_of(project_px(T2, X, K_TRI), K_TRI))
                c.append(_case(A, "dlt/cos=%g" % cos))
    for lab, dl in (("1e-2", 1e-2), ("1e-6", 1e-6), ("1e-10", 1e-10)):
        for _ in range(8):
            c.append(_case(_qsq(rng, (3.0, 2.0, 1.0, 1.0 - dl)), "diag/1-s3/s2=" + lab))
    return c


# ---------------------------------------------------------------- d_jacobi 12 x 12 on fill_M's M^T M
def mtm_of(pw, uv, K4):
    """EPnP's M^T M (12 x 12) of noise-free points: control points from the covariance's eigenvectors, barycentric coordinates through the
    pseudo-inverse (a planar or collinear set leaves exact zero columns), fill_M (reference :441-456).  The input need not have the device's
    bits: it is the Jacobi on it that is under test."""
    fu, fv, uc, vc = K4
    n = len(pw)
    c0 = pw.mean(0); d = pw - c0
    w, E = np.linalg.eigh(d.T @ d)
    w = np.where(w < 1e-12 * w.max(), 0.0, w)
    cws = np.vstack([c0] + [c0 + np.sqrt(w[i] / n) * E[:, i] for i in (2, 1, 0)])
    cc = (cws[1:] - cws[0]).T
    al = np.empty((n, 4))
    al[:, 1:] = d @ np.linalg.pinv(cc, rcond=1e-12).T
    al[:, 0] = 1.0 - al[:, 1:].sum(1)
    Mm = np.zeros((2 * n, 12))
    for k in range(4):
        Mm[0::2, 3 * k] = al[:, k] * fu; Mm[0::2, 3 * k + 2] = al[:, k] * (uc - uv[:, 0])
        Mm[1::2, 3 * k + 1] = al[:, k] * fv; Mm[1::2, 3 * k + 2] = al[:, k] * (vc - uv[:, 1])
    G = Mm.T @ Mm
    return np.triu(G) + np.triu(G, 1).T


def _djac_cases():
    rng = np.random.default_rng(105)
    K4 = (520.0, 515.0, 320.0, 240.0)
    th = 0.4
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    c = []
    for kind, ns in (("general", (4, 5, 6, 8, 12, 20)), ("planar", (4, 5, 6, 8, 12, 20)), ("ortho", (4, 6, 8, 12, 20))):
        for n in ns:
            pw = rng.uniform(-1, 1, (n, 3))
            if kind == "planar":
                pw[:, 2] = 0.0
            t = np.array([0.2, -0.1, 400.0 if kind == "ortho" else 5.0])
            f = 40.0 if kind == "ortho" else 1.0                  # a long lens far away: depth varies by 0.5 % over the set
            pc = pw @ R.T + t
            uv = np.stack([f * K4[0] * pc[:, 0] / pc[:, 2] + K4[2], f * K4[1] * pc[:, 1] / pc[:, 2] + K4[3]], 1)
            c.append(_case(mtm_of(pw, uv, (f * K4[0], f * K4[1], K4[2], K4[3])), "%s" % kind, n=n))
    assert len(c) == 17                                           # one full block of 16 lanes and a ragged one
    return c


# ---------------------------------------------------------------- d_lstsq
def _lstsq_cases(n):
    rng = np.random.default_rng(106 + n)
    c = []

    def add(sig, lab):
        for where in ("in", "out"):
            for _ in range(5):
                Q1 = _orth(rng, 6); Q2 = _orth(rng, n)
                A = (Q1[:, :n] * np.asarray(sig)) @ Q2.T
                b = A @ rng.normal(size=n)
                if where == "out":
                    b = b + 0.5 * np.abs(b).max() * Q1[:, n]
                c.append(_case(np.concatenate([A.reshape(-1), b]), "%s/b=%s" % (lab, where)))
    for lab, cond in (("cond=1e2", 1e2), ("cond=1e6", 1e6), ("cond=1e10", 1e10)):
        add(cond ** (-np.arange(n) / (n - 1.0)), lab)
    add(np.concatenate([2.0 ** -np.arange(n - 1), [0.0]]), "dependent")
    return c


# ---------------------------------------------------------------- i_jacobi_sym4
def _sym4_cases():
    rng = np.random.default_rng(107)
    c = []

    def horn(a, kind):
        Rm = _orth(rng, 3, 1); s = rng.uniform(0.5, 2.0)
        b = s * a @ Rm.T + rng.normal(size=3)
        N, *_ = npsim3solver.horn_N(a, b)
        c.append(_case(np.array(N), kind))
    for _ in range(10):
        horn(rng.normal(size=(3, 3)), "horn/generic")
    for _ in range(6):
        d = rng.normal(size=3); o = rng.normal(size=3)
        horn(np.stack([o + s * d for s in (-1.0, 0.25, 2.0)]), "horn/collinear")
    for lab, lam in (("pairs", (2, 1, -1, -2)), ("pairs11", (1, 1, -1, -1)), ("tie4", (1, 1, 1, 1)), ("2,2,2,-6", (2, 2, 2, -6)), ("graded", (1, 1e-5, -1e-10, 1e-15))):
        for _ in range(6):
            Q = _orth(rng, 4)
            A = (Q * np.array(lam, np.float64)) @ Q.T
            c.append(_case((A + A.T) / 2, lab))
    c.append(_case(np.eye(4), "tie4")); c.append(_case(-3.0 * np.eye(4), "tie4"))
    c.append(_case(np.zeros((4, 4)), "zero"))
    A = np.array(c[0]["A"]); A[1, 1] = np.nan                                    # on the diagonal: the output keeps it (fro is NaN, nothing is rotated)
    c.append(_case(A, "nonfinite", nonfinite=True, noscale=True))
    return _with_scales(c)


@functools.lru_cache(maxsize=None)
def cases():
    H, F = _hyp_cases()
    dj = _djac_cases()
    return dict(svd3=_svd3_cases(), inv3=_inv3_cases(), jach=H, jacf=F, null4=_null4_cases(), djac=dj, djac16=dj,
                lstsq63=_lstsq_cases(3), lstsq64=_lstsq_cases(4), lstsq65=_lstsq_cases(5), sym4=_sym4_cases())


def inputs(name):
    return np.stack([c["A"].reshape(-1) for c in cases()[name]])


def n_cases():
    return sum(len(v) for v in cases().values())


# ---------------------------------------------------------------- the probe's files (the section format of the Sim(3) probe, device values only)
def pack():
    out = []
    for name in ORDER:
        a = inputs(name)
        assert a.shape[1] == NIN[name]
        out += [np.array([FID[name], len(a)], np.float64), a.reshape(-1)]
    return np.concatenate(out).astype("<f8").tobytes()


def unpack(blob):
    a = np.frombuffer(blob, "<f8")
    pos, dev = 0, {}
    for name in ORDER:
        f, n, no = int(a[pos]), int(a[pos + 1]), int(a[pos + 2]); pos += 3
        assert (f, n, no) == (FID[name], len(cases()[name]), NOUT[name]), (name, f, n, no)
        dev[name] = a[pos:pos + n * no].reshape(n, no); pos += n * no
    assert pos == len(a)
    return dev


def run_probe(exe, workdir):
    import subprocess
    cin, cout = os.path.join(str(workdir), "cases.bin"), os.path.join(str(workdir), "results.bin")
    with open(cin, "wb") as f:
        f.write(pack())
    r = subprocess.run([exe, cin, cout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(cout, "rb") as f:
        return unpack(f.read())


# ---------------------------------------------------------------- the numpy restatements, in the probe's output layout
@functools.lru_cache(maxsize=None)
def restate():
    out = {}
    with np.errstate(all="ignore"):
        A = inputs("svd3").reshape(-1, 3, 3)
        U, S, V = npinit.svd3(A)
        out["svd3"] = np.concatenate([U.reshape(-1, 9), S, V.reshape(-1, 9)], 1)
        A = inputs("inv3").reshape(-1, 3, 3)
        out["inv3"] = np.concatenate([npinit.inv3(A).reshape(-1, 9), npinit.det3(A)[:, None]], 1)
        for name, m in (("jach", 16), ("jacf", 8)):
            A = inputs(name).reshape(-1, m, 9)
            U, V = npinit.jacobi(A)
            out[name] = np.concatenate([U.reshape(len(A), -1), V.reshape(len(A), -1), npinit.min_col(U)[:, None].astype(np.float64)], 1)
        out["null4"] = npinit.null_vector(inputs("null4").reshape(-1, 4, 4), tol=1e-16, null_rule=False)
        A = inputs("djac").reshape(-1, 12, 12)
        U, V = npinit.jacobi(A)
        out["djac"] = out["djac16"] = np.concatenate([U.reshape(-1, 144), V.reshape(-1, 144)], 1)
        for n in (3, 4, 5):
            a = inputs("lstsq6%d" % n)
            out["lstsq6%d" % n] = nppnp.lstsq(a[:, :6 * n].reshape(-1, 6, n), a[:, 6 * n:])
        rows = []
        for a in inputs("sym4"):
            lam, V = npsim3solver.jacobi_sym4(a.reshape(4, 4))
            rows.append(np.concatenate([lam, np.array(V).reshape(-1)]))
        out["sym4"] = np.array(rows)
    return out


# ---------------------------------------------------------------- truth (mp), once per process
def _rel_gaps(sig):
    """relative gap of each sigma to its nearest neighbour, in units of sigma0"""
    s0 = sig[0] if sig[0] > 0 else mpf(1)
    return [min(abs(sig[i] - sig[j]) for j in range(len(sig)) if j != i) / s0 for i in range(len(sig))]


@functools.lru_cache(maxsize=None)
def truth(name):
    out = []
    with mp.workdps(D.DPS):
        for c in cases()[name]:
            if c["base"] is not None:
                out.append(out[c["base"]]); continue
            A = c["A"]
            if name == "svd3":
                U, S, V = D.svd(A.reshape(3, 3))
                out.append(dict(U=U, S=S, V=V, gaps=_rel_gaps(S)))
            elif name == "inv3":
                out.append(None if c.get("singular") else dict(inv=D.inv3(A.reshape(3, 3)), det=D.det3(A.reshape(3, 3))))
            elif name in ("jach", "jacf", "null4"):
                m = dict(jach=16, jacf=8, null4=4)[name]
                sig, V = D.right_vectors(A.reshape(m, -1))
                out.append(dict(sig=sig, x=[V[r, V.cols - 1] for r in range(V.rows)], gap=(sig[-2] - sig[-1]) / sig[0]))
            elif name in ("djac", "djac16"):
                sig, V = D.right_vectors(A.reshape(12, 12))
                out.append(dict(sig=sig, V4=V[:, 8:12], gap=(sig[7] - sig[8]) / sig[0]))
            elif name.startswith("lstsq"):
                n = int(name[-1])
                x, S = D.lstsq(A[:6 * n].reshape(6, n), A[6 * n:])
                out.append(dict(x=x, S=S))
            elif name == "sym4":
                if c.get("nonfinite"):
                    out.append(None); continue
                E, Q = D.eigsy4(A.reshape(4, 4))
                lm = max(abs(e) for e in E); lm = lm if lm > 0 else mpf(1)
                out.append(dict(lam=E, top=[Q[r, 3] for r in range(4)], gap=(E[3] - E[2]) / lm))
    return out


VEC_MIN_GAP = 1e-12                                               # below this a vector is tied to working precision: not measured


def unscale(name, row, k):
    r = np.array(row, np.float64, copy=True)
    if k:
        r[SCALED_PART[name]] = np.ldexp(r[SCALED_PART[name]], -k)
    return r


def case_errors(name, c, base_A, row, tr):
    """metric -> e of one case; row = the probe's (or the restatement's) output row, already rescaled for a x2^k case"""
    A = base_A
    if name == "svd3":
        A = A.reshape(3, 3); U = row[:9].reshape(3, 3); S = row[9:12]; V = row[12:].reshape(3, 3)
        e = D.svd3_metrics(A, U, S, V, tr["S"])
        if np.all(np.isfinite(row)):
            for k in range(3):
                g = float(tr["gaps"][k])
                if g >= VEC_MIN_GAP:
                    lab = "vec/" + _gap_label(g)
                    e[lab] = max(e.get(lab, 0.0), D.vec_dist(U[:, k], tr["U"][:, k]), D.vec_dist(V[:, k], tr["V"][:, k]))
        if c.get("proper"):                                       # an exactly null third column: U and V both proper, so that U V^T is a rotation
            e["proper"] = float(abs(np.linalg.det(U) * np.linalg.det(V) - 1.0)) if np.all(np.isfinite(row)) else D.INF
        return e
    if name == "inv3":
        if c.get("singular"):
            return {"nonfinite": 0.0 if not np.all(np.isfinite(row[:9])) else D.INF}
        d = float(abs(mpf(float(row[9])) - tr["det"]) / abs(tr["det"])) if np.isfinite(row[9]) else D.INF
        return {"x": D.rel_err(row[:9], [tr["inv"][i, j] for i in range(3) for j in range(3)]), "det": d}
    if name in ("jach", "jacf"):
        m = 16 if name == "jach" else 8
        A = A.reshape(m, 9); U = row[:m * 9].reshape(m, 9); V = row[m * 9:m * 9 + 81].reshape(9, 9)
        e = D.jacobi_metrics(A, U, V, tr["sig"])
        col = int(row[-1]) if np.isfinite(row[-1]) and 0 <= row[-1] < 9 else 0
        x = V[:, col]
        if c["resid_only"]:
            e["resid"] = D.residual_excess(A, x, tr["sig"][-1], tr["sig"][0])
        else:
            e["vec/" + _gap_label(float(tr["gap"]))] = D.vec_dist(x, tr["x"])
        return e
    if name == "null4":
        A = A.reshape(4, 4)
        return {"vec/" + _gap_label(float(tr["gap"])): D.vec_dist(row, tr["x"]), "resid": D.residual_excess(A, row, tr["sig"][-1], tr["sig"][0])}
    if name in ("djac", "djac16"):
        A = A.reshape(12, 12); U = row[:144].reshape(12, 12); V = row[144:].reshape(12, 12)
        e = D.jacobi_metrics(A, U, V, tr["sig"])
        if np.all(np.isfinite(row)):
            order = np.argsort(-(U * U).sum(0), kind="stable")
            e["proj/" + _gap_label(float(tr["gap"]))] = D.projector_err(V[:, order[8:]], tr["V4"])
        else:
            e["proj/" + _gap_label(float(tr["gap"]))] = D.INF
        return e
    if name.startswith("lstsq"):
        return {"x": D.rel_err(row, [tr["x"][i] for i in range(len(row))])}
    if name == "sym4":
        if c.get("nonfinite"):
            return {"returns": 0.0 if not np.all(np.isfinite(row)) else D.INF}
        A = A.reshape(4, 4); lam = row[:4]; V = row[4:].reshape(4, 4)
        e = D.sym4_metrics(A, lam, V, tr["lam"])
        g = float(tr["gap"])
        if g >= VEC_MIN_GAP:
            e["vec/" + _gap_label(g)] = D.vec_dist(V[:, int(np.argmax(lam))], tr["top"]) if np.all(np.isfinite(row)) else D.INF
        return e
    raise KeyError(name)


def errors(outs, names=ORDER):
    """bucket -> max e over the sections `names` of outs (name -> [n, NOUT])"""
    m = {}
    for name in names:
        cs, tr = cases()[name], truth(name)
        for i, c in enumerate(cs):
            base = cs[c["base"]]["A"] if c["base"] is not None else c["A"]
            e = case_errors(name, c, base, unscale(name, outs[name][i], c["k"]), tr[i])
            fold(m, ["%s/%s/%s" % (name, c["bucket"], k) for k in e], list(e.values()))
    return m


def scale_mismatches(outs):
    """the x2^k cases whose rescaled outputs are not == the outputs of their unscaled case: [(function, case index, k)]"""
    bad = []
    for name in SCALED_PART:
        for i, c in enumerate(cases()[name]):
            if c["base"] is not None and not np.array_equal(unscale(name, outs[name][i], c["k"]), outs[name][c["base"]]):
                bad.append((name, i, c["k"]))
    return bad


def is_gapfree(bucket):
    return bucket.rsplit("/", 1)[1] in GAPFREE


def per_function(m):
    fn = {}
    for b, e in m.items():
        fn[b.split("/")[0]] = max(fn.get(b.split("/")[0], 0.0), e)
    return fn


def device_to_restatement(dev):
    """function -> max |device - restatement| / max(1, max |restatement|) over the cases both give finite values for (reported, not asserted)"""
    R = restate()
    out = {}
    for name in ORDER:
        worst = 0.0
        for i, c in enumerate(cases()[name]):
            a, b = unscale(name, dev[name][i], c["k"]), unscale(name, R[name][i], c["k"])
            if np.all(np.isfinite(a)) and np.all(np.isfinite(b)):
                worst = max(worst, float(np.abs(a - b).max() / max(1.0, np.abs(b).max())))
            elif not np.array_equal(np.isfinite(a), np.isfinite(b)):
                worst = float("inf")
        out[name] = worst
    return out


def load_golden():
    z = np.load(GOLDEN)
    return {str(k): float(v) for k, v in zip(z["bucket"], z["max_err"])}


def measure_ref():
    return errors(restate())


def write_golden(extra=None):
    E = measure_ref()
    E.update(extra or {})
    k = sorted(E)
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, bucket=np.array(k), max_err=np.array([E[b] for b in k]))
    return E


# ================================================================ the library's entry points on problems from the same ladders
# ---------------------------------------------------------------- frame.TriangulateMatches
TRI_N = 257                                                       # one match past a 256-thread block
TRI_COS = (0.6, 0.9, 0.99, 0.999, 0.9995, 0.99995, 1 - 5e-7)      # depths of 1 to 1e3 baselines; the last two lie past the 0.9998 gate
TRI_EDGE = 0.99979                                                # the last rung of the ladder lies within TRI_BAND of the gate: every 32nd match only
TRI_BAND = 1e-4                                                   # the device evaluates the gates in float
TRI_RATIO = float(np.float32(1.5) * np.float32(1.2))


@functools.lru_cache(maxsize=None)
def tri_problem():
    """257 matches of one keyframe pair a baseline apart: every rung of the parallax ladder, pixel offsets on both sides of the
    reprojection gate, octave pairs on both sides of the scale gate"""
    rng = np.random.default_rng(108)
    K = np.array(K_TRI, np.float32)
    th = 0.01
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    T1 = np.hstack([np.eye(3), np.zeros((3, 1))]); T2 = np.hstack([R, -R @ np.array([[1.0], [0], [0]])])
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32); ls = (sf * sf).astype(np.float32)
    kp1 = np.zeros((TRI_N, 3), np.float32); kp2 = np.zeros((TRI_N, 3), np.float32); rung = []
    for i in range(TRI_N):
        cos = TRI_EDGE if i % 32 == 31 else TRI_COS[i % len(TRI_COS)]
        z = 0.5 / np.tan(0.5 * np.arccos(cos))
        X = np.array([0.5 + rng.uniform(-0.15, 0.15) * z, rng.uniform(-0.1, 0.1) * z, z])
        o1 = int(rng.integers(0, 4)); o2 = o1 + (4 if i % 11 == 5 else 0)
        dy = 0.0 if cos > 0.9996 else (0.0, 0.0, 0.7, 3.0, 8.0)[i % 5] * float(sf[o2])    # (a pixel offset would move a far rung's parallax into the band)
        kp1[i] = (*project_px(T1, X, K), o1)
        kp2[i] = (*(project_px(T2, X, K).astype(np.float64) + np.array([0.0, dy])), o2)
        rung.append("cos=%g" % cos)
    return dict(T1=T1, T2=T2, K=K, kp1=kp1, kp2=kp2, ls=ls, sf=sf, ratio=TRI_RATIO, rung=rung)


@functools.lru_cache(maxsize=None)
def tri_truth():
    """per match: (flag or None when a gate quantity lies within TRI_BAND of its threshold, the mp point, the float64 DLT system):
    the gates of triangulate_one (csrc/tri_math.h) evaluated in mp on the mp point"""
    p = tri_problem()
    out = []
    with mp.workdps(D.DPS):
        T = [[mpf(float(v)) for v in Tm.reshape(12)] for Tm in (p["T1"], p["T2"])]
        Ow = [[-sum(T[c][4 * r + k] * T[c][4 * r + 3] for r in range(3)) for k in range(3)] for c in range(2)]
        K = [mpf(float(v)) for v in p["K"]]
        for a, b in zip(p["kp1"], p["kp2"]):
            xn = [xn_of(a[:2], p["K"]), xn_of(b[:2], p["K"])]
            A = dlt_f64(p["T1"], p["T2"], xn[0], xn[1])
            rays = [[T[c][k] * mpf(xn[c][0]) + T[c][4 + k] * mpf(xn[c][1]) + T[c][8 + k] for k in range(3)] for c in range(2)]
            nr = [mp.sqrt(sum(v * v for v in r)) for r in rays]
            cosp = sum(x * y for x, y in zip(rays[0], rays[1])) / (nr[0] * nr[1])
            X, _ = D.dlt_point(p["T1"], p["T2"], xn[0], xn[1])
            near, flag = False, 1
            gates = [(cosp, mpf(0.9998), -1)]                     # (quantity, threshold, +1: must be above / -1: must be below)
            pc = [[sum(T[c][4 * r + k] * X[k] for k in range(3)) + T[c][4 * r + 3] for r in range(3)] for c in range(2)]
            for c, kp in ((0, a), (1, b)):
                u = K[0] * pc[c][0] / pc[c][2] + K[2]; v = K[1] * pc[c][1] / pc[c][2] + K[3]
                e2 = (u - mpf(float(kp[0]))) ** 2 + (v - mpf(float(kp[1]))) ** 2
                gates.append((e2, mpf(5.991) * mpf(float(p["ls"][int(kp[2])])), -1))
            d = [mp.sqrt(sum((X[k] - Ow[c][k]) ** 2 for k in range(3))) for c in range(2)]
            rd = d[1] / d[0]; ro = mpf(float(p["sf"][int(a[2])] / p["sf"][int(b[2])])); rf = mpf(p["ratio"])
            gates += [(rd * rf, ro, +1), (rd, ro * rf, -1)]
            zs = [pc[0][2], pc[1][2]]
            nX = mp.sqrt(sum(v * v for v in X))
            for gi, (q, thr, side) in enumerate(gates):
                if gi == 1:                                       # after the parallax gate: both depths positive
                    if any(abs(zv) < TRI_BAND * nX for zv in zs):
                        near = True
                    if any(zv <= 0 for zv in zs):
                        flag = 0
                    if near or not flag:
                        break
                if abs(q / thr - 1) < TRI_BAND:
                    near = True; break
                if (side > 0 and q < thr) or (side < 0 and not q < thr if gi == 0 else side < 0 and q > thr):
                    flag = 0; break
            out.append((None if near else flag, X, A))
    return out


def tri_errors(X, ok):
    """(bucket -> max e over the matches both sides accept, the matches whose flag differs from mp's, the fraction left out)"""
    tr, p = tri_truth(), tri_problem()
    m, wrong, left = {}, [], 0
    for i, (flag, Xt, _) in enumerate(tr):
        if flag is None:
            left += 1; continue
        if int(ok[i]) != flag:
            wrong.append(i); continue
        if flag:
            fold(m, ["tri/%s/X" % p["rung"][i]], [D.rel_err(X[i], Xt)])
    return m, wrong, left / float(len(tr))


def tri_restated():
    """the restatement of null_vector4_dev on the same systems: (X [n, 3], ok = mp's own flags, so that only the points are measured)"""
    tr = tri_truth()
    x = npinit.null_vector(np.stack([t[2] for t in tr]), tol=1e-16, null_rule=False)
    with np.errstate(all="ignore"):
        return x[:, :3] / x[:, 3:4], np.array([t[0] if t[0] is not None else 0 for t in tr])


# ---------------------------------------------------------------- initializer.initialize: the traced H21 and F21 of every iteration
INIT_ITERS = 65                                                   # one lane past a 64-lane block
INIT_K4 = (500.0, 500.0, 320.0, 240.0)


@functools.lru_cache(maxsize=None)
def init_problems():
    """a general and a planar scene of 40 matches among 44 keypoints; 65 hand-made sets: 18 distinct ones (6 of them with a repeated
    position) tiled over the iterations"""
    out = []
    for si, planar in enumerate((False, True)):
        rng = np.random.default_rng(109 + si)
        n, nm = 44, 40
        X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), (np.full(n, 6.0) if planar else rng.uniform(4, 9, n))], 1)
        if planar:
            X[:, 2] += 0.3 * X[:, 0] - 0.2 * X[:, 1]
        th = 0.12
        R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]]); t = np.array([-0.8, 0.05, 0.1])
        k1 = (INIT_K4[0] * X[:, :2] / X[:, 2:3] + np.array(INIT_K4[2:])).astype(np.float32)
        X2 = X @ R.T + t
        perm = rng.permutation(n)
        k2 = np.empty((n, 2), np.float32); k2[perm] = (INIT_K4[0] * X2[:, :2] / X2[:, 2:3] + np.array(INIT_K4[2:])).astype(np.float32)
        m12 = perm.astype(np.int32); m12[rng.choice(n, n - nm, replace=False)] = -1
        base = np.stack([rng.choice(nm, 8, replace=False) for _ in range(18)]).astype(np.int32)
        base[12:, 7] = base[12:, 2]; base[15:, 6] = base[15:, 0]
        sets = base[np.arange(INIT_ITERS) % 18]
        out.append(dict(kind="planar" if planar else "general", kps1=k1, kps2=k2, m12=m12, sets=sets, base=base, repeated=np.arange(18) >= 12))
    return out


def _unit9(Mx):
    n = mp.sqrt(sum(v * v for v in Mx))
    return [v / n for v in Mx]


@functools.lru_cache(maxsize=None)
def init_truth():
    """per problem and distinct set: the unit H21 and F21 in mp (the null vector of the system as init_hyp builds it, carried through
    T2^-1 Hn T1 and, after the rank-2 cut, T2^T Fn T1), the systems' gaps, and whether F is 'residual only'"""
    out = []
    for p in init_problems():
        pn1, T1 = npinit.normalize(p["kps1"]); pn2, T2 = npinit.normalize(p["kps2"])
        i1, i2 = npinit.match_list(p["m12"])
        Ah, Af = hyp_systems(pn1[i1], pn2[i2], p["base"])
        rows = []
        with mp.workdps(D.DPS):
            T1m, T2m = D.M(T1), D.M(T2)
            for s in range(len(p["base"])):
                sh, Vh = D.right_vectors(Ah[s]); sf_, Vf = D.right_vectors(Af[s])
                Hn = mp.matrix(3, 3); Fp = mp.matrix(3, 3)
                for k in range(9):
                    Hn[k // 3, k % 3] = Vh[k, 8]; Fp[k // 3, k % 3] = Vf[k, 8]
                H = T2m ** -1 * Hn * T1m
                U, S, Vt = mp.svd_r(Fp)
                F = T2m.T * (U * mp.diag([S[0], S[1], 0]) * Vt) * T1m
                rows.append(dict(H=_unit9(list(H)), F=_unit9(list(F)), gap_h=float((sh[7] - sh[8]) / sh[0]), gap_f=float(sf_[7] / sf_[0]),
                                 resid_f=p["kind"] == "planar" or bool(p["repeated"][s])))
        out.append(rows)
    return out


def init_errors(traces):
    """traces: per problem (H21 [65, 3, 3], F21 [65, 3, 3]) -> (bucket -> max e, the largest sigma2 / sigma0 of a traced F)"""
    m, rank2 = {}, 0.0
    for p, rows, (H21, F21) in zip(init_problems(), init_truth(), traces):
        i1, i2 = npinit.match_list(p["m12"])
        for it in range(INIT_ITERS):
            r = rows[it % 18]
            rep = "repeat" if p["repeated"][it % 18] else "distinct"
            h = np.asarray(H21[it], np.float64).reshape(9); f = np.asarray(F21[it], np.float64).reshape(9)
            ok = np.all(np.isfinite(h)) and np.all(np.isfinite(f))
            with np.errstate(all="ignore"):
                h = h / np.sqrt((h * h).sum()); f = f / np.sqrt((f * f).sum())
            fold(m, ["init/H/%s/%s/vec/%s" % (p["kind"], rep, _gap_label(r["gap_h"]))], [D.vec_dist(h, r["H"]) if ok else D.INF])
            if r["resid_f"]:
                x1 = np.concatenate([p["kps1"][i1[p["sets"][it]]].astype(np.float64), np.ones((8, 1))], 1)
                x2 = np.concatenate([p["kps2"][i2[p["sets"][it]]].astype(np.float64), np.ones((8, 1))], 1)
                with mp.workdps(D.DPS):
                    Fm = D.M(f.reshape(3, 3)) if ok else None
                    e = D.INF if not ok else float(max(abs((D.M(b).T * Fm * D.M(a))[0]) / (mp.norm(D.M(a)) * mp.norm(D.M(b))) for a, b in zip(x1, x2)))
                fold(m, ["init/F/%s/%s/resid" % (p["kind"], rep)], [e])
            else:
                fold(m, ["init/F/%s/%s/vec/%s" % (p["kind"], rep, _gap_label(r["gap_f"]))], [D.vec_dist(f, r["F"]) if ok else D.INF])
            if ok:
                S = D.svd(f.reshape(3, 3))[1]
                rank2 = max(rank2, float(S[2] / S[0]))
            else:
                rank2 = D.INF
    m["init/F/rank2"] = rank2
    return m


def init_restated():
    out = []
    for p in init_problems():
        H21, _, F21 = npinit.hypotheses(p["kps1"], p["kps2"], p["m12"], p["sets"])
        out.append((H21, F21))
    return out


# ---------------------------------------------------------------- pnp.iterate: the traced R, t of every set against the ground truth
PNP_SETS = 17                                                     # one past PNP_HYP_LANES
PNP_K4 = (520.0, 515.0, 320.0, 240.0)
PNP_NONDEGENERATE = 1e-3                                          # a set counts where nppnp(lapack=True) recovers the pose this well, whatever the null basis


@functools.lru_cache(maxsize=None)
def pnp_problems():
    """noise-free candidates of 12 points: general, exactly planar (z = 0), and collinear on the x axis; 17 sets of 4 each"""
    out = []
    th = 0.3
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [0, np.cos(0.2), -np.sin(0.2)], [0, np.sin(0.2), np.cos(0.2)]])
    t = np.array([0.2, -0.1, 5.0])
    for si, kind in enumerate(("general", "planar", "collinear")):
        rng = np.random.default_rng(120 + si)
        pw = rng.uniform(-1, 1, (12, 3))
        if kind == "planar":
            pw[:, 2] = 0.0
        if kind == "collinear":
            pw[:, 1:] = 0.0
        pw = pw.astype(np.float32)
        pc = pw.astype(np.float64) @ R.T + t
        uv = np.stack([PNP_K4[0] * pc[:, 0] / pc[:, 2] + PNP_K4[2], PNP_K4[1] * pc[:, 1] / pc[:, 2] + PNP_K4[3]], 1).astype(np.float32)
        sets = np.stack([rng.choice(12, 4, replace=False) for _ in range(PNP_SETS)]).astype(np.int32)
        out.append(dict(kind=kind, p3d=pw, p2d=uv, K4=np.array(PNP_K4, np.float32), sets=sets, R=R, t=t))
    return out


@functools.lru_cache(maxsize=None)
def pnp_lapack():
    """per problem: nppnp(lapack=True)'s (R [17, 3, 3], t [17, 3]) of every set"""
    out = []
    for p in pnp_problems():
        R, t, *_ = nppnp.hypotheses(p["p3d"], p["p2d"], p["K4"], p["sets"], lapack=True)
        out.append((R, t))
    return out


def _rotated_null_basis(orig, seed):
    """nppnp.eig_smallest4 with the vectors of the (numerically) null eigenvalues among the four rotated by a seeded orthogonal matrix:
    an equally valid basis of the same null space"""
    def f(A, lapack=False):
        v = orig(A, lapack)
        w = np.linalg.eigvalsh(A)
        out = v.copy()
        rng = np.random.default_rng(seed)
        for b in range(len(A)):
            d = int((w[b, :4] < 1e-9 * w[b, -1]).sum())
            if d >= 2:
                out[b, :d] = _orth(rng, d) @ v[b, :d]
        return out
    return f


@functools.lru_cache(maxsize=None)
def pnp_nondegenerate():
    """per problem: the sets whose pose is a function of the problem - nppnp(lapack=True) recovers the ground truth to 1e-3 with LAPACK's
    basis of M^T M's null space AND with three seeded rotations of it.  Four points in general position leave a null space of dimension 4
    whose basis is free, and EPnP's approximations start from the basis vectors one by one: there the pose changes from 1e-7 to 1 with the
    basis (whichever solver supplies it), and no such set is compared.  The exactly planar sets are invariant to the last digit."""
    out = []
    orig = nppnp.eig_smallest4
    for p, (R, t) in zip(pnp_problems(), pnp_lapack()):
        keep = pnp_pose_err(p, R, t) <= PNP_NONDEGENERATE
        try:
            for seed in (1, 2, 3):
                nppnp.eig_smallest4 = _rotated_null_basis(orig, seed)
                Rr, tr, *_ = nppnp.hypotheses(p["p3d"], p["p2d"], p["K4"], p["sets"], lapack=True)
                keep &= pnp_pose_err(p, Rr, tr) <= PNP_NONDEGENERATE
        finally:
            nppnp.eig_smallest4 = orig
        out.append(keep)
    return out


def pnp_pose_err(p, R, t):
    with np.errstate(all="ignore"):
        e = np.maximum(np.abs(R - p["R"]).reshape(len(R), -1).max(1), np.sqrt(((t - p["t"]) ** 2).sum(1)) / np.sqrt((p["t"] ** 2).sum()))
    return np.where(np.isfinite(e), e, np.inf)


def pnp_errors(poses):
    """poses: per problem (R [17, 3, 3], t [17, 3]) -> bucket -> the largest pose error over the non-degenerate sets (pnp_nondegenerate)"""
    m = {}
    for p, keep, (R, t) in zip(pnp_problems(), pnp_nondegenerate(), poses):
        if p["kind"] == "collinear":
            continue
        m["pnp/%s/pose" % p["kind"]] = float(pnp_pose_err(p, np.asarray(R), np.asarray(t))[keep].max()) if keep.any() else 0.0
    return m


def pnp_finite(R, t):
    return np.isfinite(np.asarray(R).reshape(len(R), -1)).all(1) & np.isfinite(np.asarray(t)).all(1)


def library_ref():
    """E_ref of the library-level buckets: the restatements (tri, init) and nppnp(lapack=True) (pnp) against the same truths"""
    E = {}
    E.update(tri_errors(*tri_restated())[0])
    E.update(init_errors(init_restated()))
    E.update(pnp_errors(pnp_lapack()))
    return E
