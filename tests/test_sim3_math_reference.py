"""CPU side of the Sim(3) arithmetic tests: the mp reference tests/npsim3.py pinned by hand values and identities, the CPU oracle
(oracle/sim3_oracle.cpp) measured against it on the case table of tests/sim3mathcases.py, the host half of csrc/sim3_math.h (through
tools/ubench/sim3_math_probe.hip --host-only) held to the acceptance rule, and the conditions on the table itself.  No GPU.

e = max|out - truth| / max(1, max|truth|) per function and case; a bucket's figure is its maximum.  Measured here (mp at 50 digits):
  1322 cases, 512 buckets (227 of the header's functions, 285 of the library-level problems built from the same tables).
  oracle = oracle/sim3_oracle.cpp (g++), host = the __host__ half of sim3_math.h (hipcc): the two agree to the last bit on every
  bucket both have, except s3_term_eval (the oracle evaluates a term from the tangent and without the loss) and s3_to_pose34 (no oracle
  entry: its bound is the floor of the rule).  Largest e per function, oracle / host:
      exp 9.62e-7 / 9.62e-7    log 1.78e-6 / 1.78e-6    plus 6.16e-14 / 6.14e-14    inverse 3.89e-16    mul 4.61e-16    adj 4.02e-16
      act 2.43e-16    graph edge (r, J_i) 1.61e-13 / 1.60e-13    term 4.88e-13 / 3.18e-13    to_pose34 - / 4.02e-16
      exp(log(S)) 1.44e-6    write-back poses 9.62e-7, points 9.86e-7    graph initial cost 2.34e-14    consistent-edge solution 1.9e-16
  CheckOutlier's flags and the Huber side of the host half equal mp's on every case; no case lies within 1e-6 of either threshold.
  92 buckets are above 1e-9.  All are exp, log and what rides on them, in three regimes:
    - exp, sigma from 1.01e-10 to 1e-8 at any theta (and 1e-7, 1e-6 up to 6e-10): C = (e^sigma - 1) / sigma, and A and B beside it,
      cancel: half an ulp of e^sigma over sigma.  9.6e-7 at 1.01e-10, 8.2e-8 at 1e-9, 1.1e-8 at 1e-8.  The write-back buckets
      correct_T / correct_pts carry the same figures.
    - exp, theta = 1e-8 with |sigma| < 1e-10: A = (1 - cos theta) / theta^2 has no digit left (1 - cos 1e-8 = 5e-17 is below half an ulp
      of 1), an error of A theta = 5e-9 in W.  explog/th=1e-8 shows the same.
    - log and exp(log(S)), |sigma| from 1e-8 to 1.01e-5 with theta of 1e-3 and more: the sigma^2 < 1e-10 branch takes a = -1/2 and b at sigma = 0, a
      TRUNCATION of first order in sigma, not rounding: about 0.18 sigma at theta = pi (1.78e-6 at sigma = 1e-5, 5.0e-7 at 1e-6, 5.0e-8 at
      1e-7), 1.7e-7 at theta <= 1 and sigma = 1e-5.  For small theta the branch is good to sigma^2 / 12 (8e-12).  It is Sophus' own
      approximation, kept as it is; oracle, host and device share it.
  Below 1e-9 the same three regimes fall off in proportion (6.1e-10 at sigma = 1e-7, 9.6e-10 for log at sigma = 1e-8); outside exp, log and
  what rides on them the largest figure is 4.9e-13 (term), and 239 of the 512 buckets are below 1e-13.
"""
import numpy as np
import pytest
from mpmath import mp, mpf

from tests import npsim3 as N
from tests import sim3mathcases as C


def _close(a, b, tol):
    with mp.workdps(N.DPS):
        a = [a[i, j] for i in range(a.rows) for j in range(a.cols)] if isinstance(a, mp.matrix) else list(a)
        b = [b[i, j] for i in range(b.rows) for j in range(b.cols)] if isinstance(b, mp.matrix) else list(b)
        return len(a) == len(b) and all(abs(mpf(x) - mpf(y)) <= mpf(tol) for x, y in zip(a, b))


# ---------------------------------------------------------------- npsim3 itself
def test_exp_by_hand():
    with mp.workdps(N.DPS):
        assert _close(N.mp_exp(np.zeros(7)), mp.eye(4), 0)
        # a pure scale: sigma = log 2 (as a float64) -> diag(s, s, s, 1), no translation; with upsilon: t = (e^sigma - 1) / sigma upsilon
        sg = float(np.log(2.0)); s = mp.exp(mpf(sg))
        assert _close(N.mp_exp([0, 0, 0, 0, 0, 0, sg]), mp.diag([s, s, s, 1]), "1e-45")
        M = N.mp_exp([1.0, 0, 0, 0, 0, 0, sg])
        assert abs(M[0, 3] - (s - 1) / mpf(sg)) < mpf("1e-45") and M[1, 3] == 0 and M[2, 3] == 0
        # a quarter turn about z with upsilon = (1, 0, 0), sigma = 0: R = [[0, -1, 0], [1, 0, 0], [0, 0, 1]] and the SE(3) closed form
        # t = (sin th / th, (1 - cos th) / th, 0) at th = pi / 2 (the float64 nearest it)
        th = float(np.pi / 2)
        M = N.mp_exp([1.0, 0, 0, 0, 0, th, 0.0])
        c, s_ = mp.cos(mpf(th)), mp.sin(mpf(th))
        want = mp.matrix([[c, -s_, 0, s_ / mpf(th)], [s_, c, 0, (1 - c) / mpf(th)], [0, 0, 1, 0], [0, 0, 0, 1]])
        assert _close(M, want, "1e-45")
        assert abs(M[0, 0]) < 1e-16 and abs(M[1, 0] - 1) < 1e-16
        # the stored quaternion: |q|^2 = e^sigma, and its sign is cos(theta / 2)'s
        q = N.mp_exp_qt([0, 0, 0, 0, 0, 6.5, 0.3])
        assert abs(sum(c * c for c in q[:4]) - mp.exp(mpf(0.3))) < mpf("1e-45") and q[3] < 0


def test_W_is_its_power_series():
    """mp_W sums the series in the basis {I, Om, Om^2}; the same series summed on the 3x3 matrices themselves gives the same matrix"""
    for om, sg in (([0.3, -0.2, 0.5], 0.7), ([0, 0, 6.5], -5.0), ([1e-10, 0, 0], 1.01e-10), ([0, 0, 0], 0.0), ([2.0, 2.0, -1.0], 5.0), ([0, np.pi, 0], 1e-7)):
        assert _close(N.mp_W(om, sg), N.mp_W_matrix_series(om, sg), "1e-44"), (om, sg)
    assert _close(N.mp_W([0, 0, 0], 0.0), mp.eye(3), 0)


def test_log_inverts_exp():
    rng = np.random.default_rng(3)
    cases = [np.concatenate([rng.normal(0, 2, 3), th * C._unit(rng.normal(0, 1, 3)), [sg]])
             for th in (0.0, 1e-12, 1.01e-10, 1e-5, 0.1, 1.0, 3.0, np.pi - 1e-9) for sg in (0.0, 1e-10, -1e-5, 0.3, -5.0, 5.0)]
    for a in cases:
        assert _close(N.mp_log(N.mp_exp(a)), N._v(a), "1e-40"), a
        assert _close(N.mp_log(N.mp_exp_qt(a)), N._v(a), "1e-40"), a                 # through the quaternion as well as the matrix
    with mp.workdps(N.DPS):
        # past pi the canonical vector is the other one: theta - 2 pi about the same axis
        a = np.array([0.5, -1.0, 2.0, 0, 0, 4.0, 0.2])
        l = N.mp_log(N.mp_exp_qt(a))
        assert abs(l[5] - (mpf(4.0) - 2 * mp.pi)) < mpf("1e-40") and abs(l[6] - mpf(0.2)) < mpf("1e-40")
    for S in C.table()["log"]["inputs"]:                             # every quaternion of the table, w < 0 and w == 0 included
        tol = mpf("1e-38") * max(1, float(np.abs(S).max())) ** 2
        assert _close(N.mp_exp(N.mp_log(S)), N.mat_of(S), tol), S
    assert (C.table()["log"]["inputs"][:, 3] < 0).sum() >= 40 and (C.table()["log"]["inputs"][:, 3] == 0).sum() >= 12


def test_group_algebra_by_hand():
    with mp.workdps(N.DPS):
        S = np.array([0, 0, np.sqrt(0.5), np.sqrt(0.5), 1.0, 2.0, 3.0]) * np.array([2, 2, 2, 2, 1, 1, 1.0])      # scale 4 (to rounding), a quarter turn about z
        p = N.mp_act(S, [1.0, 0, 0])
        assert abs(p[0] - 1) < 1e-15 and abs(p[1] - 6) < 1e-14 and p[2] == 3
        assert _close(N.mp_mul(S, N.mp_inverse(S)), mp.eye(4), "1e-45")
        T = N.mp_to_pose34(S)
        assert abs(T[3] - mpf(1) / 4) < 1e-15 and abs(T[4] - 1) < 1e-15 and abs(T[0]) < 1e-15
        # Adj: log(S exp(d) S^-1) = Adj(S) d, exactly
        d = [0.01, -0.02, 0.03, 0.02, 0.01, -0.03, 0.015]
        lhs = N.mp_log(N.mat_of(S) * N.mp_exp(d) * N.mp_inverse(S))
        A = N.mp_adj(S)
        assert _close(lhs, [sum(A[i, k] * mpf(d[k]) for k in range(7)) for i in range(7)], "1e-40")
        # plus: the clamp
        x = [0.1, 0.2, 0.3, 0.1, 0.0, -0.1, 0.2]
        assert _close(N.mp_plus(x, [0, 0, 0, 0, 0, 0, -25.0]), N.mp_plus(x, [0, 0, 0, 0, 0, 0, -20.0]), 0)
        assert abs(N.mp_plus(x, [0, 0, 0, 0, 0, 0, -19.9])[6] - (mpf(0.2) + mpf(-19.9))) < mpf("1e-40")


def test_graph_edge_residual_and_jacobian():
    """r == 0 when Sji is consistent; J_i against a central difference of r under mp_plus, to the size of the first dropped term of the
    series, ad^4 / 720 (times Adj), for |r| <= 1e-2"""
    rng = np.random.default_rng(8)
    with mp.workdps(N.DPS):
        for size in (0.0, 1e-9, 1e-5, 1e-2):
            li = np.concatenate([rng.uniform(-5, 5, 3), 0.8 * C._unit(rng.normal(0, 1, 3)), [0.1]])
            lj = np.concatenate([rng.uniform(-5, 5, 3), 3.0 * C._unit(rng.normal(0, 1, 3)), [-0.1]])
            delta = size * C._unit(rng.normal(0, 1, 7))
            Sji = N.mp_exp(delta) * N.mp_exp(lj) * N.mp_inverse(N.mp_exp(li))          # in mp: consistent up to delta, exactly
            r, J = N.mp_graph_edge(lj, li, Sji)
            assert _close(r, N._v(delta), "1e-40")
            if size == 0.0:
                assert all(abs(c) < mpf("1e-45") for c in r)
            h = mpf("1e-18")
            ad, Adj = N.mp_ad(r), N.mp_adj(N.mp_exp(lj))
            ad4 = ad * ad * ad * ad
            dropped = max(sum(abs((ad4 * Adj)[i, k]) for k in range(7)) for i in range(7)) / 720
            for k in range(7):
                e = [h if i == k else mpf(0) for i in range(7)]
                rp, _ = N.mp_graph_edge(lj, N.mp_plus(li, e), Sji, jacobian=False)
                rm, _ = N.mp_graph_edge(lj, N.mp_plus(li, [-c for c in e]), Sji, jacobian=False)
                for i in range(7):
                    assert abs((rp[i] - rm[i]) / (2 * h) - J[i, k]) <= 2 * dropped + mpf("1e-25"), (size, i, k)


def test_term_and_outlier_by_hand():
    with mp.workdps(N.DPS):
        K = np.array([1.0, 1.0, 0.0, 0.0]); I7 = np.array([0, 0, 0, 1.0, 0, 0, 0])
        t = N.mp_term(K, I7, [0, 0, 1.0], [3.0, 4.0], 0.5, 10.0)                       # r = -(1.5, 2), s = 6.25 <= 100
        assert [float(c) for c in t["r"]] == [-1.5, -2.0] and float(t["rho0"]) == 6.25 and not t["linear"] and float(t["ratio"]) == 0.0625
        assert [float(c) for c in t["J"][0]] == [0.5, 0, 0, 0, 0.5, 0, 0] and [float(c) for c in t["J"][1]] == [0, 0.5, 0, -0.5, 0, 0, 0]
        t = N.mp_term(K, I7, [0, 0, 1.0], [3.0, 4.0], 0.5, 2.0)                        # s = 6.25 > 4: rho0 = 2 * 2 * 2.5 - 4, rho' = 2 / 2.5
        assert t["linear"] and abs(t["rho0"] - 6) < mpf("1e-45") and abs(t["r"][0] + mpf(1.5) * mp.sqrt(mpf(4) / 5)) < mpf("1e-45")
        # the outlier gate at scale 1 is the plain projection; at scale 4 the quaternion of the scaled matrix is not a unit one
        f, ratio, arm = N.mp_check_outlier(K, I7, [0, 0, 2.0], [3.0, 4.0], 0.5, 10.0)
        assert (f, float(ratio), arm) == (1, 1.25, 3)
        c, arm = N.mp_outlier_camera_point(2 * I7, [1.0, 2.0, 3.0])                    # M = 4 I: q = (0, 0, 0, sqrt(13) / 2), the point unmoved
        assert arm == 3 and [float(v) for v in c] == [1.0, 2.0, 3.0]
        Sx = np.concatenate([C._quat(3.0, [1.0, 0, 0], 0.0), [0, 0, 0]])
        assert N.mp_outlier_camera_point(Sx, [0, 0, 1.0])[1] == 0


# ---------------------------------------------------------------- the table
def test_table_conditions():
    T = C.table()
    assert C.n_cases() <= C.MAX_CASES
    for name in C.ORDER:
        assert len(T[name]["buckets"]) == len(T[name]["inputs"]) > 0 and np.all(np.isfinite(T[name]["inputs"]))
    # every theta and |sigma| value, both signs of sigma, every |upsilon|, in the exp table
    a = T["exp"]["inputs"]
    th = np.linalg.norm(a[:, 3:6], axis=1)
    for v, _ in C.THETAS:
        assert np.any(np.abs(th - v) <= 2e-16 * max(v, 1e-300)), v
    for v, _ in C.SIGMAS:
        assert np.any(a[:, 6] == v), v
    assert {float(np.round(np.linalg.norm(r[:3]), 12)) for r in a} == set(C.UPS)
    # the quaternions of the log table: w < 0, w == 0, |v|^2 on both sides of 1e-20, scales e^+-5
    q = T["log"]["inputs"]
    s = (q[:, :4] ** 2).sum(1); v2 = (q[:, :3] ** 2).sum(1) / s
    assert (q[:, 3] < 0).any() and (q[:, 3] == 0).any() and ((v2 < 1e-20) & (v2 > 0.9e-20)).any() and ((v2 > 1e-20) & (v2 < 1.1e-20)).any()
    assert (np.abs(np.log(s) - 5) < 1e-12).any() and (np.abs(np.log(s) + 5) < 1e-12).any()
    # plus: every tiny regime of d, and the clamp on both sides
    d = T["plus"]["inputs"][:, 7:]
    assert {-19.9, -20.0, -25.0} <= set(d[:, 6].tolist())
    for v, _ in C.TINY:
        assert np.any(np.abs(d[:, 6]) == v) and np.any(np.abs(np.linalg.norm(d[:, 3:6], axis=1) - v) <= 2e-16 * v)
    # terms and outlier cases: only those within 1e-6 of their threshold would be left out - none is - and every arm has its share
    for name in ("term", "outlier"):
        assert np.all(np.abs(T[name]["ratio"] - 1) >= C.KEEP_BAND)
        assert T[name]["n_built"] - len(T[name]["buckets"]) == 0
    assert T["term"]["linear"].sum() >= 20 and (~T["term"]["linear"]).sum() >= 20 and set(T["term"]["inverse"].tolist()) == {0, 1}
    assert np.abs(T["term"]["ratio"] - 1).min() < 2e-5 and np.abs(T["outlier"]["ratio"] - 1).min() < 2e-5
    arms = np.bincount(T["outlier"]["arm"], minlength=4)
    print("outlier cases per arm (x, y, z, trace):", arms.tolist())
    assert arms.min() >= 8
    for arm in range(4):
        assert set(T["outlier"]["flag"][T["outlier"]["arm"] == arm].tolist()) == {0, 1}
    # the library-level problems
    assert len(C.graph_problems()) <= 40 and sum(g["consistent"] for g in C.graph_problems()) == 8
    m, idx = C.assemble_map()
    assert m["nkf"] == 130 and len(m["conn_group_kf"]) == 130
    assert {b.split("/")[1] for b in T["log"]["buckets"]} == {T["log"]["buckets"][i].split("/")[1] for i in idx}


# ---------------------------------------------------------------- the oracle and the host half
@pytest.fixture(scope="module")
def oracle_measured():
    return C.measure_oracle()


def test_oracle_reproduces_the_committed_table(oracle_measured):
    E = C.load_golden()
    assert sorted(E) == sorted(oracle_measured)
    bad = [(b, oracle_measured[b], E[b]) for b in E if not (oracle_measured[b] <= 2 * E[b] and E[b] <= 2 * oracle_measured[b])]
    assert not bad, bad[:10]
    big = {b: e for b, e in E.items() if e > 1e-9}
    print("%d buckets, %d above 1e-9, largest %.3g (%s)" % (len(E), len(big), max(E.values()), max(E, key=E.get)))
    # what is above 1e-9 is what the docstring names: sigma from 1e-10 to 1e-6 (the cancellations), exp's Taylor branches and what rides on them
    for b in big:
        fn, rest = b.split("/", 1)
        assert fn in ("exp", "log", "explog", "correct_T", "correct_pts"), b
        assert any(k in rest for k in ("sg=1.01e-10", "sg=1e-9", "sg=1e-8", "sg=1e-7", "sg=1e-6", "sg=~1e-5", "sg=<1e-10")), b


def test_probe_host_half_obeys_the_rule(tmp_path):
    exe = C.build_probe(tmp_path)
    dev, host = C.run_probe(exe, tmp_path, host_only=True)
    assert dev is None
    m, flags, sides = C.probe_report(host)
    E = C.load_golden()
    T = C.table()
    assert np.array_equal(flags, T["outlier"]["flag"])
    assert np.array_equal(sides, T["term"]["linear"])
    print("host half: largest e %.3g (%s); largest e / bound %.3g" % (max(m.values()), max(m, key=m.get), max(e / C.bound(E, b) for b, e in m.items())))
    C.check(m, E, "the host half of sim3_math.h")
