"""csrc/sim3_math.h on the MI355X at its branch points, against the mp reference tests/npsim3.py on the case table of
tests/sim3mathcases.py: once through the stand-alone probe tools/ubench/sim3_math_probe.hip (every function of the header, one lane per
case), and once through the shipped library's own kernels - k_pg_poses / k_pg_points (essential_graph_correct), k_sim3_lm
(optimize_sim3 without terms: exp(log(S))), k_pg_eval and the solver (optimize_essential_graph on two-vertex graphs) and k_eg_vertices
(essential_graph_assemble on the device).

The rule everywhere: per bucket, max e <= max(64 * 2.2e-16, 8 * E_oracle[bucket]); e = max|out - truth| / max(1, max|truth|), E_oracle the
CPU oracle's figure against mp, committed in tests/golden/sim3_math_oracle_err.npz and reproduced by tests/test_sim3_math_reference.py
(whose docstring lists the buckets above 1e-9 and why).  CheckOutlier's flags and the side of the Huber corrector are compared ==.

Measured on the device:
  probe, device half: 227 buckets; largest e 1.78e-6 (log/th=~pi/sg=~1e-5, the oracle's own figure there); nearest to its bound
      edge/r=0.3/generic, 6.9e-15 of 4.4e-14; flags and Huber sides identical; largest device-to-host difference 1.5e-14
      (edge/r=1e-2/lie_j near pi): in the cancellation buckets the device's exp / sin / cos / log / atan2 give the host's figures
  essential_graph_correct: 180 buckets; largest 9.86e-7 (correct_pts/th=1e-7/sg=1.01e-10); nearest correct_T/th=~pi/sg=1e-3..1, 2.4e-14 of 1.9e-13
  optimize_sim3 without terms: 93 buckets; largest 1.44e-6 (explog/th=~pi/sg=~1e-5); nearest explog/th=1e-9/sg=~1e-5, 1.9e-14 of 1.6e-13
  optimize_essential_graph: 12 buckets; largest 2.45e-14 (cost/r=0.3/lie_j near pi); nearest cost/r=0.3/generic, 1.9e-15 of 1.4e-14
  essential_graph_assemble: 69 buckets; largest 1.78e-6 (log/th=~pi/sg=~1e-5); nearest log/th=~2pi/sg=1.01e-10, 3.3e-12 of 2.6e-11
No bucket breaks the rule on the device: nothing in sim3_math.h had to change.

What bites where (checked on scratch copies of the header, host half of the probe): the sign of B's term in s3_poly_apply flipped - 83
buckets of exp, log, plus and edge, and the write-back test; 1.0 / 12. turned into 1.0 / 6. in s3_graph_edge - 6 edge buckets of the probe
only, since no entry of the library returns J_i and a Gauss-Newton step with a slightly wrong Jacobian still ends at the same answer; the
w < 0 arm of s3_log removed - 23 buckets of log and edge, and the exp(log(S)) and table-builder tests.
"""
import numpy as np
import pytest

from tests import sim3mathcases as C

pytestmark = pytest.mark.gpu


def _summary(what, m, E):
    worst = max(m, key=lambda b: m[b] / C.bound(E, b))
    fn = {}
    for b, e in m.items():
        fn[b.split("/")[0]] = max(fn.get(b.split("/")[0], 0.0), e)
    print("%s, largest e per function: %s" % (what, "  ".join("%s %.3g" % kv for kv in sorted(fn.items()))))
    print("%s: %d buckets, largest e %.3g (%s); nearest to its bound %s: %.3g of %.3g" % (what, len(m), max(m.values()), max(m, key=m.get), worst, m[worst], C.bound(E, worst)))


def test_probe_device_half(tmp_path):
    exe = C.build_probe(tmp_path)
    dev, host = C.run_probe(exe, tmp_path, host_only=False)
    assert dev is not None
    T = C.table()
    E = C.load_golden()
    m, flags, sides = C.probe_report(dev)
    # the largest device-to-host difference per bucket, in the same metric: reported, not asserted
    d2h = {}
    for name in C.ORDER:
        if name == "outlier":
            continue
        d = [float(np.abs(a - b).max() / max(1.0, np.abs(b).max())) if np.all(np.isfinite(a)) and np.all(np.isfinite(b)) else float("inf") for a, b in zip(dev[name], host[name])]
        C.fold(d2h, T[name]["buckets"], d)
    _summary("device half", m, E)
    print("largest device-to-host difference %.3g (%s)" % (max(d2h.values()), max(d2h, key=d2h.get)))
    assert np.array_equal(flags, T["outlier"]["flag"]), np.nonzero(flags != T["outlier"]["flag"])[0]
    assert np.array_equal(sides, T["term"]["linear"]), np.nonzero(sides != T["term"]["linear"])[0]
    C.check(m, E, "the device half of sim3_math.h", other=d2h)


def test_write_back_kernels_over_the_exp_table():
    """essential_graph_correct: T = [R | t / s] of exp(x), points through exp(x)^-1 exp(x0); 129 vertices and 257 points a call"""
    from ceres_mono_orb_slam2_amd import optimizer
    res = [optimizer.essential_graph_correct(p["x0"], p["x"], p["ref"], p["pts"]) for p in C.correct_problems()]
    m = C.correct_errors(res)
    E = C.load_golden()
    _summary("essential_graph_correct", m, E)
    C.check(m, E, "essential_graph_correct")


def test_sim3_solver_returns_the_element_it_was_given():
    """optimize_sim3 without terms returns exp(log(S)), computed in k_sim3_lm: the same group element (as a matrix: for w < 0 the
    quaternion's sign may flip)"""
    from ceres_mono_orb_slam2_amd import optimizer
    e3 = np.zeros((0, 3)); e2 = np.zeros((0, 2)); e1 = np.zeros(0, np.float32)
    out = []
    for S in C.table()["log"]["inputs"]:
        n, S12, _, s = optimizer.optimize_sim3(C.K4, C.K4, S, e3, e2, e1, e3, e2, e1)
        assert n == 0 and s["iterations"] == 0
        out.append(S12)
    m = C.explog_errors(np.stack(out))
    E = C.load_golden()
    _summary("optimize_sim3 without terms", m, E)
    C.check(m, E, "exp(log(S)) in k_sim3_lm")


def test_graph_solver_on_two_vertex_graphs():
    """initial_cost against |r|^2 / 2 in mp; a consistent edge leaves the free vertex at the known answer exp(x_j) = Sji exp(x_i) with a
    final cost of rounding size"""
    from ceres_mono_orb_slam2_amd import optimizer
    G = C.graph_problems()
    res = [optimizer.optimize_essential_graph(g["lie"], g["fixed"], g["ej"], g["ei"], g["Sji"]) for g in G]
    for g, (x, s) in zip(G, res):
        assert np.array_equal(x[0], g["lie"][0])                     # the fixed vertex
        if g["consistent"]:
            assert s["final_cost"] <= 1e-16 * max(s["initial_cost"], 1.0) + 1e-18, (g["bucket"], s)
    m = C.graph_errors(res, None)
    E = C.load_golden()
    _summary("optimize_essential_graph", m, E)
    C.check(m, E, "optimize_essential_graph on two-vertex graphs")


def test_table_builder_takes_the_log_of_every_corrected_sim3():
    """essential_graph_assemble on the device: lie7 of 130 keyframes whose corrected Sim(3)s are cases of the log table"""
    import torch
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    from tests.test_gpu_essgraph import TABLES
    mp_, idx = C.assemble_map()
    tab = {k: (None if mp_.get(k) is None else torch.as_tensor(np.array(mp_[k])).cuda()) for k in TABLES}
    r = lc.essential_graph_assemble(mp_["loop"], mp_["cur"], tab, min_weight=mp_["min_weight"], device=True)
    torch.cuda.synchronize()
    assert int(r["status"].item()) == 0
    n = int(r["counts"][0].item())
    assert n == C.N_KF
    vtx_kf = r["vtx_kf"].cpu().numpy()[:n]; lie7 = r["lie7"].cpu().numpy()[:7 * n].reshape(n, 7)
    assert sorted(vtx_kf.tolist()) == list(range(C.N_KF))
    m = C.assemble_errors(vtx_kf, lie7)
    E = C.load_golden()
    _summary("essential_graph_assemble", m, E)
    C.check(m, E, "lie7 of essential_graph_assemble")
