"""Initializer::Initialize on the GPU (orbt_initialize*) against the numpy restatement tests/npinit.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import initcases  # noqa: E402
import npinit  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def init():
    from ceres_mono_orb_slam2_amd import initializer
    return initializer


def _run(init, case):
    k1, k2, m, K, sets = initcases.make_case(case)
    d = init.initialize(k1, k2, m, K, 1.0, len(sets), sets, trace=True)
    return (k1, k2, m, K, sets), d


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)) if a.size else 0.0


@pytest.mark.parametrize("case", [initcases.WITNESS[k] for k in ("H success", "F success", "parallax")] + [initcases.CASES[21]])
def test_scoring_pinned_exactly(init, case):
    """The trace's per-iteration matrices through the restatement's Check*: scores, best indices, inlier masks and RH identical."""
    (k1, k2, m, K, sets), d = _run(init, case)
    sh, inl_h = npinit.check_homography(d["H21"], d["H12"], k1, k2, m)
    sf, inl_f = npinit.check_fundamental(d["F21"], k1, k2, m)
    assert np.array_equal(sh.view(np.uint32), d["scores_h"].view(np.uint32))
    assert np.array_equal(sf.view(np.uint32), d["scores_f"].view(np.uint32))
    SH, bh = npinit.best_of(sh)
    SF, bf = npinit.best_of(sf)
    assert (bh, bf) == (d["best_h"], d["best_f"])
    assert np.float32(d["score_h"]) == SH and np.float32(d["score_f"]) == SF
    assert np.array_equal(inl_h[bh], d["inliers_h"]) and np.array_equal(inl_f[bf], d["inliers_f"])
    # the scores are exactly invariant under H -> -H and F -> -F
    assert np.array_equal(npinit.check_homography(-d["H21"], -d["H12"], k1, k2, m)[0].view(np.uint32), sh.view(np.uint32))
    assert np.array_equal(npinit.check_fundamental(-d["F21"], k1, k2, m)[0].view(np.uint32), sf.view(np.uint32))
    RH = np.float32(SH / (SH + SF))
    assert np.float32(d["rh"]).view(np.uint32) == RH.view(np.uint32)
    assert d["model"] == (0 if np.float64(RH) > 0.40 else 1)


@pytest.mark.parametrize("case", [initcases.WITNESS[k] for k in ("H success", "F success", "parallax")] + [initcases.CASES[22]])
def test_reconstruction_pinned(init, case):
    """The trace's motions through the restatement's CheckRT: n_good and triangulated identical, P3D 1e-9 relative, parallax 2 ulp."""
    (k1, k2, m, K, sets), d = _run(init, case)
    inl = d["inliers_h"] if d["model"] == 0 else d["inliers_f"]
    nmot = 8 if d["model"] == 0 else 4
    for mo in range(nmot):
        r = npinit.check_rt(d["motion_R"][mo], d["motion_t"][mo], k1, k2, m, inl, K)
        assert r["n_good"] == d["n_good"][mo], mo
        p_ref, p_dev = np.float32(r["parallax"]), np.float32(d["parallax"][mo])
        assert abs(int(p_ref.view(np.int32)) - int(p_dev.view(np.int32))) <= 2, (mo, p_ref, p_dev)
    if d["success"]:
        i1, _ = npinit.match_list(m)
        r = npinit.check_rt(d["motion_R"][d["motion"]], d["motion_t"][d["motion"]], k1, k2, m, inl, K)
        tri = np.zeros(len(k1), bool); tri[i1[r["tri"]]] = True
        assert np.array_equal(tri, d["triangulated"].astype(bool))
        rows = i1[r["good"]]
        assert _rel(d["P3D"][rows], r["P"][r["good"]]) <= 1e-9


def test_end_to_end_matrix(init):
    """>= 40 seeded cases (all four kinds, 9 to ~4 000 matches, 1 / 200 / 1 000 iterations, outliers 0 to 0.6, degenerate sets)
    against the whole restatement; the matrix must reach H success, F success, a parallax and a count rejection."""
    reached, skips = set(), 0
    for case in initcases.CASES:
        (k1, k2, m, K, sets), d = _run(init, case)
        ref = npinit.initialize(k1, k2, m, K, 1.0, len(sets), sets)
        near_tie = False
        for sc in (ref["score_h"], ref["score_f"]):
            top = np.sort(np.asarray(sc, np.float64))[-2:]
            if len(top) == 2 and top[1] > 0 and (top[1] - top[0]) <= 1e-6 * top[1]:
                near_tie = True
        if abs(float(ref["rh"]) - 0.40) <= 1e-6:
            near_tie = True
        same = (d["success"], d["model"], d["reason"], d["best_h"], d["best_f"], d["motion"]) == \
            (ref["success"], ref["model"], ref["reason"], ref["best_h"], ref["best_f"], ref["motion"])
        if not same:
            assert near_tie, (case, {k: d[k] for k in ("success", "model", "reason", "best_h", "best_f", "motion")},
                              {k: ref[k] for k in ("success", "model", "reason", "best_h", "best_f", "motion")})
            skips += 1
            continue
        reached.add(("H" if d["model"] == 0 else "F") + " success" if d["success"] else d["reason"])
        if d["success"]:
            assert _rel(d["R21"], ref["R21"]) <= 1e-9 and _rel(d["t21"], ref["t21"]) <= 1e-9
            w = ~np.isnan(ref["P3D"][:, 0])
            assert _rel(d["P3D"][w], ref["P3D"][w]) <= 1e-9
            assert np.array_equal(d["triangulated"].astype(bool), ref["triangulated"])
    assert skips <= 2
    assert {"H success", "F success"} <= reached, reached
    assert reached & {npinit.H_PARALLAX, npinit.F_PARALLAX}, reached
    assert reached & {npinit.H_FEW, npinit.F_FEW}, reached


def test_no_model_is_a_rejection(init):
    """Every hypothesis scores NaN (all frame-1 keypoints at one position: Normalize divides by a zero deviation), so no model
    scores above 0: ORBT_INIT_NO_MODEL, the outputs untouched, as the restatement says.  The position is (256, 128): the float sums
    of Normalize are then exact and the deviation is exactly zero.  (At an arbitrary position the deviation is a rounding residue, the
    normalised points are all (+-1, +-1), every F system has rank 1, and since i_svd3 returns a finite SVD at rank 1 such a pair is
    rejected for too few triangulated points instead - test_gpu_small_dense.py has the rank-1 cases.)"""
    k1, k2, m, K, sets = initcases.make_case(initcases.WITNESS["F success"])
    k1 = k1.copy(); k1[:] = (256.0, 128.0)
    out = {"R21": np.full((3, 3), 7.0), "t21": np.full(3, 7.0), "P3D": np.full((len(k1), 3), -1.0), "triangulated": np.full(len(k1), 9, np.uint8)}
    d = init.initialize(k1, k2, m, K, 1.0, len(sets), sets, out=out)
    ref = npinit.initialize(k1, k2, m, K, 1.0, len(sets), sets)
    assert d["reason"] == ref["reason"] == npinit.NO_MODEL
    assert (d["best_h"], d["best_f"], d["motion"]) == (-1, -1, -1) and d["n_inliers"] == 0
    assert (out["R21"] == 7).all() and (out["P3D"] == -1).all() and (out["triangulated"] == 9).all()


def test_outputs_untouched_on_failure_and_unaccepted_rows_stay(init):
    for key in ("F success", "count"):
        k1, k2, m, K, sets = initcases.make_case(initcases.WITNESS[key])
        n1 = len(k1)
        out = {"R21": np.full((3, 3), 7.0), "t21": np.full(3, 7.0), "P3D": np.full((n1, 3), -123.0), "triangulated": np.full(n1, 9, np.uint8)}
        d = init.initialize(k1, k2, m, K, 1.0, len(sets), sets, out=out)
        if key == "count":
            assert not d["success"]
            assert (out["R21"] == 7).all() and (out["t21"] == 7).all() and (out["P3D"] == -123).all() and (out["triangulated"] == 9).all()
        else:
            assert d["success"]
            ref = npinit.initialize(k1, k2, m, K, 1.0, len(sets), sets)
            w = ~np.isnan(ref["P3D"][:, 0])
            assert (out["P3D"][~w] == -123).all() and not (out["P3D"][w] == -123).any()
            assert set(np.unique(out["triangulated"])) <= {0, 1}


def test_batch_matches_single_calls(init):
    """A 64-pair batch of mixed sizes is bit-identical to 64 single calls."""
    import torch
    cases = [initcases.CASES[i % len(initcases.CASES)] for i in range(64)]
    cases = [(c[0], c[1], c[2], c[3], c[4], 200, c[6]) for c in cases]
    data = [initcases.make_case(c) for c in cases]
    singles = [init.initialize(k1, k2, m, K, 1.0, 200, s) for (k1, k2, m, K, s) in data[:62]]
    # pair 62: a matches12 entry outside [-1, n2); pair 63: fewer than 8 matches.  Each fails alone (ORBT_INIT_BAD_INPUT).
    k1, k2, m, K, s = data[62]; m = m.copy(); m[np.nonzero(m >= 0)[0][3]] = len(k2); data[62] = (k1, k2, m, K, s)
    k1, k2, m, K, s = data[63]; m = m.copy(); m[np.nonzero(m >= 0)[0][7:]] = -1; data[63] = (k1, k2, m, K, s)
    off1 = np.cumsum([0] + [len(d[0]) for d in data]).astype(np.int32)
    off2 = np.cumsum([0] + [len(d[1]) for d in data]).astype(np.int32)
    dev = torch.device("cuda")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731
    n1t = int(off1[-1])
    out = {"R21": torch.zeros((64, 3, 3), dtype=torch.float64, device=dev), "t21": torch.zeros((64, 3), dtype=torch.float64, device=dev),
           "P3D": torch.full((n1t, 3), -5.0, dtype=torch.float64, device=dev), "triangulated": torch.full((n1t,), 7, dtype=torch.uint8, device=dev),
           "report": torch.zeros(init.report_bytes(64), dtype=torch.uint8, device=dev)}
    init.initialize_batch_device(t(np.concatenate([d[0] for d in data]), np.float32), t(off1, np.int32), t(np.concatenate([d[1] for d in data]), np.float32),
                                 t(off2, np.int32), t(np.concatenate([d[2] for d in data]), np.int32), t(np.stack([d[3] for d in data]), np.float32),
                                 1.0, 200, t(np.stack([d[4] for d in data]), np.int32), out)
    torch.cuda.synchronize()
    reps = init.decode_reports(out["report"].cpu().numpy())
    P = out["P3D"].cpu().numpy(); tri = out["triangulated"].cpu().numpy(); R = out["R21"].cpu().numpy(); tt = out["t21"].cpu().numpy()
    for p in (62, 63):
        r = reps[p]
        assert r["reason"] == init.BAD_INPUT and r["model"] == -1 and (r["best_h"], r["best_f"], r["motion"]) == (-1, -1, -1)
        assert r["score_h"] == 0 and r["score_f"] == 0 and r["n_inliers"] == 0 and not r["n_good"].any() and not r["parallax"].any()
        rows = slice(off1[p], off1[p + 1])
        assert (P[rows] == -5).all() and (tri[rows] == 7).all() and (R[p] == 0).all()
    n_ok = 0
    for p, s in enumerate(singles):
        r = reps[p]
        for k in init.REPORT_FIELDS:
            assert np.array_equal(np.asarray(r[k]), np.asarray(s[k])), (p, k)
        assert np.array_equal(r["n_good"], s["n_good"]) and np.array_equal(r["parallax"].view(np.uint32), s["parallax"].view(np.uint32))
        rows = slice(off1[p], off1[p + 1])
        if s["success"]:
            n_ok += 1
            assert np.array_equal(R[p], s["R21"]) and np.array_equal(tt[p], s["t21"])
            w = s["P3D"][:, 0] != 0
            assert np.array_equal(P[rows][w], s["P3D"][w]) and (P[rows][~w] == -5).all()
            assert np.array_equal(tri[rows], s["triangulated"])
        else:
            assert (P[rows] == -5).all() and (tri[rows] == 7).all() and (R[p] == 0).all()
    assert n_ok >= 4
