"""PnPsolver::iterate on the GPU (orbt_pnp_*) against the numpy restatement tests/nppnp.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nppnp  # noqa: E402
import pnpcases  # noqa: E402

pytestmark = pytest.mark.gpu

# ground truth on noise-free `general` scenes with 30 % outliers (pnpcases.GT_CASES), nppnp(lapack=True) on the CPU: the maximum over
# the cases of max |R - R_gt| and of |t - t_gt| / |t_gt|; the device may be 10 x that (see test_ground_truth's docstring)
GT_LAPACK_MAX_DR = 1.2e-7
GT_LAPACK_MAX_DT = 7.7e-7


@pytest.fixture(scope="module")
def pnp():
    from ceres_mono_orb_slam2_amd import pnp
    return pnp


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300) if a.size else 0.0


def _call(pnp, c, sets=None, state=None, trace=True):
    return pnp.iterate(c["p3d"], c["p2d"], c["max_err"], c["K4"], c["min_inliers"], c["sets"] if sets is None else sets, state=state, trace=trace)


def _ref(c, sets=None, state=None):
    return nppnp.iterate(c["p3d"], c["p2d"], c["max_err"], c["K4"], c["min_inliers"], c["sets"] if sets is None else sets, state=state)


def _same_state(a, b):
    return a.best_count == b.best_count and np.array_equal(a.best_mask != 0, b.best_mask != 0)


def _check_equal(d, r, what=""):
    assert (d["status"], d["consumed"], d["n_inliers"], d["n_refits"]) == (r["status"], r["consumed"], r["n_inliers"], r["n_refits"]), what
    assert np.array_equal(d["inliers"], r["inliers"]), what
    assert _same_state(d["state"], r["state"]), what
    if r["status"] in (nppnp.REFINED, nppnp.EXHAUSTED_BEST):
        assert _rel(d["Tcw"][:3, :3], r["Tcw"][:3, :3]) <= 1e-9 and _rel(d["Tcw"][:3, 3], r["Tcw"][:3, 3]) <= 1e-9, what
    else:
        assert np.array_equal(d["Tcw"], np.eye(4)), what
    if r["state"].best_count:
        assert _rel(d["state"].best_Tcw, r["state"].best_Tcw) <= 1e-9, what


HYP_CASES = pnpcases.HYP_CASES


@pytest.mark.parametrize("case", HYP_CASES)
def test_check_inliers_pinned_exactly(pnp, case):
    """The trace's per-iteration R, t through nppnp.check_inliers: identical counts; identical masks for the best and the returned
    hypothesis."""
    c = pnpcases.make_case(case)
    d = _call(pnp, c)
    assert d["consumed"] >= 1
    best = 0
    for it in range(d["consumed"]):
        m = nppnp.check_inliers(d["R"][it], d["t"][it], c["K4"], c["p3d"], c["p2d"], c["max_err"])
        assert int(m.sum()) == d["count"][it], it
        if m.sum() >= c["min_inliers"] and m.sum() > best:
            best = int(m.sum())
            best_mask = m
    if best:
        assert d["state"].best_count == best and np.array_equal(d["state"].best_mask != 0, best_mask)
    for k in range(d["n_refits"]):
        m = nppnp.check_inliers(d["refit_R"][k], d["refit_t"][k], c["K4"], c["p3d"], c["p2d"], c["max_err"])
        assert int(m.sum()) == d["refit_count"][k]
        if d["status"] == nppnp.REFINED and k == d["n_refits"] - 1:
            assert np.array_equal(m, d["inliers"])


@pytest.mark.parametrize("case", HYP_CASES)
def test_hypotheses_match_restatement(pnp, case):
    """Every set of the case as a hypothesis (a rejecting caller: 300 sets in chained calls would stop early, so the sets are
    evaluated through a min_inliers nobody reaches): R, t and the chosen approximation against nppnp in device order within 1e-9
    relative.  Hypotheses whose two best approximations are within 1e-9 relative may pick another N: excluded and counted, at most 2 %."""
    c = pnpcases.make_case(case, iterations=300)
    n = len(c["p3d"])
    # max_err = 0 and min_inliers = n: no point is ever an inlier (error2 < 0 is false), so the walk uses every set
    d = pnp.iterate(c["p3d"], c["p2d"], np.zeros_like(c["max_err"]), c["K4"], n, c["sets"], trace=True)
    assert d["consumed"] == 300 and d["status"] == nppnp.EXHAUSTED_NONE
    R, t, N, err, errs = nppnp.hypotheses(c["p3d"], c["p2d"], c["K4"], c["sets"])
    excluded = compared = 0
    for it in range(300):
        e = np.sort(errs[it])
        close = np.isfinite(e[1]) and abs(e[1] - e[0]) <= 1e-9 * abs(e[1])
        if close and d["approx"][it] != N[it]:
            excluded += 1
            continue
        if not np.all(np.isfinite(R[it])):
            assert not np.all(np.isfinite(d["R"][it]))
            continue
        assert d["approx"][it] == N[it], it
        assert _rel(d["R"][it], R[it]) <= 1e-9 and _rel(d["t"][it], t[it]) <= 1e-9 and _rel(d["rep_error"][it], err[it]) <= 1e-9, it
        compared += 1
    print("hypotheses: %d compared, %d excluded" % (compared, excluded))
    assert excluded <= 0.02 * 300


@pytest.mark.parametrize("case", pnpcases.CASES, ids=lambda c: "%s-n%d-o%g-s%g" % (c[1], c[2], c[3], c[4]))
def test_end_to_end_matrix(pnp, case):
    c = pnpcases.make_case(case)
    _check_equal(_call(pnp, c), _ref(c), str(case))


def test_matrix_reaches_every_status():
    seen = {_ref(pnpcases.make_case(c))["status"] for c in pnpcases.CASES}
    assert seen == {nppnp.REFINED, nppnp.EXHAUSTED_BEST, nppnp.EXHAUSTED_NONE, nppnp.TOO_FEW}


def test_success_from_incoming_state(pnp):
    """The incoming best mask holds every true inlier: the first qualifying hypothesis is no record, Refine runs on the incoming
    mask and succeeds."""
    c = pnpcases.make_case((5000, "general", 50, 0.3, 0.0))
    good = ~c["scene"]["outlier"]
    states = []
    for mk in (pnp.PnPState, nppnp.State):
        st = mk(50)
        st.best_mask = good.astype(np.uint8); st.best_count = int(good.sum()); st.best_Tcw = np.eye(4) * 3.0
        states.append(st)
    d, r = _call(pnp, c, state=states[0]), _ref(c, state=states[1])
    assert r["status"] == nppnp.REFINED and r["state"].best_count == int(good.sum()) and np.array_equal(r["state"].best_Tcw, np.eye(4) * 3.0)
    _check_equal(d, r)
    assert np.array_equal(d["state"].best_Tcw, np.eye(4) * 3.0)


def test_refit_that_fails(pnp):
    """Exactly min_inliers true inliers among 2 min_inliers points: a clean hypothesis qualifies and becomes the record, its refit has
    min_inliers inliers, which is not MORE than the minimum: the walk goes on to exhaustion and returns the best."""
    c = pnpcases.make_case(pnpcases.REFIT_FAILS)
    d, r = _call(pnp, c), _ref(c)
    assert r["status"] == nppnp.EXHAUSTED_BEST and r["n_refits"] >= 1 and r["n_inliers"] == c["min_inliers"]
    _check_equal(d, r)


def test_continuation(pnp):
    """One call with 300 sets against the chain a rejecting caller makes: after every returned pose, call again with the remaining
    sets and the returned state.  A single call stops at its first success, so the chain is compared link by link with the
    restatement's chain, and the chain's first link with the single call, bit for bit."""
    c = pnpcases.make_case((5001, "general", 200, 0.3, 0.5), iterations=300)
    single = _call(pnp, c)
    pos, st_d, st_r, links = 0, None, None, 0
    while pos < 300:
        d = _call(pnp, c, sets=c["sets"][pos:], state=st_d)
        r = _ref(c, sets=c["sets"][pos:], state=st_r)
        _check_equal(d, r, "link %d" % links)
        if links == 0:
            assert d["consumed"] == single["consumed"] and np.array_equal(d["Tcw"], single["Tcw"]) and np.array_equal(d["inliers"], single["inliers"])
            k = single["consumed"]
            assert np.array_equal(d["R"][:k], single["R"][:k]) and np.array_equal(d["t"][:k], single["t"][:k])
        st_d, st_r = d["state"], r["state"]
        pos += d["consumed"]
        links += 1
        if d["status"] != nppnp.REFINED:
            break
    assert pos == 300 and links >= 3
    # the hypotheses do not depend on where a call starts: the chain's traces concatenate to those of one walk over all sets
    n = len(c["p3d"])
    walk = pnp.iterate(c["p3d"], c["p2d"], np.zeros_like(c["max_err"]), c["K4"], n, c["sets"], trace=True)
    k = single["consumed"]
    assert np.array_equal(walk["R"][:k], single["R"][:k]) and np.array_equal(walk["t"][:k], single["t"][:k])


def test_batch_equals_singles(pnp):
    """64 candidates of ragged N, two BAD_INPUT and one TOO_FEW, against 64 single calls, bit for bit; the poisoned outputs of the
    failed candidates stay untouched."""
    import torch
    rng = np.random.default_rng(11)
    cands, singles = [], []
    for i in range(64):
        n = int(rng.integers(12, 400))
        kind, of, noise = ("general", "planar")[i % 2], (0.0, 0.3, 0.6)[i % 3], (0.0, 0.5, 1.0)[(i // 3) % 3]
        if i == 20:
            kind, n = "few", 6
        c = pnpcases.make_case((6000 + i, kind, n, of, noise))
        cands.append(dict(p3d=c["p3d"], p2d=c["p2d"], max_err=c["max_err"], K4=c["K4"], min_inliers=c["min_inliers"], sets=c["sets"].copy()))
    cands[7]["sets"][0, 2] = len(cands[7]["p3d"])                # out of range
    cands[33]["sets"][1, 3] = cands[33]["sets"][1, 0]            # repeated inside a set
    for i, c in enumerate(cands):
        if i in (7, 33):
            singles.append(None)
            continue
        singles.append(pnp.iterate(c["p3d"], c["p2d"], c["max_err"], c["K4"], c["min_inliers"], c["sets"]))
    # the device entry, with poisoned outputs
    dev = torch.device("cuda")
    ns = [len(c["sets"]) for c in cands]
    I = max(ns)
    off = np.concatenate([[0], np.cumsum([len(c["p3d"]) for c in cands])]).astype(np.int32)
    sets = np.zeros((64, I, 4), np.int32)
    for i, c in enumerate(cands):
        sets[i, :ns[i]] = c["sets"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    nt = int(off[-1])
    d_bc = up(np.zeros(64, np.int32)); d_bm = up(np.zeros(nt, np.uint8)); d_bt = up(np.full((64, 4, 4), 7.0))
    d_res = up(np.full(pnp.result_bytes(64), 0x5a, np.uint8)); d_inl = up(np.full(nt, 0x5a, np.uint8))
    ws = pnp.iterate_batch_device(up(np.concatenate([c["p3d"] for c in cands])), up(np.concatenate([c["p2d"] for c in cands])),
                                  up(np.concatenate([c["max_err"] for c in cands])), up(off), up(np.stack([c["K4"] for c in cands])),
                                  up(np.array([c["min_inliers"] for c in cands], np.int32)), up(np.array(ns, np.int32)), up(sets), d_bc, d_bm, d_bt,
                                  d_res, d_inl)
    torch.cuda.synchronize()
    del ws
    raw = d_res.cpu().numpy()
    res = pnp.decode_results(raw)
    inl, bm, bc, bt = d_inl.cpu().numpy(), d_bm.cpu().numpy(), d_bc.cpu().numpy(), d_bt.cpu().numpy()
    sz = pnp.result_bytes(1)
    for i in range(64):
        a, b = int(off[i]), int(off[i + 1])
        if i in (7, 33):
            assert res[i]["status"] == pnp.BAD_INPUT and res[i]["consumed"] == 0
            assert np.all(raw[i * sz + 16:(i + 1) * sz] == 0x5a) and np.all(inl[a:b] == 0x5a)
            assert bc[i] == 0 and not bm[a:b].any() and np.all(bt[i] == 7.0)
            continue
        s = singles[i]
        assert (res[i]["status"], res[i]["consumed"], res[i]["n_inliers"], res[i]["n_refits"]) == (s["status"], s["consumed"], s["n_inliers"], s["n_refits"]), i
        assert np.array_equal(res[i]["Tcw"], s["Tcw"]) and np.array_equal(inl[a:b] != 0, s["inliers"]), i
        assert bc[i] == s["state"].best_count and np.array_equal(bm[a:b], s["state"].best_mask), i
        if i == 20:
            assert res[i]["status"] == pnp.TOO_FEW and np.all(bt[i] == 7.0)
        elif bc[i]:
            assert np.array_equal(bt[i], s["state"].best_Tcw), i
    # the convenience wrapper gives the same
    out = pnp.iterate_batch([dict(c) for i, c in enumerate(cands) if i not in (7, 33)])
    k = 0
    for i in range(64):
        if i in (7, 33):
            continue
        assert out[k]["status"] == singles[i]["status"] and np.array_equal(out[k]["Tcw"], singles[i]["Tcw"]), i
        k += 1


def test_ground_truth(pnp):
    """Noise-free `general` scenes with 30 % outliers: the returned pose against the ground truth.  nppnp(lapack=True) on the same
    cases on the CPU gives max |R - R_gt| = 1.2e-7 and |t - t_gt| / |t_gt| = 7.7e-7 at most over pnpcases.GT_CASES (per-case values
    scatter by two orders of magnitude; the float32 world points and pixels bound both).  The device may be 10 x that maximum: the
    factor covers its different null-space basis and Jacobi against LAPACK rounding (measured on an MI355X: 5.6e-8 and 9.2e-7).  Planar
    scenes are printed, not bounded (measured: at most 6.9e-8 and 3.7e-7)."""
    for case in pnpcases.GT_CASES + pnpcases.PLANAR_GT_CASES:
        c = pnpcases.make_case(case)
        d = _call(pnp, c, trace=False)
        dR = np.abs(d["Tcw"][:3, :3] - c["scene"]["R"]).max()
        dt = np.linalg.norm(d["Tcw"][:3, 3] - c["scene"]["t"]) / np.linalg.norm(c["scene"]["t"])
        print("ground truth %s: status %d consumed %d dR %.3g dt %.3g" % (case, d["status"], d["consumed"], dR, dt))
        if case[1] == "general":
            assert d["status"] == nppnp.REFINED
            assert dR <= 10 * GT_LAPACK_MAX_DR and dt <= 10 * GT_LAPACK_MAX_DT, case
