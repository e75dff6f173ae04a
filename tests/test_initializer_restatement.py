"""CPU checks of the numpy restatement of Initializer::Initialize (tests/npinit.py): its SVDs against LAPACK, recovery of
noise-free ground truth, every decision rule of ReconstructH / ReconstructF, the RANSAC set draw, and the witness cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import initcases  # noqa: E402
import npinit  # noqa: E402
from ceres_mono_orb_slam2_amd import synth  # noqa: E402
from ceres_mono_orb_slam2_amd.initializer import draw_ransac_sets  # noqa: E402


def _norm_sign(v):
    v = v / np.linalg.norm(v)
    return v * np.sign(v[np.argmax(np.abs(v))])


@pytest.mark.parametrize("m", [8, 16])
def test_null_vector_matches_lapack(m):
    rng = np.random.default_rng(m)
    A = rng.normal(size=(60, m, 9))
    if m == 16:                                                 # a known null vector; sigma_8 >= 1e-3 sigma_1 by construction
        x = rng.normal(size=(60, 9))
        A = A - (A @ x[:, :, None]) @ x[:, None, :] / (x * x).sum(1)[:, None, None]
    got = npinit.null_vector(A)
    n = 0
    for a, g in zip(A, got):
        s = np.linalg.svd(a, compute_uv=False)
        if s[7] < 1e-3 * s[0]:
            continue
        vt = np.linalg.svd(a)[2]
        assert np.abs(_norm_sign(g) - _norm_sign(vt[-1])).max() < 1e-9
        n += 1
    assert n >= 40


def test_svd3_matches_lapack():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(50, 3, 3))
    U, S, V = npinit.svd3(A)
    for a, u, s, v in zip(A, U, S, V):
        sl = np.linalg.svd(a, compute_uv=False)
        assert np.allclose(s, sl, rtol=1e-12, atol=0)
        assert np.allclose(u @ np.diag(s) @ v.T, a, atol=1e-12)
        assert np.allclose(u.T @ u, np.eye(3), atol=1e-12) and np.allclose(v.T @ v, np.eye(3), atol=1e-12)
        ul, _, vtl = np.linalg.svd(a)
        for k in range(3):
            assert np.abs(_norm_sign(v[:, k]) - _norm_sign(vtl[k])).max() < 1e-9
    # rank 2: the third left vector is still defined (u0 x u1)
    A[:, 2] = A[:, 0] + A[:, 1]
    U, S, V = npinit.svd3(A)
    assert np.allclose(np.einsum("bij,bik->bjk", U, U), np.eye(3), atol=1e-12)


@pytest.mark.parametrize("kind,model,seed", [("general", 1, 10), ("planar", 0, 0)])
def test_noise_free_scene_recovers_ground_truth(kind, model, seed):
    s = synth.make_two_view(seed, kind, 400, 0.0, 0.0)
    nm = int((s["matches12"] >= 0).sum())
    r = npinit.initialize(s["kps1"], s["kps2"], s["matches12"], s["K4"], 1.0, 200, draw_ransac_sets(nm, 200))
    assert r["success"] and r["model"] == model
    tg = s["t"] / np.linalg.norm(s["t"])
    # (float32 keypoints and float32 normalised coordinates, as in the reference, bound the agreement)
    assert np.abs(r["R21"] - s["R"]).max() < 1e-6
    assert np.abs(r["t21"] - tg).max() < 1e-5
    w = ~np.isnan(r["P3D"][:, 0])
    assert w.sum() > 300
    Xg = s["X"][w] / np.linalg.norm(s["t"])
    assert (np.linalg.norm(r["P3D"][w] - Xg, axis=1) / np.linalg.norm(Xg, axis=1)).max() < 1e-5


@pytest.mark.parametrize("key,reason,model", [("H success", npinit.OK, 0), ("F success", npinit.OK, 1), ("parallax", npinit.F_PARALLAX, 1),
                                              ("count", npinit.F_FEW, 1)])
def test_witness_cases_reach_their_branch(key, reason, model):
    k1, k2, m, K, sets = initcases.make_case(initcases.WITNESS[key])
    r = npinit.initialize(k1, k2, m, K, 1.0, len(sets), sets)
    assert (r["reason"], r["model"]) == (reason, model)


H = npinit.decide_h
F = npinit.decide_f
f = np.float32


@pytest.mark.parametrize("ng,par,N,exp", [
    ([100, 10, 0, 0, 0, 0, 0, 0], [2] * 8, 100, (0, npinit.OK)),
    ([10, 100, 0, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0, 0, 0], 100, (1, npinit.OK)),
    ([100, 75, 0, 0, 0, 0, 0, 0], [2] * 8, 100, (-1, npinit.H_AMBIGUOUS)),     # second == 0.75 best: not <
    ([100, 74, 0, 0, 0, 0, 0, 0], [2] * 8, 100, (0, npinit.OK)),
    ([100, 0, 0, 0, 0, 0, 0, 0], [1.0] + [0] * 7, 100, (0, npinit.OK)),        # bestParallax >= 1 (ReconstructH's >=)
    ([100, 0, 0, 0, 0, 0, 0, 0], [np.nextafter(f(1), f(0))] + [0] * 7, 100, (-1, npinit.H_PARALLAX)),
    ([50, 0, 0, 0, 0, 0, 0, 0], [2] * 8, 50, (-1, npinit.H_FEW)),              # bestGood > 50
    ([51, 0, 0, 0, 0, 0, 0, 0], [2] * 8, 56, (0, npinit.OK)),                  # 51 > 0.9 * 56 = 50.4
    ([51, 0, 0, 0, 0, 0, 0, 0], [2] * 8, 57, (-1, npinit.H_FEW)),              # 51 > 51.3 fails
    ([0] * 8, [0] * 8, 10, (-1, npinit.H_AMBIGUOUS)),                          # nothing triangulated: 0 < 0 fails first
    ([80, 90, 0, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0, 0, 0], 100, (-1, npinit.H_AMBIGUOUS)),   # the first best becomes the second
])
def test_reconstruct_h_rules(ng, par, N, exp):
    assert H(np.array(ng), np.array(par, np.float32), N) == exp


@pytest.mark.parametrize("ng,par,N,exp", [
    ([100, 0, 0, 0], [2, 0, 0, 0], 100, (0, npinit.OK)),
    ([0, 0, 100, 0], [0, 0, 2, 0], 100, (2, npinit.OK)),
    ([89, 0, 0, 0], [2, 0, 0, 0], 100, (-1, npinit.F_FEW)),                    # maxGood < int(0.9 N) = 90
    ([90, 0, 0, 0], [2, 0, 0, 0], 100, (0, npinit.OK)),
    ([49, 0, 0, 0], [2, 0, 0, 0], 40, (-1, npinit.F_FEW)),                     # ... or < 50
    ([100, 71, 0, 0], [2, 2, 0, 0], 100, (-1, npinit.F_AMBIGUOUS)),            # 71 > 0.7 * 100
    ([100, 70, 0, 0], [2, 2, 0, 0], 100, (0, npinit.OK)),
    ([100, 0, 0, 0], [1.0, 0, 0, 0], 100, (-1, npinit.F_PARALLAX)),            # strict > (ReconstructF), unlike ReconstructH's >=
    ([100, 0, 0, 0], [np.nextafter(f(1), f(2)), 0, 0, 0], 100, (0, npinit.OK)),
    ([0, 100, 0, 100], [0, 0.5, 0, 9], 100, (-1, npinit.F_AMBIGUOUS)),
    ([0, 100, 0, 0], [0, 0.5, 0, 0], 100, (-1, npinit.F_PARALLAX)),
    ([0, 0, 0, 0], [0, 0, 0, 0], 0, (-1, npinit.F_FEW)),
])
def test_reconstruct_f_rules(ng, par, N, exp):
    assert F(np.array(ng), np.array(par, np.float32), N) == exp


def test_reconstruct_f_does_not_fall_through():
    # two motions tie at maxGood only if nsimilar > 1 rejects first; so the chain's first match is the only one tried:
    # the first motion with maxGood fails its parallax -> F fails although a later branch would not be reached anyway
    assert F(np.array([100, 0, 0, 0]), np.array([0.5, 0, 0, 9], np.float32), 100) == (-1, npinit.F_PARALLAX)
    assert F(np.array([0, 0, 0, 100]), np.array([9, 9, 9, 0.9], np.float32), 100) == (-1, npinit.F_PARALLAX)


def test_draw_ransac_sets_scripted():
    seq = iter([0, 1, 2, 3, 4, 0, 0, 0, 9, 0, 0, 0, 0, 0, 0, 0])
    calls = []

    def randint(lo, hi):
        calls.append((lo, hi))
        return next(seq)
    s = draw_ransac_sets(10, 2, randint)
    # it 0 on [0..9]: r=0 -> 0, list [9,1..8]; r=1 -> 1, [9,8,2..7]; r=2 -> 2, [9,8,7,3..6]; r=3 -> 3, [9,8,7,6,4,5]; r=4 -> 4,
    # [9,8,7,6,5]; r=0 -> 9, [5,8,7,6]; r=0 -> 5, [6,8,7]; r=0 -> 6
    assert s[0].tolist() == [0, 1, 2, 3, 4, 9, 5, 6]
    # it 1 on [0..9] again: r=9 -> 9 (the back, popped), then r=0 each time: 0, [8,1..7]; 8, [7,1..6]; 7; 6; 5; 4; 3
    assert s[1].tolist() == [9, 0, 8, 7, 6, 5, 4, 3]
    assert calls[:8] == [(0, 9), (0, 8), (0, 7), (0, 6), (0, 5), (0, 4), (0, 3), (0, 2)]
    rng = np.random.default_rng(5)
    vals = [int(v) for v in rng.integers(0, 1000, 4000)]
    a = draw_ransac_sets(57, 50, lambda lo, hi, it=iter(vals): lo + next(it) % (hi - lo + 1))
    b = npinit.draw_ransac_sets_ref(57, 50, lambda lo, hi, it=iter(vals): lo + next(it) % (hi - lo + 1))
    assert np.array_equal(a, b)
    assert all(len(set(r)) == 8 for r in a.tolist())


def test_nan_cosines_sort_after_every_number():
    """The order defined for a NaN cosine reaching std::sort: after every number."""
    nan = np.float32("nan")
    assert np.isnan(npinit.parallax_of([nan, 0.9, 0.99]))                 # nGood = 3: index 2 is the NaN
    c = np.concatenate([np.full(5, nan, np.float32), np.linspace(0.5, 0.99, 60).astype(np.float32)])
    np.random.default_rng(0).shuffle(c)
    ref = npinit.parallax_of(np.linspace(0.5, 0.99, 60).astype(np.float32))
    assert npinit.parallax_of(c) == ref                                    # index 50 of 65: a number, the NaNs are behind it
    assert npinit.parallax_of([]) == 0


def test_scores_invariant_under_model_sign():
    """H -> -H and F -> -F leave every score term and inlier bit exactly unchanged (the sign convention argument of section 2)."""
    k1, k2, m, K, sets = initcases.make_case(initcases.WITNESS["F success"])
    H21, H12, F21 = npinit.hypotheses(k1, k2, m, sets[:40])
    a = npinit.homography_terms(H21, H12, k1, k2, m); b = npinit.homography_terms(-H21, -H12, k1, k2, m)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    a = npinit.fundamental_terms(F21, k1, k2, m); b = npinit.fundamental_terms(-F21, k1, k2, m)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    assert np.array_equal(npinit.inv3(-H21), -npinit.inv3(H21))


def test_jacobi_stops_before_the_sweep_cap():
    """F's 8 x 9 systems keep one column at rounding-noise size; the null-column rule stops them like H's 16 x 9."""
    k1, k2, m, K, sets = initcases.make_case(initcases.WITNESS["F success"])
    pn1, _ = npinit.normalize(k1); pn2, _ = npinit.normalize(k2)
    i1, i2 = npinit.match_list(m)
    u1 = pn1[i1[sets], 0]; v1 = pn1[i1[sets], 1]; u2 = pn2[i2[sets], 0]; v2 = pn2[i2[sets], 1]
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], 2).astype(np.float64)
    _, _, sweeps = npinit.jacobi(A, return_sweeps=True)
    assert sweeps.max() <= 15, np.bincount(sweeps)
