"""orbl_update_map_points(_device) on the MI355X against the numpy restatement tests/npmappoint.py (src/MapPoint.cc:256-315,
:335-378): best_obs, the descriptor bytes, the normal and min / max bit-identical; untouched outputs stay poisoned."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import npmappoint as npm  # noqa: E402

pytestmark = pytest.mark.gpu

BOTH = npm.DESC | npm.NORMAL_DEPTH


def _run(b, what, poison=True):
    from ceres_mono_orb_slam2_amd import localmapping
    npts = len(b["obs_off"]) - 1
    out = npm.fresh_outputs(npts, poison=poison)
    exp = npm.update_map_points(b, what, {k: v.copy() for k, v in out.items()})
    got = localmapping.update_map_points(b["obs_off"], b["obs_desc"], b["obs_kf_good"], b["X"], b["ref_kf"], b["ref_level"], b["obs_kf"],
                                         b["kf_center"], b["scale_factors"], b["pt_good"], what, out)
    return got, exp


def _same(got, exp):
    for k in ("best_obs", "desc", "nd_written"):
        assert np.array_equal(got[k], exp[k]), k
    for k in ("normal", "min_max"):                                 # bit-identical, NaN-free
        assert np.array_equal(got[k].view(np.uint8), exp[k].view(np.uint8)), k


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 16, 17, 63, 64, 65, 127, 128, 129, 500, 1024])
def test_single_point(n):
    for seed, kw in ((n, {}), (1000 + n, dict(flip=(0, 3), bad_kf_frac=0.3))):
        b = npm.make_batch(seed, [n], nkf=max(8, n // 4), **kw)
        got, exp = _run(b, BOTH)
        _same(got, exp)


def test_single_point_long_list_mostly_bad_keyframes():
    """a list of 200 entries of which few are good: the point lands in a small-N bucket but stages from a long list"""
    for good in (2, 5, 9, 40, 70):
        b = npm.make_batch(7 + good, [200], nkf=60)
        g = np.zeros(200, np.uint8); g[np.random.default_rng(good).choice(200, good, replace=False)] = 1
        b["obs_kf_good"] = g
        got, exp = _run(b, BOTH)
        _same(got, exp)


def test_skewed_batch_2000():
    ns = npm.skewed_ns(3, 2000)
    b = npm.make_batch(3, ns, nkf=80, bad_kf_frac=0.1, bad_pt_frac=0.02)
    for what in (BOTH, npm.DESC, npm.NORMAL_DEPTH):
        got, exp = _run(b, what)
        _same(got, exp)


def test_c4_normal_depth_10000():
    b = npm.c4_normal_depth_batch(0)
    got, exp = _run(b, npm.NORMAL_DEPTH)
    _same(got, exp)
    assert got["nd_written"].sum() == (b["pt_good"] != 0).sum()
    assert (got["best_obs"] == -7).all() and (got["desc"] == 0xA5).all()       # the descriptor part was not selected


def test_unchanged_points_keep_poisoned_outputs():
    ns = [0, 3, 0, 70, 5, 1, 2]
    b = npm.make_batch(21, ns, nkf=30)
    b["pt_good"][:] = 1; b["pt_good"][4] = 0
    b["obs_kf_good"][b["obs_off"][1]:b["obs_off"][2]] = 0                        # point 1: every keyframe bad
    got, exp = _run(b, BOTH)
    _same(got, exp)
    for p in (0, 1, 2, 4):
        assert got["best_obs"][p] == -1 and (got["desc"][p] == 0xA5).all()
    for p in (0, 2, 4):
        assert got["nd_written"][p] == 0 and (got["normal"][p] == -12345.5).all() and (got["min_max"][p] == np.float32(-77.25)).all()
    assert got["nd_written"][1] == 1                                # bad keyframes still count for the normal


def test_adversarial_descriptors():
    rng = np.random.default_rng(9)
    ns = rng.integers(2, 140, 300)
    for kw in (dict(equal_frac=0.5), dict(dup_frac=0.4), dict(flip=(1, 2)), dict(flip=(120, 136))):
        b = npm.make_batch(int(rng.integers(1 << 30)), ns, nkf=50, **kw)
        got, exp = _run(b, BOTH)
        _same(got, exp)
    # many equal medians: every descriptor 2 bits from every other (disjoint bit pairs)
    for n in (4, 12, 40, 64, 100):
        d = np.zeros((n, 256), np.uint8)
        for i in range(n):
            d[i, 2 * i] = d[i, 2 * i + 1] = 1
        b = npm.make_batch(n, [n], nkf=10)
        b["obs_desc"] = np.packbits(d, axis=1)
        got, exp = _run(b, BOTH)
        _same(got, exp)
        assert got["best_obs"][0] == 0


def test_host_entry_equals_device_entry():
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    ns = np.concatenate([npm.skewed_ns(5, 1500), [100, 700, 1024]])
    b = npm.make_batch(5, ns, nkf=60, bad_pt_frac=0.02)
    host, _ = _run(b, BOTH)
    dev = torch.device("cuda:0")
    T = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)     # noqa: E731
    poison = npm.fresh_outputs(len(ns), poison=True)
    out = {k: torch.from_numpy(v.copy()).to(dev) for k, v in poison.items()}
    localmapping.update_map_points_device(T(b["obs_off"], np.int32), T(b["obs_desc"], np.uint8), T(b["obs_kf_good"], np.uint8), T(b["X"], np.float64),
                                          T(b["ref_kf"], np.int32), T(b["ref_level"], np.int32), T(b["obs_kf"], np.int32), T(b["kf_center"], np.float64),
                                          T(b["scale_factors"], np.float32), T(b["pt_good"], np.uint8), BOTH, out)
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in poison}
    assert np.array_equal(got["best_obs"], host["best_obs"]) and np.array_equal(got["nd_written"], host["nd_written"])
    w = got["best_obs"] >= 0
    assert np.array_equal(got["desc"][w], host["desc"][w]) and (got["desc"][~w] == 0xA5).all()
    nd = got["nd_written"] == 1
    assert np.array_equal(got["normal"][nd].view(np.uint8), host["normal"][nd].view(np.uint8))
    assert np.array_equal(got["min_max"][nd].view(np.uint8), host["min_max"][nd].view(np.uint8))
    assert (got["normal"][~nd] == -12345.5).all()


def test_repeated_calls_are_deterministic():
    b = npm.make_batch(77, npm.skewed_ns(77, 800), nkf=40)
    a, _ = _run(b, BOTH)
    c, _ = _run(b, BOTH)
    _same(a, c)
