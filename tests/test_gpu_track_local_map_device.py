"""UpdateLocalMap feeding TrackLocalMap on the device: orbt_update_local_map_device -> orbt_track_local_map_device at 1241 x 376 against
orbt_track_local_map on the arrays the restatement tests/nplocalmap.py gathers on the host.  The device path runs the same kernels on
the same bytes, so in-view flags, matches, owners, outliers and counts are identical and pose7 is BIT-identical.  n_mp = the count and
n_mp = the capacity give the same answer up to the padding rows, which are all "not in view, -1"."""
import numpy as np
import pytest

from tests import localmapcases as lc
from tests import nplocalmap as nlm
from tests.test_gpu_track import _scenario, K4, BOUNDS, F32
from tests.test_gpu_track_local_map import _local_map

pytestmark = pytest.mark.gpu


def _tables(S, got1, M, seed, nkf=5):
    """The local map M as map tables: nkf keyframes whose slot tables cover M's points with overlaps (point p sits in keyframe p % nkf
    and, one time in four, in a second one), a small graph, the frame's slots as the first stage left them."""
    rng = np.random.default_rng(2000 + seed)
    npts = len(M["X"])
    owner1 = got1["owner"].copy(); owner1[got1["outlier"]] = -1
    held = np.zeros(npts, bool); held[owner1[owner1 >= 0]] = True
    slots = [[] for _ in range(nkf)]
    for p in rng.permutation(npts):
        ks = {int(p) % nkf} | ({int(rng.integers(nkf))} if rng.random() < 0.25 else set())
        for k in ks:
            if rng.random() < 0.1:
                slots[k].append(-1)
            slots[k].append(int(p))
    obs = [[] for _ in range(npts)]
    for k in range(nkf):
        for p in slots[k]:
            if p >= 0 and k not in obs[p]:
                obs[p].append(k)
    seen = sorted(set(int(p) for p in got1["owner"][got1["outlier"] & (got1["owner"] >= 0)]) - set(int(p) for p in owner1[owner1 >= 0]))
    pr = lc.build(nkf, slots, [int(p) for p in owner1], obs=obs, npts=npts, cov={k: [(k + 1) % nkf, (k + 2) % nkf] for k in range(nkf)},
                  children={k: [k + 1] for k in range(nkf - 1)}, parent={k: k - 1 for k in range(1, nkf)}, pt_bad=np.nonzero((M["state"] == 0) & ~held)[0],
                  rank=[int(r) for r in rng.permutation(nkf)], seen=seen, nobs0=np.nonzero(M["state"] == 3)[0])
    pr.update(pt_Xw=np.ascontiguousarray(M["X"], np.float64), pt_normal=np.ascontiguousarray(M["Pn"], np.float64), pt_min_dist=M["mind"].astype(np.float32),
              pt_max_dist=M["maxd"].astype(np.float32), pt_desc=np.ascontiguousarray(M["D"], np.uint8))
    return pr


@pytest.mark.parametrize("seed,th,kw", [(3, 1.0, {}), (6, 3.0, dict(extra=4000))])
def test_update_local_map_device_feeds_track_local_map_device(oracle, seed, th, kw):
    import torch
    from ceres_mono_orb_slam2_amd import ORBextractor, tracking
    S = _scenario(oracle, seed)
    ex = ORBextractor(2000, 1.2, 8, 20, 7)
    got1 = tracking.track_with_motion_model(ex, S["img"], K4, BOUNDS, S["T"], S["X"], S["desc"], S["octave"], S["angle"], S["valid"], 15.0, True)
    Tcw = oracle.pose7_to_matrix4d(got1["pose7"])
    M = _local_map(oracle, S, got1, seed, **kw)
    pr = _tables(S, got1, M, seed)
    cap_pt = len(M["X"]) + 37
    assert cap_pt <= 16384
    exp = nlm.update_local_map(pr, cap_pt=cap_pt)
    n = exp["n_local_pt"]
    assert exp["n_local_kf"] == 5 and n > 1000 and (exp["mp_state"] == 1).sum() > 500 and (exp["mp_state"] == 3).sum() > 20 and (exp["slot_state"] != 0).sum() > 100
    log_scale = F32(np.log(F32(1.2)))
    want = tracking.track_local_map(ex, K4, BOUNDS, Tcw, log_scale, exp["mp_Xw"], exp["mp_normal"], exp["mp_min_dist"], exp["mp_max_dist"], exp["mp_desc"], exp["mp_state"][:n],
                                    exp["slot_Xw"], exp["slot_state"], th, 0.8)
    assert want["n_in_view"] > 300 and want["nmatches"] > 100, (want["n_in_view"], want["nmatches"])
    T = {k: (None if v is None else torch.as_tensor(np.array(v)).cuda()) for k, v in pr.items()}
    d = tracking.update_local_map_device(T, 8, cap_pt)
    for n_mp in (n, cap_pt):
        got = tracking.track_local_map_device(ex, K4, BOUNDS, Tcw, log_scale, d, n_mp, th, 0.8)
        for k in ("in_view", "match"):
            assert np.array_equal(got[k][:n], want[k]), (n_mp, k)
        assert not got["in_view"][n:].any() and (got["match"][n:] == -1).all()
        for k in ("owner", "outlier"):
            assert np.array_equal(got[k], want[k]), (n_mp, k)
        for k in ("nmatches", "n_inliers", "n_correspondences", "n_in_view", "greedy_rounds"):
            assert got[k] == want[k], (n_mp, k)
        assert got["pose7"].tobytes() == want["pose7"].tobytes(), n_mp
    c = d["counts"].cpu().numpy()
    assert list(c) == [5, exp["ref_kf"], n, 0] and int(d["status"].item()) == 0
    assert np.array_equal(d["local_pt"].cpu().numpy()[:n], exp["local_pt"]) and np.array_equal(d["mp_state"].cpu().numpy(), exp["mp_state"])
    print("UpdateLocalMap -> TrackLocalMap on the device: %d local points of %d, %d in view, %d matched, %d inliers" % (n, len(M["X"]), got["n_in_view"], got["nmatches"], got["n_inliers"]))
