"""GPU parity of the device-resident second stage of Tracking (csrc/orb_track.hip, include/orbslam_hip.h::orbt_track_local_map;
reference src/Tracking.cc:673-750 TrackLocalMap, :793-842 SearchLocalPoints) against the CPU oracle's COMPOSITION of the stages at
1241 x 376: Frame::isInFrustum + PredictScale (oracle is_in_frustum), ORBmatcher::SearchByProjection(Frame&, vpMapPoints, th)
(src/ORBmatcher.cc:42-119: the oracle's projection search with best / second best + level rule, the slots closed before the call
and the :83-84 claim rule), the last-writer slot ownership of :110 and PoseOptimization over every slot that holds a point, in
feature order.  In-view flags, matches, slot owners and outlier flags must be identical, the pose within 1e-7.  The frame is the
one orbt_track_with_motion_model left on the device."""
import numpy as np
import pytest

from ceres_mono_orb_slam2_amd import synth
from tests.test_gpu_track import _scenario, K4, BOUNDS, F32

pytestmark = pytest.mark.gpu


def _local_map(oracle, S, got, seed, extra=600, no_obs_frac=0.1):
    """Local map of the second stage: the last frame's points (the ones stage 1 matched are marked 'already in the frame'),
    duplicates of some of them under another index (look-alikes competing for the same features) and points with random descriptors."""
    rng = np.random.default_rng(1000 + seed)
    E = S["E"]
    n = len(S["X"])
    dup = rng.choice(n, size=min(n, 300), replace=False)
    Xr = np.stack([rng.uniform(-20, 20, extra), rng.uniform(-6, 6, extra), rng.uniform(8, 40, extra)], 1)
    X = np.concatenate([S["X"], S["X"][dup] * (1.0 + 2e-4 * rng.standard_normal((len(dup), 1))), Xr])
    D = np.concatenate([S["desc"], S["desc"][dup], rng.integers(0, 256, (extra, 32), dtype=np.uint8)])
    # a few bits flipped in the duplicates so that best / second best are close (the ratio test fires)
    flip = rng.integers(0, 256, (len(dup), 32), dtype=np.uint8) & rng.integers(0, 256, (len(dup), 32), dtype=np.uint8) & rng.integers(0, 256, (len(dup), 32), dtype=np.uint8) & rng.integers(0, 256, (len(dup), 32), dtype=np.uint8)
    D[n:n + len(dup)] ^= flip
    octave = np.concatenate([S["octave"], S["octave"][dup], rng.integers(0, 8, extra)]).astype(np.int32)
    m = len(X)
    # GetNormal(): mean viewing direction = from the (last) camera centre, the world origin, to the point, perturbed
    Pn = X / np.linalg.norm(X, axis=1, keepdims=True) + 0.25 * rng.standard_normal((m, 3))
    Pn[rng.random(m) < 0.05] *= -1.0                                           # seen from behind: fails the 0.5 cosine limit
    Pn /= np.linalg.norm(Pn, axis=1, keepdims=True)
    dist = np.linalg.norm(X, axis=1)
    maxd = (dist * E.scale[octave] * (1.0 + 0.05 * rng.standard_normal(m))).astype(np.float32)      # MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:338-377)
    mind = (maxd / E.scale[7]).astype(np.float32)
    maxd[rng.random(m) < 0.03] *= 0.3                                           # out of the scale-invariance range
    state = np.ones(m, np.uint8)
    state[rng.random(m) < no_obs_frac] = 3
    state[rng.random(m) < 0.04] = 0                                             # isBad()
    # stage 1: slots that hold a point (outliers were emptied, src/Tracking.cc:648-660); those points are not searched again (:816)
    nk = len(got["kps"])
    owner1 = got["owner"].copy(); owner1[got["outlier"]] = -1
    slot_state = np.zeros(nk, np.uint8); slot_X = np.zeros((nk, 3))
    has = owner1 >= 0
    slot_state[has] = S["valid"][owner1[has]]
    slot_X[has] = S["X"][owner1[has]]
    state[owner1[has]] = 0
    return dict(X=X, Pn=Pn, mind=mind, maxd=maxd, D=D, state=state, slot_state=slot_state, slot_X=slot_X)


def _expected(oracle, S, got, M, T, th, ratio=0.8):
    E = S["E"]
    kps = got["kps"]; desc = got["desc"]
    kps4 = np.stack([kps["x"], kps["y"], kps["octave"].astype(np.float32), kps["angle"]], 1).astype(np.float32)
    log_scale = F32(np.log(F32(1.2)))
    iv, uv, lv, vc = oracle.is_in_frustum(T[:3, :3], T[:3, 3], K4, BOUNDS, M["X"], M["Pn"], M["mind"], M["maxd"], 0.5, log_scale, 8)
    iv = iv.astype(bool) & (M["state"] != 0)
    r = np.where(vc > F32(0.998), F32(2.5), F32(4.0)).astype(np.float32)
    if th != 1.0: r = (r * F32(th)).astype(np.float32)
    rad = (r * E.scale[lv]).astype(np.float32)
    qv = np.where(iv, M["state"], 0).astype(np.uint8)
    taken = (M["slot_state"] == 1).astype(np.uint8)
    nm, m, _, _ = oracle.search_by_projection(kps4, desc, BOUNDS, uv, rad, M["D"], q_min_level=lv - 1, q_max_level=lv, q_valid=qv, taken=taken, mode_best2=True,
                                              ratio=ratio, th=100, check_ori=False)
    owner = np.full(len(kps4), -1, np.int32)
    for q in range(len(m)):
        if m[q] >= 0: owner[m[q]] = q
    hasp = (owner >= 0) | (M["slot_state"] != 0)
    feat = np.nonzero(hasp)[0]
    Xo = np.where((owner[feat] >= 0)[:, None], M["X"][np.maximum(owner[feat], 0)], M["slot_X"][feat])
    pose0 = oracle.matrix4d_to_pose7(T)
    outl = np.zeros(len(kps4), bool)
    if len(feat) >= 3:
        ninl, pose, out, _ = oracle.pose_optimization(K4.astype(np.float64), pose0, Xo, kps4[feat, :2].astype(np.float64), E.inv_sigma2[kps4[feat, 2].astype(int)])
        outl[feat] = out.astype(bool)
    else:
        ninl, pose = 0, pose0
    return dict(in_view=iv, match=m, nmatches=nm, owner=owner, outlier=outl, pose7=pose, n_inliers=int(ninl), ncorr=len(feat))


@pytest.mark.parametrize("seed,th,kw", [(3, 1.0, {}), (4, 5.0, {}), (5, 1.0, dict(no_obs_frac=0.5)), (6, 3.0, dict(extra=4000)), (7, 1.0, dict(no_obs_frac=0.0))])
def test_track_local_map_vs_oracle_composition(oracle, seed, th, kw):
    from ceres_mono_orb_slam2_amd import ORBextractor, tracking
    S = _scenario(oracle, seed)
    ex = ORBextractor(2000, 1.2, 8, 20, 7)
    got1 = tracking.track_with_motion_model(ex, S["img"], K4, BOUNDS, S["T"], S["X"], S["desc"], S["octave"], S["angle"], S["valid"], 15.0, True)
    T = oracle.pose7_to_matrix4d(got1["pose7"])
    M = _local_map(oracle, S, got1, seed, **kw)
    want = _expected(oracle, S, got1, M, T, th)
    got = tracking.track_local_map(ex, K4, BOUNDS, T, F32(np.log(F32(1.2))), M["X"], M["Pn"], M["mind"], M["maxd"], M["D"], M["state"], M["slot_X"], M["slot_state"], th, 0.8)
    assert want["in_view"].sum() > 300 and want["nmatches"] > 100, (want["in_view"].sum(), want["nmatches"])
    assert np.array_equal(got["in_view"] & (M["state"] != 0), want["in_view"])
    assert np.array_equal(got["match"], want["match"])
    assert got["nmatches"] == want["nmatches"]
    assert np.array_equal(got["owner"], want["owner"])
    assert got["n_correspondences"] == want["ncorr"]
    assert np.array_equal(got["outlier"], want["outlier"])
    assert got["n_inliers"] == want["n_inliers"]
    assert np.allclose(got["pose7"], want["pose7"], rtol=0, atol=1e-7)
    print("TrackLocalMap: %d points, %d in view, %d matched in %d rounds, %d correspondences, %d inliers" % (len(M["X"]), want["in_view"].sum(), got["nmatches"], got["greedy_rounds"], got["n_correspondences"], got["n_inliers"]))


def test_track_local_map_needs_the_resident_frame_and_handles_empty_maps(oracle):
    from ceres_mono_orb_slam2_amd import ORBextractor, tracking, _lib
    import threading
    S = _scenario(oracle, 12)
    ex = ORBextractor(2000, 1.2, 8, 20, 7)
    got1 = tracking.track_with_motion_model(ex, S["img"], K4, BOUNDS, S["T"], S["X"], S["desc"], S["octave"], S["angle"], S["valid"], 15.0, True)
    T = oracle.pose7_to_matrix4d(got1["pose7"])
    nk = len(got1["kps"])
    z = lambda shape, dt=np.float64: np.zeros(shape, dt)
    # no local map points: PoseOptimization over the slots that already hold a point = stage 1's inliers
    M = _local_map(oracle, S, got1, 12)
    r = tracking.track_local_map(ex, K4, BOUNDS, T, F32(np.log(F32(1.2))), z((0, 3)), z((0, 3)), z(0, np.float32), z(0, np.float32), z((0, 32), np.uint8), z(0, np.uint8),
                                 M["slot_X"], M["slot_state"])
    assert r["nmatches"] == 0 and r["n_correspondences"] == int((M["slot_state"] != 0).sum()) and (r["owner"] == -1).all()
    # wrong keypoint count / another host thread (no resident frame there): loud errors
    with pytest.raises(_lib.OrbHipError, match="n_kp"):
        tracking.track_local_map(ex, K4, BOUNDS, T, 0.18, z((0, 3)), z((0, 3)), z(0, np.float32), z(0, np.float32), z((0, 32), np.uint8), z(0, np.uint8), M["slot_X"][:-1], M["slot_state"][:-1])
    err = []
    def other():
        try:
            tracking.track_local_map(ex, K4, BOUNDS, T, 0.18, z((0, 3)), z((0, 3)), z(0, np.float32), z(0, np.float32), z((0, 32), np.uint8), z(0, np.uint8), M["slot_X"], M["slot_state"])
        except _lib.OrbHipError as e:
            err.append(str(e))
    t = threading.Thread(target=other); t.start(); t.join()
    assert err and "no frame resident" in err[0]


def test_track_local_map_4000_features_pose_solve_streams_its_observations(oracle):
    """A 4000-feature frame (the initialisation extractor's size) with ~90 % of its keypoints bound to map points: more than 2048
    correspondences, so the pose solve behind the device-resident call takes k_pose_lm's streaming path (csrc/ba_small_lm.inc: the
    observations stay in registers only up to 2048).  Empty local map, caller-supplied slots: each keypoint back-projected at a depth
    of 4 - 60 m under a true pose from a pixel 1 px x scale off, 3 % wrong associations, the predicted pose perturbed as _scenario's.
    Expected: the oracle's PoseOptimization over the slots in feature order, as _expected composes it."""
    from ceres_mono_orb_slam2_amd import ORBextractor, tracking
    rng = np.random.default_rng(20)
    img = synth.make_frame(20, 1241, 376, "checker")
    ex = ORBextractor(4000, 1.2, 8, 20, 7)
    E = oracle.OracleExtractor(4000)
    pose_true = np.concatenate([0.3 * rng.standard_normal(3), synth.quat_from_rotvec(0.05 * rng.standard_normal(3))])
    pose_pred = np.concatenate([pose_true[:3] + 0.02 * rng.standard_normal(3), synth.quat_mul(synth.quat_from_rotvec(2e-3 * rng.standard_normal(3)), pose_true[3:])])
    T = oracle.pose7_to_matrix4d(pose_pred)
    z = np.zeros
    got1 = tracking.track_with_motion_model(ex, img, K4, BOUNDS, T, z((0, 3)), z((0, 32), np.uint8), z(0, np.int32), z(0, np.float32), z(0, np.uint8))
    kps = got1["kps"]
    nk = len(kps)
    assert np.array_equal(kps, E.extract(img)[0]) and nk > 3000
    octave = kps["octave"].astype(int)
    px = np.stack([kps["x"], kps["y"]], 1).astype(np.float64) + rng.standard_normal((nk, 2)) * E.scale[octave][:, None]
    depth = rng.uniform(4, 60, nk)
    pc = np.stack([(px[:, 0] - K4[2]) / K4[0] * depth, (px[:, 1] - K4[3]) / K4[1] * depth, depth], 1)
    slot_X = (pc - pose_true[:3]) @ synth.quat_to_R(pose_true[3:])              # X = R^T (pc - t)
    slot_X[rng.random(nk) < 0.03] *= 1.4                                       # wrong associations -> outliers
    slot_state = np.ones(nk, np.uint8)
    slot_state[rng.random(nk) < 0.1] = 3
    slot_state[rng.random(nk) < 0.1] = 0
    got = tracking.track_local_map(ex, K4, BOUNDS, T, F32(np.log(F32(1.2))), z((0, 3)), z((0, 3)), z(0, np.float32), z(0, np.float32), z((0, 32), np.uint8), z(0, np.uint8),
                                   slot_X, slot_state)
    feat = np.nonzero(slot_state != 0)[0]
    uv = np.stack([kps["x"], kps["y"]], 1).astype(np.float32)
    ninl, pose, out, s = oracle.pose_optimization(K4.astype(np.float64), oracle.matrix4d_to_pose7(T), slot_X[feat], uv[feat].astype(np.float64), E.inv_sigma2[octave[feat]])
    outl = np.zeros(nk, bool); outl[feat] = out.astype(bool)
    print("TrackLocalMap, 4000 features: %d keypoints, %d correspondences, %d inliers, oracle %s" % (nk, got["n_correspondences"], got["n_inliers"], s))
    assert got["n_correspondences"] == len(feat) and got["n_correspondences"] > 2048
    assert got["nmatches"] == 0 and (got["owner"] == -1).all()
    assert np.array_equal(got["outlier"], outl)
    assert got["n_inliers"] == int(ninl) and 0.8 * len(feat) < ninl < len(feat)
    assert np.allclose(got["pose7"], pose, rtol=0, atol=1e-7)
    assert s["successful_steps"] >= 2 and np.abs(pose[:3] - pose_true[:3]).max() < 0.02
