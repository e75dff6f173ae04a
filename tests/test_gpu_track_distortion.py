"""GPU parity of the device-resident Tracking calls under LENS DISTORTION (orbt_set_distortion / orbt_image_bounds /
orbt_last_undistorted_keypoints, csrc/orb_track.hip k_trk_prepare<true>; reference Frame::Frame src/Frame.cc:115-155: UndistortKeyPoints
:329-355 between the extractor and AssignFeaturesToGrid, ComputeImageBounds :357-385) against the CPU oracle's COMPOSITION of the same
stages, as tests/test_gpu_track.py, test_gpu_track_local_map.py and test_gpu_track_reference_keyframe.py compose them, with
oracle.undistort_keypoints inserted behind the oracle's extraction: the frame's records take the undistorted x, y, the bounds come from
the undistorted corners, the scenario's map points are back-projected from the UNDISTORTED last-frame keypoints.  Raw keypoints,
descriptors, matches, owners, outlier flags and counts identical, kps_undistorted bit-equal, pose within 1e-7.  Cameras: the reference's
TUM1 and EuRoC configurations and the KITTI intrinsics with k1 = +0.3, under which keypoints leave the 64 x 48 grid (PosInGrid false:
in no cell, still in their slot)."""
import functools

import numpy as np
import pytest

from ceres_mono_orb_slam2_amd import synth
from tests.trackdist_cases import CAMERAS, oracle_bounds, outside_grid

pytestmark = pytest.mark.gpu
F32 = np.float32
KEYS = ("node_desc", "child_off", "children", "word_id", "weight", "L")
SEED = {"TUM1": 3, "EuRoC": 4, "KITTI_k1": 5}


def _kps4(oracle, cam, kps):
    """undistort_keypoints_ as {x, y, octave, angle} records"""
    und = oracle.undistort_keypoints(np.stack([kps["x"], kps["y"]], 1).astype(F32), cam["K4"], cam["dist"])
    return np.stack([und[:, 0], und[:, 1], kps["octave"].astype(F32), kps["angle"]], 1).astype(F32)


@functools.lru_cache(maxsize=None)
def _scenario(oracle, name, seed, nfeat=2000, family="blocks", no_obs_frac=0.1, drop_frac=0.1, depth=18.0, pose_noise=2e-3):
    """tests/test_gpu_track.py's scenario for camera `name`: two crops of one canvas; the last frame's camera is the world frame, its
    map points lie at one depth on the rays of its UNDISTORTED keypoints."""
    cam = CAMERAS[name]
    K4 = cam["K4"]
    rng = np.random.default_rng(seed)
    seq, offs = synth.make_sequence(seed, cam["w"], cam["h"], 2, family, max_shift=6)
    E = oracle.OracleExtractor(nfeat)
    k_last, d_last = E.extract(seq[0])
    n = len(k_last)
    u_last = _kps4(oracle, cam, k_last)
    shift = (offs[1] - offs[0]).astype(np.float64)
    z = depth * (1.0 + 0.002 * rng.standard_normal(n))
    X = np.stack([(u_last[:, 0] - K4[2]) / K4[0] * z, (u_last[:, 1] - K4[3]) / K4[1] * z, z], 1).astype(np.float64)
    t_true = np.array([-shift[0] * depth / K4[0], -shift[1] * depth / K4[1], 0.0])
    q = synth.quat_from_rotvec(pose_noise * rng.standard_normal(3))
    T = oracle.pose7_to_matrix4d(np.concatenate([t_true + 0.02 * rng.standard_normal(3), q]))
    valid = np.ones(n, np.uint8)
    valid[rng.random(n) < no_obs_frac] = 3
    valid[rng.random(n) < drop_frac] = 0
    X[rng.random(n) < 0.03] *= 1.4                                              # wrong associations -> outliers of the pose optimisation
    kps, desc = E.extract(seq[1])
    bounds = oracle_bounds(oracle, cam)
    kps4 = _kps4(oracle, cam, kps)
    return dict(cam=cam, K4=K4, dist=cam["dist"], bounds=bounds, img=seq[1], E=E, X=X, desc=d_last, octave=k_last["octave"].astype(np.int32),
                angle=k_last["angle"].astype(F32), valid=valid, T=T, kps=kps, fdesc=desc, kps4=kps4, outside=outside_grid(oracle, kps4, bounds), nfeat=nfeat)


def _project(S, th):
    """The loop head of src/ORBmatcher.cc:1185-1212: double camera coordinates, float u / v, bounds, radius."""
    T, X, valid, octave, scale, B = S["T"], S["X"], S["valid"], S["octave"], S["E"].scale, S["bounds"]
    n = len(X)
    uv = np.zeros((n, 2), F32); rad = np.zeros(n, F32); v = valid.copy()
    R = [[float(T[r, c]) for c in range(3)] for r in range(3)]; t = [float(T[r, 3]) for r in range(3)]
    fx, fy, cx, cy = [F32(k) for k in S["K4"]]
    for i in range(n):
        if not v[i]:
            continue
        P = [float(x) for x in X[i]]
        c = [(R[r][0] * P[0] + R[r][1] * P[1] + R[r][2] * P[2]) + t[r] for r in range(3)]
        xc, yc = F32(c[0]), F32(c[1])
        with np.errstate(divide="ignore"):
            invz = F32(np.float64(1.0) / np.float64(c[2]))
        if invz < 0:
            v[i] = 0; continue
        u = F32(F32(fx * xc) * invz) + cx
        w = F32(F32(fy * yc) * invz) + cy
        if u < B[0] or u > B[1] or w < B[2] or w > B[3]:
            v[i] = 0; continue
        uv[i] = (u, w); rad[i] = F32(th) * scale[octave[i]]
    return uv, rad, v


def _pose(oracle, S, feat, Xw):
    """PoseOptimization over the features `feat` (feature order) with the undistorted observations"""
    kps4, E = S["kps4"], S["E"]
    pose0 = oracle.matrix4d_to_pose7(S["T"])
    outl = np.zeros(len(kps4), bool)
    if len(feat) < 3:
        return 0, pose0, outl
    ninl, pose, out, _ = oracle.pose_optimization(S["K4"].astype(np.float64), pose0, Xw, kps4[feat, :2].astype(np.float64), E.inv_sigma2[kps4[feat, 2].astype(int)])
    outl[feat] = out.astype(bool)
    return int(ninl), pose, outl


@functools.lru_cache(maxsize=None)
def _expected_mm(oracle, name, seed, th, nfeat=2000, family="blocks"):
    S = _scenario(oracle, name, seed, nfeat, family)
    kps4 = S["kps4"]
    uv, rad, v = _project(S, th)
    nm, m, _, _ = oracle.search_by_projection(kps4, S["fdesc"], S["bounds"], uv, rad, S["desc"], q_min_level=S["octave"] - 1, q_max_level=S["octave"] + 1, q_valid=v,
                                              taken=np.zeros(len(kps4), np.uint8), q_angle=S["angle"], ratio=0.9, th=100, check_ori=True)
    owner = np.full(len(kps4), -1, np.int32)
    for q in range(len(m)):                                                     # assignments in query order (:1232) ...
        if m[q] >= 0: owner[m[q]] = q
        elif m[q] <= -2: owner[-2 - m[q]] = q
    for q in range(len(m)):                                                     # ... then the removed rotation bins empty their slots (:1260-1264)
        if m[q] <= -2: owner[-2 - m[q]] = -1
    feat = np.nonzero(owner >= 0)[0]
    ninl, pose, outl = _pose(oracle, S, feat, S["X"][owner[feat]])
    return dict(match=m, nmatches=nm, owner=owner, outlier=outl, pose7=pose, n_inliers=ninl, ncorr=len(feat))


def _extractor(S):
    from ceres_mono_orb_slam2_amd import ORBextractor, tracking
    ex = ORBextractor(S["nfeat"], 1.2, 8, 20, 7)
    tracking.set_distortion(ex, S["dist"])
    return ex


def _mm(ex, S, th):
    from ceres_mono_orb_slam2_amd import tracking
    assert np.array_equal(tracking.image_bounds(S["cam"]["w"], S["cam"]["h"], S["K4"], S["dist"]).view(np.uint32), S["bounds"].view(np.uint32))
    return tracking.track_with_motion_model(ex, S["img"], S["K4"], S["bounds"], S["T"], S["X"], S["desc"], S["octave"], S["angle"], S["valid"], th, True)


def _check_frame(got, S):
    assert np.array_equal(got["kps"], S["kps"]) and np.array_equal(got["desc"], S["fdesc"])                  # kps stay the RAW keypoints
    assert got["kps_undistorted"].dtype == np.float32 and got["kps_undistorted"].shape == (len(S["kps"]), 2)
    assert np.array_equal(got["kps_undistorted"].view(np.uint32), S["kps4"][:, :2].copy().view(np.uint32))


def _check_mm(got, exp, S):
    _check_frame(got, S)
    assert got["nmatches"] == exp["nmatches"] and np.array_equal(got["match"], exp["match"])
    assert np.array_equal(got["owner"], exp["owner"]) and got["n_correspondences"] == exp["ncorr"]
    assert got["n_inliers"] == exp["n_inliers"] and np.array_equal(got["outlier"], exp["outlier"])
    assert np.abs(got["pose7"] - exp["pose7"]).max() < 1e-7


@pytest.mark.parametrize("name", ["TUM1", "EuRoC", "KITTI_k1"])
def test_motion_model_with_distortion_vs_oracle_composition(oracle, name):
    """th = 15, then the reference's retry with 2 * th on the same frame (src/Tracking.cc:635-641)."""
    S = _scenario(oracle, name, SEED[name])
    moved = np.abs(S["kps4"][:, :2] - np.stack([S["kps"]["x"], S["kps"]["y"]], 1)).max()
    print("%s: %d keypoints, %d outside the grid, bounds %s, largest undistortion shift %.2f px" % (name, len(S["kps"]), S["outside"].sum(), S["bounds"].tolist(), moved))
    assert moved > 2.0
    if name == "KITTI_k1":
        assert S["outside"].sum() >= 1                                          # the 0xFFFF branch of k_trk_prepare is exercised
    if name == "EuRoC":
        assert S["bounds"][0] < -100 and S["bounds"][1] > S["cam"]["w"] + 100   # bounds well outside the image
    ex = _extractor(S)
    for th in (15.0, 30.0):
        exp = _expected_mm(oracle, name, SEED[name], th)
        got = _mm(ex, S, th)
        _check_mm(got, exp, S)
        print("  th %.0f: %d matches (%d removed by rotation), %d inliers, %d greedy rounds" % (th, got["nmatches"], int((got["match"] <= -2).sum()), got["n_inliers"], got["greedy_rounds"]))
        assert exp["nmatches"] > 200 and exp["n_inliers"] > 150


def _expected_lm(oracle, S, kps4, desc, M, T, th, ratio=0.8):
    """tests/test_gpu_track_local_map.py::_expected with the camera's intrinsics and bounds and the undistorted records"""
    E = S["E"]
    log_scale = F32(np.log(F32(1.2)))
    iv, uv, lv, vc = oracle.is_in_frustum(T[:3, :3], T[:3, 3], S["K4"], S["bounds"], M["X"], M["Pn"], M["mind"], M["maxd"], 0.5, log_scale, 8)
    iv = iv.astype(bool) & (M["state"] != 0)
    r = np.where(vc > F32(0.998), F32(2.5), F32(4.0)).astype(F32)
    if th != 1.0: r = (r * F32(th)).astype(F32)
    rad = (r * E.scale[lv]).astype(F32)
    qv = np.where(iv, M["state"], 0).astype(np.uint8)
    taken = (M["slot_state"] == 1).astype(np.uint8)
    nm, m, _, _ = oracle.search_by_projection(kps4, desc, S["bounds"], uv, rad, M["D"], q_min_level=lv - 1, q_max_level=lv, q_valid=qv, taken=taken, mode_best2=True,
                                              ratio=ratio, th=100, check_ori=False)
    owner = np.full(len(kps4), -1, np.int32)
    for q in range(len(m)):
        if m[q] >= 0: owner[m[q]] = q
    feat = np.nonzero((owner >= 0) | (M["slot_state"] != 0))[0]
    Xo = np.where((owner[feat] >= 0)[:, None], M["X"][np.maximum(owner[feat], 0)], M["slot_X"][feat])
    pose0 = oracle.matrix4d_to_pose7(T)
    outl = np.zeros(len(kps4), bool)
    if len(feat) >= 3:
        ninl, pose, out, _ = oracle.pose_optimization(S["K4"].astype(np.float64), pose0, Xo, kps4[feat, :2].astype(np.float64), E.inv_sigma2[kps4[feat, 2].astype(int)])
        outl[feat] = out.astype(bool)
    else:
        ninl, pose = 0, pose0
    return dict(in_view=iv, match=m, nmatches=nm, owner=owner, outlier=outl, pose7=pose, n_inliers=int(ninl), ncorr=len(feat))


@pytest.mark.parametrize("name,th", [("TUM1", 1.0), ("EuRoC", 5.0), ("KITTI_k1", 1.0)])
def test_local_map_on_the_distorted_resident_frame(oracle, name, th):
    """The second stage sees the undistorted grid and records of the frame the first stage left on the device."""
    from ceres_mono_orb_slam2_amd import tracking
    from tests.test_gpu_track_local_map import _local_map
    S = _scenario(oracle, name, SEED[name])
    ex = _extractor(S)
    got1 = _mm(ex, S, 15.0)
    _check_mm(got1, _expected_mm(oracle, name, SEED[name], 15.0), S)
    T = oracle.pose7_to_matrix4d(got1["pose7"])
    M = _local_map(oracle, S, got1, SEED[name])
    want = _expected_lm(oracle, S, S["kps4"], S["fdesc"], M, T, th)
    got = tracking.track_local_map(ex, S["K4"], S["bounds"], T, F32(np.log(F32(1.2))), M["X"], M["Pn"], M["mind"], M["maxd"], M["D"], M["state"], M["slot_X"], M["slot_state"], th, 0.8)
    print("TrackLocalMap %s: %d points, %d in view, %d matched, %d correspondences, %d inliers" % (name, len(M["X"]), want["in_view"].sum(), want["nmatches"], want["ncorr"], want["n_inliers"]))
    assert want["in_view"].sum() > 300 and want["nmatches"] > 100
    assert np.array_equal(got["in_view"] & (M["state"] != 0), want["in_view"])
    assert np.array_equal(got["match"], want["match"]) and got["nmatches"] == want["nmatches"]
    assert np.array_equal(got["owner"], want["owner"]) and got["n_correspondences"] == want["ncorr"]
    assert np.array_equal(got["outlier"], want["outlier"]) and got["n_inliers"] == want["n_inliers"]
    assert np.allclose(got["pose7"], want["pose7"], rtol=0, atol=1e-7)


def _bow_expected(oracle, voc, S, kf_desc, kf_valid, kf_angle, ratio, fv):
    """SearchByBoW(keyframe, frame) + slot owners; the frame's angles are the keypoints' (undistortion leaves them alone)"""
    _, _, kfn, kfo, kfi = oracle.bow_transform(voc, kf_desc, 4) if len(kf_desc) else (None, None, np.zeros(0, np.uint32), np.zeros(1, np.uint32), np.zeros(0, np.uint32))
    if len(kf_desc):
        nm, m = oracle.search_by_bow(kf_desc, kf_valid, kf_angle, S["fdesc"], None, S["kps"]["angle"].astype(F32), (kfn, kfo, kfi), fv, ratio=ratio, th=50, strict=False, check_ori=True)
    else:
        nm, m = 0, np.zeros(0, np.int32)
    owner = np.full(len(S["kps"]), -1, np.int32)
    for q in range(len(m)):
        if m[q] >= 0: owner[m[q]] = q
    return nm, m, owner, (kfn, kfo, kfi)


def test_reference_keyframe_and_relocalization_with_keypoints_outside_the_grid(oracle):
    """The k1 = +0.3 camera: a keypoint outside the grid receives a BoW match (SearchByBoW does not look at the grid) and so reaches
    PoseOptimization with its undistorted coordinates.  With the image, with image=None on the resident frame, and the relocalisation
    search over three candidates."""
    from ceres_mono_orb_slam2_amd import tracking
    from ceres_mono_orb_slam2_amd.vocabulary import ORBVocabulary
    name = "KITTI_k1"
    S = _scenario(oracle, name, SEED[name])
    voc = synth.make_vocabulary(3, k=6, L=6)
    V = ORBVocabulary(*[voc[x] for x in KEYS])
    bw, bv, fn, fo, fi = oracle.bow_transform(voc, S["fdesc"], 4)
    kf_valid = (S["valid"] != 0).astype(np.uint8)
    nm, m, owner, kf_fv = _bow_expected(oracle, voc, S, S["desc"], kf_valid, S["angle"], 0.7, (fn, fo, fi))
    feat = np.nonzero(owner >= 0)[0]
    n_out = int(S["outside"][feat].sum())
    print("TrackReferenceKeyFrame %s: %d matches, %d of them on keypoints outside the grid (of %d outside)" % (name, nm, n_out, S["outside"].sum()))
    assert nm > 100 and n_out >= 1
    ninl, pose, outl = _pose(oracle, S, feat, S["X"][owner[feat]])
    ex = _extractor(S)
    a = (S["K4"], S["bounds"], S["T"], S["desc"], kf_valid, S["angle"], S["X"], kf_fv, 0.7, True)
    got = tracking.track_reference_keyframe(ex, V, S["img"], *a)
    _check_frame(got, S)
    assert np.array_equal(got["bow"][0], bw) and np.array_equal(got["bow"][1].view(np.uint64), bv.view(np.uint64))
    assert all(np.array_equal(x, y) for x, y in zip(got["fv"], (fn, fo, fi)))
    assert np.array_equal(got["match"], m) and got["nmatches"] == nm
    assert np.array_equal(got["owner"], owner) and got["n_correspondences"] == len(feat)
    assert np.array_equal(got["outlier"], outl) and got["n_inliers"] == ninl
    assert np.allclose(got["pose7"], pose, rtol=0, atol=1e-7)
    # the pose solve saw the UNDISTORTED observations: with the raw ones the oracle arrives somewhere else
    raw = dict(S, kps4=np.stack([S["kps"]["x"], S["kps"]["y"], S["kps4"][:, 2], S["kps4"][:, 3]], 1).astype(F32))
    assert np.abs(_pose(oracle, raw, feat, S["X"][owner[feat]])[1] - pose).max() > 1e-4
    again = tracking.track_reference_keyframe(ex, V, None, *a)                   # the resident frame of a producing call
    assert again["kps"] is None and again["kps_undistorted"] is None
    assert np.array_equal(again["match"], got["match"]) and np.array_equal(again["owner"], got["owner"]) and np.array_equal(again["pose7"], got["pose7"])
    # Relocalization's first stage, three candidates
    rng = np.random.default_rng(8)
    cands, wants = [], []
    for i in range(3):
        d = S["desc"].copy(); valid = kf_valid.copy(); ang = S["angle"].copy()
        if i == 1: valid &= (rng.random(len(valid)) < 0.6).astype(np.uint8)
        if i == 2:
            flip = rng.random(len(d)) < 0.5
            d[flip, rng.integers(0, 32, flip.sum())] ^= (1 << rng.integers(0, 8, flip.sum())).astype(np.uint8)
        cnm, cm, cowner, cfv = _bow_expected(oracle, voc, S, d, valid, ang, 0.75, (fn, fo, fi))
        cands.append(dict(desc=d, valid=valid, angle=ang, fv=cfv)); wants.append((cnm, cowner))
    assert any(S["outside"][np.nonzero(o >= 0)[0]].any() for _, o in wants)
    got = tracking.relocalization_search_by_bow(ex, V, S["img"], S["K4"], S["bounds"], cands, 0.75, True)
    _check_frame(got, S)
    assert all(np.array_equal(x, y) for x, y in zip(got["fv"], (fn, fo, fi)))
    for i, (cnm, cowner) in enumerate(wants):
        assert int(got["nmatches"][i]) == cnm and np.array_equal(got["owner"][i], cowner), "candidate %d" % i
    assert wants[0][0] > 100 and wants[1][0] < wants[0][0]
    again = tracking.relocalization_search_by_bow(ex, V, None, S["K4"], S["bounds"], cands, 0.75, True)
    assert np.array_equal(again["owner"], got["owner"]) and np.array_equal(again["nmatches"], got["nmatches"])


@pytest.mark.parametrize("name,nfeat,family", [("KITTI_k1", 4000, "checker"), ("TUM1", 30, "blocks")])
def test_every_slot_of_the_lone_workgroup(oracle, name, nfeat, family):
    """k_trk_prepare holds up to four keypoints per thread of ONE 1024-thread workgroup: more than 3072 keypoints reach the fourth slot
    of a thread (the k1 = +0.3 camera, an extractor asked for 4000 features), fewer than 64 leave all but one wave without a keypoint
    (640 x 480: the extractor's floor per level is lowest on a 4 : 3 image)."""
    S = _scenario(oracle, name, 20, nfeat, family)
    n = len(S["kps"])
    print("%d features asked: %d keypoints, %d outside the grid" % (nfeat, n, S["outside"].sum()))
    assert n > 3072 if nfeat == 4000 else 0 < n < 64
    exp = _expected_mm(oracle, name, 20, 15.0, nfeat, family)
    got = _mm(_extractor(S), S, 15.0)
    _check_mm(got, exp, S)
    if nfeat == 4000:
        assert S["outside"].sum() >= 1 and exp["nmatches"] > 200


def test_distortion_state(oracle):
    """set_distortion(ex, None) restores the zero-distortion results bit for bit; k1 == 0 with the other coefficients set is no
    distortion; a second extractor of the thread is unaffected; without distortion orbt_last_undistorted_keypoints returns the raw
    coordinates; ORBHIP_ECAP with a short buffer."""
    import ctypes as C
    from ceres_mono_orb_slam2_amd import ORBextractor, tracking, _lib
    name = "KITTI_k1"
    S = _scenario(oracle, name, SEED[name])
    B0 = np.array([0, S["cam"]["w"], 0, S["cam"]["h"]], F32)
    a0 = (S["img"], S["K4"], B0, S["T"], S["X"], S["desc"], S["octave"], S["angle"], S["valid"], 15.0, True)
    keys = ("kps", "kps_undistorted", "desc", "match", "owner", "outlier", "pose7")
    same = lambda x, y: all(np.array_equal(x[k], y[k]) for k in keys) and all(x[k] == y[k] for k in ("nmatches", "n_inliers", "n_correspondences"))
    raw = np.stack([S["kps"]["x"], S["kps"]["y"]], 1).astype(F32)
    L = _lib.load()
    n = C.c_int(0); xy = np.full((len(raw), 2), -1, F32)
    plain = ORBextractor(2000, 1.2, 8, 20, 7)                                            # an extractor that never had coefficients
    fresh = tracking.track_with_motion_model(plain, *a0)
    assert np.array_equal(fresh["kps"], S["kps"]) and np.array_equal(fresh["kps_undistorted"], raw) and fresh["kps_undistorted"].flags.writeable
    assert L.orbt_last_undistorted_keypoints(plain._h, _lib.ptr(xy), len(raw), C.byref(n)) == 0 and n.value == len(raw) and np.array_equal(xy, raw)
    view = tracking.track_with_motion_model(plain, *a0, copy=False)["kps_undistorted"]
    assert np.array_equal(view, raw) and not view.flags.writeable
    del plain
    ex = _extractor(S)
    second = ORBextractor(2000, 1.2, 8, 20, 7)
    d = _mm(ex, S, 15.0)
    _check_mm(d, _expected_mm(oracle, name, SEED[name], 15.0), S)
    assert not np.array_equal(d["kps_undistorted"], raw)
    assert same(tracking.track_with_motion_model(second, *a0), fresh)                    # the first one's coefficients are not the second's
    again = _mm(ex, S, 15.0)                                                             # ... and the second's call left the first's alone
    assert same(again, d)
    # the C entry point on the frame `ex` produced: ECAP with a short buffer (only *n written), the full copy otherwise
    xy[:] = -1
    assert L.orbt_last_undistorted_keypoints(ex._h, _lib.ptr(xy), len(raw) - 1, C.byref(n)) == -4 and n.value == len(raw) and (xy == -1).all()
    assert L.orbt_last_undistorted_keypoints(ex._h, _lib.ptr(xy), len(raw), C.byref(n)) == 0 and np.array_equal(xy, d["kps_undistorted"])
    assert L.orbt_last_undistorted_keypoints(second._h, _lib.ptr(xy), len(raw), C.byref(n)) == -1      # the resident frame is ex's
    k1zero = S["dist"].copy(); k1zero[0] = 0.0; k1zero[1:] = (0.1, 0.01, -0.02, 0.3)
    tracking.set_distortion(ex, k1zero)
    assert same(tracking.track_with_motion_model(ex, *a0), fresh)
    tracking.set_distortion(ex, S["dist"])
    assert same(_mm(ex, S, 15.0), d)
    tracking.set_distortion(ex, None)
    assert same(tracking.track_with_motion_model(ex, *a0), fresh)
    with pytest.raises(_lib.OrbHipError):
        tracking.set_distortion(ex, [0.1, np.nan, 0, 0, 0])
    # the resident frame remembers its coefficients: going on with it under other ones is refused, a new frame is fine again
    nk = len(raw); z = np.zeros
    lm = lambda B: tracking.track_local_map(ex, S["K4"], B, S["T"], 0.18, z((0, 3)), z((0, 3)), z(0, F32), z(0, F32), z((0, 32), np.uint8), z(0, np.uint8),
                                            z((nk, 3)), z(nk, np.uint8))
    assert lm(B0)["nmatches"] == 0                                                       # (the frame above was built without distortion)
    tracking.set_distortion(ex, S["dist"])
    with pytest.raises(_lib.OrbHipError, match="coefficients"):
        lm(S["bounds"])
    _mm(ex, S, 15.0)
    assert lm(S["bounds"])["nmatches"] == 0
    tracking.set_distortion(ex, None)
    with pytest.raises(_lib.OrbHipError, match="coefficients"):
        lm(B0)
