"""Seeded cases for Relocalization's refinement behind PnP (tests/nprelocrefine.py, tests/test_gpu_relocrefine.py), in the style of
tests/test_gpu_track.py::_scenario: the keyframe is frame 1's keypoints with synthetic depths (its camera is the world frame), the
current frame is frame 2 (frame 1 moved by a few pixels = a camera translation at that depth), the PnP pose is the true one plus noise.
What steers nGood from solve to solve:
  n_correct   inlier slots that hold the right keyframe point
  n_wrong     inlier slots that hold a wrong one (outliers of the first solve; their points stay in the wide search's `found`, and are
              free again for a narrow search behind the loop)
  n_wrong_off of those (lowest pyramid levels first), the ones whose point is displaced by 2.3 scale pixels in x and in y: inside the narrow
              window and, on levels 0 and 1, an outlier of the third solve
  n_extra     keyframe points outside the slots that the wide search can find
  n_extra_off of those, the ones displaced by 8 pixels in a random direction: inside the wide window, outliers of the second solve
Every other keyframe feature has no map point."""
import numpy as np

from ceres_mono_orb_slam2_amd import synth

F32 = np.float32
K4 = np.array([517.3, 516.5, 318.6, 255.3], np.float32)
W_IMG, H_IMG = 640, 480
BOUNDS = np.array([0, W_IMG, 0, H_IMG], np.float32)
K4_WIDE = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)
DEPTH = 18.0

_POP = np.array([bin(b).count("1") for b in range(256)], np.int32)
_cache = {}


def frame_of(oracle, img, nfeatures, K4_=K4, bounds=BOUNDS, kps_desc=None):
    E = oracle.OracleExtractor(nfeatures)
    kps, desc = E.extract(img) if kps_desc is None else kps_desc
    kps4 = np.stack([kps["x"], kps["y"], kps["octave"].astype(np.float32), kps["angle"]], 1).astype(np.float32)
    return dict(kps4=kps4, desc=desc, K4=K4_, bounds=bounds, scale=E.scale.astype(F32), inv_sigma2=E.inv_sigma2.astype(F32), log_scale=F32(np.log(F32(1.2))), img=img,
                nfeatures=nfeatures)


def two_frames(oracle, seed=41, size=(W_IMG, H_IMG), nfeatures=1000, K4=K4):
    """(keyframe records, current frame, the true pairs (keyframe feature, frame feature), the true Tcw)"""
    key = ("two", seed, size, nfeatures)
    if key in _cache:
        return _cache[key]
    E = oracle.OracleExtractor(nfeatures)
    seq, offs = synth.make_sequence(seed, size[0], size[1], 2, "blocks", max_shift=6)
    k1, d1 = E.extract(seq[0])
    F = frame_of(oracle, seq[1], nfeatures, K4, np.array([0, size[0], 0, size[1]], np.float32))
    shift = (offs[1] - offs[0]).astype(np.float64)                               # u_cur = u_kf - shift
    n = len(k1)
    rng = np.random.default_rng(seed)
    z = DEPTH * (1.0 + 0.002 * rng.standard_normal(n))
    X = np.stack([(k1["x"] - K4[2]) / K4[0] * z, (k1["y"] - K4[3]) / K4[1] * z, z], 1).astype(np.float64)
    T = np.eye(4); T[:3, 3] = [-shift[0] * DEPTH / K4[0], -shift[1] * DEPTH / K4[1], 0.0]
    # true pairs: the frame feature of the same octave closest to the shifted keyframe keypoint (within 1.5 pixels), by descriptor
    pairs = []
    used = set()
    kp2 = F["kps4"]
    for i in range(n):
        d = np.abs(kp2[:, 0] - (k1["x"][i] - shift[0])) + np.abs(kp2[:, 1] - (k1["y"][i] - shift[1]))
        c = np.nonzero((d < 1.5 * E.scale[k1["octave"][i]]) & (kp2[:, 2] == k1["octave"][i]))[0]
        if len(c) == 0:
            continue
        hd = _POP[F["desc"][c] ^ d1[i]].sum(1)
        f = int(c[np.argmin(hd)])
        if hd.min() <= 40 and f not in used:
            pairs.append((i, f)); used.add(f)
    dist = np.linalg.norm(X, axis=1)
    maxd = (dist * E.scale[k1["octave"]] * 0.95).astype(F32)                     # (0.95: PredictScale's ratio stays off the powers of 1.2)
    KF = dict(X=X, desc=d1, angle=k1["angle"].astype(F32), octave=k1["octave"].astype(np.int32), max_dist=maxd, min_dist=(maxd / E.scale[7]).astype(F32), n=n)
    _cache[key] = (KF, F, np.array(pairs, np.int32), T)
    return _cache[key]


def candidate(oracle, seed, n_correct, n_wrong=0, n_wrong_off=0, n_extra=0, n_extra_off=0, pose_noise=2e-3, dup=0, frames_seed=41, has_pose=True, frames=None):
    """frames: the result of two_frames() to build on (default: the 640 x 480 pair of frames_seed)"""
    KF, F, pairs, T = two_frames(oracle, frames_seed) if frames is None else frames
    K4 = F["K4"]
    rng = np.random.default_rng(seed)
    n, n_kp = KF["n"], len(F["kps4"])
    order = rng.permutation(len(pairs))
    need = n_correct + n_wrong + n_extra
    assert need <= len(pairs), (need, len(pairs))
    pc, pw, pe = np.split(pairs[order[:need]], [n_correct, n_correct + n_wrong])
    pt = np.full(n, -1, np.int32)
    ids = 1000 + rng.permutation(4 * n)[:n].astype(np.int32)
    X = KF["X"].copy()
    slot = np.full(n_kp, -1, np.int32)
    scale = F["scale"]

    def displace(i, px, py):
        X[i, 0] += px * X[i, 2] / float(K4[0]); X[i, 1] += py * X[i, 2] / float(K4[1])
    pw = pw[np.argsort(KF["octave"][pw[:, 0]], kind="stable")]                   # (the displaced wrong points: the lowest levels first)
    for i, f in pc:
        pt[i] = ids[i]; slot[f] = i
    # a wrong slot: the point of pw[j] sits in a frame feature that is nobody's true match
    free = np.setdiff1d(np.arange(n_kp), pairs[:, 1])
    wrong_f = rng.choice(free, size=len(pw), replace=False) if len(pw) else []
    for j, (i, f) in enumerate(pw):
        pt[i] = ids[i]; slot[wrong_f[j]] = i
        if j < n_wrong_off:
            d = 2.3 * float(scale[KF["octave"][i]])
            displace(i, d * rng.choice([-1, 1]), d * rng.choice([-1, 1]))
    for j, (i, f) in enumerate(pe):
        pt[i] = ids[i]
        if j < n_extra_off:
            a = rng.uniform(0, 2 * np.pi)
            displace(i, 8.0 * np.cos(a), 8.0 * np.sin(a))
    D = KF["desc"].copy()
    for j in range(dup):                                                         # one point id at two keyframe features: the second is a feature without a true pair
        a = int(pe[j, 0]) if j < len(pe) else int(pc[j, 0])
        b = int(np.setdiff1d(np.arange(n), pairs[:, 0])[j])
        pt[b] = pt[a]; X[b] = X[a]; D[b] = D[a]
    Tn = T.copy()
    Tn[:3, :3] = synth.quat_to_R(synth.quat_from_rotvec(pose_noise * rng.standard_normal(3)))
    Tn[:3, 3] += 0.02 * rng.standard_normal(3)
    return dict(pt=pt, Xw=X, desc=D, min_dist=KF["min_dist"], max_dist=KF["max_dist"], angle=KF["angle"], Tcw=Tn if has_pose else None,
                slot_kf=slot if has_pose else None)


# name -> keyword arguments of candidate(); the stage each reaches is asserted by tests/test_relocrefine_restatement.py
CASES = {
    "no_pose": dict(seed=1, n_correct=40, has_pose=False),
    "two_correspondences": dict(seed=2, n_correct=2),
    "three_correspondences": dict(seed=3, n_correct=3),
    "few_inliers": dict(seed=4, n_correct=6, n_wrong=12),
    "match_first": dict(seed=5, n_correct=120, n_wrong=10, n_extra=50),
    "fail_wide": dict(seed=6, n_correct=25, n_wrong=8, n_extra=12),
    "match_second": dict(seed=7, n_correct=25, n_wrong=8, n_extra=200, dup=3),
    "fail_second": dict(seed=8, n_correct=14, n_wrong=4, n_extra=60, n_extra_off=50),
    "narrow": dict(seed=9, n_correct=30, n_wrong=20, n_extra=30, n_extra_off=18, dup=2),
    "narrow_third_fails": dict(seed=9, n_correct=30, n_wrong=20, n_wrong_off=20, n_extra=30, n_extra_off=18),
}


def empty_keyframe_candidate(oracle):
    """a candidate whose keyframe has no features (n = 0) but a pose"""
    _, F, _, T = two_frames(oracle)
    z = np.zeros
    return dict(pt=z(0, np.int32), Xw=z((0, 3)), desc=z((0, 32), np.uint8), min_dist=z(0, F32), max_dist=z(0, F32), angle=z(0, F32), Tcw=T.copy(),
                slot_kf=np.full(len(F["kps4"]), -1, np.int32))


def empty_slots_candidate(oracle):
    c = candidate(oracle, 11, n_correct=30, n_extra=60)
    c["slot_kf"] = np.full(len(c["slot_kf"]), -1, np.int32)
    return c


def _periodic_image(W, H):
    rng = np.random.default_rng(42)
    patch = (rng.random((20, 20)) < 0.5).astype(np.uint8) * 170 + 40
    patch = np.kron(patch[::4, ::4], np.ones((4, 4), np.uint8))
    img = np.tile(patch, (H // 20 + 1, W // 20 + 1))[:H, :W].copy()
    img[::37, ::41] ^= 0x55
    return img


def _same_frame_candidate(F, K4_, seed):
    """the frame as its own keyframe, identity motion, every point at 18 m, 30 correct inlier slots, one point in ten missing"""
    rng = np.random.default_rng(seed)
    kp = F["kps4"]; n = len(kp)
    z = np.full(n, DEPTH)
    X = np.stack([(kp[:, 0] - K4_[2]) / K4_[0] * z, (kp[:, 1] - K4_[3]) / K4_[1] * z, z], 1).astype(np.float64)
    oc = kp[:, 2].astype(int)
    maxd = (np.linalg.norm(X, axis=1) * F["scale"][oc] * 0.95).astype(F32)
    slot = np.full(n, -1, np.int32)
    keep = rng.choice(n, size=30, replace=False)
    slot[keep] = keep
    pt = np.arange(n, dtype=np.int32); pt[rng.random(n) < 0.1] = -1; pt[keep] = keep
    return dict(pt=pt, Xw=X, desc=F["desc"].copy(), min_dist=(maxd / F["scale"][7]).astype(F32), max_dist=maxd, angle=kp[:, 3].copy(), Tcw=np.eye(4), slot_kf=slot)


def periodic(oracle):
    """The periodic-texture frame of tests/test_gpu_track.py (one 20 x 20 patch tiled over 1241 x 376: every corner has dozens of
    bit-identical look-alikes), as keyframe and as current frame.  Returns (frame, candidate)."""
    if "periodic" not in _cache:
        W, H = 1241, 376
        F = frame_of(oracle, _periodic_image(W, H), 2000, K4_WIDE, np.array([0, W, 0, H], np.float32))
        _cache["periodic"] = (F, _same_frame_candidate(F, K4_WIDE, 42))
    return _cache["periodic"]


K4_SMALL = np.array([300.0, 300.0, 160.0, 120.0], np.float32)


def dense_periodic(oracle):
    """The same texture at 320 x 240 with 3500 features asked for (2654 found): dense enough for windows of 10 scale pixels to hold more
    than 16 acceptable candidates - the full window lists."""
    if "dense" not in _cache:
        W, H = 320, 240
        F = frame_of(oracle, _periodic_image(W, H), 3500, K4_SMALL, np.array([0, W, 0, H], np.float32))
        _cache["dense"] = (F, _same_frame_candidate(F, K4_SMALL, 43))
    return _cache["dense"]
