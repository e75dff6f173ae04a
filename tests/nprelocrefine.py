"""A literal restatement of what Tracking::Relocalization does behind a PnP pose (reference src/Tracking.cc:1056-1126) over flat arrays,
with the narrow SearchByProjection(F, KF, found, 3, 64) LITERALLY inside the `for (ip < N_)` loop (:1097-1104).  It is built on a
backend's search_by_projection and pose_optimization: the CPU oracle (oracle.pyoracle) for the expected values, or the library's
per-call host entries (ChainBackend, below) for the chain the fused call replaces.  refine() counts the paths it takes.

The frame is a dict(kps4[n_kp, 4] = {x, y, octave, angle} of the undistorted keypoints, desc[n_kp, 32], K4, bounds, scale[nlevels],
inv_sigma2[nlevels], log_scale); a candidate is a dict(pt[n] point ids or -1, Xw[n, 3], desc[n, 32] = MapPoint::GetDescriptor(),
min_dist[n], max_dist[n] raw, angle[n], Tcw (4, 4) or None, slot_kf[n_kp] = current_frame_.map_points_ as keyframe features).

Also here: the toy model of the loop (lists of candidate features per point, no geometry) in its literal and its early-exit form."""
import numpy as np

F32 = np.float32
NO_POSE, FEW_INLIERS, MATCH_FIRST, MATCH_SECOND, MATCH_THIRD, FAIL_WIDE, FAIL_SECOND, FAIL_NARROW, FAIL_THIRD = range(9)
STAGE_NAMES = ("NO_POSE", "FEW_INLIERS", "MATCH_FIRST", "MATCH_SECOND", "MATCH_THIRD", "FAIL_WIDE", "FAIL_SECOND", "FAIL_NARROW", "FAIL_THIRD")


def project(frame, kf, T, th):
    """The loop head of src/ORBmatcher.cc:1292-1321 for every keyframe point at once, in the reference's float / double mix: double camera
    coordinates, float u / v, the image bounds, the float distance to the camera centre against 0.8 min / 1.2 max, PredictScale, the
    radius.  Returns (uv[n, 2] float32, radius[n] float32, level[n] int32, ok[n] bool); pt and `found` are the caller's."""
    X = np.asarray(kf["Xw"], np.float64).reshape(-1, 3)
    n = len(X)
    T = np.asarray(T, np.float64)
    R = T[:3, :3]; t = T[:3, 3]
    c = [((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)]
    fx, fy, cx, cy = [F32(k) for k in frame["K4"]]
    b = [F32(v) for v in frame["bounds"]]
    with np.errstate(all="ignore"):
        xc, yc = c[0].astype(F32), c[1].astype(F32)
        invz = (1.0 / c[2]).astype(F32)
        u = (fx * xc) * invz + cx
        v = (fy * yc) * invz + cy
        ok = ~((u < b[0]) | (u > b[1])) & ~((v < b[2]) | (v > b[3]))
        Ow = [-((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2]) for k in range(3)]
        P = [X[:, k] - Ow[k] for k in range(3)]
        dist = np.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2]).astype(F32)
        maxd = np.asarray(kf["max_dist"], F32); mind = np.asarray(kf["min_dist"], F32)
        ok &= ~((dist < F32(0.8) * mind) | (dist > F32(1.2) * maxd))
        ratio = maxd / dist
        lvl = np.ceil(np.log(ratio) / F32(frame["log_scale"]))
        nlevels = len(frame["scale"])
        lvl = np.where(lvl >= 0, np.minimum(lvl, nlevels - 1), 0)
        lvl = np.where(np.isfinite(lvl), lvl, 0).astype(np.int32)
    radius = (F32(th) * np.asarray(frame["scale"], F32)[lvl]).astype(F32)
    assert u.dtype == F32 and dist.dtype == F32 and ratio.dtype == F32
    return np.stack([u, v], 1).astype(F32), radius, lvl, ok[:n]


def search_by_projection(backend, frame, kf, S, found, geom, orb_dist, check_ori):
    """ORBmatcher::SearchByProjection(Frame&, KeyFrame*, found, th, ORBdist) (src/ORBmatcher.cc:1273-1384) on the slots S (in place): a
    point is tried when it is not NULL / bad, not in `found` and passes the geometric gates; only features with an empty slot can be
    taken, the first minimum wins, every assignment closes the feature, the rotation check runs over this call's matches and a removed
    match leaves its slot empty.  Returns nmatches."""
    uv, radius, lvl, ok = geom
    pt = kf["pt"]
    valid = ok & (pt >= 0)
    if found:
        valid &= ~np.isin(pt, np.fromiter(found, np.int64, len(found)))
    if not valid.any():
        return 0
    q = np.nonzero(valid)[0]
    taken = (S >= 0).astype(np.uint8)
    n, m, _, _ = backend.search_by_projection(frame["kps4"], frame["desc"], frame["bounds"], uv[q], radius[q], kf["desc"][q], q_min_level=lvl[q] - 1,
                                              q_max_level=lvl[q] + 1, q_valid=np.ones(len(q), np.uint8), q_angle=kf["angle"][q], taken=taken, th=orb_dist,
                                              check_ori=check_ori)
    hit = m >= 0
    S[m[hit]] = q[hit]
    return int(n)


def pose_optimization(backend, frame, kf, S, pose7, outl):
    """CeresOptimizer::PoseOptimization (src/CeresOptimizer.cc:275-342): the slots that hold a point, in feature order; their flags are
    reset, and below 3 of them nothing else happens (0 is returned, the pose stays).  Returns (nGood, pose7, correspondences)."""
    feat = np.nonzero(S >= 0)[0]
    outl[feat] = False
    if len(feat) < 3:
        return 0, pose7, len(feat)
    kp = frame["kps4"]
    n, pose, out, _ = backend.pose_optimization(np.asarray(frame["K4"], np.float64), pose7, kf["Xw"][S[feat]], kp[feat, :2].astype(np.float64),
                                                np.asarray(frame["inv_sigma2"], F32)[kp[feat, 2].astype(int)])
    outl[feat] = out.astype(bool)
    return int(n), np.asarray(pose, np.float64), len(feat)


def refine(backend, frame, cand, check_ori=True, narrow_in_loop=True, early_exit=False, paths=None, trace=None):
    """src/Tracking.cc:1056-1126 for one candidate.  early_exit: the loop stops at its first empty pass (the form the device runs).
    paths: a dict that counts the branches taken.  trace: a dict that receives the poses the two searches ran with (T_wide, T_narrow)."""
    paths = {} if paths is None else paths
    trace = {} if trace is None else trace

    def took(k):
        paths[k] = paths.get(k, 0) + 1
    n_kp = len(frame["kps4"])
    r = dict(stage=NO_POSE, matched=False, narrow_passes=0, n_good=[-1] * 3, n_additional=[-1] * 2, n_correspondences=[-1] * 3,
             pose7=np.array([0, 0, 0, 0, 0, 0, 1.0]), slot_kf=np.full(n_kp, -1, np.int32), outlier=np.zeros(n_kp, bool))
    if cand.get("Tcw") is None:                                                  # :1059
        took("no_pose")
        return r
    kf = dict(pt=np.asarray(cand["pt"], np.int64).reshape(-1), Xw=np.asarray(cand["Xw"], np.float64).reshape(-1, 3), desc=np.asarray(cand["desc"], np.uint8).reshape(-1, 32),
              min_dist=np.asarray(cand["min_dist"], F32), max_dist=np.asarray(cand["max_dist"], F32), angle=np.asarray(cand["angle"], F32))
    T = np.eye(4); T[:3] = np.asarray(cand["Tcw"], np.float64).reshape(-1)[:12].reshape(3, 4)
    pose7 = np.asarray(backend.matrix4d_to_pose7(T), np.float64)
    S = np.asarray(cand["slot_kf"], np.int32).copy()                             # :1066-1072
    outl = r["outlier"]
    found = set(int(p) for p in kf["pt"][S[S >= 0]])
    r["slot_kf"] = S

    def solve(k):
        nonlocal pose7, T
        pose7 = np.asarray(backend.matrix4d_to_pose7(T), np.float64)             # Eigen::Quaterniond(frame_R) of the CURRENT Tcw_ (src/CeresOptimizer.cc:286-291)
        nGood, pose, ncorr = pose_optimization(backend, frame, kf, S, pose7, outl)
        r["n_good"][k] = nGood; r["n_correspondences"][k] = ncorr
        if ncorr >= 3:
            pose7 = pose
            T = np.asarray(backend.pose7_to_matrix4d(pose7), np.float64).reshape(4, 4)
        r["pose7"] = pose7
        return nGood
    nGood = solve(0)                                                             # :1074
    if nGood < 10:                                                               # :1076
        r["stage"] = NO_POSE if r["n_correspondences"][0] < 3 else FEW_INLIERS
        took("few_inliers")
        return r
    S[outl] = -1                                                                 # :1078-1080
    if nGood < 50:                                                               # :1084
        took("wide_search")
        trace["T_wide"] = T.copy()
        nadd = search_by_projection(backend, frame, kf, S, found, project(frame, kf, T, 10.0), 100, check_ori)
        r["n_additional"][0] = nadd
        if nadd + nGood >= 50:                                                   # :1089
            took("second_solve")
            nGood = solve(1)                                                     # (:1090; the outlier slots are NOT cleared here)
            if 30 < nGood < 50:                                                  # :1095
                took("narrow_search")
                trace["T_narrow"] = T.copy()
                found = set()
                geom = project(frame, kf, T, 3.0)                                # (the pose does not change inside the loop)
                if narrow_in_loop:
                    for ip in range(n_kp):                                       # :1097-1104
                        if S[ip] >= 0:
                            found.add(int(kf["pt"][S[ip]]))
                        before = S.copy() if early_exit else None
                        nadd = search_by_projection(backend, frame, kf, S, found, geom, 64, check_ori)
                        r["narrow_passes"] += 1
                        if early_exit and nadd == 0 and np.array_equal(before, S) and not _assigns(backend, frame, kf, S, found, geom):
                            nadd = 0
                            took("early_exit")
                            break
                else:
                    found = set(int(p) for p in kf["pt"][S[S >= 0]])
                    nadd = search_by_projection(backend, frame, kf, S, found, geom, 64, check_ori)
                    r["narrow_passes"] = 1
                r["n_additional"][1] = nadd
                if nadd != 0:
                    took("narrow_added")
                if nGood + nadd >= 50:                                           # :1107
                    took("third_solve")
                    nGood = solve(2)
                    S[outl] = -1                                                 # :1110-1114
                    r["stage"] = MATCH_THIRD if nGood >= 50 else FAIL_THIRD
                else:
                    r["stage"] = FAIL_NARROW
            else:
                r["stage"] = MATCH_SECOND if nGood >= 50 else FAIL_SECOND
        else:
            r["stage"] = FAIL_WIDE
    else:
        r["stage"] = MATCH_FIRST
    r["matched"] = nGood >= 50                                                   # :1122
    if r["matched"]:
        took("matched")
    return r


def _assigns(backend, frame, kf, S, found, geom):
    """Whether a pass with these slots and this `found` assigns anything BEFORE its rotation check (an empty pass in the sense of the
    early-exit argument): the same search without the check."""
    return search_by_projection(backend, frame, kf, S.copy(), found, geom, 64, False) > 0


def refine_round(backend, frame, candidates, check_ori=True, narrow_in_loop=True, early_exit=False, paths=None):
    """Every candidate of a round, as the fused call refines them; first_match = where the reference breaks out of its loop."""
    res = [refine(backend, frame, c, check_ori, narrow_in_loop, early_exit, paths) for c in candidates]
    first = next((i for i, r in enumerate(res) if r["matched"]), -1)
    return dict(first_match=first, results=res)


class ChainBackend:
    """The chain of per-call host entries the fused call replaces: ba_pose_optimization and orbm_search_by_projection in its
    SearchByProjection(Frame&, KeyFrame*, ...) form, one host round trip each (needs a GPU)."""

    def __init__(self):
        from ceres_mono_orb_slam2_amd import ORBmatcher, optimizer
        self._M, self._opt = ORBmatcher, optimizer
        self.calls = 0

    def search_by_projection(self, kps4, desc, bounds, q_uv, q_radius, q_desc, check_ori=True, **kw):
        self.calls += 1
        return self._M(0.9, bool(check_ori)).search_by_projection(kps4, desc, bounds, q_uv, q_radius, q_desc, **kw)

    def pose_optimization(self, K4, pose7, Xw, uv, inv_sigma2):
        self.calls += 1
        return self._opt.pose_optimization(K4, pose7, Xw, uv, inv_sigma2)

    def matrix4d_to_pose7(self, T):
        return self._opt.matrix4d_to_pose7(T)

    def pose7_to_matrix4d(self, p):
        return self._opt.pose7_to_matrix4d(p)


# ---------------------------------------------------------------------------------------------------------------- the toy model
def three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:1386-1418): the bins that survive."""
    m1 = m2 = m3 = 0; i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > m1:
            m3, m2, m1 = m2, m1, s; i3, i2, i1 = i2, i1, i
        elif s > m2:
            m3, m2 = m2, s; i3, i2 = i2, i
        elif s > m3:
            m3 = s; i3 = i
    if m2 < 0.1 * m1:
        i2 = i3 = -1
    elif m3 < 0.1 * m1:
        i3 = -1
    return i1, i2, i3


def toy_search(S, found, cands, pid, bins, th, ori):
    """One SearchByProjection over candidate lists: cands[i] = [(feature, distance), ...] in window order, pid[i] = the point's id or
    -1, bins[i][f] = the rotation bin of the pair.  Returns (net matches, assignments made before the rotation check)."""
    n = raw = 0
    hist = [[] for _ in range(30)]
    for i, c in enumerate(cands):
        if pid[i] < 0 or pid[i] in found:
            continue
        bd, bi = 256, -1
        for f, d in c:
            if S[f] >= 0:
                continue
            if d < bd:
                bd, bi = d, f
        if bd <= th:
            S[bi] = pid[i]; n += 1; raw += 1
            if ori:
                hist[bins[i][bi]].append(bi)
    if ori:
        keep = three_maxima([len(x) for x in hist])
        for b in range(30):
            if b not in keep:
                for f in hist[b]:
                    S[f] = -1; n -= 1
    return n, raw


def toy_instance(seed):
    r = np.random.default_rng(seed)
    N = int(r.integers(5, 60)); M = int(r.integers(5, 60))
    pid = [int(x) if r.random() < 0.85 else -1 for x in r.permutation(M)]
    if r.random() < 0.3 and M > 3:
        pid[1] = pid[0]                                                          # one point at two keyframe features
    cands = [[(int(f), int(r.integers(20, 120))) for f in r.choice(N, size=int(r.integers(0, min(N, 6))), replace=False)] for _ in range(M)]
    bins = r.integers(0, 30 if r.random() < 0.5 else 3, (M, N))
    S = [-1] * N
    for f in r.choice(N, size=N // 3, replace=False):
        S[int(f)] = int(r.integers(0, M))
    return N, pid, cands, bins, S


def toy_loop(seed, ori, early):
    """The loop of :1096-1104 on a toy instance: literal (every ip) or stopped at its first empty pass.  Returns (slots, nadditional, passes)."""
    N, pid, cands, bins, S = toy_instance(seed)
    nadd = -7; found = set(); passes = 0
    for ip in range(N):
        if S[ip] >= 0:
            found.add(S[ip])
        nadd, raw = toy_search(S, found, cands, pid, bins, 64, ori)
        passes += 1
        if early and raw == 0:
            nadd = 0
            break
    return S, nadd, passes
