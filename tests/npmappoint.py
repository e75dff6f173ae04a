"""Independent numpy restatement of MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:256-315) and
MapPoint::UpdateNormalAndDepth (:335-378), one point at a time, in the layout of orbl_update_map_points (include/orbslam_hip.h).
The parity reference of tests/test_gpu_mappoint.py; plus the seeded batch generators those tests and tools/mappoint_time.py use."""
import numpy as np

DESC, NORMAL_DEPTH = 1, 2
INT_MAX = 2 ** 31 - 1
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming_matrix(D):
    """N x N Hamming distances of D[N, 32] uint8 (ORBmatcher::DescriptorDistance for every pair; the diagonal is 0)."""
    D = np.asarray(D, np.uint8)
    if len(D) <= 64:
        return _POP[D[:, None, :] ^ D[None, :, :]].sum(-1)
    b = np.unpackbits(D, axis=1).astype(np.float64)               # (exact: integers far below 2^53)
    return np.rint(b @ (1.0 - b).T + (1.0 - b) @ b.T).astype(np.int64)


def distinctive_descriptor(desc, kf_good):
    """:256-315 for ONE point: desc[L, 32] its observations' descriptors in list order, kf_good[L] = !keyframe->isBad().
    Returns the list position of the chosen descriptor, or -1 (no good observation: descriptor_ unchanged)."""
    idx = [e for e in range(len(desc)) if kf_good[e]]              # (:272-279) descriptors of good keyframes, in order
    if not idx:
        return -1
    N = len(idx)
    dist = hamming_matrix(np.asarray(desc, np.uint8)[idx])         # (:286-296)
    best_median, best_index = INT_MAX, 0
    for i in range(N):                                             # (:299-308)
        dists = sorted(int(v) for v in dist[i])
        median = dists[int(0.5 * (N - 1))]
        if median < best_median:
            best_median, best_index = median, i
    return idx[best_index]


def normal_and_depth(X, centers, ref_center, level, scale_factors):
    """:335-378 for ONE point: X[3] world position, centers[n, 3] = GetCameraCenter() of every observing keyframe in list order
    (bad ones included), ref_center = the reference keyframe's, level = the octave resolved by reference_level().
    Returns (normal[3] float64, min float32, max float32)."""
    X = [float(v) for v in X]
    normal = np.zeros(3)
    for O in centers:                                              # (:356-364)
        v = np.array([X[0] - float(O[0]), X[1] - float(O[1]), X[2] - float(O[2])])
        nn = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        normal = normal + v / nn
    pc = [X[0] - float(ref_center[0]), X[1] - float(ref_center[1]), X[2] - float(ref_center[2])]
    dist = np.float32(np.sqrt((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]))       # (:366-368)
    sf = np.asarray(scale_factors, np.float32)
    mx = np.float32(dist * sf[level])                              # (:374-375)
    mn = np.float32(mx / sf[len(sf) - 1])
    return normal / len(centers), mn, mx


def reference_level(obs_kfs, obs_idx, ref_kf, octave_of):
    """The octave :369-371 reads: undistort_keypoints_[observations[reference_keyframe]] on the method's local copy of the map -
    std::map::operator[] inserts index 0 when the reference keyframe is not in it.  octave_of(kf, i) = keyframe kf's keypoint i."""
    for k, i in zip(obs_kfs, obs_idx):
        if k == ref_kf:
            return octave_of(k, i)
    return octave_of(ref_kf, 0)


def update_map_points(b, what, out=None):
    """The whole batch in the layout of orbl_update_map_points: b = dict(obs_off, obs_desc, obs_kf_good, X, ref_kf, ref_level, obs_kf,
    kf_center, scale_factors, pt_good); out = preset outputs (points and parts the call leaves alone keep them)."""
    off = np.asarray(b["obs_off"], np.int64)
    npts = len(off) - 1
    o = fresh_outputs(npts) if out is None else {k: v.copy() for k, v in out.items()}
    pg = b.get("pt_good")
    kg = b.get("obs_kf_good")
    for p in range(npts):
        lo, hi = int(off[p]), int(off[p + 1])
        live = hi > lo and (pg is None or pg[p])
        if what & DESC:
            o["best_obs"][p] = -1
            if live:
                g = np.ones(hi - lo, bool) if kg is None else np.asarray(kg[lo:hi]).astype(bool)
                e = distinctive_descriptor(b["obs_desc"][lo:hi], g)
                o["best_obs"][p] = e
                if e >= 0:
                    o["desc"][p] = b["obs_desc"][lo + e]
        if what & NORMAL_DEPTH:
            o["nd_written"][p] = 0
            if live:
                kc = np.asarray(b["kf_center"], np.float64)
                n, mn, mx = normal_and_depth(b["X"][p], kc[b["obs_kf"][lo:hi]], kc[b["ref_kf"][p]], int(b["ref_level"][p]), b["scale_factors"])
                o["normal"][p] = n
                o["min_max"][p] = (mn, mx)
                o["nd_written"][p] = 1
    return o


def fresh_outputs(npts, poison=False):
    """Output arrays; poison=True fills them with a pattern no call writes (0xA5 bytes, NaN-free doubles, -7 indices)."""
    if not poison:
        return dict(best_obs=np.full(npts, -1, np.int32), desc=np.zeros((npts, 32), np.uint8), normal=np.zeros((npts, 3)),
                    min_max=np.zeros((npts, 2), np.float32), nd_written=np.zeros(npts, np.uint8))
    return dict(best_obs=np.full(npts, -7, np.int32), desc=np.full((npts, 32), 0xA5, np.uint8), normal=np.full((npts, 3), -12345.5),
                min_max=np.full((npts, 2), -77.25, np.float32), nd_written=np.full(npts, 0xA5, np.uint8))


# ------------------------------------------------------------------------------------------------------------ generators
SCALE_FACTORS = (1.2 ** np.arange(8)).astype(np.float32)


def make_batch(seed, ns, nkf=40, bad_kf_frac=0.1, bad_pt_frac=0.0, flip=(4, 24), dup_frac=0.0, equal_frac=0.0):
    """A batch of len(ns) points, point p observed by ns[p] entries.  Descriptors = a per-point base with `flip` bits flipped per
    observation; dup_frac of the observations copy an earlier one of the same point, equal_frac of the points observe one
    descriptor only (every median 0: ties everywhere).  Keyframe indices may repeat inside a list (the normal reads centres only)."""
    rng = np.random.default_rng(seed)
    ns = np.asarray(ns, np.int64)
    npts = len(ns)
    off = np.zeros(npts + 1, np.int32)
    off[1:] = np.cumsum(ns)
    nobs = int(off[-1])
    desc = np.zeros((nobs, 32), np.uint8)
    for p in range(npts):
        lo, hi = off[p], off[p + 1]
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        d = np.repeat(base[None], hi - lo, 0)
        if rng.random() >= equal_frac:
            bits = np.unpackbits(d, axis=1)
            for r in range(hi - lo):
                k = rng.choice(256, int(rng.integers(flip[0], flip[1] + 1)), replace=False)
                bits[r, k] ^= 1
            d = np.packbits(bits, axis=1)
            if dup_frac > 0:
                for r in range(1, hi - lo):
                    if rng.random() < dup_frac:
                        d[r] = d[rng.integers(0, r)]
        desc[lo:hi] = d
    kf_center = np.stack([rng.normal(0, 0.3, nkf), rng.normal(0, 0.1, nkf), 0.8 * np.arange(nkf) + rng.normal(0, 0.05, nkf)], 1)
    X = np.stack([rng.uniform(-15, 15, npts), rng.uniform(-3, 3, npts), rng.uniform(5, 60, npts) + 0.8 * nkf / 2], 1)
    obs_kf = rng.integers(0, nkf, nobs).astype(np.int32)
    kf_bad = rng.random(nkf) < bad_kf_frac
    ref_kf = np.array([obs_kf[off[p]] if ns[p] else 0 for p in range(npts)], np.int32)
    ref_level = rng.integers(0, 8, npts).astype(np.int32)
    pt_good = (rng.random(npts) >= bad_pt_frac).astype(np.uint8)
    return dict(obs_off=off, obs_desc=desc, obs_kf_good=(~kf_bad[obs_kf]).astype(np.uint8), X=X, ref_kf=ref_kf, ref_level=ref_level,
                obs_kf=obs_kf, kf_center=kf_center, scale_factors=SCALE_FACTORS.copy(), pt_good=pt_good)


def skewed_ns(seed, npts=2000):
    """SearchInNeighbors-sized: most points seen by 2-6 keyframes, a tail to a few hundred."""
    rng = np.random.default_rng(seed)
    n = 2 + rng.geometric(0.3, npts) - 1
    tail = rng.random(npts) < 0.03
    n[tail] = rng.integers(9, 300, int(tail.sum()))
    n[rng.random(npts) < 0.01] = 0
    n[rng.random(npts) < 0.02] = 1
    return n


def c4_normal_depth_batch(seed=0):
    """10 000 points of synth's C4 graph (100 keyframes, 50 000 observations): the LocalBA write-back's UpdateNormalAndDepth."""
    from ceres_mono_orb_slam2_amd import synth
    g = synth.make_ba_graph(seed, ncam=100, npts=10000, nobs=50000, n_fixed=2)
    order = np.argsort(g["obs_pt"], kind="stable")
    op, oc = g["obs_pt"][order], g["obs_cam"][order]
    npts = len(g["pts0"])
    off = np.zeros(npts + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(op, minlength=npts))
    centers = np.zeros((len(g["poses0"]), 3))
    for c, pose in enumerate(g["poses0"]):
        R = synth.quat_to_R(pose[3:])
        centers[c] = -R.T @ pose[:3]
    rng = np.random.default_rng(seed + 1)
    ref_kf = oc[off[:-1]].astype(np.int32)
    return dict(obs_off=off, obs_desc=None, obs_kf_good=None, X=g["pts0"].copy(), ref_kf=ref_kf, ref_level=g["octave"][order][off[:-1]].astype(np.int32),
                obs_kf=oc.astype(np.int32), kf_center=centers, scale_factors=SCALE_FACTORS.copy(), pt_good=(rng.random(npts) >= 0.01).astype(np.uint8))
