"""Restatement of the two map-moving steps of a loop closure over the flattened arrays of orbl_correct_loop and
orbl_propagate_global_ba: the LITERAL loops of src/LoopClosing.cc:446-523 and :681-739 over Python objects - a rank-ordered map for
sophus_corrected_sim3, a FIFO for keyframes_to_check, SetPose mutating a keyframe's centre as the loop goes - TEST INFRASTRUCTURE,
independent of the closed forms the kernels use.  Every operation is a float64 scalar (a Python float) in the order of csrc/sim3_math.h,
the pose codec (rot_to_quat, quat_to_R) and k_mp_prep; the float32 steps of the depth range are numpy float32 scalars.

correct_loop problem: dict(nkf, kf_Tcw[nkf][12], kf_center[nkf][3] | None, conn_kf[nconn], conn_rank | None, Scw[7], slot_off, slot_pt, npts,
X[npts][3], pt_bad | None, pt_done | None, and as a set or all None: obs_off, obs_kf, ref_kf, ref_level, scale_factors).
propagate problem: dict(nkf, kf_Tcw, kf_gba_Tcw, kf_in_gba, kf_parent, origin_kf, kf_center | None, npts, X, pt_bad | None, pt_in_gba | None,
pt_gba_X | None, pt_ref_kf)."""
import math
from collections import deque

import numpy as np

F32 = np.float32


# ---- the arithmetic, scalar by scalar --------------------------------------------------------------------------------------------
def rot_to_quat(m):
    """Eigen::Quaterniond(R).coeffs() = [x, y, z, w] for a 3x3 list of lists (csrc/ba_math.h rot_to_quat)"""
    q = [0.0] * 4
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2][1] - m[1][2]) * t; q[1] = (m[0][2] - m[2][0]) * t; q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k][j] - m[j][k]) * t; q[j] = (m[j][i] + m[i][j]) * t; q[k] = (m[k][i] + m[i][k]) * t
    return q


def se3_as_sim3(T):
    m = [[T[0], T[1], T[2]], [T[4], T[5], T[6]], [T[8], T[9], T[10]]]
    return rot_to_quat(m) + [T[3], T[7], T[11]]


def affine_mul(A, B):
    """A o B as 4x4 matrices whose last row is 0 0 0 1, every sum in index order k = 0..3"""
    C = [0.0] * 12
    for i in range(3):
        for j in range(4):
            b3 = 1.0 if j == 3 else 0.0
            C[4 * i + j] = ((A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]) + A[4 * i + 3] * b3
    return C


def pose_inverse(T):
    """Twc of KeyFrame::SetPose: Rwc = Rcw^T, Ow = -(Rwc tcw)"""
    W = [0.0] * 12
    for i in range(3):
        for j in range(3):
            W[4 * i + j] = T[4 * j + i]
        W[4 * i + 3] = -((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11])
    return W


def apply34(T, x):
    return [((T[4 * i] * x[0] + T[4 * i + 1] * x[1]) + T[4 * i + 2] * x[2]) + T[4 * i + 3] for i in range(3)]


def s3_rot_scale(q, p):
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    cx = 2 * (q[1] * p[2] - q[2] * p[1]); cy = 2 * (q[2] * p[0] - q[0] * p[2]); cz = 2 * (q[0] * p[1] - q[1] * p[0])
    return [n2 * p[0] + (q[3] * cx + (q[1] * cz - q[2] * cy)),
            n2 * p[1] + (q[3] * cy + (q[2] * cx - q[0] * cz)),
            n2 * p[2] + (q[3] * cz + (q[0] * cy - q[1] * cx))]


def s3_act(S, p):
    o = s3_rot_scale(S, p)
    return [o[0] + S[4], o[1] + S[5], o[2] + S[6]]


def s3_inverse(S):
    n2 = S[0] * S[0] + S[1] * S[1] + S[2] * S[2] + S[3] * S[3]
    q = [-S[0] / n2, -S[1] / n2, -S[2] / n2, S[3] / n2]
    t = s3_rot_scale(q, S[4:7])
    return q + [-t[0], -t[1], -t[2]]


def s3_mul(A, B):
    t = s3_rot_scale(A, B[4:7])
    x = A[3] * B[0] + A[0] * B[3] + A[1] * B[2] - A[2] * B[1]
    y = A[3] * B[1] + A[1] * B[3] + A[2] * B[0] - A[0] * B[2]
    z = A[3] * B[2] + A[2] * B[3] + A[0] * B[1] - A[1] * B[0]
    w = A[3] * B[3] - A[0] * B[0] - A[1] * B[1] - A[2] * B[2]
    return [x, y, z, w, A[4] + t[0], A[5] + t[1], A[6] + t[2]]


def quat_to_R(q):
    x, y, z, w = q
    tx = 2 * x; ty = 2 * y; tz = 2 * z
    twx = tx * w; twy = ty * w; twz = tz * w; txx = tx * x; txy = ty * x; txz = tz * x; tyy = ty * y; tyz = tz * y; tzz = tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]


def s3_to_pose34(S):
    """[R | t / s] (csrc/sim3_math.h s3_to_pose34)"""
    s = S[0] * S[0] + S[1] * S[1] + S[2] * S[2] + S[3] * S[3]
    inv = 1.0 / math.sqrt(s)
    R = quat_to_R([S[0] * inv, S[1] * inv, S[2] * inv, S[3] * inv])
    inv_s = 1.0 / s
    T = [0.0] * 12
    for i in range(3):
        for j in range(3):
            T[4 * i + j] = R[3 * i + j]
        T[4 * i + 3] = inv_s * S[4 + i]
    return T


# ---- the reference's objects -------------------------------------------------------------------------------------------------------
class KeyFrame:
    def __init__(self, Tcw, Ow):
        self.Tcw = [float(v) for v in Tcw]
        self.Twc = pose_inverse(self.Tcw)
        self.Ow = None if Ow is None else [float(v) for v in Ow]          # (the centre the caller holds, not re-derived)

    def SetPose(self, T):
        self.Tcw = list(T)
        self.Twc = pose_inverse(self.Tcw)
        self.Ow = [self.Twc[3], self.Twc[7], self.Twc[11]]


def _keyframes(pr):
    C = pr.get("kf_center")
    return [KeyFrame(pr["kf_Tcw"][k], None if C is None else C[k]) for k in range(int(pr["nkf"]))]


def _flags(v, n):
    return [0] * n if v is None else [int(x) for x in v]


def correct_loop(pr, centres="loop", normal=None, min_max=None, nd_written=None):
    """-> dict(kf_Tcw, kf_center, X, corrected, non_corrected [nconn][7] by list position, pt_owner, counts = {n_moved, n_contested},
    normal, min_max, nd_written (None without the normal inputs; only the rows of moved points are written into the given presets)).
    centres = "old" / "new": every normal sees the centres at entry / after every SetPose - used ONLY to show that the test problems
    tell the loop's half-old, half-new centres from both."""
    nkf, npts = int(pr["nkf"]), int(pr["npts"])
    conn = [int(k) for k in pr["conn_kf"]]
    nconn = len(conn)
    rank = list(range(nconn)) if pr.get("conn_rank") is None else [int(r) for r in pr["conn_rank"]]
    Scw = [float(v) for v in pr["Scw"]]
    kfs = _keyframes(pr)
    X = [[float(v) for v in x] for x in np.asarray(pr["X"], np.float64).reshape(-1, 3)]
    bad = _flags(pr.get("pt_bad"), npts); done = _flags(pr.get("pt_done"), npts)
    nd = pr.get("obs_off") is not None
    owner = [-1] * npts
    if nd:
        normal = np.zeros((npts, 3)) if normal is None else np.array(normal, np.float64).reshape(npts, 3)
        min_max = np.zeros((npts, 2), F32) if min_max is None else np.array(min_max, F32).reshape(npts, 2)
        nd_written = np.zeros(npts, np.uint8) if nd_written is None else np.array(nd_written, np.uint8)
        sf = [F32(v) for v in pr["scale_factors"]]

    def UpdateNormalAndDepth(p):                                     # src/MapPoint.cc:335-378
        nd_written[p] = 0
        lo, hi = int(pr["obs_off"][p]), int(pr["obs_off"][p + 1])
        if hi == lo:
            return
        pos = X[p]
        n = [0.0, 0.0, 0.0]
        cnt = 0
        for e in range(lo, hi):
            Owi = kfs[int(pr["obs_kf"][e])].Ow
            v = [pos[0] - Owi[0], pos[1] - Owi[1], pos[2] - Owi[2]]
            nn = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            n = [n[0] + v[0] / nn, n[1] + v[1] / nn, n[2] + v[2] / nn]
            cnt += 1
        Ow = kfs[int(pr["ref_kf"][p])].Ow
        pc = [pos[0] - Ow[0], pos[1] - Ow[1], pos[2] - Ow[2]]
        dist = F32(math.sqrt((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]))
        mx = dist * sf[int(pr["ref_level"][p])]
        min_max[p, 0] = mx / sf[len(sf) - 1]
        min_max[p, 1] = mx
        normal[p] = [n[0] / float(cnt), n[1] / float(cnt), n[2] / float(cnt)]
        nd_written[p] = 1

    cur = conn[nconn - 1]
    corrected, non_corrected = {}, {}                                 # std::map<KeyFrame*, Sim3>: key = the pointer's rank
    pos_of_rank = {}
    corrected[rank[nconn - 1]] = Scw
    Twc = kfs[cur].Twc
    for c, k in enumerate(conn):                                      # :446-469
        Tiw = kfs[k].Tcw
        if k != cur:
            Tic = affine_mul(Tiw, Twc)
            corrected[rank[c]] = s3_mul(se3_as_sim3(Tic), Scw)
        non_corrected[rank[c]] = se3_as_sim3(Tiw)
        pos_of_rank[rank[c]] = c
    new_poses = {}
    if centres == "new":
        for r in corrected:
            kfs[conn[pos_of_rank[r]]].SetPose(s3_to_pose34(corrected[r]))
    for r in sorted(corrected):                                       # :473-523, in the map's order
        c = pos_of_rank[r]; k = conn[c]
        Swi = s3_inverse(corrected[r])
        Siw = non_corrected[r]
        for s in range(int(pr["slot_off"][c]), int(pr["slot_off"][c + 1])):
            p = int(pr["slot_pt"][s])
            if p < 0 or bad[p] or done[p]:
                continue
            X[p] = s3_act(Swi, s3_act(Siw, X[p]))
            done[p] = 1
            owner[p] = k
            if nd:
                UpdateNormalAndDepth(p)
        new_poses[k] = s3_to_pose34(corrected[r])
        if centres == "loop":
            kfs[k].SetPose(new_poses[k])
    if centres != "loop":
        for k, T in new_poses.items():
            kfs[k].SetPose(T)
    listed = [set() for _ in range(npts)]
    for c in range(nconn):
        for s in range(int(pr["slot_off"][c]), int(pr["slot_off"][c + 1])):
            if int(pr["slot_pt"][s]) >= 0:
                listed[int(pr["slot_pt"][s])].add(c)
    n_moved = sum(o >= 0 for o in owner)
    n_cont = sum(owner[p] >= 0 and len(listed[p]) >= 2 for p in range(npts))
    have_c = pr.get("kf_center") is not None
    return dict(kf_Tcw=np.array([kf.Tcw for kf in kfs], np.float64).reshape(nkf, 12),
                kf_center=np.array([kf.Ow for kf in kfs], np.float64).reshape(nkf, 3) if have_c else None,
                X=np.array(X, np.float64).reshape(npts, 3),
                corrected=np.array([corrected[rank[c]] for c in range(nconn)], np.float64), non_corrected=np.array([non_corrected[rank[c]] for c in range(nconn)], np.float64),
                pt_owner=np.array(owner, np.int32), counts=np.array([n_moved, n_cont], np.int32),
                normal=normal if nd else None, min_max=min_max if nd else None, nd_written=nd_written if nd else None)


def propagate_global_ba(pr, kf_bef_Tcw=None):
    """-> dict(kf_Tcw, kf_gba_Tcw, kf_in_gba, kf_center, X, kf_bef_Tcw (rows of unreached keyframes keep the preset), kf_reached, pt_moved,
    counts = {n_reached, n_propagated, n_points_moved, n_stale}, depth = the longest run of keyframes outside the BA the walk crossed)"""
    nkf, npts = int(pr["nkf"]), int(pr["npts"])
    kfs = _keyframes(pr)
    gba = [[float(v) for v in g] for g in np.asarray(pr["kf_gba_Tcw"], np.float64).reshape(nkf, 12)]
    flag = [int(v) for v in pr["kf_in_gba"]]
    flag_in = list(flag)
    children = [[] for _ in range(nkf)]
    for k in range(nkf):
        if int(pr["kf_parent"][k]) >= 0:
            children[int(pr["kf_parent"][k])].append(k)
    bef = np.zeros((nkf, 12)) if kf_bef_Tcw is None else np.array(kf_bef_Tcw, np.float64).reshape(nkf, 12)
    reached = [0] * nkf
    run = [0] * nkf
    n_prop = 0
    todo = deque(int(k) for k in pr["origin_kf"])                     # :682-703
    while todo:
        k = todo[0]
        Twc = kfs[k].Twc
        for child in children[k]:
            if not flag[child]:
                Tchildc = affine_mul(kfs[child].Tcw, Twc)
                gba[child] = affine_mul(Tchildc, gba[k])
                flag[child] = 1
                n_prop += 1
                run[child] = run[k] + 1
            todo.append(child)
        bef[k] = kfs[k].Tcw
        kfs[k].SetPose(gba[k])
        reached[k] = 1
        todo.popleft()
    X = [[float(v) for v in x] for x in np.asarray(pr["X"], np.float64).reshape(-1, 3)]
    bad = _flags(pr.get("pt_bad"), npts); pin = _flags(pr.get("pt_in_gba"), npts)
    moved = [0] * npts
    n_stale = 0
    for p in range(npts):                                             # :708-739
        if bad[p]:
            continue
        if pin[p]:
            X[p] = [float(v) for v in pr["pt_gba_X"][p]]
            moved[p] = 1
            continue
        r = int(pr["pt_ref_kf"][p])
        if not flag[r]:
            continue
        if not reached[r]:                                            # (the stated departure: the reference would read a stale global_BA_Bef_Tcw_)
            n_stale += 1
            continue
        Xc = apply34([float(v) for v in bef[r]], X[p])
        X[p] = apply34(kfs[r].Twc, Xc)
        moved[p] = 2
    have_c = pr.get("kf_center") is not None
    return dict(kf_Tcw=np.array([kf.Tcw for kf in kfs], np.float64).reshape(nkf, 12), kf_gba_Tcw=np.array(gba, np.float64).reshape(nkf, 12),
                kf_in_gba=np.array(flag, np.uint8), kf_center=np.array([kf.Ow for kf in kfs], np.float64).reshape(nkf, 3) if have_c else None,
                X=np.array(X, np.float64).reshape(npts, 3), kf_bef_Tcw=bef, kf_reached=np.array(reached, np.uint8), pt_moved=np.array(moved, np.uint8),
                counts=np.array([sum(reached), n_prop, sum(m != 0 for m in moved), n_stale], np.int32), depth=max(run) if nkf else 0,
                flag_in=np.array(flag_in, np.uint8))
