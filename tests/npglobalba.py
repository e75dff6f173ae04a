"""Restatement of the two halves of CeresOptimizer::BundleAdjustment (GlobalBundleAdjustemnt) around the optimisation over the flattened
tables of orbl_global_ba_assemble and orbl_global_ba_apply: the LITERAL loops of src/CeresOptimizer.cc:59-176 and :190-224 in the reading
csrc/compat/orbslam_dropin.h fixed (cameras by keyframe id through a stable sort, an observer outside `keyframes` gives no row, a point
without rows is left out) with MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:335-378) over Python containers - a dict of cameras, one
keyframe and one point after the other - TEST INFRASTRUCTURE, independent of the stamps, the all-pairs count and the scans the kernels use.
Every floating operation is a float64 scalar (a Python float) in the order of the pose codec (tests/npmapcorrect.py rot_to_quat,
quat_to_R, pose_inverse) and k_mp_prep; the float32 steps of the depth range are numpy float32 scalars.

map: dict(nkf, npts, ba_kf | None, ba_pt | None, kf_id, kf_bad | None, kf_Tcw[nkf][12], kf_K4[nkf][4], X, pt_bad | None, obs_off, obs_kf,
obs_uv[nobs][2] float32, obs_level, inv_level_sigma2, and for apply: kf_center | None, pt_ref_kf, ref_level, scale_factors, and the presets
kf_gba_Tcw | None, pt_gba_X | None of stage 1)."""
import math

import numpy as np

from tests import npmapcorrect as npm
from tests.nplocalba import matrix4d_to_pose7, pose7_to_pose34

F32 = np.float32


def _flags(v, n):
    return [0] * n if v is None else [int(x) for x in v]


def _list(v, n):
    return list(range(n)) if v is None else [int(x) for x in v]


def assemble(m, is_robust=True, blind=False):
    """-> dict(counts, cam_kf, kf_cam, K4, poses7, cam_fixed, gpt_pt, pt_idx, pts3, gobs_cam, gobs_pt, gobs_uv, gobs_weight, gobs_robust,
    gobs_src).  blind=True: the ORDER-BLIND variant - cameras in list order, points in index order, points without rows kept - used only to
    show that the test maps tell the stated order from it."""
    nkf, npts = int(m["nkf"]), int(m["npts"])
    keyframes = _list(m.get("ba_kf"), nkf); map_points = _list(m.get("ba_pt"), npts)
    kbad = _flags(m.get("kf_bad"), nkf); pbad = _flags(m.get("pt_bad"), npts)
    kid = [int(v) for v in m["kf_id"]]
    oo, ok = m["obs_off"], m["obs_kf"]
    cam_of, cams = {}, []                                             # ided_keyframe_pose (:75), in the drop-in's order
    kf_by_id = list(keyframes) if blind else sorted(keyframes, key=lambda k: kid[k])      # (sorted() is stable: std::stable_sort)
    for k in kf_by_id:                                                # (:87-121)
        if kbad[k]:
            continue
        if k in cam_of:
            continue
        cam_of[k] = len(cams)
        cams.append(k)
    poses7 = [matrix4d_to_pose7([float(v) for v in m["kf_Tcw"][k]]) for k in cams]
    pt_of, gpt, rows = {}, [], []
    seen = set()
    for p in (sorted(map_points) if blind else map_points):           # (:128-176)
        if p in seen:                                                 # (Map holds a std::set; the device form takes the first position)
            continue
        seen.add(p)
        if pbad[p]:
            continue
        pid = len(gpt)
        n_edges = 0
        for e in range(int(oo[p]), int(oo[p + 1])):
            k = int(ok[e])
            if kbad[k]:                                               # (:142; id_ > max_keyframe_id cannot hold for a camera)
                continue
            if k not in cam_of:                                       # (dropin :831)
                continue
            n_edges += 1
            rows.append((cam_of[k], pid, float(m["obs_uv"][e][0]), float(m["obs_uv"][e][1]), float(F32(m["inv_level_sigma2"][int(m["obs_level"][e])])), e))
        if n_edges == 0 and not (blind and cams):                     # (:170-172)
            continue
        pt_of[p] = pid
        gpt.append(p)
    return dict(counts=np.array([len(cams), len(gpt), len(rows)], np.int32), cam_kf=np.array(cams, np.int32),
                kf_cam=np.array([cam_of.get(k, -1) for k in range(nkf)], np.int32), K4=np.array([m["kf_K4"][k] for k in cams], np.float64).reshape(-1, 4),
                poses7=np.array(poses7, np.float64).reshape(-1, 7), cam_fixed=np.array([1 if kid[k] == 0 else 0 for k in cams], np.uint8),
                gpt_pt=np.array(gpt, np.int32), pt_idx=np.array([pt_of.get(p, -1) for p in range(npts)], np.int32),
                pts3=np.array([m["X"][p] for p in gpt], np.float64).reshape(-1, 3), gobs_cam=np.array([r[0] for r in rows], np.int32),
                gobs_pt=np.array([r[1] for r in rows], np.int32), gobs_uv=np.array([[r[2], r[3]] for r in rows], np.float64).reshape(-1, 2),
                gobs_weight=np.array([r[4] for r in rows], np.float64), gobs_robust=np.full(len(rows), 1 if is_robust else 0, np.uint8),
                gobs_src=np.array([r[5] for r in rows], np.int32))


def apply(m, cam_kf, gpt_pt, poses7, pts3, stage=0, normals=True, normal=None, min_max=None, nd_written=None):
    """-> stage 0: dict(kf_Tcw, kf_center, X, normal, min_max, nd_written, counts); stage 1: dict(kf_gba_Tcw, kf_in_gba, pt_gba_X, pt_in_gba,
    counts).  kf_bad / pt_bad of m are the flags at the time of the write-back.  Only the rows of points with a new normal are written into
    the given presets (nd_written wholly); the rows of kf_gba_Tcw / pt_gba_X that are not written keep m's presets (zeros without)."""
    nkf, npts = int(m["nkf"]), int(m["npts"])
    kbad = _flags(m.get("kf_bad"), nkf); pbad = _flags(m.get("pt_bad"), npts)
    oo, ok = m["obs_off"], m["obs_kf"]
    poses7 = np.asarray(poses7, np.float64).reshape(-1, 7); pts3 = np.asarray(pts3, np.float64).reshape(-1, 3)
    pose_of, pos_of = {}, {}
    for c, k in enumerate(int(v) for v in cam_kf):                    # (:190-205) one keyframe after the other; a later entry overwrites
        if kbad[k]:
            continue
        pose_of[k] = pose7_to_pose34([float(v) for v in poses7[c]])
    for j, p in enumerate(int(v) for v in gpt_pt):                    # (:208-224)
        if pbad[p]:
            continue
        pos_of[p] = [float(v) for v in pts3[j]]
    if stage:
        gT = np.zeros((nkf, 12)) if m.get("kf_gba_Tcw") is None else np.array(m["kf_gba_Tcw"], np.float64).reshape(nkf, 12)
        gX = np.zeros((npts, 3)) if m.get("pt_gba_X") is None else np.array(m["pt_gba_X"], np.float64).reshape(npts, 3)
        for k, T in pose_of.items():
            gT[k] = T
        for p, x in pos_of.items():
            gX[p] = x
        return dict(kf_gba_Tcw=gT, kf_in_gba=np.array([1 if k in pose_of else 0 for k in range(nkf)], np.uint8), pt_gba_X=gX,
                    pt_in_gba=np.array([1 if p in pos_of else 0 for p in range(npts)], np.uint8), counts=np.array([len(pose_of), len(pos_of), 0], np.int32))
    Tcw = [[float(v) for v in T] for T in np.asarray(m["kf_Tcw"], np.float64).reshape(nkf, 12)]
    have_c = m.get("kf_center") is not None
    Ow = [[float(v) for v in c] for c in np.asarray(m["kf_center"], np.float64).reshape(nkf, 3)] if have_c else [None] * nkf
    X = [[float(v) for v in x] for x in np.asarray(m["X"], np.float64).reshape(npts, 3)]
    for k, T in pose_of.items():                                      # SetPose: every one precedes the point loop
        Tcw[k] = T
        if have_c:
            Twc = npm.pose_inverse(T)
            Ow[k] = [Twc[3], Twc[7], Twc[11]]
    if normals:
        normal = np.zeros((npts, 3)) if normal is None else np.array(normal, np.float64).reshape(npts, 3)
        min_max = np.zeros((npts, 2), F32) if min_max is None else np.array(min_max, F32).reshape(npts, 2)
        nd_written = np.zeros(npts, np.uint8)
        sf = [F32(v) for v in m["scale_factors"]]
    n_normals = 0
    for p in sorted(pos_of):
        X[p] = pos_of[p]                                              # SetWorldPos
        if not normals:
            continue
        es = list(range(int(oo[p]), int(oo[p + 1])))                  # UpdateNormalAndDepth: the whole list, bad keyframes included
        ref = int(m["pt_ref_kf"][p])
        if not es or ref == -1:                                       # (src/MapPoint.cc:348)
            continue
        pos = X[p]
        n = [0.0, 0.0, 0.0]
        for e in es:
            O = Ow[int(ok[e])]
            v = [pos[0] - O[0], pos[1] - O[1], pos[2] - O[2]]
            nn = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            n = [n[0] + v[0] / nn, n[1] + v[1] / nn, n[2] + v[2] / nn]
        O = Ow[ref]
        pc = [pos[0] - O[0], pos[1] - O[1], pos[2] - O[2]]
        dist = F32(math.sqrt((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]))
        mx = dist * sf[int(m["ref_level"][p])]
        min_max[p, 0] = mx / sf[len(sf) - 1]
        min_max[p, 1] = mx
        cnt = float(len(es))
        normal[p] = [n[0] / cnt, n[1] / cnt, n[2] / cnt]
        nd_written[p] = 1
        n_normals += 1
    return dict(kf_Tcw=np.array(Tcw, np.float64).reshape(nkf, 12), kf_center=np.array(Ow, np.float64).reshape(nkf, 3) if have_c else None,
                X=np.array(X, np.float64).reshape(npts, 3), normal=normal if normals else None, min_max=min_max if normals else None,
                nd_written=nd_written if normals else None, counts=np.array([len(pose_of), len(pos_of), n_normals], np.int32))
