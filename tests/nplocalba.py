"""Restatement of the two halves of CeresOptimizer::LocalBundleAdjustment around the optimisation over the flattened tables of
orbl_local_ba_assemble and orbl_local_ba_apply: the LITERAL loops of src/CeresOptimizer.cc:346-406, :423-506 and :573-598 with
MapPoint::EraseObservation / SetBadFlag (src/MapPoint.cc:140-191), UpdateNormalAndDepth (:335-378) and KeyFrame::EraseMapPointMatch
(src/KeyFrame.cc:250-260) over Python objects - stamps on the keyframes, containers iterated in rank order, one observation erased after
the other - TEST INFRASTRUCTURE, independent of the scans and per-point walks the kernels use.  Every operation is a float64 scalar (a
Python float) in the order of the pose codec (tests/npmapcorrect.py rot_to_quat, quat_to_R, pose_inverse) and k_mp_prep; the float32 steps
of the depth range are numpy float32 scalars.

map: dict(nkf, npts, cur_kf, nbr_kf, kf_id, kf_bad | None, kf_rank | None, kf_Tcw[nkf][12], kf_K4[nkf][4], kf_slot_off, kf_slot_pt, X,
pt_bad | None, pt_rank | None, obs_off, obs_kf, obs_uv[nobs][2] float32, obs_level, inv_level_sigma2, and for apply: kf_center, pt_nobs,
pt_ref_kf, obs_slot, kf_level0 | None, scale_factors)."""
import math

import numpy as np

from tests import npmapcorrect as npm

F32 = np.float32


def _flags(v, n):
    return [0] * n if v is None else [int(x) for x in v]


def _ranks(v, n):
    return list(range(n)) if v is None else [int(x) for x in v]


def matrix4d_to_pose7(T):
    """MatEigenConverter::Matrix4dToMatrix_7_1: [t, Eigen::Quaterniond(R).coeffs()]"""
    q = npm.rot_to_quat([[T[0], T[1], T[2]], [T[4], T[5], T[6]], [T[8], T[9], T[10]]])
    return [T[3], T[7], T[11]] + q


def pose7_to_pose34(s):
    """Matrix_7_1_ToMatrix4d: q.normalized().toRotationMatrix(), the first three rows"""
    n = math.sqrt(((s[3] * s[3] + s[4] * s[4]) + s[5] * s[5]) + s[6] * s[6])
    R = npm.quat_to_R([s[3] / n, s[4] / n, s[5] / n, s[6] / n])
    T = [0.0] * 12
    for i in range(3):
        T[4 * i:4 * i + 3] = R[3 * i:3 * i + 3]
        T[4 * i + 3] = s[i]
    return T


def assemble(m, order="rank"):
    """-> dict(counts, cam_kf, K4, poses7, cam_fixed, cam_local, lpt_pt, pts3, lobs_cam, lobs_pt, lobs_uv, lobs_inv_sigma2, lobs_src, kf_role,
    pt_local).  order="index": the ORDER-BLIND variant that ignores kf_rank and pt_rank - used only to show that the test maps tell the
    containers' order from it."""
    nkf, npts = int(m["nkf"]), int(m["npts"])
    cur = int(m["cur_kf"])
    kbad = _flags(m.get("kf_bad"), nkf); pbad = _flags(m.get("pt_bad"), npts)
    krank = _ranks(m.get("kf_rank") if order == "rank" else None, nkf); prank = _ranks(m.get("pt_rank") if order == "rank" else None, npts)
    kid = [int(v) for v in m["kf_id"]]
    so, sp, oo, ok = m["kf_slot_off"], m["kf_slot_pt"], m["obs_off"], m["obs_kf"]
    stamp_local = [False] * nkf; stamp_fixed = [False] * nkf; pt_stamp = [False] * npts
    local_kfs = [cur]                                                 # (:348-363) the collection order
    stamp_local[cur] = True
    for k in (int(v) for v in m["nbr_kf"]):
        stamp_local[k] = True
        if not kbad[k] and k not in local_kfs:
            local_kfs.append(k)
    local_pts = []                                                    # (:366-384)
    for k in local_kfs:
        for s in range(int(so[k]), int(so[k + 1])):
            p = int(sp[s])
            if p >= 0 and not pbad[p] and not pt_stamp[p]:
                pt_stamp[p] = True
                local_pts.append(p)
    local_pts.sort(key=lambda p: prank[p])                            # (std::map<MapPoint*, ...>)
    fixed = []                                                        # (:388-406)
    for p in local_pts:
        for e in range(int(oo[p]), int(oo[p + 1])):
            k = int(ok[e])
            if not stamp_local[k] and not stamp_fixed[k]:
                stamp_fixed[k] = True
                if not kbad[k]:
                    fixed.append(k)
    fixed.sort(key=lambda k: krank[k])                                # (std::map<KeyFrame*, ...>)
    cams = sorted(local_kfs, key=lambda k: kid[k]) + fixed            # (stable: ties keep the collection order)
    cam_of = {k: c for c, k in enumerate(cams)}
    n_local = len(local_kfs)
    poses7 = [matrix4d_to_pose7([float(v) for v in m["kf_Tcw"][k]]) for k in cams]
    rows = []
    for j, p in enumerate(local_pts):                                 # (:423-506)
        for e in range(int(oo[p]), int(oo[p + 1])):
            k = int(ok[e])
            if kbad[k] or k not in cam_of:
                continue
            rows.append((cam_of[k], j, float(m["obs_uv"][e][0]), float(m["obs_uv"][e][1]), m["inv_level_sigma2"][int(m["obs_level"][e])], e))
    role = [0] * nkf
    for k in range(nkf):
        role[k] = (1 if k in cam_of and cam_of[k] < n_local else 3) if stamp_local[k] else (2 if k in cam_of else 0)
    return dict(counts=np.array([len(cams), n_local, len(local_pts), len(rows)], np.int32), cam_kf=np.array(cams, np.int32),
                K4=np.array([m["kf_K4"][k] for k in cams], np.float64).reshape(-1, 4), poses7=np.array(poses7, np.float64).reshape(-1, 7),
                cam_fixed=np.array([1 if (c >= n_local or kid[k] == 0) else 0 for c, k in enumerate(cams)], np.uint8),
                cam_local=np.array([1 if c < n_local else 0 for c in range(len(cams))], np.uint8), lpt_pt=np.array(local_pts, np.int32),
                pts3=np.array([m["X"][p] for p in local_pts], np.float64).reshape(-1, 3), lobs_cam=np.array([r[0] for r in rows], np.int32),
                lobs_pt=np.array([r[1] for r in rows], np.int32), lobs_uv=np.array([[r[2], r[3]] for r in rows], np.float64).reshape(-1, 2),
                lobs_inv_sigma2=np.array([r[4] for r in rows], np.float32), lobs_src=np.array([r[5] for r in rows], np.int32),
                kf_role=np.array(role, np.uint8), pt_local=np.array([1 if s else 0 for s in pt_stamp], np.uint8))


def apply(m, asm, poses7, pts3, obs_erase, blind=False, normals=True, normal=None, min_max=None, nd_written=None):
    """-> dict(kf_Tcw, kf_center, kf_slot_pt, X, pt_bad, pt_nobs, pt_ref_kf, obs_erased, normal, min_max, nd_written, counts, diag).  Only the
    rows of points with a new normal are written into the given presets (nd_written wholly).  diag = {ref_moved, dead_rows, turned_bad}:
    what the test maps must contain.  blind=True: the ORDER-BLIND variant - every erase row scored against the state at entry, the normals
    from the centres at entry."""
    nkf, npts = int(m["nkf"]), int(m["npts"])
    oo, ok = m["obs_off"], m["obs_kf"]
    nobs = len(ok)
    Tcw = [[float(v) for v in T] for T in np.asarray(m["kf_Tcw"], np.float64).reshape(nkf, 12)]
    have_c = m.get("kf_center") is not None
    Ow = [[float(v) for v in c] for c in np.asarray(m["kf_center"], np.float64).reshape(nkf, 3)] if have_c else [None] * nkf
    Ow_entry = [None if c is None else list(c) for c in Ow]
    slots = [int(v) for v in m["kf_slot_pt"]]
    X = [[float(v) for v in x] for x in np.asarray(m["X"], np.float64).reshape(npts, 3)]
    bad = _flags(m.get("pt_bad"), npts); n_obs = [int(v) for v in m["pt_nobs"]]; ref = [int(v) for v in m["pt_ref_kf"]]
    alive = [True] * nobs
    point_of = [0] * nobs
    for p in range(npts):
        for e in range(int(oo[p]), int(oo[p + 1])):
            point_of[e] = p
    n_erased = n_dead = 0
    diag = dict(ref_moved=0, dead_rows=0, turned_bad=0)

    def EraseMapPointMatch(e):                                        # KeyFrame::EraseMapPointMatch(index)
        slots[int(m["kf_slot_off"][int(ok[e])]) + int(m["obs_slot"][e])] = -1

    def kill(e):
        nonlocal n_dead
        alive[e] = False
        EraseMapPointMatch(e)
        n_dead += 1

    def SetBadFlag(p):                                                # src/MapPoint.cc:174-188
        bad[p] = 1
        diag["turned_bad"] += 1
        for e in range(int(oo[p]), int(oo[p + 1])):
            if alive[e]:
                kill(e)

    if blind:
        hit = sorted({int(asm["lobs_src"][i]) for i in range(len(asm["lobs_src"])) if obs_erase[i]})
        for e in hit:
            kill(e); n_erased += 1; n_obs[point_of[e]] -= 1
        for p in sorted({point_of[e] for e in hit}):
            left = [e for e in range(int(oo[p]), int(oo[p + 1])) if alive[e]]
            if any(int(ok[e]) == ref[p] for e in hit if point_of[e] == p) and left:
                ref[p] = int(ok[left[0]])
            if n_obs[p] <= 2:
                SetBadFlag(p)
    else:
        for i in range(len(asm["lobs_src"])):                         # (:574-581) one row after the other
            if not obs_erase[i]:
                continue
            e = int(asm["lobs_src"][i]); k = int(ok[e]); p = point_of[e]
            if not alive[e]:                                          # GetIndexInKeyFrame == -1, observations_.count() == 0
                diag["dead_rows"] += 1
                continue
            kill(e)                                                   # keyframe->EraseMapPointMatch(map_point); then EraseObservation (:144-151)
            n_erased += 1
            n_obs[p] -= 1
            if ref[p] == k:                                           # (:153-154; stays when the map is empty: the stated departure)
                left = [f for f in range(int(oo[p]), int(oo[p + 1])) if alive[f]]
                if left:
                    ref[p] = int(ok[left[0]])
                    diag["ref_moved"] += 1
            if n_obs[p] <= 2:                                         # (:157-161)
                SetBadFlag(p)
    for c in range(len(asm["cam_kf"])):                               # (:585-591)
        if asm["cam_local"][c]:
            k = int(asm["cam_kf"][c])
            Tcw[k] = pose7_to_pose34([float(v) for v in poses7[c]])
            if have_c:
                Twc = npm.pose_inverse(Tcw[k])
                Ow[k] = [Twc[3], Twc[7], Twc[11]]
    centres = Ow_entry if blind else Ow
    if normals:
        normal = np.zeros((npts, 3)) if normal is None else np.array(normal, np.float64).reshape(npts, 3)
        min_max = np.zeros((npts, 2), F32) if min_max is None else np.array(min_max, F32).reshape(npts, 2)
        nd_written = np.zeros(npts, np.uint8)
        sf = [F32(v) for v in m["scale_factors"]]
    n_normals = 0
    for j, p in enumerate(int(v) for v in asm["lpt_pt"]):             # (:593-598)
        X[p] = [float(v) for v in pts3[j]]                            # SetWorldPos
        if not normals or bad[p]:                                     # UpdateNormalAndDepth (src/MapPoint.cc:342)
            continue
        es = [e for e in range(int(oo[p]), int(oo[p + 1])) if alive[e]]
        if not es:                                                    # (:348)
            continue
        pos = X[p]
        n = [0.0, 0.0, 0.0]
        level = None
        for e in es:
            O = centres[int(ok[e])]
            v = [pos[0] - O[0], pos[1] - O[1], pos[2] - O[2]]
            nn = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            n = [n[0] + v[0] / nn, n[1] + v[1] / nn, n[2] + v[2] / nn]
            if int(ok[e]) == ref[p]:
                level = int(m["obs_level"][e])
        if level is None:                                             # (:366: operator[] on the copy inserts index 0)
            level = 0 if m.get("kf_level0") is None else int(m["kf_level0"][ref[p]])
        O = centres[ref[p]]
        pc = [pos[0] - O[0], pos[1] - O[1], pos[2] - O[2]]
        dist = F32(math.sqrt((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]))
        mx = dist * sf[level]
        min_max[p, 0] = mx / sf[len(sf) - 1]
        min_max[p, 1] = mx
        cnt = float(len(es))
        normal[p] = [n[0] / cnt, n[1] / cnt, n[2] / cnt]
        nd_written[p] = 1
        n_normals += 1
    return dict(kf_Tcw=np.array(Tcw, np.float64).reshape(nkf, 12), kf_center=np.array(Ow, np.float64).reshape(nkf, 3) if have_c else None,
                kf_slot_pt=np.array(slots, np.int32), X=np.array(X, np.float64).reshape(npts, 3), pt_bad=np.array(bad, np.uint8), pt_nobs=np.array(n_obs, np.int32),
                pt_ref_kf=np.array(ref, np.int32), obs_erased=np.array([0 if a else 1 for a in alive], np.uint8), normal=normal if normals else None,
                min_max=min_max if normals else None, nd_written=nd_written if normals else None,
                counts=np.array([n_erased, diag["turned_bad"], n_dead, n_normals], np.int32), diag=diag)
