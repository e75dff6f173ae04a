"""Test maps for orbl_global_ba_assemble and orbl_global_ba_apply (tests/npglobalba.py states the dict layout): hand-worked cases whose
expected outputs are written here, and a seeded generator.  TEST INFRASTRUCTURE.

The hand cases use axis-parallel poses ([I | t]) and solver results with q = (0, 0, 0, 2), so that every figure is exact and can be
followed on paper: the new pose is [I | t] and the new centre -t."""
import numpy as np

from tests.mapcorrectcases import POISON, SF, _centre, _csr, _pose, _rand_pose  # noqa: F401

ISG = np.array([1.0 / 1.44 ** i for i in range(8)], np.float32)
K4 = (458.654, 457.296, 367.215, 248.375)


def table_map(Tcw, kf_id, X, obs, ba_kf=None, ba_pt=None, kf_bad=None, pt_bad=None, obs_uv=None, obs_level=None, pt_ref_kf=None, ref_level=None, kf_K4=None):
    """obs: per point its observers in list order"""
    Tcw = np.ascontiguousarray(Tcw, np.float64).reshape(-1, 12)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    nkf, npts = len(Tcw), len(X)
    oo, ok = _csr(obs)
    nobs = len(ok)
    if obs_uv is None:
        obs_uv = [[100.0 + e, 50.0 + 2 * e] for e in range(nobs)]
    if obs_level is None:
        obs_level = [e % 8 for e in range(nobs)]
    if pt_ref_kf is None:
        pt_ref_kf = [o[0] if o else -1 for o in obs]
    if ref_level is None:
        ref_level = [p % 8 for p in range(npts)]
    return dict(nkf=nkf, npts=npts, ba_kf=None if ba_kf is None else np.array(ba_kf, np.int32), ba_pt=None if ba_pt is None else np.array(ba_pt, np.int32),
                kf_id=np.array(kf_id, np.int32), kf_bad=None if kf_bad is None else np.array(kf_bad, np.uint8), kf_Tcw=Tcw,
                kf_K4=np.tile(np.array(K4), (nkf, 1)) if kf_K4 is None else np.ascontiguousarray(kf_K4, np.float64).reshape(nkf, 4), X=X,
                pt_bad=None if pt_bad is None else np.array(pt_bad, np.uint8), obs_off=oo, obs_kf=ok, obs_uv=np.array(obs_uv, np.float32).reshape(-1, 2),
                obs_level=np.array(obs_level, np.int32), inv_level_sigma2=ISG.copy(), kf_center=np.array([_centre(T) for T in Tcw]).reshape(nkf, 3),
                pt_ref_kf=np.array(pt_ref_kf, np.int32), ref_level=np.array(ref_level, np.int32), scale_factors=SF.copy())


# ---- hand cases: assemble -----------------------------------------------------------------------------------------------------------
def _hand(**kw):
    # keyframes 0..5 at t = (k, 0, 0) with ids out of index order and larger than nkf; 1 and 4 share id 7; 3 has id 0; 5 is bad.  The list
    # names 2 twice, the bad 5, and leaves 0 out.  Observations e: p0 = {0: kf0, 1: kf1, 2: kf2}, p1 = {3: kf5}, p2 = {4: kf1} (bad point),
    # p3 = {5: kf3, 6: kf4, 7: kf5}, p4 = {8: kf0}, p5 = {}, p6 = {9: kf2, 10: kf4}
    a = dict(Tcw=[_pose((k, 0.0, 0.0)) for k in range(6)], kf_id=[50, 7, 1000, 0, 7, 20], kf_bad=[0, 0, 0, 0, 0, 1], ba_kf=[4, 2, 1, 5, 3, 2],
             X=[(p, 1.0, 2.0) for p in range(7)], obs=[[0, 1, 2], [5], [1], [3, 4, 5], [0], [], [2, 4]], pt_bad=[0, 0, 1, 0, 0, 0, 0])
    a.update(kw)
    return table_map(**a)


def hand_assemble_cases():
    """name -> (map, is_robust, the outputs worked by hand)"""
    c = {}
    # cameras by id: 3 (id 0, fixed), then id 7 twice: 4 (list position 0) before 1 (position 2), then 2 (id 1000, its first position counts).
    # p0 keeps the rows of keyframes 1 and 2 (0 is outside the list); p1 has a bad observer only; p2 is bad; p3 loses the bad 5; p4's
    # only observer is outside the list; p5 has no observations
    base = dict(counts=[4, 3, 6], cam_kf=[3, 4, 1, 2], kf_cam=[-1, 2, 3, 0, 1, -1], cam_fixed=[1, 0, 0, 0], gpt_pt=[0, 3, 6], pt_idx=[0, -1, -1, 1, -1, -1, 2],
                gobs_cam=[2, 3, 0, 1, 3, 1], gobs_pt=[0, 0, 1, 1, 2, 2], gobs_src=[1, 2, 5, 6, 9, 10], gobs_robust=[1] * 6,
                gobs_weight=[float(ISG[i]) for i in (1, 2, 5, 6, 1, 2)], gobs_uv=[[100.0 + e, 50.0 + 2 * e] for e in (1, 2, 5, 6, 9, 10)],
                pts3=[(0.0, 1.0, 2.0), (3.0, 1.0, 2.0), (6.0, 1.0, 2.0)], poses7=[[k, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0] for k in (3.0, 4.0, 1.0, 2.0)])
    c["ids out of index order, equal ids, a bad and a repeated keyframe in the list, an observer outside it, points without rows"] = (_hand(), 1, base)
    c["not robust"] = (_hand(), 0, dict(base, gobs_robust=[0] * 6))
    c["a map without id 0"] = (_hand(kf_id=[50, 7, 1000, 3, 7, 20]), 1, dict(base, cam_fixed=[0, 0, 0, 0]))
    c["ba_pt a permuted subset"] = (_hand(ba_pt=[6, 1, 0]), 1, dict(
        counts=[4, 2, 4], cam_kf=[3, 4, 1, 2], kf_cam=[-1, 2, 3, 0, 1, -1], cam_fixed=[1, 0, 0, 0], gpt_pt=[6, 0], pt_idx=[1, -1, -1, -1, -1, -1, 0],
        gobs_cam=[3, 1, 2, 3], gobs_pt=[0, 0, 1, 1], gobs_src=[9, 10, 1, 2], gobs_robust=[1] * 4, gobs_weight=[float(ISG[i]) for i in (1, 2, 1, 2)],
        pts3=[(6.0, 1.0, 2.0), (0.0, 1.0, 2.0)]))
    # every nullable input left out: all six keyframes (5 is no longer bad) and all seven points (2 is no longer bad); 1 before 4 now
    c["every nullable input left out"] = (_hand(ba_kf=None, kf_bad=None, pt_bad=None), 1, dict(
        counts=[6, 6, 11], cam_kf=[3, 1, 4, 5, 0, 2], kf_cam=[4, 1, 5, 0, 2, 3], cam_fixed=[1, 0, 0, 0, 0, 0], gpt_pt=[0, 1, 2, 3, 4, 6], pt_idx=[0, 1, 2, 3, 4, -1, 5],
        gobs_cam=[4, 1, 5, 3, 1, 0, 2, 3, 4, 5, 2], gobs_pt=[0, 0, 0, 1, 2, 3, 3, 3, 4, 5, 5], gobs_src=list(range(11)), gobs_robust=[1] * 11))
    empty = dict(cam_kf=[], cam_fixed=[], gpt_pt=[], gobs_cam=[], gobs_pt=[], gobs_src=[], gobs_robust=[])
    c["an empty keyframe list"] = (_hand(ba_kf=[]), 1, dict(empty, counts=[0, 0, 0], kf_cam=[-1] * 6, pt_idx=[-1] * 7))
    c["an empty point list"] = (_hand(ba_pt=[]), 1, dict(empty, counts=[4, 0, 0], cam_kf=[3, 4, 1, 2], kf_cam=[-1, 2, 3, 0, 1, -1], cam_fixed=[1, 0, 0, 0], pt_idx=[-1] * 7))
    c["only bad keyframes in the list"] = (_hand(ba_kf=[5, 5]), 1, dict(empty, counts=[0, 0, 0], kf_cam=[-1] * 6, pt_idx=[-1] * 7))
    return c


# ---- hand case: apply -----------------------------------------------------------------------------------------------------------------
def hand_apply_case():
    """-> (map at the time of the write-back, (cam_kf, gpt_pt, poses7, pts3), the outputs worked by hand per stage).  The problem is the
    first hand case's: cameras 3, 4, 1, 2 and points 0, 3, 6.  Since the assembly keyframe 4 and point 3 turned bad.  The quaternions are
    (0, 0, 0, 2): un-normalised, R = I.  New centres: keyframe 3 (10, 0, 0), 1 (12, 0, 0), 2 (-1, -1, 4); keyframe 4 keeps (-4, 0, 0).
    p6 moves to (-4, 3, 4): (-3, 4, 0) from keyframe 2 - its reference, 5 away, level 6 - and (0, 3, 4) from the bad keyframe 4."""
    m = _hand(kf_bad=[0, 0, 0, 0, 1, 1], pt_bad=[0, 0, 1, 1, 0, 0, 0])
    m["kf_gba_Tcw"] = np.full((6, 12), POISON); m["pt_gba_X"] = np.full((7, 3), POISON)
    centres = [(10.0, 0.0, 0.0), (11.0, 0.0, 0.0), (12.0, 0.0, 0.0), (-1.0, -1.0, 4.0)]
    poses7 = np.array([[-c[0], -c[1], -c[2], 0.0, 0.0, 0.0, 2.0] for c in centres])
    pts3 = np.array([(20.0, 0.0, 0.0), (21.0, 0.0, 0.0), (-4.0, 3.0, 4.0)])
    new_T = {3: _pose((-10.0, 0.0, 0.0)), 1: _pose((-12.0, 0.0, 0.0)), 2: _pose((1.0, 1.0, -4.0))}
    T0 = np.array([new_T.get(k, _pose((k, 0.0, 0.0))) for k in range(6)])
    X0 = np.array([(p, 1.0, 2.0) for p in range(7)], np.float64); X0[0] = pts3[0]; X0[6] = pts3[2]
    mx = np.float32(5.0) * SF[6]
    stage0 = dict(kf_Tcw=T0, kf_center=[(0.0, 0.0, 0.0), (12.0, 0.0, 0.0), (-1.0, -1.0, 4.0), (10.0, 0.0, 0.0), (-4.0, 0.0, 0.0), (-5.0, 0.0, 0.0)], X=X0,
                  nd_written=[1, 0, 0, 0, 0, 0, 1], counts=[3, 2, 2],
                  normal6=[((0.0 + -3.0 / 5.0) + 0.0 / 5.0) / 2.0, ((0.0 + 4.0 / 5.0) + 3.0 / 5.0) / 2.0, ((0.0 + 0.0 / 5.0) + 4.0 / 5.0) / 2.0], min_max6=[mx / SF[7], mx])
    gT = np.full((6, 12), POISON); gX = np.full((7, 3), POISON)
    for k, T in new_T.items():
        gT[k] = T
    gX[0] = pts3[0]; gX[6] = pts3[2]
    stage1 = dict(kf_gba_Tcw=gT, kf_in_gba=[0, 1, 1, 1, 0, 0], pt_gba_X=gX, pt_in_gba=[1, 0, 0, 0, 0, 0, 1], counts=[3, 2, 0])
    return m, (np.array([3, 4, 1, 2], np.int32), np.array([0, 3, 6], np.int32), poses7, pts3), stage0, stage1


# ---- seeded maps ------------------------------------------------------------------------------------------------------------------------
def make_map(seed, nkf, npts, reach=3, max_obs=None, listed=0.8, pt_listed=0.9, bad=0.1):
    """keyframes with ids that are no table indices (one 0, one pair equal, all in shuffled order); the keyframe list names `listed` of them
    shuffled, bad ones (the share `bad` of all keyframes) among them, two of them twice; the point list is a shuffled `pt_listed` of the
    points; a point is seen from up to 2 * reach + 1 keyframes around its place (max_obs: at most that many), 5% of the points from none"""
    rng = np.random.RandomState(seed)
    Tcw = np.array([_rand_pose(rng) for _ in range(nkf)])
    kf_bad = (rng.rand(nkf) < bad).astype(np.uint8)
    kf_id = rng.permutation(nkf) * 7 + 3
    kf_id[nkf // 2] = kf_id[nkf // 3]                                            # (equal ids)
    ba_kf = rng.permutation(nkf)[:max(2, int(listed * nkf))].tolist()
    ba_kf = ba_kf + [ba_kf[0], ba_kf[len(ba_kf) // 2]]
    kf_bad[ba_kf[0]] = 0; kf_bad[ba_kf[2]] = 0
    kf_bad[ba_kf[1]] = 1                                                         # (a bad keyframe in the list)
    kf_id[ba_kf[0]] = 7 * nkf + 10; kf_id[ba_kf[2]] = 0                          # (the list's first camera is the last by id; the first keyframe of the map)
    ba_pt = rng.permutation(npts)[:max(1, int(pt_listed * npts))]
    pt_bad = (rng.rand(npts) < 0.05).astype(np.uint8)
    obs, ref = [], []
    for p in range(npts):
        place = int(rng.randint(0, nkf))
        cand = [k for k in range(place - reach, place + reach + 1) if 0 <= k < nkf]
        n = int(rng.randint(1, len(cand) + 1))
        if max_obs:
            n = min(n, int(rng.randint(1, max_obs + 1)))
        ks = [] if rng.rand() < 0.05 else rng.permutation(cand)[:n].tolist()
        obs.append(ks)
        ref.append(-1 if not ks else (ks[int(rng.randint(0, len(ks)))] if rng.rand() < 0.9 else int(rng.randint(0, nkf))))
    nobs = sum(len(o) for o in obs)
    K = np.array(K4) * (1.0 + 0.01 * rng.rand(nkf, 1))
    return table_map(Tcw, kf_id, rng.uniform(-10, 10, (npts, 3)), obs, ba_kf=ba_kf, ba_pt=ba_pt, kf_bad=kf_bad, pt_bad=pt_bad, obs_uv=rng.uniform(0, 700, (nobs, 2)),
                     obs_level=rng.randint(0, 8, nobs), pt_ref_kf=ref, ref_level=rng.randint(0, 8, npts), kf_K4=K)


def solver_result(seed, asm):
    """a synthetic result of ba_solve for the assembled problem: perturbed poses with un-normalised quaternions, moved points"""
    rng = np.random.RandomState(seed)
    ncam, npb = int(asm["counts"][0]), int(asm["counts"][1])
    poses7 = np.array(asm["poses7"], np.float64).reshape(-1, 7)[:ncam].copy()
    poses7[:, :3] += 0.05 * rng.randn(ncam, 3)
    poses7[:, 3:] = (poses7[:, 3:] + 0.01 * rng.randn(ncam, 4)) * rng.uniform(0.5, 2.0, (ncam, 1))
    pts3 = np.array(asm["pts3"], np.float64).reshape(-1, 3)[:npb] + 0.05 * rng.randn(npb, 3)
    return poses7, pts3


def turned_bad(seed, m, asm):
    """the map at the time of the write-back: a copy of m in which a tenth of the cameras' keyframes and of the problem's points turned bad"""
    rng = np.random.RandomState(seed)
    w = dict(m)
    kb = np.zeros(m["nkf"], np.uint8) if m.get("kf_bad") is None else m["kf_bad"].copy()
    pb = np.zeros(m["npts"], np.uint8) if m.get("pt_bad") is None else m["pt_bad"].copy()
    ck, gp = np.asarray(asm["cam_kf"])[:int(asm["counts"][0])], np.asarray(asm["gpt_pt"])[:int(asm["counts"][1])]
    if len(ck):
        kb[ck[rng.rand(len(ck)) < 0.1]] = 1; kb[ck[0]] = 1
    if len(gp):
        pb[gp[rng.rand(len(gp)) < 0.1]] = 1; pb[gp[0]] = 1
    w.update(kf_bad=kb, pt_bad=pb)
    return w


SMALL = ((400, 8, 60), (401, 8, 60), (402, 8, 60))
LARGE = ((410, 300, 3000), (411, 300, 3000))


def seeded_maps(large=True):
    """(name, map): 8 keyframes / 60 points; 300 keyframes / 3000 points (more cameras than one 256-key tile of the all-pairs count, more
    points than one workgroup of the scan); 3 keyframes / 70000 points, all listed, with one or two observations each (more than 256
    workgroup sums)"""
    out = [("map seed %d nkf %d npts %d" % (s, nkf, npts), make_map(s, nkf, npts)) for s, nkf, npts in SMALL]
    if large:
        out += [("map seed %d nkf %d npts %d" % (s, nkf, npts), make_map(s, nkf, npts, listed=0.97, bad=0.05)) for s, nkf, npts in LARGE]
        out.append(("map seed 420 nkf 3 npts 70000", make_map(420, 3, 70000, reach=1, max_obs=2, listed=1.0, pt_listed=1.0)))
    return out
