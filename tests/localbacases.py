"""Test maps for orbl_local_ba_assemble and orbl_local_ba_apply (tests/nplocalba.py states the dict layout): hand-worked cases whose
expected outputs are written here, and a seeded generator.  TEST INFRASTRUCTURE.

The hand cases use axis-parallel poses ([I | t]) and solver results with q = (0, 0, 0, 2), so that every figure is exact and can be
followed on paper: the new pose is [I | t] and the new centre -t."""
import numpy as np

from tests.mapcorrectcases import POISON, SF, _centre, _csr, _pose, _rand_pose  # noqa: F401

ISG = np.array([1.0 / 1.44 ** i for i in range(8)], np.float32)
K4 = (458.654, 457.296, 367.215, 248.375)


def table_map(cur_kf, nbr_kf, Tcw, kf_id, slots, X, obs, obs_slot=None, kf_bad=None, kf_rank=None, pt_bad=None, pt_rank=None, obs_uv=None, obs_level=None, pt_ref_kf=None,
              kf_level0=None, pt_nobs=None, kf_K4=None):
    """slots: per keyframe its GetMapPointMatches() (point or -1); obs: per point its observers in list order; obs_slot: per point the
    slots of those observations (default: where the keyframe lists the point, else 0)"""
    Tcw = np.ascontiguousarray(Tcw, np.float64).reshape(-1, 12)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    nkf, npts = len(Tcw), len(X)
    so, sp = _csr(slots)
    oo, ok = _csr(obs)
    nobs = len(ok)
    if obs_slot is None:
        obs_slot = [[(slots[k].index(p) if p in slots[k] else 0) for k in o] for p, o in enumerate(obs)]
    if obs_uv is None:
        obs_uv = [[100.0 + e, 50.0 + 2 * e] for e in range(nobs)]
    if obs_level is None:
        obs_level = [e % 8 for e in range(nobs)]
    if pt_ref_kf is None:
        pt_ref_kf = [o[0] if o else 0 for o in obs]
    return dict(nkf=nkf, npts=npts, cur_kf=int(cur_kf), nbr_kf=np.array(nbr_kf, np.int32), kf_id=np.array(kf_id, np.int32),
                kf_bad=None if kf_bad is None else np.array(kf_bad, np.uint8), kf_rank=None if kf_rank is None else np.array(kf_rank, np.int32), kf_Tcw=Tcw,
                kf_K4=np.tile(np.array(K4), (nkf, 1)) if kf_K4 is None else np.ascontiguousarray(kf_K4, np.float64).reshape(nkf, 4), kf_slot_off=so, kf_slot_pt=sp, X=X,
                pt_bad=None if pt_bad is None else np.array(pt_bad, np.uint8), pt_rank=None if pt_rank is None else np.array(pt_rank, np.int32), obs_off=oo, obs_kf=ok,
                obs_uv=np.array(obs_uv, np.float32).reshape(-1, 2), obs_level=np.array(obs_level, np.int32), inv_level_sigma2=ISG.copy(),
                kf_center=np.array([_centre(T) for T in Tcw]).reshape(nkf, 3), pt_nobs=np.array([len(o) for o in obs] if pt_nobs is None else pt_nobs, np.int32),
                pt_ref_kf=np.array(pt_ref_kf, np.int32), obs_slot=np.array([v for r in obs_slot for v in r], np.int32),
                kf_level0=None if kf_level0 is None else np.array(kf_level0, np.int32), scale_factors=SF.copy())


# ---- hand cases: assemble -----------------------------------------------------------------------------------------------------------
def _hand_a(**kw):
    # keyframes 0..5 at t = (k, 0, 0); 4 is bad.  p0 sits in two local keyframes; p1 is seen by the bad neighbour 4 and by 5; p2 sits in a
    # slot of keyframe 0 whose list names only keyframe 3; p3 is seen by the bad keyframe alone; p4 is not local; p5 is bad
    a = dict(cur_kf=2, nbr_kf=[1, 4, 0], Tcw=[_pose((k, 0.0, 0.0)) for k in range(6)], kf_id=[0, 10, 20, 30, 40, 50], kf_bad=[0, 0, 0, 0, 1, 0],
             slots=[[2], [0, 3], [0, 1, -1, 5], [2], [1, 3], [1, 4]], X=[(p, 1.0, 2.0) for p in range(6)], obs=[[1, 2], [2, 4, 5], [3], [4], [5], []],
             pt_bad=[0, 0, 0, 0, 0, 1])
    a.update(kw)
    return table_map(**a)


def hand_assemble_cases():
    """name -> (map, the outputs worked by hand)"""
    c = {}
    # local cameras by id: 0 (id 0: fixed, still local), 1, 2; fixed by index: 3 (through p2), 5 (through p1); 4 is stamped and bad
    c["bad neighbour, id 0, two local keyframes, a list without the slot's keyframe, no rows"] = (_hand_a(), dict(
        counts=[5, 3, 4, 5], cam_kf=[0, 1, 2, 3, 5], cam_fixed=[1, 0, 0, 1, 1], cam_local=[1, 1, 1, 0, 0], lpt_pt=[0, 1, 2, 3], lobs_cam=[1, 2, 2, 4, 3],
        lobs_pt=[0, 0, 1, 1, 2], lobs_src=[0, 1, 2, 4, 5], kf_role=[1, 1, 1, 2, 3, 2], pt_local=[1, 1, 1, 1, 0, 0]))
    # both ranks reverse the index order; the list names the current keyframe, keyframe 1 and keyframe 0 twice
    c["ranks reverse the index order, repeats in the list"] = (_hand_a(nbr_kf=[1, 2, 1, 4, 0, 0], kf_rank=[5, 4, 3, 2, 1, 0], pt_rank=[5, 4, 3, 2, 1, 0]), dict(
        counts=[5, 3, 4, 5], cam_kf=[0, 1, 2, 5, 3], cam_fixed=[1, 0, 0, 1, 1], cam_local=[1, 1, 1, 0, 0], lpt_pt=[3, 2, 1, 0], lobs_cam=[4, 2, 3, 1, 2],
        lobs_pt=[1, 2, 2, 3, 3], lobs_src=[5, 2, 4, 0, 1], kf_role=[1, 1, 1, 2, 3, 2], pt_local=[1, 1, 1, 1, 0, 0]))
    # equal ids: the current keyframe first, then the list's order
    c["equal ids"] = (_hand_a(nbr_kf=[1, 0], kf_id=[7, 7, 7, 7, 7, 7]), dict(
        counts=[5, 3, 4, 5], cam_kf=[2, 1, 0, 3, 5], cam_fixed=[0, 0, 0, 1, 1], cam_local=[1, 1, 1, 0, 0], lpt_pt=[0, 1, 2, 3], lobs_cam=[1, 0, 0, 4, 3],
        lobs_pt=[0, 0, 1, 1, 2], lobs_src=[0, 1, 2, 4, 5], kf_role=[1, 1, 1, 2, 0, 2], pt_local=[1, 1, 1, 1, 0, 0]))
    c["empty inputs"] = (table_map(0, [], [_pose((0.0, 0.0, 0.0))], [3], [[]], np.zeros((0, 3)), []), dict(
        counts=[1, 1, 0, 0], cam_kf=[0], cam_fixed=[0], cam_local=[1], lpt_pt=[], lobs_cam=[], lobs_pt=[], lobs_src=[], kf_role=[1], pt_local=[]))
    return c


# ---- hand case: apply -----------------------------------------------------------------------------------------------------------------
def hand_apply_case():
    """-> (map, solver result = (poses7, pts3, obs_erase), the outputs worked by hand).  Keyframes 0..3 are local (0 has id 0), 4 is fixed.
    p0 (5 observations, reference 1) loses keyframe 1: the reference moves to keyframe 0.  p1 (3 observations) loses keyframe 1: 2 are left,
    it turns bad, the observations of 0 and 2 die with their slots; the row on keyframe 2 then finds nothing.  p2 loses its only
    observation: bad, the reference stays.  p3's reference keyframe 0 does not observe it: kf_level0.  p4 (3-4-5 triangles) is untouched."""
    slots = [[0, 1], [0, 1, 3], [0, 1, 3, 4], [0, 2, 3, 4], [0, 3]]
    obs = [[0, 1, 2, 3, 4], [0, 1, 2], [3], [1, 2, 3, 4], [2, 3]]
    m = table_map(0, [1, 2, 3], [_pose((k, 0.0, 0.0)) for k in range(5)], [0, 1, 2, 3, 4], slots, [(p, 1.0, 2.0) for p in range(5)], obs, pt_ref_kf=[1, 0, 3, 0, 2],
                  kf_level0=[5, 1, 1, 1, 1], obs_level=[0, 1, 2, 3, 4, 0, 1, 2, 3, 1, 1, 1, 1, 2, 6])
    centres = [(10.0, 0.0, 0.0), (11.0, 0.0, 0.0), (12.0, 0.0, 0.0), (15.0, -1.0, 4.0)]
    poses7 = np.array([[-c[0], -c[1], -c[2], 0.0, 0.0, 0.0, 2.0] for c in centres] + [[9.0, 9.0, 9.0, 0.0, 0.0, 0.0, 1.0]])       # (camera 4 is fixed: not written back)
    pts3 = np.array([(20.0, 0.0, 0.0), (21.0, 0.0, 0.0), (22.0, 0.0, 0.0), (23.0, 0.0, 0.0), (12.0, 3.0, 4.0)])
    erase = np.zeros(15, np.uint8); erase[[1, 6, 7, 8]] = 1
    mx = np.float32(5.0) * SF[2]
    hand = dict(kf_slot_pt=[0, -1, -1, -1, 3, 0, -1, 3, 4, 0, -1, 3, 4, 0, 3], pt_bad=[0, 1, 1, 0, 0], pt_nobs=[4, 2, 0, 4, 2], pt_ref_kf=[0, 0, 3, 0, 2],
                obs_erased=[0, 1, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0], counts=[3, 2, 5, 3], nd_written=[1, 0, 0, 1, 1], diag=dict(ref_moved=1, dead_rows=1, turned_bad=2),
                kf_center=list(centres) + [(-4.0, 0.0, 0.0)], X=[tuple(x) for x in pts3.tolist()],
                normal4=[(0.0 + -3.0 / 5.0) / 2.0, (3.0 / 5.0 + 4.0 / 5.0) / 2.0, (4.0 / 5.0 + 0.0) / 2.0], min_max4=[mx / SF[7], mx],
                # p3: reference keyframe 0 at (10, 0, 0), 13 away, level kf_level0[0] = 5
                min_max3=[np.float32(13.0) * SF[5] / SF[7], np.float32(13.0) * SF[5]])
    return m, (poses7, pts3, erase), hand


# ---- seeded maps ------------------------------------------------------------------------------------------------------------------------
def make_map(seed, nkf, npts, half=4, reach=3, local_share=0.0, long_list=0, reverse_ranks=False, rest_outside=False):
    """keyframes along a chain; a point is seen from up to 2 * reach + 1 keyframes around its own place (long_list: point npts // 2 from that
    many); the current keyframe sits in the middle and its list names the keyframes within `half` of it, shuffled, with a repeat, itself
    and the bad ones among them; local_share: the share of points placed inside that window (the rest anywhere, or outside the window only
    with rest_outside).  Lists are in kf_rank order."""
    rng = np.random.RandomState(seed)
    Tcw = np.array([_rand_pose(rng) for _ in range(nkf)])
    cur = nkf // 2
    window = [k for k in range(max(0, cur - half), min(nkf, cur + half + 1))]
    kf_bad = (rng.rand(nkf) < 0.1).astype(np.uint8)
    kf_bad[cur] = 0
    kf_bad[window[0]] = 1                                                      # (a bad neighbour)
    far = [k for k in range(nkf) if k not in window]
    if far:
        kf_bad[far[len(far) // 2]] = 0; kf_bad[far[0]] = 0
    nbr = [k for k in rng.permutation(window) if k != cur]
    nbr = nbr + [nbr[1 % len(nbr)], cur]
    kf_id = rng.permutation(nkf) * 3 + 1
    kf_id[window[-1]] = 0                                                      # (the first keyframe of the map is local)
    if len(window) > 3:
        kf_id[window[2]] = kf_id[window[1]]                                    # (equal ids)
    kf_rank = np.arange(nkf)[::-1].copy() if reverse_ranks else rng.permutation(nkf)
    pt_rank = np.arange(npts)[::-1].copy() if reverse_ranks else rng.permutation(npts)
    pt_bad = (rng.rand(npts) < 0.05).astype(np.uint8)
    slots = [[] for _ in range(nkf)]
    obs, obs_slot, ref = [], [], []
    for p in range(npts):
        inside = rng.rand() < local_share
        place = int(rng.randint(window[0], window[-1] + 1)) if inside else int(rng.randint(0, nkf))
        if rest_outside and far and not inside:
            place = far[int(rng.randint(0, len(far)))]
        cand = [k for k in range(place - reach, place + reach + 1) if 0 <= k < nkf]
        n = int(rng.randint(1, len(cand) + 1)) if rng.rand() < 0.85 else min(3, len(cand))
        ks = rng.permutation(cand)[:n].tolist()
        if long_list and p == npts // 2:
            ks = rng.permutation(nkf)[:long_list].tolist()
            pt_bad[p] = 0
            if cur not in ks:
                ks[0] = cur
        ks.sort(key=lambda k: kf_rank[k])
        ss = []
        for k in ks:
            if rng.rand() < 0.1:
                slots[k].append(-1)
            ss.append(len(slots[k])); slots[k].append(p)
        if pt_bad[p]:                                                            # (SetBadFlag cleared its list; a stale slot or two is left)
            ks, ss = [], []
        obs.append(ks); obs_slot.append(ss)
        ref.append((ks[int(rng.randint(0, len(ks)))] if rng.rand() < 0.9 else int(rng.randint(0, nkf))) if ks else 0)
    for k in window[1:3]:                                                        # (slots whose point does not list the keyframe)
        slots[k] += rng.randint(0, npts, 3).tolist()
    nobs = sum(len(o) for o in obs)
    K = np.array(K4) * (1.0 + 0.01 * rng.rand(nkf, 1))
    return table_map(cur, nbr, Tcw, kf_id, slots, rng.uniform(-10, 10, (npts, 3)), obs, obs_slot=obs_slot, kf_bad=kf_bad, kf_rank=kf_rank, pt_bad=pt_bad, pt_rank=pt_rank,
                     obs_uv=rng.uniform(0, 700, (nobs, 2)), obs_level=rng.randint(0, 8, nobs), pt_ref_kf=ref, kf_level0=rng.randint(0, 8, nkf), kf_K4=K)


def solver_result(seed, m, asm, share=0.2):
    """a synthetic result of ba_local_bundle_adjustment for the assembled problem: perturbed poses with un-normalised quaternions, moved
    points, erase flags on `share` of the rows - and, so that no map is vacuous, on the first two rows of a point with three observations
    (it turns bad at the first, the second finds it dead) and on the reference keyframe's row of a point with five or more"""
    rng = np.random.RandomState(seed)
    ncam, npl, nol = (int(asm["counts"][i]) for i in (0, 2, 3))
    poses7 = np.array(asm["poses7"], np.float64).reshape(ncam, 7).copy()
    poses7[:, :3] += 0.05 * rng.randn(ncam, 3)
    poses7[:, 3:] = (poses7[:, 3:] + 0.01 * rng.randn(ncam, 4)) * rng.uniform(0.5, 2.0, (ncam, 1))
    pts3 = np.array(asm["pts3"], np.float64).reshape(npl, 3) + 0.05 * rng.randn(npl, 3)
    erase = (rng.rand(nol) < share).astype(np.uint8)
    rows_of = {}
    for i in range(nol):
        rows_of.setdefault(int(asm["lobs_pt"][i]), []).append(i)
    forced = [False, False]
    for j, rows in rows_of.items():
        p = int(asm["lpt_pt"][j])
        if not forced[0] and m["pt_nobs"][p] == 3 and len(rows) >= 2:
            erase[rows] = 0; erase[rows[:2]] = 1; forced[0] = True
        elif not forced[1] and m["pt_nobs"][p] >= 5 and len(rows) == m["pt_nobs"][p] and m["pt_ref_kf"][p] in [int(m["obs_kf"][asm["lobs_src"][i]]) for i in rows[1:]]:
            erase[rows] = 0
            erase[[i for i in rows if int(m["obs_kf"][asm["lobs_src"][i]]) == m["pt_ref_kf"][p]]] = 1
            forced[1] = True
    return poses7, pts3, erase


def seeded_maps():
    """(name, map): 12 to 40 keyframes with 300 to 2000 points, reversed ranks once; then one map whose scans cross wavefronts and
    workgroups (more than 64 cameras, more than 4096 local points) with one point of more than 256 observations"""
    out = [("map seed %d nkf %d npts %d" % (s, nkf, npts), make_map(s, nkf, npts, half=half, reverse_ranks=rev))
           for s, nkf, npts, half, rev in ((300, 12, 300, 2, False), (301, 25, 513, 4, True), (302, 40, 2000, 6, False), (303, 33, 1025, 5, False))]
    out.append(("map seed 304 nkf 300 npts 7000", make_map(304, 300, 7000, half=40, local_share=0.75, long_list=280)))
    return out
