"""Test problems for orbl_correct_loop and orbl_propagate_global_ba (tests/npmapcorrect.py states the dict layouts): hand-worked cases
whose expected values are written here, and a seeded generator.  TEST INFRASTRUCTURE.

The hand cases of correct_loop use axis-parallel poses ([I | t]), so that every figure is exact and can be followed on paper: with
Scw = (q = sqrt(s) [0 0 0 1], tS) the corrected Sim3 of keyframe i is x -> s x + (t_i - t_cur + tS), its new pose [I | (t_i - t_cur + tS) / s],
and every moved point goes to (X + t_cur - tS) / s whichever keyframe moves it - WHO moves it shows in pt_owner and in the normals."""
import math

import numpy as np

SF = np.array([1.2 ** i for i in range(8)], np.float32)
POISON = -7777.0


def _pose(t, R=None):
    T = np.zeros((3, 4))
    T[:, :3] = np.eye(3) if R is None else R
    T[:, 3] = t
    return T.reshape(12)


def _centre(T):
    T = np.asarray(T).reshape(3, 4)
    return -(T[:, :3].T @ T[:, 3])


def _csr(rows, dtype=np.int32):
    off = np.zeros(len(rows) + 1, np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    flat = np.array([v for r in rows for v in r], dtype)
    return off, flat


def loop_problem(Tcw, conn_kf, Scw, slots, X, conn_rank=None, pt_bad=None, pt_done=None, obs=None, ref_kf=None, ref_level=None, centres=True):
    Tcw = np.ascontiguousarray(Tcw, np.float64).reshape(-1, 12)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    so, sp = _csr(slots)
    pr = dict(nkf=len(Tcw), kf_Tcw=Tcw, kf_center=np.array([_centre(T) for T in Tcw]) if centres else None, conn_kf=np.array(conn_kf, np.int32),
              conn_rank=None if conn_rank is None else np.array(conn_rank, np.int32), Scw=np.array(Scw, np.float64), slot_off=so, slot_pt=sp, npts=len(X), X=X,
              pt_bad=None if pt_bad is None else np.array(pt_bad, np.uint8), pt_done=None if pt_done is None else np.array(pt_done, np.uint8),
              obs_off=None, obs_kf=None, ref_kf=None, ref_level=None, scale_factors=None)
    if obs is not None:
        oo, ok = _csr(obs)
        pr.update(obs_off=oo, obs_kf=ok, ref_kf=np.array(ref_kf, np.int32), ref_level=np.array(ref_level, np.int32), scale_factors=SF.copy())
    return pr


def gba_problem(Tcw, gba, in_gba, parent, origins, X, ref, pt_bad=None, pt_in_gba=None, pt_gba_X=None, centres=True):
    Tcw = np.ascontiguousarray(Tcw, np.float64).reshape(-1, 12)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    return dict(nkf=len(Tcw), kf_Tcw=Tcw, kf_gba_Tcw=np.ascontiguousarray(gba, np.float64).reshape(-1, 12), kf_in_gba=np.array(in_gba, np.uint8),
                kf_parent=np.array(parent, np.int32), origin_kf=np.array(origins, np.int32), kf_center=np.array([_centre(T) for T in Tcw]) if centres else None,
                npts=len(X), X=X, pt_bad=None if pt_bad is None else np.array(pt_bad, np.uint8),
                pt_in_gba=None if pt_in_gba is None else np.array(pt_in_gba, np.uint8),
                pt_gba_X=None if pt_gba_X is None else np.ascontiguousarray(pt_gba_X, np.float64).reshape(-1, 3), pt_ref_kf=np.array(ref, np.int32))


# ---- hand cases: correct_loop ------------------------------------------------------------------------------------------------------
T_HAND = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, 0.0, 3.0), (4.0, 4.0, 0.0)]       # t of keyframes 0..4, R = I
TS = (0.5, 0.0, -0.25)


def _hand_loop(conn_kf, slots, X, s=1.0, **kw):
    Scw = [0.0, 0.0, 0.0, math.sqrt(s)] + list(TS)
    return loop_problem([_pose(t) for t in T_HAND], conn_kf, Scw, slots, X, **kw)


def _hand_expect(pr, s, owner):
    """the values the note at the top of the file gives: new poses of the group, new positions of the moved points"""
    cur = int(pr["conn_kf"][-1])
    tc = np.array(T_HAND[cur]); ts = np.array(TS)
    T = pr["kf_Tcw"].copy()
    for k in pr["conn_kf"]:
        T[k] = _pose((np.array(T_HAND[k]) - tc + ts) / s)
    X = pr["X"].copy()
    for p, o in enumerate(owner):
        if o >= 0:
            X[p] = (X[p] + tc - ts) / s
    return dict(pt_owner=np.array(owner, np.int32), kf_Tcw=T, X=X)


def hand_loop_cases():
    """name -> (problem, expected dict: pt_owner, kf_Tcw, X, counts, and for the normals `new_centre_for`: per point the observers whose
    NEW centre its normal sees)"""
    H = {}
    # (a) point 0 held by keyframes 1 and 2 (list positions 0 and 1); the ranks reverse the list order, so keyframe 2 moves it, not 1;
    # point 1 is held by 1 alone, point 2 by nobody
    pr = _hand_loop([1, 2, 0], [[0, 1], [0], []], [[1.0, 2.0, 4.0], [0.0, 1.0, 8.0], [5.0, 5.0, 5.0]], conn_rank=[2, 1, 0])
    H["a_rank_reverses_list_order"] = (pr, dict(_hand_expect(pr, 1.0, [2, 1, -1]), counts=[2, 1]))
    # (b) point 0 was corrected by this loop closure already
    pr = _hand_loop([1, 0], [[0, 1], [0, 1]], [[1.0, 2.0, 4.0], [0.0, 1.0, 8.0]], pt_done=[1, 0])
    H["b_done_point"] = (pr, dict(_hand_expect(pr, 1.0, [-1, 1]), counts=[1, 1]))
    # (c) a bad point (0), a null slot, and point 1 listed twice by keyframe 1 alone: moved once, not contested
    pr = _hand_loop([1, 0], [[0, -1, 1, 1], [0, 2]], [[1.0, 2.0, 4.0], [0.0, 1.0, 8.0], [2.0, 2.0, 2.0]], pt_bad=[1, 0, 0])
    H["c_bad_null_twice"] = (pr, dict(_hand_expect(pr, 1.0, [-1, 1, 0]), counts=[2, 0]))
    # (d) the current keyframe alone: corrected = Scw
    pr = _hand_loop([3], [[0]], [[1.0, 2.0, 4.0]])
    H["d_nconn_1"] = (pr, dict(_hand_expect(pr, 1.0, [3]), counts=[1, 0]))
    # (e) scale 1.04: the new translations are t / s
    pr = _hand_loop([1, 2, 0], [[0], [1], [0, 1]], [[1.0, 2.0, 4.0], [0.0, 1.0, 8.0]], s=1.04)
    H["e_scale"] = (pr, dict(_hand_expect(pr, 1.04, [1, 2]), counts=[2, 2], scale=1.04))
    # (f) point 0 is held by keyframes 0 and 2, moved by keyframe 2 (rank 1) and observed by 1 (rank 0: SetPose done, NEW centre), 2 (its owner: old), 0 (rank 2: old)
    # and 4 (outside the group: old); its reference keyframe is 1 (new centre)
    pr = _hand_loop([0, 1, 2], [[0], [], [0]], [[1.0, 2.0, 4.0]], conn_rank=[2, 0, 1], obs=[[0, 1, 2, 4]], ref_kf=[1], ref_level=[2])
    H["f_centres_half_new"] = (pr, dict(_hand_expect(pr, 1.0, [2]), counts=[1, 1], new_centre_for=[[1]]))
    # (g) the reference keyframe (4) is outside the group; point 1 has no observation at all (moved, no normal)
    pr = _hand_loop([1, 0], [[0, 1], []], [[1.0, 2.0, 4.0], [3.0, 3.0, 3.0]], obs=[[1, 4], []], ref_kf=[4, 0], ref_level=[0, 0])
    H["g_reference_outside"] = (pr, dict(_hand_expect(pr, 1.0, [1, 1]), counts=[2, 0], new_centre_for=[[], []], nd_written=[1, 0]))
    return H


# ---- hand cases: propagate_global_ba --------------------------------------------------------------------------------------------
def _chain(n_out, extra_in=2):
    """origin 0 and `extra_in` keyframes inside the BA in a chain, then n_out keyframes outside it, each the child of the one before:
    translations only, Tcw[k] = [I | (k, 0, 0)], the BA moved every keyframe by (0, 10, 0)"""
    n = 1 + extra_in + n_out
    Tcw = [_pose((float(k), 0.0, 0.0)) for k in range(n)]
    gba = [_pose((float(k), 10.0, 0.0)) if k <= extra_in else _pose((POISON, POISON, POISON)) for k in range(n)]
    in_gba = [1] * (1 + extra_in) + [0] * n_out
    parent = [-1] + list(range(n - 1))
    return Tcw, gba, in_gba, parent


def hand_gba_cases():
    """name -> (problem, expected dict with the hand values)"""
    H = {}
    # (a) every keyframe in the BA: the matrices are taken as they are; point 0 follows keyframe 1: Xc = X + (1, 0, 0), X' = Xc - (1, 10, 0)
    Tcw, gba, in_gba, parent = _chain(0)
    pr = gba_problem(Tcw, gba, in_gba, parent, [0], [[1.0, 2.0, 3.0]], [1])
    H["a_all_in_ba"] = (pr, dict(kf_reached=[1, 1, 1], counts=[3, 0, 1, 0], kf_Tcw=np.array(gba), X=[[1.0, -8.0, 3.0]], pt_moved=[2]))
    # (b) three keyframes outside the BA under keyframe 2: gba[k] = (Tcw[k] o Twc[k-1]) o gba[k-1] = [I | (k, 10, 0)]
    Tcw, gba, in_gba, parent = _chain(3)
    pr = gba_problem(Tcw, gba, in_gba, parent, [0], [[1.0, 2.0, 3.0]], [5])
    H["b_run_of_three"] = (pr, dict(kf_reached=[1] * 6, counts=[6, 3, 1, 0], kf_Tcw=np.array([_pose((float(k), 10.0, 0.0)) for k in range(6)]),
                                    X=[[1.0, -8.0, 3.0]], pt_moved=[2], kf_in_gba=[1] * 6))
    # (c) two origins (0 and 3), each with one child; the child of 3 is outside the BA
    Tcw = [_pose((float(k), 0.0, 0.0)) for k in range(5)]
    gba = [_pose((float(k), 10.0, 0.0)) for k in range(5)]; gba[4] = _pose((POISON,) * 3)
    pr = gba_problem(Tcw, gba, [1, 1, 0, 1, 0], [-1, 0, -1, -1, 3], [0, 3], [[0.0, 0.0, 0.0]], [4])
    H["c_two_origins"] = (pr, dict(kf_reached=[1, 1, 0, 1, 1], counts=[4, 1, 1, 0], X=[[0.0, -10.0, 0.0]], pt_moved=[2], kf_in_gba=[1, 1, 0, 1, 1]))
    # (d) keyframe 2 is flagged as in the BA but hangs on nothing (its parent erased it): not reached, its point stays and is counted
    pr = gba_problem(Tcw[:3], gba[:3], [1, 1, 1], [-1, 0, -1], [0], [[1.0, 1.0, 1.0], [2.0, 2.0, 2.0]], [2, 1])
    H["d_flagged_unreached"] = (pr, dict(kf_reached=[1, 1, 0], counts=[2, 0, 1, 1], X=[[1.0, 1.0, 1.0], [2.0, -8.0, 2.0]], pt_moved=[0, 2]))
    # (e) points of all three kinds and a bad one: in the BA (0), through its reference keyframe (1), reference keyframe neither flagged nor
    # reached (2: stays, not stale), bad (3, although in the BA)
    pr = gba_problem(Tcw[:3], gba[:3], [1, 1, 0], [-1, 0, -1], [0], [[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0], [4.0, 4.0, 4.0]], [0, 1, 2, 0],
                     pt_bad=[0, 0, 0, 1], pt_in_gba=[1, 0, 0, 1], pt_gba_X=[[9.0, 9.0, 9.0], [8.0, 8.0, 8.0], [7.0, 7.0, 7.0], [6.0, 6.0, 6.0]])
    H["e_point_kinds"] = (pr, dict(kf_reached=[1, 1, 0], counts=[2, 0, 2, 0], X=[[9.0, 9.0, 9.0], [2.0, -8.0, 2.0], [3.0, 3.0, 3.0], [4.0, 4.0, 4.0]],
                                   pt_moved=[1, 2, 0, 0]))
    # (f), (g) chains of 70 and 1 100 keyframes outside the BA below one origin: more rounds than a wave, than a workgroup has lanes
    for name, n in (("f_chain_70", 70), ("g_chain_1100", 1100)):
        Tcw, gba, in_gba, parent = _chain(n, extra_in=0)
        pr = gba_problem(Tcw, gba, in_gba, parent, [0], [[1.0, 2.0, 3.0]], [n])
        H[name] = (pr, dict(kf_reached=[1] * (n + 1), counts=[n + 1, n, 1, 0], kf_Tcw=np.array([_pose((float(k), 10.0, 0.0)) for k in range(n + 1)]),
                            X=[[1.0, -8.0, 3.0]], pt_moved=[2], depth=n))
    return H


# ---- seeded problems ----------------------------------------------------------------------------------------------------------------
def _rand_pose(rng, spread=4.0):
    q = rng.randn(4); q /= np.linalg.norm(q)
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return _pose(rng.uniform(-spread, spread, 3), R)


def make_loop(seed, nconn, npts, nkf=None, max_slots=300, long_list=False, nulls=True):
    """a covisibility group of nconn keyframes among nkf, shuffled ranks, each holding up to max_slots slots drawn from a window of points
    that overlaps its neighbours' (so that most points are contested); observation lists of <= 12 keyframes (one of 600 with long_list)"""
    rng = np.random.RandomState(seed)
    nkf = max(nconn + 3, 8) if nkf is None else nkf
    Tcw = np.array([_rand_pose(rng) for _ in range(nkf)])
    conn = rng.permutation(nkf)[:nconn].astype(np.int32)
    rank = rng.permutation(nconn).astype(np.int32)
    rank[[0, int(np.argmax(rank))]] = rank[[int(np.argmax(rank)), 0]]          # (the first keyframe of the list comes last in the map: it wins no contest)
    s = 1.0 + 0.08 * rng.rand()
    q = rng.randn(4); q *= math.sqrt(s) / np.linalg.norm(q)
    Scw = np.concatenate([q, rng.uniform(-2, 2, 3)])
    X = rng.uniform(-10, 10, (npts, 3))
    slots = []
    base = int(rng.randint(0, npts))
    for c in range(nconn):
        n = int(rng.randint(max_slots // 2, max_slots))                           # (one slot is added below: at most max_slots)
        centre = base + int(rng.randint(0, max_slots * nconn // 6 + 1))         # (the windows of a small group overlap, those of a large one cover the map)
        pts = (centre + rng.randint(-min(npts, 2 * max_slots) // 2, min(npts, 2 * max_slots) // 2 + 1, n)) % npts
        pts = list(dict.fromkeys(pts.tolist()))
        if nulls:
            for i in rng.randint(0, len(pts), max(1, len(pts) // 10)):
                pts[i] = -1
            pts.insert(int(rng.randint(0, len(pts))), int(pts[0]))             # (a slot list naming a point twice)
        slots.append(pts)
    group = conn.tolist()
    obs = []
    for p in range(npts):
        n = int(rng.randint(1, 13))
        # most observers come from the group, so that the half-old, half-new centres matter
        cand = [group[i] for i in rng.randint(0, nconn, n)] + rng.randint(0, nkf, 2).tolist()
        ks = list(dict.fromkeys(cand))[:12]
        obs.append(sorted(ks))
    if long_list:
        obs[npts // 2] = rng.randint(0, nkf, 600).tolist()                     # (the walk does not need distinct observers)
    obs[0] = []
    ref_kf = [o[int(rng.randint(0, len(o)))] if o else 0 for o in obs]
    ref_level = rng.randint(0, 8, npts)
    pt_bad = (rng.rand(npts) < 0.05).astype(np.uint8)
    pt_done = (rng.rand(npts) < 0.05).astype(np.uint8)
    return loop_problem(Tcw, conn, Scw, slots, X, conn_rank=rank, pt_bad=pt_bad, pt_done=pt_done, obs=obs, ref_kf=ref_kf, ref_level=ref_level)


def make_gba(seed, nkf, npts=400):
    """a random forest over nkf keyframes (two origins from 5 keyframes on, a few keyframes cut off), a third of the keyframes outside the
    BA in runs along the tree, points of the three kinds"""
    rng = np.random.RandomState(seed)
    Tcw = np.array([_rand_pose(rng) for _ in range(nkf)])
    gba = np.array([_rand_pose(rng) for _ in range(nkf)])
    order = rng.permutation(nkf)
    origins = order[:2 if nkf >= 5 else 1]
    parent = np.full(nkf, -1, np.int32)
    in_gba = np.ones(nkf, np.uint8)
    placed = list(origins)
    for k in order[len(origins):]:
        # the parent is one of the last few placed: deep enough for runs outside the BA, bushy enough for a cut to cost a subtree only
        parent[k] = placed[-1 - int(rng.randint(0, min(6, len(placed))))]
        in_gba[k] = 0 if (not in_gba[parent[k]] and rng.rand() < 0.7) or rng.rand() < 0.15 else 1
        placed.append(k)
    if nkf >= 64:
        for k in rng.permutation(order[-(nkf // 4):])[:nkf // 16]:             # (erased by its parent: the subtree below is not reached)
            parent[k] = -1
    X = rng.uniform(-10, 10, (npts, 3))
    kind = rng.rand(npts)
    pt_in_gba = (kind < 0.4).astype(np.uint8)
    pt_bad = (rng.rand(npts) < 0.05).astype(np.uint8)
    ref = rng.randint(0, nkf, npts)
    return gba_problem(Tcw, gba, in_gba, parent, origins, X, ref, pt_bad=pt_bad, pt_in_gba=pt_in_gba, pt_gba_X=rng.uniform(-10, 10, (npts, 3)))


def seeded_loop():
    out = []
    for i, (nconn, npts, long_list) in enumerate(((1, 255, False), (3, 257, False), (20, 3000, True), (65, 3000, False), (20, 255, False), (3, 3000, False))):
        out.append(("loop nconn %d npts %d" % (nconn, npts), make_loop(100 + i, nconn, npts, long_list=long_list)))
    return out


def seeded_gba():
    return [("gba nkf %d" % nkf, make_gba(200 + nkf, nkf)) for nkf in (1, 5, 64, 65, 1100)]
