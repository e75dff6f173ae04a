"""Hand-worked cases, with their expected outputs written out, and a seeded map generator for the SearchInNeighbors entries
(orbl_fuse_targets, orbl_fuse_rows, orbl_fuse_candidates, orbl_update_map_points_on_tables, localmapping.search_in_neighbors_on_tables).
TEST INFRASTRUCTURE; the maps are dicts of flat numpy arrays, named as tests/npsearchneighbors.py names them."""
import numpy as np

from tests import npsearchneighbors as ns

F32 = np.float32
SF = (F32(1.2) ** np.arange(8)).astype(F32)
INV_SIGMA2 = (F32(1.0) / (SF * SF)).astype(F32)
SEEDS = (4, 6)                        # the committed seeds: tests/test_searchneighbors_restatement.py holds their path counters to be non-zero
NEAR_INTEGER = 1e-3                   # the generator redraws a point whose PredictScale quotient is this close to an integer in any keyframe


# ------------------------------------------------------------------------------------------------------------------ targets
def _ord_tables(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(v) for v in lists])
    return off, np.array([k for v in lists for k in v], np.int32)


def target_cases():
    """name -> dict(tab, cur_kf, cur_id, nn, nn2, tgt_kf, counts, kf_fuse_target): the last three are the expected outputs, worked by hand"""
    cases = {}
    # cur = 0, id 7.  Its list: 1, 2 (bad), 3 (stamped at entry), 4.
    #   1: pushed, stamped.  Its list: 0 = the current keyframe (skipped), 4 = a LATER first neighbour (pushed, not stamped), 5 (pushed).
    #   2: bad.  3: stamped 7 at entry.
    #   4: not stamped by the push above, so pushed again and stamped.  Its list: 1 = an EARLIER first neighbour (stamped: skipped), 5 =
    #      reached through 1 already (pushed again), 6 (pushed), 2 (bad: skipped).
    off, kf = _ord_tables([[1, 2, 3, 4], [0, 4, 5], [0], [0], [1, 5, 6, 2], [1], [4], []])
    cases["mixed"] = dict(tab=dict(kf_bad=np.array([0, 0, 1, 0, 0, 0, 0, 0], np.uint8), ord_off=off, ord_kf=kf, kf_fuse_target=np.array([0, 0, 0, 7, 0, 0, 0, 7], np.int32)),
                          cur_kf=0, cur_id=7, nn=20, nn2=5, tgt_kf=[1, 4, 5, 4, 5, 6], counts=[6, 2], kf_fuse_target=[0, 7, 0, 7, 7, 0, 0, 7])
    # both lists longer than the limits: nn = 2 cuts 3 off the first list, nn2 = 1 leaves one second neighbour each.
    #   1: pushed, stamped; its first entry 2: pushed.  2: not stamped, pushed and stamped; its first entry 3: pushed.
    off, kf = _ord_tables([[1, 2, 3], [2, 3], [3, 1], [0]])
    cases["cut"] = dict(tab=dict(kf_bad=None, ord_off=off, ord_kf=kf, kf_fuse_target=np.zeros(4, np.int32)), cur_kf=0, cur_id=1, nn=2, nn2=1, tgt_kf=[1, 2, 2, 3],
                        counts=[4, 2], kf_fuse_target=[0, 1, 1, 0])
    # the current keyframe has no neighbour
    off, kf = _ord_tables([[], [0]])
    cases["empty"] = dict(tab=dict(kf_bad=None, ord_off=off, ord_kf=kf, kf_fuse_target=np.zeros(2, np.int32)), cur_kf=0, cur_id=5, nn=20, nn2=5, tgt_kf=[], counts=[0, 0],
                          kf_fuse_target=[0, 0])
    return cases


# ------------------------------------------------------------------------------------------------------------------ rows
def _bits(d):
    """a descriptor at Hamming distance d from the all-zero one"""
    b = np.zeros(256, np.uint8)
    b[:d] = 1
    return np.packbits(b)


def row_case():
    """One keyframe (0) with 69 keypoints under [I | 0], fx = fy = 128, cx = 320, cy = 240, image [0, 640) x [0, 480); keyframe 1 has no
    keypoint.  A point at (x, y, 4) projects to (320 + 32 x, 240 + 32 y) exactly.  Unless said otherwise a point has its normal towards the
    camera, min_dist far below and max_dist = dist * 1.2^(L - 0.2), so that PredictScale gives L (4: the radius is 3 * 1.2^4 = 6.22) with the
    quotient 0.2 away from an integer.  Every point's descriptor is zero, a keypoint's has `d` bits set: its distance.
    Returns dict(tab, pts, expect = {keyframe: dict(op_kind, op_slot, best_idx, best_dist, q_level)}), the expectations worked by hand."""
    kps, pts = [], []

    def kp(x, y, lvl, d):
        kps.append((x, y, lvl, d))
        return len(kps) - 1

    def pt(X, L=4, normal=None, min_dist=None, max_dist=None):
        X = np.array(X, np.float64)
        dist = float(np.sqrt((X[0] * X[0] + X[1] * X[1]) + X[2] * X[2]))
        pts.append(dict(X=X, normal=X / dist if normal is None else np.array(normal, np.float64), min_dist=F32(0.01 * dist if min_dist is None else min_dist),
                        max_dist=F32(dist * 1.2 ** (L - 0.2) if max_dist is None else max_dist)))
        return len(pts) - 1

    E = []                                                                   # per point: (kind, slot, best_idx, best_dist, q_level) for keyframe 0
    pt((0, 0, -4)); E.append((0, -1, -1, 256, -1))                            # 0: negative depth
    # 1: u == min_x is kept.  (-10, 0, 4): invz = 0.25, x = -2.5, u = 128 * -2.5 + 320 = 0 exactly; dist = sqrt(116) = 10.77, L = 1, radius 3.6
    pt((-10, 0, 4), L=1); k = kp(0.5, 240, 1, 0); E.append((4, k, k, 0, 1))
    pt((10, 0, 4), L=1); E.append((0, -1, -1, 256, -1))                       # 2: u == max_x = 640 is dropped
    pt((-6, 0, 4), min_dist=100.0); E.append((0, -1, -1, 256, -1))           # 3: dist 7.2 < 0.8 * 100
    pt((-5, 0, 4), max_dist=5.0); E.append((0, -1, -1, 256, -1))             # 4: dist 6.4 > 1.2 * 5
    # 5: PO.Pn == 0.5 dist is kept: PO = (0, 0, 4), Pn = (0, 0, 0.5): 2.0 < 2.0 is false
    pt((0, 0, 4), normal=(0, 0, 0.5)); k = kp(320, 240, 4, 3); E.append((4, k, k, 3, 4))
    pt((0, 2, 4), normal=(0, 0.49 * 2 / np.sqrt(20.0), 0.49 * 4 / np.sqrt(20.0))); E.append((0, -1, -1, 256, -1))          # 6: PO.Pn = 0.49 dist
    # 7: the level clamped at the top: (2, 0, 1) -> (576, 240), quotient 11.8 -> 12 -> 7, radius 10.75; the level-6 keypoint is in the window too
    pt((2, 0, 1), L=12); k = kp(576, 240, 7, 5); kp(578, 240, 6, 9); E.append((4, k, k, 5, 7))
    # 8: the bottom of the level range: the quotient is -0.2, whose ceiling is (minus) zero: level 0, window [-1, 0], radius 3.  The distance gate
    # keeps the quotient above -1, so a ceiling below zero passes it only when dist == 1.2 max exactly, which would pin logf to the bit: the
    # clamp itself (`level < 0`) is covered by the restatement's counter alone.  The level-1 keypoint with distance 0 is outside the window.
    pt((-4, 2, 4), L=0); k = kp(192, 304, 0, 7); kp(193, 304, 1, 0); E.append((4, k, k, 7, 0))
    pt((-3, 2, 4)); kp(224, 304, 2, 0); kp(225, 304, 5, 0); E.append((0, -1, -1, 256, 4))              # 9: the level window [3, 4]: no candidate passes
    # 10: chi-square: inv_level_sigma2[3] = 1.2^-6 = 0.3349: e = 4.5 gives 6.78 > 5.99 (rejected, distance 0), e = 4 gives 5.36 (kept, distance 9)
    pt((-2, 2, 4)); kp(260.5, 304, 3, 0); k = kp(260, 304, 3, 9); E.append((4, k, k, 9, 4))
    pt((-1, 2, 4)); k = kp(288, 304, 4, 50); E.append((4, k, k, 50, 4))      # 11: TH_LOW itself is kept
    pt((1, 2, 4)); k = kp(352, 304, 4, 51); E.append((0, -1, k, 51, 4))      # 12: 51 is dropped; the best is still reported
    # 13: equal distances where cell order and index order disagree: (0.15625, -2, 4) -> (325, 176).  The keypoint with the LOWER index is at
    # x = 326: cell round(32.6) = 33; the one with the higher index at x = 323: cell 32, which GetFeaturesInArea visits first, so it wins.
    pt((0.15625, -2, 4)); kp(326, 176, 4, 6); k = kp(323, 176, 4, 6); E.append((4, k, k, 6, 4))
    # 14: a keypoint outside the grid: x = 639.9 -> round(63.99) = 64 >= 64 columns: in no cell, though 1.9 px from the projection (638, 176)
    pt((9.9375, -2, 4)); kp(639.9, 176, 4, 0); E.append((0, -1, -1, 256, 4))
    pts.append(None); E.append((0, -1, -1, 256, -1))                         # 15: a null point
    while len(kps) < 68:                                                     # more than 64 keypoints: the match of point 16 is index 68
        kp(600, 440, 7, 200)
    pt((-7, -2, 4)); k = kp(96, 176, 4, 2); E.append((4, k, k, 2, 4))        # 16
    assert k == 68
    real = [p for p in pts if p is not None]
    n = len(kps)
    tab = dict(kf_bad=None, kf_rank=None, kf_Tcw=np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64), (2, 1)), kf_center=np.zeros((2, 3)),
               kf_K4=np.tile(np.array([128, 128, 320, 240], F32), (2, 1)), kf_bounds=np.tile(np.array([0, 640, 0, 480], F32), (2, 1)),
               kf_slot_off=np.array([0, n, n], np.int32), kf_slot_pt=np.full(n, -1, np.int32), kf_slot_uv=np.array([(k[0], k[1]) for k in kps], F32),
               kf_slot_level=np.array([k[2] for k in kps], np.int32), kf_slot_desc=np.stack([_bits(k[3]) for k in kps]),
               X=np.stack([p["X"] for p in real]), pt_normal=np.stack([p["normal"] for p in real]), pt_min_dist=np.array([p["min_dist"] for p in real], F32),
               pt_max_dist=np.array([p["max_dist"] for p in real], F32), pt_desc=np.zeros((len(real), 32), np.uint8), pt_bad=np.zeros(len(real), np.uint8),
               pt_nobs=np.zeros(len(real), np.int32), obs_off=np.zeros(len(real) + 1, np.int32), obs_kf=np.zeros(0, np.int32), obs_slot=np.zeros(0, np.int32),
               scale_factors=SF.copy(), inv_level_sigma2=INV_SIGMA2.copy())
    ids, nxt = [], 0
    for p in pts:
        ids.append(-1 if p is None else nxt)
        nxt += p is not None
    names = ("op_kind", "op_slot", "best_idx", "best_dist", "q_level")
    e0 = {k: [e[i] for e in E] for i, k in enumerate(names)}
    # keyframe 1 has no keypoint: the same projections, no candidate anywhere
    e1 = dict(op_kind=[0] * len(E), op_slot=[-1] * len(E), best_idx=[-1] * len(E), best_dist=[256] * len(E), q_level=list(e0["q_level"]))
    return dict(tab=tab, pts=np.array(ids, np.int32), expect={0: e0, 1: e1})


# ------------------------------------------------------------------------------------------------------------------ candidates
def candidate_case():
    """targets 1, 2, 1 (one listed twice); cur_id 9.  Keyframe 1 holds 0, null, 1 (bad), 2 (stamped 9 at entry), 3; keyframe 2 holds 3 (held by two
    targets: emitted once, by the first), 4, 0 (emitted already), 5.  The second walk of keyframe 1 finds everything stamped."""
    tab = dict(kf_slot_off=np.array([0, 0, 5, 9], np.int32), kf_slot_pt=np.array([0, -1, 1, 2, 3, 3, 4, 0, 5], np.int32), pt_bad=np.array([0, 1, 0, 0, 0, 0, 0], np.uint8),
               pt_fuse_cand=np.array([0, 0, 9, 0, 8, 0, 0], np.int32))
    return dict(tab=tab, tgt_kf=[1, 2, 1], cur_id=9, cand_pt=[0, 3, 4, 5], counts=[4, 3], pt_fuse_cand=[9, 0, 9, 9, 9, 9, 0])


# ------------------------------------------------------------------------------------------------------------------ the seeded maps
def _flip(rng, d, n):
    b = np.unpackbits(d)
    b[rng.choice(256, n, replace=False)] ^= 1
    return np.packbits(b)


def make(seed, nkf=12, ngroups=190):
    """A corridor of nkf keyframes looking along z and ngroups places, each holding one to three map points a few millimetres apart with
    similar descriptors (the duplicates SearchInNeighbors exists to fuse).  A keyframe that sees a place has a keypoint there for ONE of its
    points, or a keypoint that holds no point, or none.  Returns dict(tab, cur_kf, cur_id, redrawn = how often the near-integer rule drew
    again)."""
    rng = np.random.default_rng(seed)
    cur_kf, cur_id = nkf // 2, 40 + seed
    T, ctr = np.zeros((nkf, 12)), np.zeros((nkf, 3))
    for k in range(nkf):
        a = rng.normal(0, 0.02)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        c = np.array([0.3 * k + rng.normal(0, 0.02), rng.normal(0, 0.02), rng.normal(0, 0.02)])
        T[k] = np.concatenate([R, (-R @ c)[:, None]], 1).reshape(-1)
        t = T[k]
        for i in range(3):                                                   # the centre as KeyFrame::SetPose stores it
            ctr[k, i] = -((t[i] * t[3] + t[4 + i] * t[7]) + t[8 + i] * t[11])
    K4 = np.tile(np.array([500, 500, 320, 240], F32), (nkf, 1)); bounds = np.tile(np.array([0, 640, 0, 480], F32), (nkf, 1))
    kf_bad = np.zeros(nkf, np.uint8)
    kf_bad[(cur_kf + 3) % nkf] = 1
    kf_rank = rng.permutation(nkf).astype(np.int32)
    slots = [[] for _ in range(nkf)]                                         # per keyframe: [u, v, level, desc, point]
    X, normal, min_d, max_d, ref_kf, obs = [], [], [], [], [], []
    redrawn = 0

    def uv_of(k, P):
        c = T[k].reshape(3, 4) @ np.append(P, 1.0)
        return (500 * c[0] / c[2] + 320, 500 * c[1] / c[2] + 240) if c[2] > 0.1 else (-1e9, -1e9)

    for _ in range(ngroups):
        place = np.array([rng.uniform(-2.5, 0.3 * nkf + 2.5), rng.uniform(-1.8, 1.8), rng.uniform(4, 11)])
        sees = [k for k in range(nkf) if 20 < uv_of(k, place)[0] < 620 and 20 < uv_of(k, place)[1] < 460]
        if len(sees) < 2:
            continue
        nm = int(rng.choice([1, 2, 3], p=[0.45, 0.35, 0.2]))
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        holder = {k: int(rng.integers(0, nm)) for k in sees if rng.random() < 0.6}            # keyframe -> the member it observes
        free = [k for k in sees if k not in holder and rng.random() < 0.25]
        first = len(X)
        for m in range(nm):
            mine = [k for k in sees if holder.get(k) == m]
            if not mine:                                                     # every point is observed somewhere
                k = int(rng.choice([k for k in sees if k not in holder] or sees))
                holder[k] = m; mine = [k]
                if k in free:
                    free.remove(k)
            mine = [k for k in sees if holder.get(k) == m]
            mbase = _flip(rng, base, int(rng.integers(0, 13)))
            while True:                                                      # the near-integer rule: draw the point again, never leave it out
                P = place + rng.normal(0, 0.002, 3)
                r = mine[0]
                dref = F32(np.linalg.norm(P - ctr[r]))
                mx = F32(dref * SF[int(rng.integers(1, 5))] * F32(rng.uniform(0.90, 0.99)))
                q = [float(ns.log_ratio(mx, F32(np.linalg.norm(P - ctr[k])))) for k in range(nkf)]
                if all(abs(v - round(v)) > NEAR_INTEGER for v in q):
                    break
                redrawn += 1
            p = len(X)
            X.append(P); max_d.append(mx); min_d.append(F32(mx / SF[7])); ref_kf.append(r)
            v = P - ctr[mine].mean(0)
            normal.append(v / np.linalg.norm(v) * (-1.0 if rng.random() < 0.05 else 1.0))         # (a few seen from behind: the viewing gate)
            obs.append({})
            for k in mine:
                u0, v0 = uv_of(k, P)
                lvl = min(7, max(0, int(np.ceil(q[k])) - int(rng.random() < 0.3)))
                obs[p][k] = len(slots[k])
                slots[k].append([F32(u0 + rng.normal(0, 0.4)), F32(v0 + rng.normal(0, 0.4)), lvl, _flip(rng, mbase, int(rng.integers(0, 15))), p])
        for k in free:
            u0, v0 = uv_of(k, X[first])
            q0 = float(ns.log_ratio(max_d[first], F32(np.linalg.norm(X[first] - ctr[k]))))
            slots[k].append([F32(u0 + rng.normal(0, 0.4)), F32(v0 + rng.normal(0, 0.4)), min(7, max(0, int(np.ceil(q0)))), _flip(rng, base, int(rng.integers(0, 20))), -1])
    w = np.zeros((nkf, nkf), np.int64)
    for o in obs:
        for a in o:
            for b in o:
                w[a, b] += a != b
    ords = [sorted([b for b in range(nkf) if w[a, b] > 0], key=lambda b: (-w[a, b], kf_rank[b])) for a in range(nkf)]
    ord_off, ord_kf = _ord_tables(ords)
    conn = [[b for b in range(nkf) if w[a, b] >= 15] for a in range(nkf)]
    conn_off, conn_kf = _ord_tables(conn)
    stamp_kf = np.zeros(nkf, np.int32)
    if len(ords[cur_kf]) > 3:
        stamp_kf[ords[cur_kf][2]] = cur_id                                   # a neighbour stamped at entry
    # The injected chain case (the covisibility lists above stay as they are: ordered_connected_keyframes_ is as old as the last
    # UpdateConnections).  Point A is seen by the current keyframe (descriptor a) and by Z (a2, 36 bits away) and holds a; its duplicate B
    # is seen by the first target T1 alone (b, 4 bits from a2).  At T1 A meets B: 1 observation against 2, Replace(B, A), and A's
    # descriptor is recomputed over {a, a2, b}: a2 or b.  A later target T2 has two keypoints without a point at the place: c1 next to a,
    # c2 next to a2.  The stale descriptor would take c1, the recomputed one takes c2.
    targets = [int(k) for k in ns.fuse_targets(dict(kf_bad=kf_bad, ord_off=ord_off, ord_kf=ord_kf, kf_fuse_target=stamp_kf), cur_kf, cur_id)["tgt_kf"]]
    T1 = targets[0]
    T2 = next(k for k in targets[1:] if k != T1)
    Z = next(k for k in range(nkf) if k not in (cur_kf, T1, T2) and not kf_bad[k])
    place = np.array([ctr[[cur_kf, T1, T2, Z], 0].mean(), 0.5, 8.0])
    da = rng.integers(0, 256, 32, dtype=np.uint8)
    da2 = _flip(rng, da, 36)
    for holders, descs in (((cur_kf, Z), (da, da2)), ((T1,), (_flip(rng, da2, 4),))):
        while True:
            P = place + rng.normal(0, 0.002, 3)
            mx = F32(F32(np.linalg.norm(P - ctr[holders[0]])) * SF[2] * F32(rng.uniform(0.90, 0.99)))
            q = [float(ns.log_ratio(mx, F32(np.linalg.norm(P - ctr[k])))) for k in range(nkf)]
            if all(abs(v - round(v)) > NEAR_INTEGER for v in q):
                break
            redrawn += 1
        p = len(X)
        X.append(P); max_d.append(mx); min_d.append(F32(mx / SF[7])); ref_kf.append(holders[0])
        v = P - ctr[list(holders)].mean(0)
        normal.append(v / np.linalg.norm(v))
        obs.append({})
        for k, d in zip(holders, descs):
            u0, v0 = uv_of(k, P)
            obs[p][k] = len(slots[k])
            slots[k].append([F32(u0), F32(v0), min(7, max(0, int(np.ceil(q[k])))), d, p])
        if len(holders) == 2:
            injected, qa = p, q
    u0, v0 = uv_of(T2, X[injected])
    for d in (_flip(rng, da, 3), _flip(rng, da2, 5)):
        slots[T2].append([F32(u0), F32(v0), min(7, max(0, int(np.ceil(qa[T2])))), d, -1])
    npts = len(X)
    # four points caught in the middle of a SetBadFlag by another thread: bad, the list cleared, the slots not yet (the isBad() tests of both
    # Fuse directions and of the candidate loop)
    pt_bad = np.zeros(npts, np.uint8)
    for p in rng.choice(injected, 4, replace=False):
        pt_bad[p] = 1
        obs[p] = {}
    off = np.zeros(nkf + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in slots])
    flat = [s for ks in slots for s in ks]
    order = lambda p: sorted(obs[p].items(), key=lambda ks: kf_rank[ks[0]])                     # noqa: E731
    obs_off = np.zeros(npts + 1, np.int32)
    obs_off[1:] = np.cumsum([len(o) for o in obs])
    stamp_pt = np.where(rng.random(npts) < 0.03, cur_id, 0).astype(np.int32)
    tab = dict(kf_bad=kf_bad, kf_rank=kf_rank, kf_Tcw=T, kf_center=ctr, kf_K4=K4, kf_bounds=bounds, kf_slot_off=off, kf_slot_pt=np.array([s[4] for s in flat], np.int32),
               kf_slot_uv=np.array([(s[0], s[1]) for s in flat], F32), kf_slot_level=np.array([s[2] for s in flat], np.int32), kf_slot_desc=np.stack([s[3] for s in flat]),
               X=np.stack(X), pt_normal=np.stack(normal), pt_min_dist=np.array(min_d, F32), pt_max_dist=np.array(max_d, F32), pt_desc=np.zeros((npts, 32), np.uint8),
               pt_bad=pt_bad, pt_nobs=np.array([len(o) for o in obs], np.int32), pt_found=rng.integers(1, 30, npts).astype(np.int32),
               pt_visible=rng.integers(30, 60, npts).astype(np.int32), pt_replaced=np.full(npts, -1, np.int32), pt_ref_kf=np.array(ref_kf, np.int32), obs_off=obs_off,
               obs_kf=np.array([k for p in range(npts) for k, _ in order(p)], np.int32), obs_slot=np.array([s for p in range(npts) for _, s in order(p)], np.int32),
               ord_off=ord_off, ord_kf=ord_kf, conn_off=conn_off, conn_kf=conn_kf, conn_w=np.array([w[a, b] for a in range(nkf) for b in conn[a]], np.int32),
               kf_fuse_target=stamp_kf, pt_fuse_cand=stamp_pt, scale_factors=SF.copy(), inv_level_sigma2=INV_SIGMA2.copy())
    M = ns.Map(tab)
    for p in range(npts):                                                    # every point starts with its distinctive descriptor
        M.compute_distinctive_descriptors(p)
    tab["pt_desc"] = M.desc.copy()
    tab["pt_desc"][injected] = da                                            # (A holds a, whichever of its two keyframes ranks first)
    return dict(tab=tab, cur_kf=cur_kf, cur_id=cur_id, redrawn=redrawn, injected=injected)
