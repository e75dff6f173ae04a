"""Map tables for the tests of orbl_essential_graph_assemble / orbl_essential_graph_apply: a hand-worked map of 7 keyframes with its edge
list written out, the empty and one-vertex cases, seeded maps whose keyframe counts cross one and two scan units of 256, and a closed
loop with drift for the end-to-end test.  Plain numpy; nothing of the library is called here.

A map is a dict: nkf, kf_id, kf_bad, kf_rank, kf_Tcw [nkf, 12], kf_center [nkf, 3], kf_parent, child_off / child_kf, loop_off / loop_kf,
conn_off / conn_kf / conn_w, ord_off / ord_kf / ord_w, conn_group_kf, corrected, non_corrected [nconn, 7], tgt_kf, link_off / link_kf,
loop, cur (keyframe indices), min_weight; npts, X, pt_bad, pt_done, pt_corr_ref, pt_ref_kf, obs_off, obs_kf, ref_level, scale_factors."""
import numpy as np

POISON = -12345.0
SF = np.array([1.2 ** i for i in range(8)], np.float32)


def rot(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose12(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], axis=1).reshape(12)


def centres(T):
    T = np.asarray(T, np.float64).reshape(-1, 3, 4)
    return np.stack([-(t[:, :3].T @ t[:, 3]) for t in T]) if len(T) else np.zeros((0, 3))


def quat_of(R):
    """a unit quaternion (x, y, z, w) of a rotation well away from angle pi (the tests' group Sim3s are inputs: any branch will do)"""
    w = 0.5 * np.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2])
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def sim3_of(R, t, s):
    """Sophus::Sim3d storage of [sR | t]: the quaternion times sqrt(s), then t"""
    return np.concatenate([quat_of(R) * np.sqrt(s), np.asarray(t, np.float64)])


def csr(rows, dt=np.int32):
    off = np.zeros(len(rows) + 1, np.int32)
    for i, r in enumerate(rows):
        off[i + 1] = off[i] + len(r)
    flat = np.array([v for r in rows for v in r], dt).reshape(-1)
    return off, flat


def _finish(m, parents, children, loops, weights, ordered, group, links, pts):
    """rows as Python lists -> the CSR tables; group: [(kf, corrected, non_corrected)], links: [(target, [kf...])],
    pts: dict(X, bad, done, corr_ref, ref, obs rows, level)"""
    nkf = m["nkf"]
    m["kf_parent"] = np.array(parents, np.int32)
    m["child_off"], m["child_kf"] = csr(children)
    m["loop_off"], m["loop_kf"] = csr(loops)
    m["conn_off"], m["conn_kf"] = csr([[k for k, _ in r] for r in weights]); m["conn_w"] = csr([[w for _, w in r] for r in weights])[1]
    m["ord_off"], m["ord_kf"] = csr([[k for k, _ in r] for r in ordered]); m["ord_w"] = csr([[w for _, w in r] for r in ordered])[1]
    m["conn_group_kf"] = np.array([g[0] for g in group], np.int32)
    m["corrected"] = np.array([g[1] for g in group], np.float64).reshape(-1, 7); m["non_corrected"] = np.array([g[2] for g in group], np.float64).reshape(-1, 7)
    m["tgt_kf"] = np.array([t for t, _ in links], np.int32)
    m["link_off"], m["link_kf"] = csr([r for _, r in links])
    m["kf_center"] = centres(m["kf_Tcw"])
    m["npts"] = len(pts["X"])
    m["X"] = np.array(pts["X"], np.float64).reshape(-1, 3)
    for k, s, dt in (("pt_bad", "bad", np.uint8), ("pt_done", "done", np.uint8), ("pt_corr_ref", "corr_ref", np.int32), ("pt_ref_kf", "ref", np.int32), ("ref_level", "level", np.int32)):
        m[k] = np.array(pts[s], dt).reshape(-1)
    m["obs_off"], m["obs_kf"] = csr(pts["obs"])
    m["scale_factors"] = SF.copy()
    m.setdefault("min_weight", 100)
    assert len(m["kf_id"]) == nkf and len(m["kf_Tcw"]) == nkf
    for v in m.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)                                 # (the maps are shared between tests)
    return m


def se3_as_sim3(T12):
    """Sim3d(RxSO3d(1, R), t) of a pose, as a test INPUT (non_corrected): the quaternion of quat_of"""
    T = np.asarray(T12, np.float64).reshape(3, 4)
    return sim3_of(T[:, :3], T[:, 3], 1.0)


def hand_map():
    """7 keyframes, keyframe 3 bad, group (4, 5, 6) ending in the current keyframe 6, loop keyframe 0 at the identity pose.  Returns the
    map and its edge list worked out by hand (tests/test_essgraph_restatement.py spells out which rule gives or takes each edge)."""
    ids = [0, 25, 20, 30, 40, 50, 60]
    rank = [3, 0, 5, 1, 6, 2, 4]                                    # ascending: keyframes 1, 3 (bad), 5, 0, 6, 2, 4
    axes = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)]
    T = [pose12(np.eye(3), (0, 0, 0))] + [pose12(rot(axes[k], 0.3 + 0.1 * k), (k, -0.5 * k, 2.0 + k)) for k in range(1, 7)]
    m = dict(nkf=7, kf_id=np.array(ids, np.int32), kf_bad=np.array([0, 0, 0, 1, 0, 0, 0], np.uint8), kf_rank=np.array(rank, np.int32), kf_Tcw=np.array(T), loop=0, cur=6)
    parents = [-1, 0, 5, 2, 3, 4, 5]                                # 2's parent is in the group, 4's parent is bad
    children = [[1], [], [3], [4], [5], [6, 2], []]
    loops = [[], [5], [], [], [], [6, 1], [5]]                      # 5 <-> 1 (smaller id seen from 5), 5 <-> 6 (larger id seen from 5)
    ordered = [[(1, 125)],                                          # every weight passes: GetCovisiblesByWeight gives nothing
               [(5, 130), (2, 110), (4, 100), (6, 90)],             # straddles 100; 2 has the smaller id: a covisibility edge
               [(5, 150), (6, 120), (0, 115), (1, 110)],            # every weight passes: NO covisibility edge, though 0 qualifies
               [],
               [(5, 200), (3, 105), (1, 100), (0, 20)],             # 5 a child, 3 the (bad) parent, 1 already in inserted_edges
               [(6, 300), (4, 200), (2, 150), (1, 130), (3, 105), (0, 40)],     # 6 and 2 children, 4 the parent, 1 a loop edge, 3 bad
               [(5, 300), (4, 150), (2, 120), (3, 110), (1, 90)]]   # 5 the parent, 4 an edge, 2 in inserted_edges, 3 bad
    weights = [list(reversed(r)) for r in ordered]                  # the same connections in another order; (6, 0) is absent: weight 0
    grp = []
    for k in (4, 5, 6):
        Tk = T[k].reshape(3, 4)
        grp.append((k, sim3_of(rot(axes[k], 0.32 + 0.1 * k), Tk[:, 3] * 1.1 + 0.05, 1.1), se3_as_sim3(T[k])))
    links = [(4, [1]), (6, [2, 0, 3, 1])]                           # 6: 1 below min_weight, 3 bad (dropped), 0 the exempt (current, loop) pair of weight 0
    pts = dict(X=[[1, 2, 8], [0, 1, 9], [2, 2, 7], [3, 3, 3], [1, 1, 6], [0, 2, 5]], bad=[0, 0, 0, 1, 0, 0], done=[0, 0, 1, 0, 0, 0], corr_ref=[-1, -1, 6, -1, -1, -1],
               ref=[1, 3, 3, 2, -1, 2], obs=[[1, 5], [3, 0], [3, 6, 2], [2], [0], []], level=[0, 1, 2, 3, 4, 5])
    m = _finish(m, parents, children, loops, weights, ordered, grp, links, pts)
    hand = dict(vtx_kf=[1, 5, 0, 6, 2, 4], kf_vtx=[2, 0, 4, -1, 5, 1, 3], vtx_fixed=[0, 0, 1, 0, 0, 0],
                edges=[(0, 6, 0), (2, 6, 0), (1, 4, 0),             # loop connections: target 6's row by rank (1 skipped, 3 dropped, 0, 2), then target 4's
                       (0, 1, 1), (2, 1, 3),                        # keyframe 1: its parent, covisible 2
                       (4, 5, 1), (1, 5, 2),                        # keyframe 5: its parent, loop edge 1 (6 has the larger id)
                       (5, 6, 1), (5, 6, 2), (4, 6, 3),             # keyframe 6: its parent, loop edge 5, covisible 4
                       (5, 2, 1)],                                  # keyframe 2: its parent; keyframe 4 gives nothing (its parent is bad: dropped)
                counts=[6, 11, 3, 2], pt_moved=[1, 0, 1, 0, 0, 1], nd_written=[1, 0, 1, 0, 0, 0], apply_counts=[6, 3])
    return m, hand


def small_cases():
    """nkf = 1 without targets and with a group of one; two keyframes without any edge"""
    I = pose12(np.eye(3), (0, 0, 0))
    T1 = pose12(rot((0, 1, 0), 0.4), (1, 2, 3))
    none = dict(X=[], bad=[], done=[], corr_ref=[], ref=[], obs=[], level=[])
    out = {}
    m = dict(nkf=1, kf_id=np.array([7], np.int32), kf_bad=None, kf_rank=None, kf_Tcw=np.array([T1]), loop=0, cur=0)
    out["one keyframe"] = _finish(m, [-1], [[]], [[]], [[]], [[]], [], [], dict(X=[[1, 2, 3]], bad=[0], done=[0], corr_ref=[-1], ref=[0], obs=[[0]], level=[1]))
    m = dict(nkf=1, kf_id=np.array([7], np.int32), kf_bad=np.array([0], np.uint8), kf_rank=np.array([0], np.int32), kf_Tcw=np.array([T1]), loop=0, cur=0)
    out["one keyframe in the group"] = _finish(m, [-1], [[]], [[]], [[]], [[]], [(0, sim3_of(rot((0, 1, 0), 0.45), (1.5, 2, 3), 1.2), se3_as_sim3(T1))], [(0, [])], none)
    m = dict(nkf=1, kf_id=np.array([7], np.int32), kf_bad=np.array([1], np.uint8), kf_rank=None, kf_Tcw=np.array([T1]), loop=0, cur=0)
    out["one bad keyframe"] = _finish(m, [-1], [[]], [[]], [[]], [[]], [], [], dict(X=[[1, 2, 3]], bad=[0], done=[0], corr_ref=[-1], ref=[0], obs=[[0]], level=[1]))
    m = dict(nkf=2, kf_id=np.array([1, 2], np.int32), kf_bad=None, kf_rank=np.array([1, 0], np.int32), kf_Tcw=np.array([I, T1]), loop=0, cur=1)
    out["no edges"] = _finish(m, [-1, -1], [[], []], [[], []], [[(1, 150)], [(0, 150)]], [[(1, 150)], [(0, 150)]], [(1, sim3_of(rot((0, 1, 0), 0.42), (1, 2, 3.5), 0.9), se3_as_sim3(T1))],
                              [], none)
    return out


def seeded_map(seed, nkf, npts, n_group=12):
    """a random map: shuffled ranks and ids, a few bad keyframes, parents by id, loop edges, symmetric weights around 100, loop connections of
    the group with entries below min_weight, bad ones and the exempt pair; rotations of 0.2 to 1.2 rad and scales of 0.9 to 1.1: well away
    from the branch points of s3_exp / s3_log"""
    rng = np.random.default_rng(seed)
    rank = rng.permutation(nkf).astype(np.int32)
    ids = (rng.permutation(nkf) * 3 + 1).astype(np.int32)
    bad = (rng.random(nkf) < 0.06).astype(np.uint8)
    by_id = np.argsort(ids)
    cur = int(by_id[-1]); loop = int(by_id[2])
    bad[cur] = 0; bad[loop] = 0
    dup = np.nonzero(bad)[0]
    if len(dup):
        ids[dup[0]] = ids[by_id[5]]                                 # (a bad keyframe may repeat an id)
    T = np.stack([pose12(rot(rng.normal(0, 1, 3), rng.uniform(0.2, 1.2)), rng.uniform(-10, 10, 3)) for _ in range(nkf)])
    m = dict(nkf=nkf, kf_id=ids, kf_bad=bad, kf_rank=rank, kf_Tcw=T, loop=loop, cur=cur)
    parents = [-1] * nkf; children = [[] for _ in range(nkf)]
    for pos in range(1, nkf):
        k = int(by_id[pos])
        if rng.random() < 0.03:
            continue
        p = int(by_id[rng.integers(max(0, pos - 8), pos)])
        parents[k] = p; children[p].append(k)
    loops = [[] for _ in range(nkf)]
    for _ in range(nkf // 10):
        a, b = (int(v) for v in rng.choice(nkf, 2, replace=False))
        if b not in loops[a]:
            loops[a].append(b); loops[b].append(a)
    w = [dict() for _ in range(nkf)]
    for k in range(nkf):
        for nb in rng.choice(nkf, 6, replace=False):
            nb = int(nb)
            if nb != k and nb not in w[k]:
                wt = int(rng.choice([15, 40, 99, 100, 101, 130, 250]))
                w[k][nb] = wt; w[nb][k] = wt
    for k in rng.choice(nkf, nkf // 8, replace=False):            # lists whose weights all pass
        for nb in list(w[int(k)]):
            w[int(k)][nb] = max(w[int(k)][nb], 100); w[nb][int(k)] = w[int(k)][nb]
    ordered = [sorted(w[k].items(), key=lambda kv: (-kv[1], rank[kv[0]])) if not bad[k] else [] for k in range(nkf)]      # (a bad keyframe's own list is gone)
    weights = [[(nb, w[k][nb]) for nb in rng.permutation(list(w[k]))] if w[k] else [] for k in range(nkf)]
    weights = [[(int(nb), int(wt)) for nb, wt in r] for r in weights]
    members = [int(v) for v in rng.choice([k for k in range(nkf) if not bad[k] and k != cur and k != loop], n_group - 1, replace=False)] + [cur]
    grp = []
    for k in members:
        Tk = T[k].reshape(3, 4)
        s = rng.uniform(0.9, 1.1)
        grp.append((k, sim3_of(Tk[:, :3] @ rot(rng.normal(0, 1, 3), 0.05), Tk[:, 3] * s + rng.normal(0, 0.1, 3), s), se3_as_sim3(T[k])))
    links = []
    for k in members:
        row = [int(v) for v in rng.choice(nkf, int(rng.integers(0, 6)), replace=False) if int(v) != k]
        row += [nb for nb in list(w[k])[:3]]
        if k == cur:
            row.append(loop)
        links.append((k, sorted(set(row), key=lambda v: -int(rank[v]))))           # (descending rank: the walk has to sort)
    order = rng.permutation(len(links))
    links = [links[i] for i in order]
    ref = rng.integers(0, nkf, npts).astype(np.int32); ref[rng.random(npts) < 0.02] = -1
    done = (rng.random(npts) < 0.3).astype(np.uint8)
    corr = np.where(done, np.array(members)[rng.integers(0, len(members), npts)], -1).astype(np.int32)
    obs = []
    for p in range(npts):
        n = int(rng.integers(0, 6))
        row = sorted(set(int(v) for v in rng.choice(nkf, n, replace=False)), key=lambda v: int(rank[v]))
        obs.append(row)
    pts = dict(X=rng.uniform(-20, 20, (npts, 3)), bad=(rng.random(npts) < 0.05).astype(np.uint8), done=done, corr_ref=corr, ref=ref, obs=obs, level=rng.integers(0, 8, npts))
    return _finish(m, parents, children, loops, weights, ordered, grp, links, pts)


def loop_map(seed, n=60, n_group=4, npts=400, drift=0.01):
    """a closed loop for the end-to-end test: n keyframes around a circle whose estimated positions drift, the last n_group carry their
    loop-corrected Sim3 (the true pose at scale 1.02), the current keyframe links to the loop keyframe 0 (weight 0: the exempt pair)"""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    Rt, tt, T = [], [], []
    d = np.zeros(3)
    for k in range(n):
        R = rot((0, 1, 0), -ang[k] + 0.3) @ rot((1, 0, 0), 0.25)
        Cw = np.array([30 * np.cos(ang[k]), 0.2 * np.sin(3 * ang[k]), 30 * np.sin(ang[k])])
        t = -R @ Cw
        Rt.append(R); tt.append(t)
        if k:
            d = d + rng.normal(0, drift, 3) + drift
        T.append(pose12(R @ rot(rng.normal(0, 1, 3), 0.002 if k else 0.0), t + d))
    rank = rng.permutation(n).astype(np.int32)
    m = dict(nkf=n, kf_id=np.arange(n, dtype=np.int32), kf_bad=np.zeros(n, np.uint8), kf_rank=rank, kf_Tcw=np.array(T), loop=0, cur=n - 1)
    parents = [-1] + list(range(n - 1)); children = [[k + 1] for k in range(n - 1)] + [[]]
    w = [dict() for _ in range(n)]
    for i in range(1, n):
        w[i][i - 1] = w[i - 1][i] = 200
        if i >= 3 and i % 5 == 0:
            w[i][i - 3] = w[i - 3][i] = 120
        if i >= 7:
            w[i][i - 7] = w[i - 7][i] = 40
    ordered = [sorted(w[k].items(), key=lambda kv: (-kv[1], kv[0])) for k in range(n)]
    weights = [list(reversed(r)) for r in ordered]
    grp = [(k, sim3_of(Rt[k], tt[k] * 1.02, 1.02), se3_as_sim3(T[k])) for k in range(n - n_group, n)]
    links = [(n - 1, [0, 1]), (n - 2, [0])]                         # (n - 1, 1) and (n - 2, 0) have weight 0 and are not exempt: skipped
    ref = rng.integers(0, n, npts).astype(np.int32)
    done = (rng.random(npts) < 0.2).astype(np.uint8)
    corr = np.where(done, rng.integers(n - n_group, n, npts), -1).astype(np.int32)
    X = np.stack([-(Rt[r].T @ tt[r]) + rng.normal(0, 2, 3) + Rt[r].T @ np.array([0, 0, 8.0]) for r in ref])
    obs = [sorted({int(r), int((r + 1) % n), int((r - 1) % n)}, key=lambda v: int(rank[v])) for r in ref]
    pts = dict(X=X, bad=(rng.random(npts) < 0.05).astype(np.uint8), done=done, corr_ref=corr, ref=ref, obs=obs, level=rng.integers(0, 8, npts))
    return _finish(m, parents, children, [[] for _ in range(n)], weights, ordered, grp, links, pts)


def solver_result(seed, lie):
    """a stand-in for ba_optimize_essential_graph's result: every tangent moved a little (the scale too)"""
    rng = np.random.default_rng(seed)
    lie = np.asarray(lie, np.float64).reshape(-1, 7)
    return lie + rng.normal(0, 1, lie.shape) * np.array([0.05, 0.05, 0.05, 0.01, 0.01, 0.01, 0.02])


def without(m, **changes):
    """a writable copy of the map with some tables replaced"""
    q = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in m.items()}
    q.update(changes)
    return q
