"""Problems for Tracking::UpdateLocalMap (orbt_update_local_*): hand-worked cases whose expected lists are written out here, and a
seeded generator of consistent random maps (a covisibility graph, a spanning tree, bad flags, kf_rank shuffles).  A problem is the
dict of tables tests/nplocalmap.py documents.  TEST INFRASTRUCTURE."""
import numpy as np


def _csr(rows):
    off = np.zeros(len(rows) + 1, np.int32)
    for i, r in enumerate(rows):
        off[i + 1] = off[i] + len(r)
    val = np.array([v for r in rows for v in r], np.int32).reshape(-1)
    return off, val


def records(npts):
    """point records that differ in every field and every point (pure functions of the id)"""
    p = np.arange(npts, dtype=np.float64)
    return dict(pt_Xw=np.stack([p + 0.25, -2.0 * p - 0.5, 0.125 * p * p + 1.0], 1).reshape(-1, 3), pt_normal=np.stack([1.0 / (p + 1.0), p * 1e-3, -p - 3.0], 1).reshape(-1, 3),
                pt_min_dist=(0.5 + 0.01 * p).astype(np.float32), pt_max_dist=(9.0 + 0.5 * p).astype(np.float32),
                pt_desc=((np.arange(npts, dtype=np.int64)[:, None] * 37 + np.arange(32)[None, :] * 11 + 5) % 256).astype(np.uint8).reshape(-1, 32))


def build(nkf, slots, frame, obs=None, npts=None, cov=None, children=None, parent=None, kf_bad=(), pt_bad=(), rank=None, prev=(), seen=(), nobs0=()):
    """slots[k]: the slot table of keyframe k (point id or -1); obs[p]: the observers of point p (default: the keyframes that hold it);
    cov / children: dict keyframe -> list; parent: dict keyframe -> parent; nobs0: points whose Observations() is 0."""
    if npts is None:
        npts = 1 + max([-1] + [p for r in slots for p in r] + list(frame) + list(seen))
    if obs is None:
        obs = [[k for k in range(nkf) if p in slots[k]] for p in range(npts)]
    obs_off, obs_kf = _csr(obs)
    cov_off, cov_kf = _csr([(cov or {}).get(k, []) for k in range(nkf)])
    child_off, child_kf = _csr([(children or {}).get(k, []) for k in range(nkf)])
    slot_off, slot_pt = _csr(slots)
    pb = np.zeros(npts, np.uint8); pb[list(pt_bad)] = 1
    kb = np.zeros(nkf, np.uint8); kb[list(kf_bad)] = 1
    nobs = np.array([len(o) for o in obs], np.int32).reshape(-1); nobs[list(nobs0)] = 0
    pr = dict(frame_pt=np.array(frame, np.int32).reshape(-1), seen_pt=np.array(seen, np.int32).reshape(-1), prev_local_kf=np.array(prev, np.int32).reshape(-1),
              pt_bad=pb, pt_nobs=nobs, obs_off=obs_off, obs_kf=obs_kf, kf_bad=kb, kf_rank=None if rank is None else np.array(rank, np.int32),
              kf_parent=np.array([(parent or {}).get(k, -1) for k in range(nkf)], np.int32).reshape(-1), cov_off=cov_off, cov_kf=cov_kf, child_off=child_off,
              child_kf=child_kf, kf_slot_off=slot_off, kf_slot_pt=slot_pt)
    pr.update(records(npts))
    return pr


def hand_cases():
    """name -> (problem, expected): the expected values are worked out by hand, key by key (a subset of the restatement's outputs)"""
    H = {}
    # (a) a chain 0 <- 1 <- 2.  The frame holds p0 (seen by 0) and p1 (seen by 0, 1): votes 2, 1.  Voted list [0, 1], reference keyframe 0.
    # Walk: keyframe 0 finds its neighbour 1 and child 1 marked, no parent; keyframe 1 takes neighbour 2 (0 is marked), child 2 is marked
    # by then, parent 0 is marked.  Points: 0, 1 from keyframe 0; 2 from keyframe 1; 3 from keyframe 2.
    H["a_chain"] = (build(3, [[0, 1], [1, 2], [2, 3]], [0, 1, -1], cov={0: [1], 1: [0, 2], 2: [1]}, children={0: [1], 1: [2]}, parent={1: 0, 2: 1}),
                    dict(votes=[2, 1, 0], local_kf=[0, 1, 2], ref_kf=0, status=0, frame_pt_out=[0, 1, -1], local_pt=[0, 1, 2, 3], mp_state=[0, 0, 1, 1], slot_state=[1, 1, 0]))
    # (b) votes 2, 1, 2 for keyframes 0, 1, 2 with ranks 2, 0, 1: the order is 1, 2, 0; keyframe 2 is the first with a count above all before
    # it (index order would pick 0).  Points: keyframe 1 holds 0, 2; keyframe 2 holds 0, 1.
    H["b_tie_by_rank"] = (build(3, [[0, 1], [0, 2], [0, 1]], [0, 1], obs=[[0, 1, 2], [0, 2], [1]], rank=[2, 0, 1]),
                          dict(votes=[2, 1, 2], local_kf=[1, 2, 0], ref_kf=2, status=0, local_pt=[0, 2, 1], mp_state=[0, 1, 0]))
    # (c) keyframes 0 and 1 are voted, 1 is bad: the list is [0].  Keyframe 0's neighbours are 1 (bad: passed over) and 2 (taken); its only
    # child is 1 (bad): nothing.  Points of keyframes 0 and 2 only.
    H["c_bad_voted"] = (build(3, [[0], [0, 1], [2]], [0], obs=[[0, 1], [1], [2]], cov={0: [1, 2]}, children={0: [1]}, kf_bad=[1]),
                        dict(votes=[1, 1, 0], local_kf=[0, 2], ref_kf=0, status=0, local_pt=[0, 2], mp_state=[0, 1]))
    # (d) the parent of the voted keyframe 0 is the bad keyframe 1: it is appended all the same, and its points are collected
    H["d_bad_parent"] = (build(2, [[0], [1]], [0], parent={0: 1}, kf_bad=[1]), dict(votes=[1, 0], local_kf=[0, 1], ref_kf=0, status=0, local_pt=[0, 1]))
    # (e) keyframes 0 and 1 are voted; keyframe 0 appends its parent 2 and the walk ends: keyframe 1's free neighbour 3 is never looked at
    H["e_parent_ends_walk"] = (build(4, [[0], [0], [1], [2]], [0], parent={0: 2}, cov={1: [3]}),
                               dict(votes=[1, 1, 0, 0], local_kf=[0, 1, 2], ref_kf=0, status=0, local_pt=[0, 1]))
    # (f) n voted keyframes 0..n-1 (one point seen by all of them), keyframe 0 has the free neighbour n, keyframe 1 the free neighbour n + 1.
    # n = 80: the size is not > 80 at the first iteration, n is appended, 81 > 80 stops the second.  n = 81: no iteration at all.
    for n, exp in ((80, list(range(81))), (81, list(range(81)))):
        H["f_voted_%d" % n] = (build(n + 2, [[0]] * n + [[1], [2]], [0], cov={0: [n], 1: [n + 1]}),
                               dict(local_kf=exp, ref_kf=0, status=0, local_pt=[0, 1] if n == 80 else [0], votes=[1] * n + [0, 0]))
    # (g) 100 voted keyframes are kept whole, the free neighbour of keyframe 0 stays out
    H["g_voted_100"] = (build(101, [[0]] * 100 + [[1]], [0], cov={0: [100]}), dict(local_kf=list(range(100)), ref_kf=0, status=0, local_pt=[0]))
    # (h) the frame holds nothing: the previous list [2, 0] is reused in its order, the reference keyframe is left alone
    H["h_no_votes"] = (build(3, [[0], [1], [2, 0]], [-1, -1], prev=[2, 0]),
                       dict(votes=[0, 0, 0], local_kf=[2, 0], ref_kf=-1, status=1, frame_pt_out=[-1, -1], local_pt=[2, 0], mp_state=[1, 1], slot_state=[0, 0]))
    # (i) the frame's second slot holds the bad point 1: it is cleared and keyframe 1, which only that point would have voted for, gets nothing
    H["i_bad_frame_point"] = (build(2, [[0], [1]], [0, 1], pt_bad=[1]),
                              dict(votes=[1, 0], local_kf=[0], ref_kf=0, status=0, frame_pt_out=[0, -1], local_pt=[0], slot_state=[1, 0]))
    # (j) point 5 sits in keyframes 0, 1 and 2 (voted through point 0, which all three see): it appears once, where keyframe 0 lists it
    H["j_first_occurrence"] = (build(3, [[0, 5, 1], [5, 0, 2], [3, 5, 0]], [0]), dict(local_kf=[0, 1, 2], local_pt=[0, 5, 1, 2, 3], mp_state=[0, 1, 1, 1, 1]))
    # (k) the bad point 1 is never emitted, from no keyframe
    H["k_bad_point"] = (build(2, [[0, 1, 2], [1, 3]], [0], obs=[[0, 1], [0, 1], [0], [1]], pt_bad=[1]), dict(local_kf=[0, 1], local_pt=[0, 2, 3]))
    # (l) point 1 is in seen_pt, point 0 sits in the frame, point 2 has no observations, point 3 is ordinary: states 0, 0, 3, 1
    H["l_states"] = (build(1, [[0, 1, 2, 3]], [0], seen=[1], nobs0=[2]), dict(local_kf=[0], local_pt=[0, 1, 2, 3], mp_state=[0, 0, 3, 1], slot_state=[1]))
    # (m) keyframe 1 has no slots at all, keyframe 2 only empty ones; all three are voted through point 0's observers
    H["m_empty_slot_tables"] = (build(4, [[0], [], [-1, -1, -1], [1]], [0], obs=[[0, 1, 2, 3], [3]]), dict(local_kf=[0, 1, 2, 3], local_pt=[0, 1], votes=[1, 1, 1, 1]))
    # (n) one more: keyframe 0 has 70 children, the first 66 of them bad - the first free one lies past the 64 entries a
    # wave looks at in one go
    H["n_child_past_a_wave"] = (build(72, [[0]] + [[]] * 66 + [[1]] + [[]] * 4, [0], children={0: list(range(1, 71))}, kf_bad=range(1, 67)),
                                dict(votes=[1] + [0] * 71, local_kf=[0, 67], ref_kf=0, status=0, local_pt=[0, 1]))
    return H


def make(seed, nkf, npts, n_kp, span=4, q=0.8, kf_bad=0.05, pt_bad=0.05, hold=0.6, window=3, empty=0.2, n_seen=5, n_prev=6, shuffle_rank=True):
    """A consistent random map: point p is seen from keyframes around a centre; a keyframe's slot table lists its points in a random
    order between empty slots; parent = an earlier keyframe close by; best covisibles = the up to 10 keyframes sharing most points;
    the frame looks at the map around a random keyframe (window: how far) and holds each candidate point with probability `hold`."""
    rng = np.random.default_rng(seed)
    obs = []
    for p in range(npts):
        c, w = int(rng.integers(nkf)), 1 + int(rng.integers(span))
        obs.append([k for k in range(max(0, c - w), min(nkf, c + w + 1)) if rng.random() < q])
    slots = [[] for _ in range(nkf)]
    for p in rng.permutation(npts):
        for k in obs[p]:
            if rng.random() < empty:
                slots[k].append(-1)
            slots[k].append(int(p))
    parent = {k: int(rng.integers(max(0, k - 3), k)) for k in range(1, nkf)}
    children = {}
    for k in rng.permutation(np.arange(1, nkf)):                    # (set order: any order the caller's set has)
        children.setdefault(parent[int(k)], []).append(int(k))
    share = np.zeros((nkf, nkf), np.int32)
    for o in obs:
        for a in o:
            for b in o:
                if a != b:
                    share[a, b] += 1
    cov = {k: [int(j) for j in np.argsort(-share[k], kind="stable")[:10] if share[k, j] > 0] for k in range(nkf)}
    cur = int(rng.integers(nkf))
    near = [p for p in range(npts) if obs[p] and min(abs(k - cur) for k in obs[p]) <= window]
    frame = [int(near[rng.integers(len(near))]) if near and rng.random() < hold else -1 for _ in range(n_kp)]
    bad_p = [p for p in range(npts) if rng.random() < pt_bad]
    bad_k = [k for k in range(nkf) if rng.random() < kf_bad]
    held = set(frame)
    seen = [int(p) for p in rng.permutation(npts)[:n_seen] if p not in held]
    prev = [int(k) for k in rng.permutation(nkf)[:min(n_prev, nkf)]]
    nobs0 = [p for p in range(npts) if rng.random() < 0.03]
    rank = [int(r) for r in rng.permutation(nkf)] if shuffle_rank else None
    return build(nkf, slots, frame, obs=obs, npts=npts, cov=cov, children=children, parent=parent, kf_bad=bad_k, pt_bad=bad_p, rank=rank, prev=prev, seen=seen, nobs0=nobs0)


# name -> (keyword arguments, seeds).  TABLE: per problem (n_local_kf, n_local_pt, paths) as tests/nplocalmap.py computes them on the CPU
# (tests/test_local_map_restatement.py keeps the table honest).
CONFIGS = {
    "tiny": (dict(nkf=6, npts=40, n_kp=12, span=2), (0, 1, 2)),
    "small": (dict(nkf=30, npts=600, n_kp=200), (0, 1, 2, 3)),
    "wide": (dict(nkf=140, npts=1500, n_kp=500, span=6, window=60, kf_bad=0.02), (0, 1)),
    "blind": (dict(nkf=20, npts=300, n_kp=64, hold=0.0), (0,)),
}
TABLE = {
    "tiny-0": (6, 37, ("parent_break",)), "tiny-1": (6, 39, ()), "tiny-2": (6, 40, ()),
    "small-0": (20, 441, ()), "small-1": (27, 557, ("parent_break",)), "small-2": (20, 433, ("parent_break",)), "small-3": (16, 375, ("parent_break",)),
    "wide-0": (81, 895, ("stop80",)), "wide-1": (83, 882, ("stop80",)),
    "blind-0": (6, 227, ("no_votes",)),
}
# The three paths: the parent-break is taken by tiny-0, small-1, small-2, small-3 (4 seeds); the > 80 stop by wide-0, wide-1 (2 seeds); the
# no-vote path by blind-0 (1 seed).


def seeded():
    """[(name, problem)] over CONFIGS"""
    return [("%s-%d" % (name, s), make(s, **kw)) for name, (kw, seeds) in CONFIGS.items() for s in seeds]
