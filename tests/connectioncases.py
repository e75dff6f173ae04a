"""Problems for orbl_update_connections: hand-worked cases with their outputs written out by hand, and a seeded generator of maps with
stale initial tables.  TEST INFRASTRUCTURE (tests/npconnections.py states the problem format)."""
import numpy as np


def _i32(x):
    return np.array(x, np.int32).reshape(-1)


def _csr(rows):
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32) if len(rows) else np.zeros(1, np.int32)
    return off, _i32([v for r in rows for v in r])


def flatten(nkf, obs, tgt, slots, conn=None, prev=None, flags=None, rank=None, pt_bad=None, th=15):
    """obs[p] = the observing keyframes of point p; tgt = the targets in call order, slots[t] = their map_points_ (-1: null); conn[k] =
    {keyframe: weight} at entry; prev[t] = the target's ordered list at entry (None: no links)."""
    conn = [{} for _ in range(nkf)] if conn is None else conn
    slot_off, slot_pt = _csr(slots)
    obs_off, obs_kf = _csr(obs)
    conn_off, conn_kf = _csr([list(c.keys()) for c in conn])
    _, conn_w = _csr([list(c.values()) for c in conn])
    pr = dict(nkf=nkf, npts=len(obs), th=th, tgt_kf=_i32(tgt), tgt_flags=None if flags is None else np.array(flags, np.uint8).reshape(-1),
              slot_off=slot_off, slot_pt=slot_pt, obs_off=obs_off, obs_kf=obs_kf, pt_bad=None if pt_bad is None else np.array(pt_bad, np.uint8).reshape(-1),
              kf_rank=None if rank is None else _i32(rank), conn_off=conn_off, conn_kf=conn_kf, conn_w=conn_w, prev_off=None, prev_kf=None)
    if prev is not None:
        pr["prev_off"], pr["prev_kf"] = _csr(prev)
    return pr


def _expect(status, parent, aff, conn_off, conn_kf, conn_w, ord_off, ord_kf, ord_w, link_off=None, link_kf=None):
    e = dict(tgt_status=_i32(status), tgt_parent=_i32(parent), aff_kf=_i32(aff), conn_off=_i32(conn_off), conn_kf=_i32(conn_kf), conn_w=_i32(conn_w),
             ord_off=_i32(ord_off), ord_kf=_i32(ord_kf), ord_w=_i32(ord_w), link_off=None if link_off is None else _i32(link_off),
             link_kf=None if link_off is None else _i32(link_kf))
    e["counts"] = _i32([len(e["aff_kf"]), len(e["conn_kf"]), len(e["ord_kf"]), 0 if link_off is None else len(e["link_kf"])])
    return e


def hand_cases():
    """name -> (problem, expected outputs); every expectation below was worked out by hand from the reference text"""
    H = {}
    # (a) the plain step.  Points 0, 1 seen by {0, 1}, point 2 by {0, 1, 2}; target 0, th 2, empty tables.  counter = {1: 3, 2: 1}: 1 reaches
    # th and receives AddConnection(1 <- 0, 3); 0's map is the WHOLE counter, its list only [1]; first connection: parent 1.  Nothing was
    # in 0's list before, so both neighbours are new links.
    H["a_plain"] = (flatten(3, [[0, 1], [0, 1], [0, 1, 2]], [0], [[0, 1, 2]], prev=[[]], flags=[1], th=2),
                    _expect([0], [1], [0, 1], [0, 2, 3], [1, 2, 0], [3, 1, 3], [0, 1, 2], [1, 0], [3, 3], [0, 2], [1, 2]))
    # (b) nothing reaches th = 15: the maximum alone.  counter = {1: 1, 2: 1}, a tie; the map is walked in rank order and keyframe 2 has the
    # lower rank, so kmax = 2 (index order would say 1).  2 already holds (0, 1): AddConnection changes nothing, 2 is not affected.  0's
    # map row comes in rank order: 2 then 1.
    H["b_fallback_tie_noop"] = (flatten(3, [[0, 1, 2]], [0], [[0]], conn=[{}, {}, {0: 1}], rank=[0, 2, 1]),
                                _expect([0], [-1], [0], [0, 2], [2, 1], [1, 1], [0, 1], [2], [1]))
    # (c) empty counter: the only point has no other observer, the second slot is null.  Status 1, nothing changes, nothing is affected; the
    # link set is the untouched map {1} minus the previous list [1].
    H["c_empty"] = (flatten(2, [[0]], [0], [[0, -1]], conn=[{1: 5}, {}], prev=[[1]], flags=[1]),
                    _expect([1], [-1], [], [0], [], [], [0], [], [], [0, 0], []))
    # (d) the re-sort quirk.  counter = {1: 2}, th 2.  Keyframe 1 came with a stale entry (2, 1) below th: AddConnection re-sorts ALL of
    # its map, so its list becomes [0 (2), 2 (1)].
    H["d_resort_brings_in_below_th"] = (flatten(3, [[0, 1], [0, 1]], [0], [[0, 1]], conn=[{}, {2: 1}, {}], flags=[1], th=2),
                                        _expect([0], [1], [0, 1], [0, 1, 3], [1, 0, 2], [2, 2, 1], [0, 1, 3], [1, 0, 2], [2, 2, 1]))
    # (e) a target whose list is re-sorted BEFORE its turn.  th 1; point 0 seen by {0, 1}, point 1 by {1, 2}; targets 0 then 1; keyframe 1
    # came with map {2: 7} but an empty list.  Turn 0: AddConnection(1 <- 0, 1) makes 1's list [2 (7), 0 (1)].  Turn 1: P(1) is that list,
    # not the empty one, so 2 is NOT a new link; counter = {0: 1, 2: 1}; 0 already holds (1, 1): no-op; 2 gets {1: 1}; 1's list is
    # [2, 0] (equal weights: the higher rank first); parent of 1 = 2.
    H["e_resorted_before_turn"] = (flatten(3, [[0, 1], [1, 2]], [0, 1], [[0], [0, 1]], conn=[{}, {2: 7}, {}], prev=[[], []], flags=[0, 1], th=1),
                                   _expect([0, 0], [-1, 2], [0, 1, 2], [0, 1, 3, 4], [1, 0, 2, 1], [1, 1, 1, 1], [0, 1, 3, 4], [1, 2, 0, 1], [1, 1, 1, 1],
                                           [0, 0, 0], []))
    # (f) a target re-sorted AFTER its turn: only an inconsistent map does it.  Keyframe 0 lists point 0 twice: counter = {1: 2}, th 2,
    # AddConnection(1 <- 0, 2).  Keyframe 1 lists it once: counter = {0: 1}, below th, so the maximum: AddConnection(0 <- 1, 1) finds
    # weight 2 in 0's map, overwrites it and re-sorts 0's list.
    H["f_resorted_after_turn"] = (flatten(2, [[0, 1]], [0, 1], [[0, 0], [0]], prev=[[], []], th=2),
                                  _expect([0, 0], [-1, -1], [0, 1], [0, 1, 2], [1, 0], [1, 1], [0, 1, 2], [1, 0], [1, 1], [0, 0, 0], []))
    # (g) links and a reversed pointer order.  th 1; points seen by {0, 1}, {0, 2}, {0, 3}; 0 came with {1: 1} and the list [1]; 1 already
    # holds (0, 1).  0's map row in ascending rank is 3, 2, 1; its list by descending (weight, rank) is 1, 2, 3; the new links are 2 and 3,
    # in rank order 3, 2.
    H["g_links_reversed_rank"] = (flatten(4, [[0, 1], [0, 2], [0, 3]], [0], [[0, 1, 2]], conn=[{1: 1}, {0: 1}, {}, {}], prev=[[1]], flags=[1], rank=[3, 2, 1, 0],
                                          th=1),
                                  _expect([0], [1], [0, 2, 3], [0, 3, 4, 5], [3, 2, 1, 0, 0], [1, 1, 1, 1, 1], [0, 3, 4, 5], [1, 2, 3, 0, 0], [1, 1, 1, 1, 1],
                                          [0, 2], [3, 2]))
    return H


def make(seed, nkf=32, ntgt=None, per_kf=40, window=3, dup=False, sparse=True, stale=0.5, th=15, null=0.05, bad=0.03, rank="random", prev=True, flags=True, n_obs=(2, 6)):
    """A map of nkf keyframes along a path: a point is seen by n_obs[0] to n_obs[1] - 1 keyframes out of a window of neighbours, so covisibility counts straddle
    th.  With sparse=True (nkf >= 8) keyframe nkf - 2 sees only points nobody else sees (empty counter) and nkf - 1 shares 4 points with
    keyframe 0 and nothing else (the maximum below th).  The tables at entry are STALE: true counts, wrong weights, missing and extra
    entries mixed.  dup=True lists some points twice in a keyframe (the counts stop being symmetric)."""
    rng = np.random.RandomState(seed)
    sparse = sparse and nkf >= 8
    body = nkf - 2 if sparse else nkf
    obs = []
    for _ in range(body * per_kf // 3):
        c = rng.randint(body)
        cand = np.arange(max(0, c - window), min(body, c + window + 1))
        obs.append(sorted(rng.choice(cand, min(len(cand), rng.randint(*n_obs)), replace=False).tolist()))
    if sparse:
        obs += [[nkf - 2]] * 5 + [[0, nkf - 1]] * 4
    npts = len(obs)
    pt_bad = (rng.rand(npts) < bad).astype(np.uint8)
    held = [[] for _ in range(nkf)]
    for p, ks in enumerate(obs):
        for k in ks:
            held[k].append(p)
    true = np.zeros((nkf, nkf), np.int64)
    for p, ks in enumerate(obs):
        if not pt_bad[p]:
            for a in ks:
                for b in ks:
                    if a != b:
                        true[a, b] += 1
    ntgt = (nkf if seed % 4 == 0 else max(1, nkf // 3)) if ntgt is None else ntgt
    tgt = rng.permutation(nkf)[:ntgt].tolist()
    if sparse and ntgt >= 3:                                         # the sparse keyframes and their one neighbour are always targets
        for want in (nkf - 2, nkf - 1, 0):
            if want not in tgt:
                tgt[[i for i, k in enumerate(tgt) if k not in (nkf - 2, nkf - 1, 0)][0]] = want
    slots = []
    for k in tgt:
        s = list(held[k])
        if dup and s:
            s += rng.choice(s, max(1, len(s) // 8)).tolist()
        s += [-1] * int(null * len(s) + 1)
        rng.shuffle(s)
        slots.append(s)
    conn = []
    for k in range(nkf):
        row = {}
        for b in np.nonzero(true[k])[0]:
            u = rng.rand()
            if u < stale:
                row[int(b)] = int(true[k, b])
            elif u < stale + 0.3:
                row[int(b)] = int(rng.randint(1, 40))
        for b in rng.randint(0, nkf, 2):
            if b != k and int(b) not in row:
                row[int(b)] = int(rng.randint(1, 40))
        items = list(row.items()); rng.shuffle(items)
        conn.append(dict(items))
    prv = None
    if prev:
        prv = [[b for b in conn[k] if rng.rand() < 0.6] for k in tgt]
    rk = None if rank is None else (np.arange(nkf)[::-1] if rank == "reversed" else rng.permutation(nkf))
    fl = (rng.rand(ntgt) < 0.4).astype(np.uint8) if flags else None
    return flatten(nkf, obs, tgt, slots, conn=conn, prev=prv, flags=fl, rank=rk, pt_bad=pt_bad, th=th)


def seeded(n=20):
    """[(name, problem)]: n maps of 24-64 keyframes; every third lists points twice, and so does every fourth, whose keyframes are ALL
    targets (on a consistent map every list would then end as its keyframe's own step-4 list and the re-sorts would leave no trace)"""
    out = []
    for seed in range(n):
        nkf = 24 + (seed * 13) % 41
        out.append(("seed%d_nkf%d" % (seed, nkf), make(seed, nkf=nkf, dup=seed % 3 == 2 or seed % 4 == 0)))
    return out
