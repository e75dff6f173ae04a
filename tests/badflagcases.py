"""Problems for orbl_set_bad_keyframes: hand-worked cases with their outputs written out by hand, and a seeded generator of consistent
maps.  TEST INFRASTRUCTURE (tests/npbadflag.py states the problem format)."""
import numpy as np


def _i32(x):
    return np.array(x, np.int32).reshape(-1)


def _csr(rows):
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32) if len(rows) else np.zeros(1, np.int32)
    return off, _i32([v for r in rows for v in r])


def _sorted_list(row, rank):
    return sorted(row.items(), key=lambda kw: (kw[1], rank[kw[0]]), reverse=True)


def flatten(nkf, parent, conn, tgt, ordl=None, child=None, rank=None, flags=None, mask=None, bad=None, Tcw=None, slots=None, nobs=None, ref=None):
    """parent[k]; conn[k] = {keyframe: weight}; ordl = {k: [(keyframe, weight)]} where the list is not the sorted map; child = {k: [..]}
    where the row is not what parent[] says; Tcw default: the translation (k, 2k, 3k); slots[k] = the map points of k (-1: null), from
    which the observation lists follow in rank order, a point listed twice by a keyframe being observed through its first slot."""
    rk = list(range(nkf)) if rank is None else list(rank)
    ordl = {} if ordl is None else ordl
    child = {} if child is None else child
    rows = [child[k] if k in child else [c for c in range(nkf) if parent[c] == k] for k in range(nkf)]
    pr = dict(nkf=nkf, npts=0, tgt_kf=_i32(tgt), tgt_flags=None if flags is None else np.array(flags, np.uint8), tgt_mask=None if mask is None else np.array(mask, np.uint8),
              kf_bad=np.array([0] * nkf if bad is None else bad, np.uint8), kf_parent=_i32(parent), kf_rank=None if rank is None else _i32(rank))
    if Tcw is None:
        Tcw = np.zeros((nkf, 12))
        Tcw[:, [0, 5, 10]] = 1.0
        for k in range(nkf):
            Tcw[k, [3, 7, 11]] = (k, 2 * k, 3 * k)
    pr["kf_Tcw"] = np.array(Tcw, np.float64).reshape(nkf, 12)
    pr["child_off"], pr["child_kf"] = _csr(rows)
    pr["conn_off"], pr["conn_kf"] = _csr([list(c.keys()) for c in conn])
    pr["conn_w"] = _csr([list(c.values()) for c in conn])[1]
    lists = [ordl[k] if k in ordl else _sorted_list(conn[k], rk) for k in range(nkf)]
    pr["ord_off"], pr["ord_kf"] = _csr([[k for k, _ in r] for r in lists])
    pr["ord_w"] = _csr([[w for _, w in r] for r in lists])[1]
    if slots is not None:
        npts = 1 + max([p for r in slots for p in r] + [-1])
        obs = [[] for _ in range(npts)]
        for k in sorted(range(nkf), key=lambda q: rk[q]):
            for s, p in enumerate(slots[k]):
                if p >= 0 and all(q != k for q, _ in obs[p]):
                    obs[p].append((k, s))
        pr["npts"] = npts
        pr["kf_slot_off"], pr["kf_slot_pt"] = _csr(slots)
        pr["obs_off"], pr["obs_kf"] = _csr([[k for k, _ in r] for r in obs])
        pr["obs_slot"] = _csr([[s for _, s in r] for r in obs])[1]
        pr["pt_bad"] = np.zeros(npts, np.uint8)
        pr["pt_nobs"] = _i32([len(r) for r in obs] if nobs is None else nobs)
        pr["pt_ref_kf"] = _i32([r[0][0] if r else -1 for r in obs] if ref is None else ref)
    return pr


def _expect(pr, status, conn, ordl, child, parent, bad, Tcp_t, adopted, fallback, slots=None, pt_bad=None, pt_nobs=None, pt_ref=None, erased=()):
    """the whole expected tables: conn[k] dicts, ordl[k] lists, child[k] in ascending rank, Tcp_t[t] = the translation of tgt_Tcp[t] (its
    rotation is the identity in every hand case) or None for zeros; erased = the (point, keyframe) observations that died"""
    e = dict(tgt_status=_i32(status), kf_parent=_i32(parent), kf_bad=np.array(bad, np.uint8))
    Tcp = np.zeros((len(status), 12))
    for t, tr in enumerate(Tcp_t):
        if tr is not None:
            Tcp[t, [0, 5, 10]] = 1.0
            Tcp[t, [3, 7, 11]] = tr
    e["tgt_Tcp"] = Tcp
    e["oconn_off"], e["oconn_kf"] = _csr([list(c.keys()) for c in conn])
    e["oconn_w"] = _csr([list(c.values()) for c in conn])[1]
    e["oord_off"], e["oord_kf"] = _csr([[k for k, _ in r] for r in ordl])
    e["oord_w"] = _csr([[w for _, w in r] for r in ordl])[1]
    e["ochild_off"], e["ochild_kf"] = _csr(child)
    e["counts"] = _i32([sum(1 for s in status if s == 0), len(e["oconn_kf"]), len(e["oord_kf"]), len(e["ochild_kf"]), adopted, fallback])
    if slots is not None:
        er = np.zeros(len(pr["obs_kf"]), np.uint8)
        for p, k in erased:
            hit = [i for i in range(pr["obs_off"][p], pr["obs_off"][p + 1]) if pr["obs_kf"][i] == k]
            assert len(hit) == 1
            er[hit[0]] = 1
        e.update(kf_slot_pt=_i32([p for r in slots for p in r]), pt_bad=np.array(pt_bad, np.uint8), pt_nobs=_i32(pt_nobs), pt_ref_kf=_i32(pt_ref), obs_erased=er)
    return e


def hand_cases():
    """name -> (problem, expected outputs); every expectation below was worked out by hand from the reference text.  Unless a case says
    otherwise keyframe 0 is the root, B = 1 is the target with parent P = 0, every other keyframe hangs under 0, kf_rank is the index and
    Tcw[k] is the translation (k, 2k, 3k), so that Tcp = Tcw[B] o Twc[P] is the translation t_B - t_P."""
    H = {}
    star = [-1, 0, 0, 0, 0, 0]

    # (a) one child adopted by P, the mutual connections erased, Tcp.  0 and 2 name 1 and are named by it: both lose the entry and are
    # re-sorted.  2's list then holds the candidate 0 (weight 30 > -1): 2 goes to 0.  1 leaves 0's children.
    par = [-1, 0, 1, 0, 0, 0]
    pr = flatten(6, par, [{1: 50, 2: 30, 3: 20}, {0: 50, 2: 40}, {1: 40, 0: 30}, {0: 20}, {}, {}], [1])
    H["a_adopt"] = (pr, _expect(pr, [0], [{2: 30, 3: 20}, {}, {0: 30}, {0: 20}, {}, {}], [[(2, 30), (3, 20)], [], [(0, 30)], [(0, 20)], [], []],
                                [[2, 3, 4, 5], [], [], [], [], []], [-1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [(1, 2, 3)], 1, 0))

    # (b) both one-sided connections.  2 names 1 but 1 does not name 2: 2 keeps the entry AND its stale list [(0, 5)] (no re-sort).
    # 1 names 3 but 3 does not name 1: 3 is untouched.  0 is mutual and ends empty.
    pr = flatten(6, star, [{1: 50}, {0: 50, 3: 10}, {1: 7, 0: 5}, {}, {}, {}], [1], ordl={2: [(0, 5)]})
    H["b_one_sided"] = (pr, _expect(pr, [0], [{}, {}, {1: 7, 0: 5}, {}, {}, {}], [[], [], [(0, 5)], [], [], []], [[2, 3, 4, 5], [], [], [], [], []], star,
                                    [0, 1, 0, 0, 0, 0], [(1, 2, 3)], 0, 0))

    # (c) 0's input list holds only its two strongest entries; after the erase it is the WHOLE remaining map: 3 entries where 2 were.
    pr = flatten(6, star, [{1: 50, 2: 30, 3: 5, 4: 3}, {0: 50}, {0: 30}, {0: 5}, {0: 3}, {}], [1], ordl={0: [(1, 50), (2, 30)]})
    H["c_list_grows"] = (pr, _expect(pr, [0], [{2: 30, 3: 5, 4: 3}, {}, {0: 30}, {0: 5}, {0: 3}, {}], [[(2, 30), (3, 5), (4, 3)], [], [(0, 30)], [(0, 5)], [(0, 3)], []],
                                     [[2, 3, 4, 5], [], [], [], [], []], star, [0, 1, 0, 0, 0, 0], [(1, 2, 3)], 0, 0))

    # (d) chain adoption: 2 and 3 are children of 1.  Round 1: 2's list is [(3, 25), (0, 20)], only 0 is a candidate -> 2 goes to 0 and
    # becomes a candidate.  Round 2: 3's list is [(2, 25)] -> 3 goes to 2.
    par = [-1, 0, 1, 1, 0, 0, 0]
    pr = flatten(7, par, [{1: 40, 2: 20}, {2: 30, 3: 10, 0: 40}, {0: 20, 1: 30, 3: 25}, {2: 25, 1: 10}, {}, {}, {}], [1])
    H["d_chain"] = (pr, _expect(pr, [0], [{2: 20}, {}, {0: 20, 3: 25}, {2: 25}, {}, {}, {}], [[(2, 20)], [], [(3, 25), (0, 20)], [(2, 25)], [], [], []],
                                [[2, 4, 5, 6], [], [3], [], [], [], []], [-1, 0, 0, 2, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0], [(1, 2, 3)], 2, 0))

    # (e) equal weights under a kf_rank that is not the identity: rank[2] = 5, rank[3] = 4.  After the erase 3's list is [(2, 10), (0, 10)]
    # and 2's is [(3, 10), (0, 10)] (descending rank inside equal weights).  Round 1 walks child 3 first (the lower RANK, though the higher
    # index): (3, 0, 10) is the best and child 2's (0, 10) does not replace it.  Round 2: child 2 finds 3 before 0 in its list, both at
    # weight 10: the earlier position wins, 2 goes to 3.  0's children come out in ascending rank: 5 (2), 4 (3), 3 (4), 6, 7.
    rank = [0, 1, 5, 4, 3, 2, 6, 7]
    par = [-1, 0, 1, 1, 0, 0, 0, 0]
    pr = flatten(8, par, [{1: 20, 2: 10, 3: 10}, {0: 20, 2: 12, 3: 11}, {0: 10, 3: 10, 1: 12}, {0: 10, 1: 11, 2: 10}, {}, {}, {}, {}], [1], rank=rank)
    H["e_ties"] = (pr, _expect(pr, [0], [{2: 10, 3: 10}, {}, {0: 10, 3: 10}, {0: 10, 2: 10}, {}, {}, {}, {}],
                               [[(2, 10), (3, 10)], [], [(3, 10), (0, 10)], [(2, 10), (0, 10)], [], [], [], []], [[5, 4, 3, 6, 7], [], [], [2], [], [], [], []],
                               [-1, 0, 3, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0, 0], [(1, 2, 3)], 2, 0))

    # (f) child 2 has no candidate in its list, child 3 is bad (its list names 0 with weight 50 and would win): no best, both go to 0 and
    # both STAY in 1's row.
    par = [-1, 0, 1, 1, 0, 0, 0]
    pr = flatten(7, par, [{1: 10, 3: 50}, {0: 10}, {4: 9}, {0: 50}, {2: 9}, {}, {}], [1], bad=[0, 0, 0, 1, 0, 0, 0])
    H["f_fallback"] = (pr, _expect(pr, [0], [{3: 50}, {}, {4: 9}, {0: 50}, {2: 9}, {}, {}], [[(3, 50)], [], [(4, 9)], [(0, 50)], [(2, 9)], [], []],
                                   [[2, 3, 4, 5, 6], [2, 3], [], [], [], [], []], [-1, 0, 0, 0, 0, 0, 0], [0, 1, 0, 1, 0, 0, 0], [(1, 2, 3)], 0, 2))

    # (g) the three skip statuses on the map of (a): nothing changes
    par = [-1, 0, 1, 0, 0, 0]
    conn = [{1: 50, 2: 30, 3: 20}, {0: 50, 2: 40}, {1: 40, 0: 30}, {0: 20}, {}, {}]
    pr = flatten(6, par, conn, [1, 2, 3], flags=[1, 2, 0], mask=[1, 1, 0])
    H["g_skips"] = (pr, _expect(pr, [1, 2, 3], conn, [[(1, 50), (2, 30), (3, 20)], [(0, 50), (2, 40)], [(1, 40), (0, 30)], [(0, 20)], [], []],
                                [[1, 3, 4, 5], [2], [], [], [], []], par, [0] * 6, [None, None, None], 0, 0))

    # (h) 2 is a child of 1 and 3 a child of 2; targets 1 then 2.  Turn of 1: 0 and 2 lose it; 2's list [(0, 20), (3, 15)] holds 0: 2 goes
    # to 0.  Turn of 2: its parent is NOW 0, Tcp = t_2 - t_0; 0 and 3 lose 2 and end empty; 3's list is empty: it goes to 0, stays in 2's row.
    par = [-1, 0, 1, 2, 0, 0, 0]
    conn = [{1: 30, 2: 20}, {0: 30, 2: 25}, {1: 25, 0: 20, 3: 15}, {2: 15}, {}, {}, {}]
    pr = flatten(7, par, conn, [1, 2])
    H["h_parent_first"] = (pr, _expect(pr, [0, 0], [{}] * 7, [[]] * 7, [[3, 4, 5, 6], [], [3], [], [], [], []], [-1, 0, 0, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0, 0],
                                       [(1, 2, 3), (2, 4, 6)], 1, 1))
    # the reverse order.  Turn of 2 (parent 1): 1, 0 and 3 lose it; 3's list is empty: it goes to 1; 2 LEAVES 1's children (step 5), Tcp =
    # t_2 - t_1.  Turn of 1: its children are {3} - 2 is bad by now but no longer in the row; 3 has no list: it goes to 0 and stays in 1's row.
    pr = flatten(7, par, conn, [2, 1])
    H["h_child_first"] = (pr, _expect(pr, [0, 0], [{}] * 7, [[]] * 7, [[3, 4, 5, 6], [3], [3], [], [], [], []], [-1, 0, 1, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0, 0],
                                      [(1, 2, 3), (1, 2, 3)], 0, 2))

    # (i) 2's stale list names 0, which its map does not hold: the weight is 0, and 0 > -1 is accepted.  The list itself is only copied.
    par = [-1, 0, 1, 0, 0, 0]
    pr = flatten(6, par, [{}] * 6, [1], ordl={2: [(0, 99)]})
    H["i_weight0"] = (pr, _expect(pr, [0], [{}] * 6, [[], [], [(0, 99)], [], [], []], [[2, 3, 4, 5], [], [], [], [], []], star, [0, 1, 0, 0, 0, 0], [(1, 2, 3)], 1, 0))

    # (j) points; targets 1 then 2.  p0 {1, 3, 4, 5} with reference 1: 3 observers stay, the reference moves to 3.  p1 {1, 3, 4}: drops to 2,
    # turns bad, 3 and 4 lose the observation and the slot.  p2 {1, 2, 3} with reference 1: the reference moves to 2, then the point turns
    # bad at 1's turn and takes the slots of 2 and 3: target 2 finds a null slot.  p3 is listed in slots 3 AND 4 of keyframe 1: the second
    # finds no observation.  p4 {2, 3, 4, 5}: loses 2 only.  1's own slots are not cleared.
    slots = [[], [0, 1, 2, 3, 3], [2, 4], [0, 1, 2, 3, 4], [0, 1, 3, 4], [0, 3, 4]]
    pr = flatten(6, star, [{}] * 6, [1, 2], slots=slots, ref=[1, 3, 1, 3, 3])
    H["j_points"] = (pr, _expect(pr, [0, 0], [{}] * 6, [[]] * 6, [[3, 4, 5], [], [], [], [], []], star, [0, 1, 1, 0, 0, 0], [(1, 2, 3), (2, 4, 6)], 0, 0,
                                 slots=[[], [0, 1, 2, 3, 3], [-1, 4], [0, -1, -1, 3, 4], [0, -1, 3, 4], [0, 3, 4]], pt_bad=[0, 1, 1, 0, 0], pt_nobs=[3, 2, 2, 3, 3],
                                 pt_ref=[3, 3, 2, 3, 3], erased=[(0, 1), (1, 1), (1, 3), (1, 4), (2, 1), (2, 2), (2, 3), (3, 1), (4, 2)]))
    return H


def make(seed, nkf, ntgt, slots_per_kf=30, big_row=0):
    """A seeded consistent map (keyframe k holds point p in slot i iff p's observations contain (k, i), but for a few points listed a second
    time by a keyframe) with stale ordered lists, one-sided connections, equal weights, bad keyframes, a target that is the child of an
    earlier target, children of targets with equal weights to the new parent or none at all, skipped targets from the fourth on, and one keyframe (`hub`) mutually connected to every target - and, with big_row,
    to that many keyframes."""
    rng = np.random.default_rng(seed)
    rank = [int(v) for v in rng.permutation(nkf)]
    parent = [-1] + [int(rng.integers(max(0, k - 6), k)) for k in range(1, nkf)]
    kids = [[c for c in range(nkf) if parent[c] == k] for k in range(nkf)]
    first = next(k for k in range(1, nkf) if kids[k] and kids[kids[k][0]])           # a target with a grandchild: its child is the second target
    tgt = [first, kids[first][0]]
    hub = next(k for k in range(nkf - 1, 0, -1) if k not in tgt)
    pool = [k for k in range(1, nkf) if k not in tgt and k != hub]
    tgt += [int(v) for v in rng.choice(pool, ntgt - 2, replace=False)]
    bad = [0] * nkf
    for k in rng.choice([k for k in pool if k not in tgt], max(1, nkf // 12), replace=False):
        bad[int(k)] = 1
    for c in kids[tgt[0]][1:] + kids[tgt[2]][:1]:                                    # bad children of targets
        if c not in tgt and c != hub:
            bad[c] = 1
    flags = [0] * ntgt
    mask = [1] * ntgt
    for t in range(3, ntgt):
        flags[t], mask[t] = [(1, 1), (2, 1), (0, 0), (0, 1)][(t - 3) % 4]
    # points seen from a window of neighbouring keyframes
    npts = nkf * slots_per_kf // 4
    slots = [[] for _ in range(nkf)]
    for p in range(npts):
        b = int(rng.integers(0, nkf))
        win = [k for k in range(max(0, b - 4), min(nkf, b + 5))]
        for k in rng.choice(win, min(len(win), int(rng.integers(2, 7))), replace=False):
            slots[int(k)].append(p)
    for k in range(nkf):
        if slots[k] and rng.random() < 0.5:
            slots[k].insert(int(rng.integers(0, len(slots[k]))), -1)
        if slots[k] and rng.random() < 0.3:
            slots[k].append(next(p for p in slots[k] if p >= 0))                     # listed twice
    share = [dict() for _ in range(nkf)]
    seen = [set(p for p in r if p >= 0) for r in slots]
    for k in range(nkf):
        for j in range(max(0, k - 8), min(nkf, k + 9)):
            w = len(seen[k] & seen[j]) // 3                                          # (coarse weights: many ties)
            if j != k and w > 0:
                share[k][j] = w
    conn = []
    for k in range(nkf):
        keys = [int(v) for v in rng.permutation(list(share[k].keys()))] if share[k] else []
        conn.append({j: share[k][j] for j in keys if rng.random() > 0.1})            # (a dropped entry leaves the other side one-sided)
    others = [k for k in range(nkf) if k != hub]
    for j in list(tgt) + [int(v) for v in rng.choice(others, min(big_row, len(others)), replace=False)]:
        if j != hub:
            conn[hub].setdefault(j, 1 + int(rng.integers(0, 3)))
            conn[j].setdefault(hub, conn[hub][j])
    stale = set()
    for B in tgt[:3]:                                                                # the children of the first targets: equal weights to the
        for i, c in enumerate(kids[B]):                                              # parent, or a parent the map no longer holds
            if i % 2 == 0:
                conn[c][parent[B]] = conn[parent[B]][c] = 2
            else:
                conn[c].pop(parent[B], None)
                conn[parent[B]].pop(c, None)
                stale.add(c)
    ordl = {}
    for k in range(nkf):
        full = _sorted_list(conn[k], rank)
        lst = [kw for kw in full if kw[1] >= 2] if rng.random() < 0.7 else full     # (entries below the threshold never entered the list)
        g = parent[parent[k]] if parent[k] >= 0 else -1
        if g >= 0 and g not in conn[k] and (k in stale or rng.random() < 0.5):
            lst = lst + [(g, 1)]                                                     # a stale entry the map no longer holds
        ordl[k] = lst
    q, _ = np.linalg.qr(rng.normal(size=(nkf, 3, 3)))
    Tcw = np.concatenate([q, rng.normal(size=(nkf, 3, 1)) * 5.0], axis=2).reshape(nkf, 12)
    pr = flatten(nkf, parent, conn, tgt, ordl=ordl, rank=rank, flags=flags, mask=mask, bad=bad, Tcw=Tcw, slots=slots)
    obs_len = np.diff(pr["obs_off"])
    pr["pt_ref_kf"] = _i32([pr["obs_kf"][pr["obs_off"][p] + int(rng.integers(0, n))] if n else -1 for p, n in enumerate(obs_len)])
    return pr


def seeded():
    """name -> problem: the maps the GPU tests run, nkf = 12, 40 and 300 (one row of 280 entries: a sort over more than one 256-entry tile)"""
    S = {"n12_s%d" % s: make(s, 12, 3 + s % 3) for s in range(4)}
    S.update({"n40_s%d" % s: make(10 + s, 40, 4 + s % 3) for s in range(4)})
    S["n300"] = make(99, 300, 6, big_row=280)
    return S


def without_points(pr):
    q = {k: v for k, v in pr.items() if k not in ("kf_slot_off", "kf_slot_pt", "pt_bad", "pt_nobs", "pt_ref_kf", "obs_off", "obs_kf", "obs_slot")}
    q["npts"] = 0
    return q
