"""Problems for orbl_apply_map_edits (tests/npmapedit.py restates it): hand-worked cases with their expected outputs written out by hand,
one per edit kind plus the corners the issue names, and a seeded generator of consistent maps whose edit lists are derived the way the
reference derives them (ProcessNewKeyFrame, CreateNewMapPoints, MapPointCulling, SearchInNeighbors, CorrectLoop, SearchAndFuse), with
injections for what random maps lack.  TEST INFRASTRUCTURE."""
import numpy as np

NOP, ADD, REPLACE, SET_BAD, FUSE, FIND_OR_ADD, REPLACE_FOUND = range(7)
OP_KEYS = ("op_kind", "op_pt", "op_arg", "op_kf", "op_slot")
TABLES = ("kf_slot_off", "kf_rank", "kf_slot_pt", "kf_slot_level", "kf_slot_uv", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced", "obs_off", "obs_kf",
          "obs_slot", "obs_dead")


def with_ops(pr, ops):
    """the problem with the edit list ops = [(kind, pt, arg, kf, slot), ...]"""
    a = np.array(ops, np.int32).reshape(-1, 5)
    return dict(pr, **{k: np.ascontiguousarray(a[:, i]) for i, k in enumerate(OP_KEYS)})


def ops_of(pr):
    return [tuple(int(pr[k][i]) for k in OP_KEYS) for i in range(len(pr["op_kind"]))]


def reversed_ops(pr):
    """the same edits in reverse order (a REPLACE_FOUND keeps naming its FIND_OR_ADD): what an order-blind implementation would be free to run"""
    ops = ops_of(pr)
    n = len(ops)
    return with_ops(pr, [(k, p, n - 1 - a if k == REPLACE_FOUND else a, kf, s) for k, p, a, kf, s in reversed(ops)])


# ------------------------------------------------------------------------------------------------------------------ hand-worked cases
def base():
    """Three keyframes of four slots, six points.  p0 {kf0: s0, kf1: s0}  p1 {kf0: s1, kf1: s1, kf2: s1}  p2 {kf2: s2}  p3 fresh (no
    observation, Observations() = 0)  p4 {kf1: s3, kf2: s3}  p5 bad, no observation, still held by slot (kf0, s3).
    Observations e0..e7 in that order; slots 0..11 = (kf0: s0..s3, kf1: s0..s3, kf2: s0..s3)."""
    return dict(nkf=3, npts=6, kf_slot_off=np.array([0, 4, 8, 12], np.int32), kf_rank=None,
                kf_slot_pt=np.array([0, 1, -1, 5, 0, 1, -1, 4, -1, 1, 2, 4], np.int32), kf_slot_level=None, kf_slot_uv=None,
                pt_bad=np.array([0, 0, 0, 0, 0, 1], np.uint8), pt_nobs=np.array([2, 3, 1, 0, 2, 0], np.int32),
                pt_found=np.array([10, 20, 30, 40, 50, 60], np.int32), pt_visible=np.array([11, 21, 31, 41, 51, 61], np.int32),
                pt_replaced=np.full(6, -1, np.int32), obs_off=np.array([0, 2, 5, 6, 6, 8, 8], np.int32),
                obs_kf=np.array([0, 1, 0, 1, 2, 2, 1, 2], np.int32), obs_slot=np.array([0, 0, 1, 1, 1, 2, 3, 3], np.int32), obs_dead=None)


def _exp(b, status, found, slot_pt, bad, nobs, touched, off, kf, slot, src, counts, pfound=None, pvisible=None, replaced=None, level=None, uv=None):
    i32 = np.int32
    return dict(op_status=np.array(status, i32), op_found=np.array(found, i32), kf_slot_pt=np.array(slot_pt, i32), pt_bad=np.array(bad, np.uint8),
                pt_nobs=np.array(nobs, i32), pt_touched=np.array(touched, np.uint8), oobs_off=np.array(off, i32), oobs_kf=np.array(kf, i32),
                oobs_slot=np.array(slot, i32), oobs_src=np.array(src, i32), counts=np.array(counts, i32),
                pt_found=np.array(b["pt_found"] if pfound is None else pfound, i32), pt_visible=np.array(b["pt_visible"] if pvisible is None else pvisible, i32),
                pt_replaced=np.array(b["pt_replaced"] if replaced is None else replaced, i32),
                oobs_level=None if level is None else np.array(level, i32), oobs_uv=None if uv is None else np.array(uv, np.float32).reshape(-1, 2))


def hand_cases():
    """name -> (problem, expected outputs)"""
    b = base()
    H = {}
    # (a) NOP: nothing changes; the tables come back as they were (the input lists are in rank order already)
    H["a_nop"] = (with_ops(b, [(NOP, 9, 9, 9, 9)]),
                  _exp(b, [0], [-1], b["kf_slot_pt"], b["pt_bad"], b["pt_nobs"], [0] * 6, b["obs_off"], b["obs_kf"], b["obs_slot"], range(8), [8, 0, 0, 0, 0, 0, 0, 0]))
    # (b) ADD: p3 gains (kf0, s2) and is touched; the second ADD finds kf0 in p3's list (6) and STILL writes slot (kf0, s3), which held p5
    H["b_add"] = (with_ops(b, [(ADD, 3, 1, 0, 2), (ADD, 3, 0, 0, 3)]),
                  _exp(b, [5, 6], [-1, -1], [0, 1, 3, 3, 0, 1, -1, 4, -1, 1, 2, 4], b["pt_bad"], [2, 3, 1, 1, 2, 0], [0, 0, 0, 1, 0, 0], [0, 2, 5, 6, 7, 9, 9],
                       [0, 1, 0, 1, 2, 2, 0, 1, 2], [0, 0, 1, 1, 1, 2, 2, 3, 3], [0, 1, 2, 3, 4, 5, 8, 6, 7], [9, 1, 0, 0, 0, 1, 0, 0]))
    # (c) REPLACE: p0 -> p1, p1 names both keyframes: both slots erased.  p2 -> p2: nothing.  p4 -> p2: (kf1, s3) moves, (kf2, s3) is erased
    H["c_replace"] = (with_ops(b, [(REPLACE, 0, 1, 0, 0), (REPLACE, 2, 2, 0, 0), (REPLACE, 4, 2, 0, 0)]),
                      _exp(b, [8, 1, 8], [-1] * 3, [-1, 1, -1, 5, -1, 1, -1, 2, -1, 1, 2, -1], [1, 0, 0, 0, 1, 1], [2, 3, 2, 0, 2, 0], [0, 1, 1, 0, 0, 0],
                           [0, 0, 3, 5, 5, 5, 5], [0, 1, 2, 1, 2], [1, 1, 1, 3, 2], [2, 3, 4, 6, 5], [5, 0, 2, 0, 0, 2, 0, 0],
                           pfound=[10, 30, 80, 40, 50, 60], pvisible=[11, 32, 82, 41, 51, 61], replaced=[1, -1, -1, -1, 2, -1]))
    # (d) SET_BAD: p1 turns bad, its three slots become null, Observations() stays
    H["d_set_bad"] = (with_ops(b, [(SET_BAD, 1, 0, 0, 0)]),
                      _exp(b, [9], [-1], [0, -1, -1, 5, 0, -1, -1, 4, -1, -1, 2, 4], [0, 1, 0, 0, 0, 1], b["pt_nobs"], [0] * 6, [0, 2, 2, 3, 3, 5, 5],
                           [0, 1, 2, 1, 2], [0, 0, 2, 3, 3], [0, 1, 5, 6, 7], [5, 0, 0, 1, 0, 0, 0, 0]))
    # (e) FUSE, every outcome.  0: p0 names kf0 (1).  1: slot (kf0, s3) holds the bad p5 (2).  2: slot (kf0, s2) is null: p2 gains it (5).
    # 3: slot (kf1, s1) holds p1, 3 > 2 observations: p2 -> p1, p1 names kf2 and kf0: both of p2's slots erased (3).  4: p2 is bad (1).
    # 5: slot (kf1, s3) holds p4, 2 > 0: the fresh p3 -> p4 (3).  6: slot (kf2, s3) holds p4, 2 > 2 is false: p4 -> p0; p0 names kf1: erased,
    # (kf2, s3) moves (4).  p4 carried p3's counters: p0 gets 10 + (50 + 40).
    H["e_fuse"] = (with_ops(b, [(FUSE, 0, 0, 0, 1), (FUSE, 2, 0, 0, 3), (FUSE, 2, 0, 0, 2), (FUSE, 2, 0, 1, 1), (FUSE, 2, 0, 1, 2), (FUSE, 3, 0, 1, 3), (FUSE, 0, 0, 2, 3)]),
                   _exp(b, [1, 2, 5, 3, 1, 3, 4], [-1, -1, -1, 1, -1, 4, 4], [0, 1, -1, 5, 0, 1, -1, -1, -1, 1, -1, 0], [0, 0, 1, 1, 1, 1], [3, 3, 2, 0, 2, 0],
                        [1, 1, 0, 0, 1, 0], [0, 3, 6, 6, 6, 6, 6], [0, 1, 2, 0, 1, 2], [0, 0, 3, 1, 1, 1], [0, 1, 7, 2, 3, 4], [6, 1, 3, 0, 5, 3, 0, 0],
                        pfound=[100, 50, 30, 40, 90, 60], pvisible=[103, 52, 31, 41, 92, 61], replaced=[-1, -1, 1, 4, 0, -1]))
    # FUSE with equal observation counts: pt_nobs[p4] > pt_nobs[p0] is 2 > 2, false: the point in the slot (q = p4) is the one replaced
    H["e_fuse_tie"] = (with_ops(b, [(FUSE, 0, 0, 2, 3)]),
                       _exp(b, [4], [4], [0, 1, -1, 5, 0, 1, -1, -1, -1, 1, 2, 0], [0, 0, 0, 0, 1, 1], [3, 3, 1, 0, 2, 0], [1, 0, 0, 0, 0, 0], [0, 3, 6, 7, 7, 7, 7],
                            [0, 1, 2, 0, 1, 2, 2], [0, 0, 3, 1, 1, 1, 2], [0, 1, 7, 2, 3, 4, 5], [7, 0, 1, 0, 1, 1, 0, 0],
                            pfound=[60, 20, 30, 40, 50, 60], pvisible=[62, 21, 31, 41, 51, 61], replaced=[-1, -1, -1, -1, 0, -1]))
    # (f) FIND_OR_ADD and REPLACE_FOUND.  0: bad p5 in the slot (2).  1, 2: null slots: p3 gains (kf2, s0) and (kf0, s2) (5, 5).  3: null slot
    # (kf1, s2) but p0 names kf1 (6): the slot is written all the same.  4, 5: p3 and p2 both find p4 (7, 7).  6: op 0 found nothing (1).
    # 7: p4 -> p3: (kf1, s3) moves, (kf2, s3) erased.  8: p4 AGAIN -> p2: its list is empty, its counters are added a second time.
    H["f_find_replace_twice"] = (
        with_ops(b, [(FIND_OR_ADD, 3, 0, 0, 3), (FIND_OR_ADD, 3, 0, 2, 0), (FIND_OR_ADD, 3, 0, 0, 2), (FIND_OR_ADD, 0, 0, 1, 2), (FIND_OR_ADD, 3, 0, 1, 3),
                     (FIND_OR_ADD, 2, 0, 2, 3), (REPLACE_FOUND, 3, 0, 0, 0), (REPLACE_FOUND, 3, 4, 0, 0), (REPLACE_FOUND, 2, 5, 0, 0)]),
        _exp(b, [2, 5, 5, 6, 7, 7, 1, 8, 8], [-1, -1, -1, -1, 4, 4, -1, -1, -1], [0, 1, 3, 5, 0, 1, 0, 3, 3, 1, 2, -1], [0, 0, 0, 0, 1, 1], [2, 3, 1, 3, 2, 0],
             [0, 0, 1, 1, 0, 0], [0, 2, 5, 6, 9, 9, 9], [0, 1, 0, 1, 2, 2, 0, 1, 2], [0, 0, 1, 1, 1, 2, 2, 3, 0], [0, 1, 2, 3, 4, 5, 10, 6, 9], [9, 2, 2, 0, 5, 2, 0, 0],
             pfound=[10, 20, 80, 90, 50, 60], pvisible=[11, 21, 82, 92, 51, 61], replaced=[-1, -1, -1, -1, 2, -1]))
    # (g) a chain p2 -> p4, p4 -> p0, then FUSE of the fresh p3 meets p0 in slot (kf2, s3), which p4 handed over: 3 > 0, p3 -> p0
    H["g_chain"] = (with_ops(b, [(REPLACE, 2, 4, 0, 0), (REPLACE, 4, 0, 0, 0), (FUSE, 3, 0, 2, 3)]),
                    _exp(b, [8, 8, 3], [-1, -1, 0], [0, 1, -1, 5, 0, 1, -1, -1, -1, 1, -1, 0], [0, 0, 1, 1, 1, 1], [3, 3, 1, 0, 2, 0], [1, 0, 0, 0, 1, 0],
                         [0, 3, 6, 6, 6, 6, 6], [0, 1, 2, 0, 1, 2], [0, 0, 3, 1, 1, 1], [0, 1, 7, 2, 3, 4], [6, 0, 3, 0, 1, 2, 0, 0],
                         pfound=[130, 20, 30, 40, 80, 60], pvisible=[134, 21, 31, 41, 82, 61], replaced=[-1, -1, 4, 0, 0, -1]))
    # (h) the pure rebuild: no edits, e1 and e7 died in an earlier call (their slots are null), the ranks reverse the index order, and the
    # level / keypoint of every observation is gathered from its slot (level = slot index mod 8, uv = (index + 0.5, 2 index))
    h = dict(b, kf_rank=np.array([2, 1, 0], np.int32), obs_dead=np.array([0, 1, 0, 0, 0, 0, 0, 1], np.uint8),
             kf_slot_pt=np.array([0, 1, -1, 5, -1, 1, -1, 4, -1, 1, 2, -1], np.int32), kf_slot_level=(np.arange(12) % 8).astype(np.int32),
             kf_slot_uv=np.array([[i + 0.5, 2 * i] for i in range(12)], np.float32))
    H["h_rebuild_dead"] = (with_ops(h, []),
                           _exp(h, [], [], h["kf_slot_pt"], h["pt_bad"], h["pt_nobs"], [0] * 6, [0, 1, 4, 5, 5, 6, 6], [0, 2, 1, 0, 2, 1], [0, 1, 1, 1, 2, 3],
                                [0, 4, 3, 2, 5, 6], [6, 0, 0, 0, 0, 0, 0, 0], level=[0, 1, 5, 1, 2, 7],
                                uv=[[0.5, 0], [9.5, 18], [5.5, 10], [1.5, 2], [10.5, 20], [7.5, 14]]))
    # (i) a late add and SetBadFlag on fused slots.  0: p3 gains the null slot (kf1, s2).  1: p2 -> p3: (kf2, s2) moves, p3 is touched.
    # 2: p3 gains (kf0, s2) AFTER its touch: a late add.  3: p3 turns bad: the three slots the edits gave it become null.
    H["i_late_add_set_bad"] = (
        with_ops(b, [(FUSE, 3, 0, 1, 2), (REPLACE, 2, 3, 0, 0), (FIND_OR_ADD, 3, 0, 0, 2), (SET_BAD, 3, 0, 0, 0)]),
        _exp(b, [5, 8, 5, 9], [-1] * 4, [0, 1, -1, 5, 0, 1, -1, 4, -1, 1, -1, 4], [0, 0, 1, 1, 0, 1], [2, 3, 1, 3, 2, 0], [0, 0, 0, 1, 0, 0], [0, 2, 5, 5, 5, 7, 7],
             [0, 1, 0, 1, 2, 1, 2], [0, 0, 1, 1, 1, 3, 3], [0, 1, 2, 3, 4, 6, 7], [7, 2, 1, 1, 2, 1, 1, 0],
             pfound=[10, 20, 30, 70, 50, 60], pvisible=[11, 21, 31, 72, 51, 61], replaced=[-1, -1, 3, -1, -1, -1]))
    return H


# ------------------------------------------------------------------------------------------------------------------ seeded maps
def make_map(seed, nkf, npts, slots_per_kf, max_obs=7, n_long=0, long_obs=0, n_fresh=None, n_stale=None):
    """a consistent map: every point observed by a random set of keyframes (n_long of them by long_obs keyframes), each observation in a slot
    of its own that holds the point, the lists in random order, the ranks a random permutation; n_fresh points without observation and
    n_stale bad ones without observation that a slot still holds; null slots left in every keyframe"""
    rng = np.random.default_rng(seed)
    n_fresh = max(2, npts // 15) if n_fresh is None else n_fresh
    n_stale = max(1, npts // 30) if n_stale is None else n_stale
    used = [0] * nkf
    lists = []
    room = slots_per_kf * 2 // 3                                        # (a third of every keyframe stays null)
    for p in range(npts):
        if p >= npts - n_fresh - n_stale:
            lists.append([])
            continue
        n = long_obs if p < n_long else int(rng.integers(2, max_obs + 1))
        kfs = [int(k) for k in rng.permutation(nkf)[:min(n, nkf)] if used[k] < room]
        row = []
        for k in kfs:
            row.append((k, used[k]))
            used[k] += 1
        lists.append(row)
    slot_off = np.arange(nkf + 1, dtype=np.int32) * slots_per_kf
    slot_pt = np.full(nkf * slots_per_kf, -1, np.int32)
    off, okf, oslot = [0], [], []
    for p, row in enumerate(lists):
        for k, s in row:
            okf.append(k); oslot.append(s)
            slot_pt[slot_off[k] + s] = p
        off.append(len(okf))
    bad = np.zeros(npts, np.uint8)
    for p in range(npts - n_stale, npts):                               # bad points a slot still holds
        k = int(rng.integers(nkf))
        bad[p] = 1
        slot_pt[slot_off[k] + used[k]] = p
        used[k] += 1
    nobs = np.array([len(r) for r in lists], np.int32)
    nslots = nkf * slots_per_kf
    return dict(nkf=nkf, npts=npts, kf_slot_off=slot_off, kf_rank=rng.permutation(nkf).astype(np.int32), kf_slot_pt=slot_pt,
                kf_slot_level=rng.integers(0, 8, nslots).astype(np.int32), kf_slot_uv=rng.uniform(0, 640, (nslots, 2)).astype(np.float32), pt_bad=bad,
                pt_nobs=(nobs + (rng.random(npts) < 0.1) * (nobs > 0)).astype(np.int32),         # Observations() is not the list length
                pt_found=rng.integers(1, 50, npts).astype(np.int32), pt_visible=rng.integers(50, 99, npts).astype(np.int32),
                pt_replaced=np.full(npts, -1, np.int32), obs_off=np.array(off, np.int32), obs_kf=np.array(okf, np.int32), obs_slot=np.array(oslot, np.int32),
                obs_dead=None, _used=used)


def _null_slot(pr, rng, K):
    so = pr["kf_slot_off"]
    free = np.flatnonzero(pr["kf_slot_pt"][so[K]:so[K + 1]] < 0)
    return int(rng.choice(free))


def _held_slot(pr, rng, K):
    so = pr["kf_slot_off"]
    held = np.flatnonzero(pr["kf_slot_pt"][so[K]:so[K + 1]] >= 0)
    return int(rng.choice(held))


def _alive_slot(pr, rng, K):
    so = pr["kf_slot_off"]
    row = pr["kf_slot_pt"][so[K]:so[K + 1]]
    return int(rng.choice([s for s in range(len(row)) if row[s] >= 0 and not pr["pt_bad"][row[s]]]))


def search_in_neighbors(pr, rng, targets, rows, p_null=0.35, p_masked=0.1):
    """ORBmatcher::Fuse over the target keyframes (src/LocalMapping.cc SearchInNeighbors): per target `rows` accepted candidates, each a point
    and the keypoint it matched - a null slot or one that holds a point; rows over TH_LOW come as NOP"""
    ops = []
    alive = np.flatnonzero(pr["pt_bad"] == 0)
    for K in targets:
        for p in rng.choice(alive, rows, replace=len(alive) < rows):
            if rng.random() < p_masked:
                ops.append((NOP, 0, 0, 0, 0))
            else:
                ops.append((FUSE, int(p), 0, int(K), _null_slot(pr, rng, K) if rng.random() < p_null else _held_slot(pr, rng, K)))
    return ops


def search_and_fuse(pr, rng, K, rows):
    """ORBmatcher::Fuse(keyframe, Scw, ...) and the replace loop (src/LoopClosing.cc:600-623) for one keyframe: the FIND_OR_ADD rows, then one
    REPLACE_FOUND per row"""
    alive = np.flatnonzero(pr["pt_bad"] == 0)
    ops = [(FIND_OR_ADD, int(p), 0, int(K), _null_slot(pr, rng, K) if rng.random() < 0.4 else _held_slot(pr, rng, K)) for p in rng.choice(alive, rows, replace=False)]
    return ops, [(REPLACE_FOUND, ops[j][1], j, 0, 0) for j in range(rows)]


def correct_loop(pr, rng, K, rows):
    """LoopClosing::CorrectLoop's fusion (src/LoopClosing.cc:527-539): per matched keypoint of the current keyframe, Replace when it holds a
    point, otherwise AddMapPoint + AddObservation + ComputeDistinctiveDescriptors"""
    so = pr["kf_slot_off"]
    ops = []
    alive = np.flatnonzero(pr["pt_bad"] == 0)
    for s in rng.choice(so[K + 1] - so[K], rows, replace=False):
        cur, loop = int(pr["kf_slot_pt"][so[K] + s]), int(rng.choice(alive))
        ops.append((REPLACE, cur, loop, 0, 0) if cur >= 0 else (ADD, loop, 1, int(K), int(s)))
    return ops


def make(seed, nkf, npts, nops, slots_per_kf=None, chain=0, n_long=0, long_obs=0):
    """a seeded map with an edit list of (about) nops edits, mixed from every call site, and the injections: a chain of `chain` Replace
    calls a -> b, b -> c, ... ended by a FUSE that meets the last; the merge of the two longest lists; a late add; an ADD that finds its
    keyframe named while the slot holds another point; SetBadFlag on a point an edit just fused; a REPLACE_FOUND of a point replaced before"""
    rng = np.random.default_rng(seed)
    slots_per_kf = slots_per_kf or max(12, 3 * npts * 5 // nkf // 2)
    pr = make_map(seed, nkf, npts, slots_per_kf, n_long=n_long, long_obs=long_obs)
    used = pr.pop("_used")
    n_fresh = max(2, npts // 15)
    n_stale = max(1, npts // 30)
    fresh = list(range(npts - n_fresh - n_stale, npts - n_stale))
    ops = []
    # ProcessNewKeyFrame (src/LocalMapping.cc:141-152): the newest keyframe's tracked points gain their observation; one is "already in"
    K = nkf - 1
    so = pr["kf_slot_off"]
    tracked = [int(p) for p in rng.choice(np.flatnonzero(pr["pt_bad"] == 0), 4, replace=False)]
    for p in tracked:
        ops.append((ADD, p, 1, K, _null_slot(pr, rng, K)))
    ops.append((ADD, tracked[0], 1, K, _held_slot(pr, rng, K)))         # the keyframe is named already: 6, and the slot changes hands
    # CreateNewMapPoints (:380-385): a fresh point gains two observations, touched at the second
    for p in fresh[:max(1, len(fresh) // 2)]:
        k1, k2 = (int(v) for v in rng.choice(nkf, 2, replace=False))
        ops += [(ADD, p, 0, k1, _null_slot(pr, rng, k1)), (ADD, p, 1, k2, _null_slot(pr, rng, k2))]
    # MapPointCulling (:167-194)
    for p in rng.choice(npts, max(2, nops // 20), replace=False):
        ops.append((SET_BAD, int(p), 0, 0, 0))
    if chain:
        c = [int(p) for p in rng.choice(np.flatnonzero((pr["pt_bad"] == 0) & (np.diff(pr["obs_off"]) > 0)), chain + 1, replace=False)]
        ops += [(REPLACE, c[i], c[i + 1], 0, 0) for i in range(chain)]
        e = int(pr["obs_off"][c[-1]])
        ops.append((FUSE, fresh[-1], 0, int(pr["obs_kf"][e]), int(pr["obs_slot"][e])))
    if n_long >= 2:
        ops.append((REPLACE, 0, 1, 0, 0))                               # the two longest lists merge
    # a late add: b is touched by a Replace, then gains a null slot of a keyframe it does not name
    short = np.flatnonzero((pr["pt_bad"] == 0) & (np.diff(pr["obs_off"]) > 0) & (np.diff(pr["obs_off"]) <= 3))
    a, bb = (int(p) for p in rng.choice(short, 2, replace=False))
    named = set(int(k) for p in (a, bb) for k in pr["obs_kf"][pr["obs_off"][p]:pr["obs_off"][p + 1]])
    Kl = next(k for k in range(nkf) if k not in named)
    ops += [(REPLACE, a, bb, 0, 0), (FIND_OR_ADD, bb, 0, Kl, _null_slot(pr, rng, Kl)), (SET_BAD, bb, 0, 0, 0)]      # ... and SetBadFlag on the fused slots
    n_rest = max(nops - len(ops), 12)
    n_sf = max(3, n_rest // 8)
    f1, r1 = search_and_fuse(pr, rng, int(rng.integers(nkf)), n_sf)
    f1[0] = f1[0][:4] + (_alive_slot(pr, rng, f1[0][3]),)
    f1.append(f1[0][:1] + (f1[1][1],) + f1[0][2:])                      # a second point that finds what the first row found
    r1.append((REPLACE_FOUND, f1[-1][1], len(f1) - 1, 0, 0))
    base_i = len(ops)
    ops += f1 + [(k, p, base_i + j, kf, s) for k, p, j, kf, s in r1]
    ops += correct_loop(pr, rng, int(rng.integers(nkf)), max(2, n_rest // 10))
    n_left = max(nops - len(ops), 6)
    targets = rng.choice(nkf, max(2, min(nkf, n_left // 30 + 1)), replace=False)
    ops += search_in_neighbors(pr, rng, targets, -(-n_left // len(targets)))
    return with_ops(pr, ops)


def seeded():
    """name -> problem: the sizes at which the kernels can still go wrong.  small: one workgroup of everything.  big: more than 1024 edits, two
    points with more than 64 observations that merge (a list longer than a wave), a component of more than 40 chained edits; big-5-dead
    is such a map after an earlier call erased a tenth of its observations (obs_dead), with its edits kept"""
    S = {"small-%d" % s: make(s, nkf=8, npts=60, nops=40) for s in (1, 2, 3)}
    S["big-4"] = make(4, nkf=80, npts=2000, nops=1500, chain=42, n_long=2, long_obs=72)
    S["big-5-dead"] = with_dead(make(5, nkf=80, npts=2000, nops=1500, chain=42, n_long=2, long_obs=72), keep_ops=True)      # rows with holes, edits on top
    for pr in S.values():
        for v in pr.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return S


def long_chain(pr):
    """the longest run of consecutive REPLACE edits in which each replaces the point the one before merged into"""
    best = run = 0
    ops = ops_of(pr)
    for i, (k, p, a, _, _) in enumerate(ops):
        run = run + 1 if (k == REPLACE and i and ops[i - 1][0] == REPLACE and ops[i - 1][2] == p) else (1 if k == REPLACE else 0)
        best = max(best, run)
    return best


def with_dead(pr, seed=7, keep_ops=False):
    """the problem as a caller holds it after an earlier table call erased a tenth of its observations: obs_dead marks them, their slots are
    null.  The edit list is dropped (the pure rebuild) or kept: its edits then meet other points and null slots, all of them still in range"""
    rng = np.random.default_rng(seed)
    dead = (rng.random(len(pr["obs_kf"])) < 0.1).astype(np.uint8)
    slot_pt = np.array(pr["kf_slot_pt"])
    slot_pt[(pr["kf_slot_off"][pr["obs_kf"]] + pr["obs_slot"])[dead != 0]] = -1
    q = dict(pr, obs_dead=dead, kf_slot_pt=slot_pt)
    return q if keep_ops else with_ops(q, [])
