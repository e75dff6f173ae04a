"""Map tables for the tests of orbl_loop_sim3_candidates (tests/test_loopsim3_*.py, tests/test_gpu_loopsim3*.py): hand-worked cases, seeded
maps and the seam shapes of the kernel.  The feature vectors are given directly as node lists - no vocabulary is needed - and the
descriptors are noisy copies of a few base descriptors, so that equal and nearly equal distances are frequent.  Test infrastructure only."""
import numpy as np

N_LEVELS = 8
LEVEL_SIGMA2 = np.array([np.float32(1.2) ** (2 * i) for i in range(N_LEVELS)], np.float32)
SEEDS = list(range(101, 111))                               # the 10 seeded maps


def flip(desc, bits):
    """a copy of the 32-byte descriptor with the listed bits (0..255) inverted"""
    d = np.array(desc, np.uint8)
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


class Builder:
    """Keyframes as slot lists, points, and the observation lists that follow from the slots unless a test edits them."""

    def __init__(self):
        self.kfs, self.X, self.pt_bad, self.obs_edit = [], [], [], {}

    def point(self, X=(0.0, 0.0, 1.0), bad=0):
        self.X.append([float(v) for v in X]); self.pt_bad.append(int(bad))
        return len(self.X) - 1

    def keyframe(self, Tcw=None, K4=(400.0, 410.0, 320.0, 240.0), bad=0):
        T = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64) if Tcw is None else np.asarray(Tcw, np.float64).reshape(12)
        self.kfs.append(dict(T=T, K4=np.asarray(K4, np.float32), bad=int(bad), slots=[], nodes={}))
        return len(self.kfs) - 1

    def slot(self, k, pt, desc, angle=0.0, level=0, node=None):
        """a keypoint of keyframe k; node: the vocabulary node whose list it joins (None: in no list)"""
        kf = self.kfs[k]
        kf["slots"].append((int(pt), np.array(desc, np.uint8), float(angle), int(level)))
        i = len(kf["slots"]) - 1
        if node is not None:
            kf["nodes"].setdefault(int(node), []).append(i)
        return i

    def observe(self, pt, k, slot):
        """what the point's observation of keyframe k names: a slot, or None for no observation"""
        self.obs_edit[(pt, k)] = slot

    def tables(self, obs_order=None):
        nkf, npts = len(self.kfs), len(self.X)
        t = dict(kf_bad=np.array([kf["bad"] for kf in self.kfs], np.uint8), kf_Tcw=np.array([kf["T"] for kf in self.kfs], np.float64).reshape(nkf, 12),
                 kf_K4=np.array([kf["K4"] for kf in self.kfs], np.float32).reshape(nkf, 4), level_sigma2=LEVEL_SIGMA2.copy(),
                 pt_bad=np.array(self.pt_bad, np.uint8), X=np.array(self.X, np.float64).reshape(npts, 3))
        so, pt, lvl, ang, desc, fo, node, eo, ent = [0], [], [], [], [], [0], [], [0], []
        obs = [[] for _ in range(npts)]
        for k, kf in enumerate(self.kfs):
            for i, (p, d, a, l) in enumerate(kf["slots"]):
                pt.append(p); desc.append(d); ang.append(a); lvl.append(l)
                if p >= 0:
                    s = self.obs_edit.get((p, k), i)
                    if s is not None and not any(e[0] == k for e in obs[p]):
                        obs[p].append((k, s))
            so.append(len(pt))
            for nd in sorted(kf["nodes"]):
                node.append(nd); ent += kf["nodes"][nd]; eo.append(len(ent))
            fo.append(len(node))
        for (p, k), s in self.obs_edit.items():                 # an observation of a keyframe that does not hold the point
            if s is not None and not any(e[0] == k for e in obs[p]):
                obs[p].append((k, s))
        if obs_order is not None:
            for lst in obs:
                obs_order.shuffle(lst)
        oo, ok, os_ = [0], [], []
        for lst in obs:
            ok += [e[0] for e in lst]; os_ += [e[1] for e in lst]; oo.append(len(ok))
        t.update(kf_slot_off=np.array(so, np.int32), kf_slot_pt=np.array(pt, np.int32), kf_slot_level=np.array(lvl, np.int32), kf_slot_angle=np.array(ang, np.float32),
                 kf_slot_desc=np.array(desc, np.uint8).reshape(-1, 32), kf_fv_off=np.array(fo, np.int32), fv_node=np.array(node, np.uint32),
                 fv_ent_off=np.array(eo, np.int32), fv_ent=np.array(ent, np.int32), obs_off=np.array(oo, np.int32), obs_kf=np.array(ok, np.int32),
                 obs_slot=np.array(os_, np.int32))
        return t


def _pose(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return np.concatenate([Q, rng.normal(0, 2, (3, 1))], 1).reshape(12)


# ------------------------------------------------------------------------------------------------ hand-worked cases
def hand_cases():
    """[(name, tab, cur_kf, cand_kf, expected)]: expected holds the outputs worked by hand (match12 rows, nmatches, cand_status, off and
    the rows' i1 / points), under nnratio 0.75, check_ori 1, min_matches as given in `args`."""
    out = []
    D = np.zeros(32, np.uint8)
    # 1. one node, order decides: current entries a (slot 0), b (slot 1); candidate entries x (slot 0), y (slot 1), z (slot 2, no point).
    #    d(a, x) = 2, d(a, y) = 5: a takes x (2 < 0.75 * 5).  d(b, x) = 0 but x is taken; d(b, y) = 3 alone: runner-up 256, b takes y.
    #    z would be b's exact copy but holds no point.  A third current entry c (slot 2) sees only taken entries: nothing.
    #    Points (1 + i, 2 - i, 4 + i / 2); the current keyframe is [I | (1, 2, 3)], the candidate a quarter turn about z plus (0.5, 0, -1).
    #    max_err: levels 1, 2 and 3, 0 -> (size_t)(9.21 * 1.2^(2 level)) = 13, 19 and 27, 9.
    B = Builder()
    k0, k1 = B.keyframe(Tcw=[1, 0, 0, 1, 0, 1, 0, 2, 0, 0, 1, 3]), B.keyframe(Tcw=[0, -1, 0, 0.5, 1, 0, 0, 0, 0, 0, 1, -1], K4=(500.0, 505.0, 300.0, 200.0))
    pa, pb, pc, px, py = [B.point((1 + i, 2 - i, 4 + 0.5 * i)) for i in range(5)]
    x = flip(D, [0, 1]); b = x.copy()
    B.slot(k0, pa, D, 10.0, 1, node=7); B.slot(k0, pb, b, 10.0, 2, node=7); B.slot(k0, pc, D, 10.0, 0, node=7)
    B.slot(k1, px, x, 5.0, 3, node=7); B.slot(k1, py, flip(b, [100, 101, 102]), 5.0, 0, node=7); B.slot(k1, -1, b, 5.0, 0, node=7)
    out.append(("order decides", B.tables(), k0, [k1], dict(args=dict(min_matches=2), match12=[[0, 1, -1]], nmatches=[2], cand_status=[0], off=[0, 2],
                                                               row_i1=[0, 1], row_pt1=[pa, pb], row_pt2=[px, py], max_err1=[13.0, 19.0], max_err2=[27.0, 9.0],
                                                               X1c=[[2, 4, 7], [3, 3, 7.5]], X2c=[[1.5, 4, 4.5], [2.5, 5, 5]])))
    # 2. ties, one node per current entry: node 3 offers two candidates at distance 4 - the ratio test fails on the tie (4 < 0.75 * 4 is
    #    false); node 4 offers 3 and 4 - 3 < 0.75 * 4 = 3 fails on equality; node 5 offers 1 and 2 - 1 < 1.5 passes and takes slot 4.
    B = Builder()
    k0, k1 = B.keyframe(), B.keyframe()
    p = [B.point((i, 1, 5)) for i in range(8)]
    B.slot(k0, p[0], D, 0.0, 0, node=3); B.slot(k0, p[1], flip(D, [200]), 0.0, 0, node=4); B.slot(k0, p[2], D, 0.0, 0, node=5)
    B.slot(k1, p[3], flip(D, [0, 1, 2, 3]), 0.0, 0, node=3); B.slot(k1, p[4], flip(D, [4, 5, 6, 7]), 0.0, 0, node=3)
    B.slot(k1, p[5], flip(D, [200, 1, 2, 3]), 0.0, 0, node=4); B.slot(k1, p[6], flip(D, [200, 4, 5, 6, 7]), 0.0, 0, node=4)
    B.slot(k1, p[7], flip(D, [9]), 0.0, 0, node=5); B.slot(k1, p[3], flip(D, [9, 10]), 0.0, 0, node=5)
    out.append(("ties", B.tables(), k0, [k1], dict(args=dict(min_matches=1), match12=[[-1, -1, 4]], nmatches=[1], cand_status=[0], off=[0, 1], row_i1=[2], row_pt1=[p[2]],
                                                      row_pt2=[p[7]])))
    # 3. the rotation check and its vbMatched2: 12 nodes, one entry each side, exact copies.  Ten pairs have rot 0 (bin 0), one has rot 90
    #    (bin 3): 1 < 0.1 * 10 is false, so bin 3 is kept too; with eleven in bin 0 it is dropped.  Node 50 holds the rejected pair and
    #    BEHIND it a second current entry whose only candidate is the one the rejected match took: it stays unmatched.
    for n0, kept in ((10, True), (11, False)):
        B = Builder()
        k0, k1 = B.keyframe(), B.keyframe()
        for i in range(n0):
            d = flip(D, [8 * i, 8 * i + 1, 8 * i + 2, 255 - i]); q = B.point((i, 0, 3))
            B.slot(k0, q, d, 40.0, 0, node=i); B.slot(k1, q, d, 40.0, 0, node=i)
        d = flip(D, [130, 140, 150, 160, 170]); q, r = B.point((0, 1, 3)), B.point((0, 2, 3))
        B.slot(k0, q, d, 130.0, 0, node=50); B.slot(k0, r, d, 40.0, 0, node=50); B.slot(k1, q, d, 40.0, 0, node=50)
        m = list(range(n0)) + ([n0] if kept else [-1]) + [-1]
        nm = n0 + (1 if kept else 0)
        out.append(("rotation, bin 3 %s" % ("kept" if kept else "dropped"), B.tables(), k0, [k1],
                    dict(args=dict(min_matches=5), match12=[m], nmatches=[nm], cand_status=[0], off=[0, nm], row_i1=[i for i in range(n0 + 1) if m[i] >= 0])))
    # 4. GetIndexInKeyFrame: the point of current slot 0 is observed in the current keyframe at slot 2 (level 5, not 1): max_err1 from
    #    level 5; the point of slot 1 has no observation of the current keyframe: no row; the candidate's point of slot 2 has none of the
    #    candidate: no row either.  A bad candidate and the current keyframe itself as a candidate ride along.
    B = Builder()
    k0, k1, k2 = B.keyframe(), B.keyframe(), B.keyframe(bad=1)
    p = [B.point((i, i, 6)) for i in range(6)]
    ds = [flip(D, [16 * i + j for j in range(6)]) for i in range(3)]
    for i in range(3):
        B.slot(k0, p[i], ds[i], 0.0, [1, 2, 5][i], node=i); B.slot(k1, p[3 + i], ds[i], 0.0, [4, 0, 3][i], node=i); B.slot(k2, p[i], ds[i], 0.0, 0, node=i)
    B.observe(p[0], k0, 2); B.observe(p[1], k0, None); B.observe(p[5], k1, None)
    out.append(("index in keyframe", B.tables(), k0, [k1, k2, k0], dict(args=dict(min_matches=3), match12=[[0, 1, 2], [-1] * 3, [0, 1, 2]], nmatches=[3, 0, 3],
                                                                        cand_status=[0, 1, 0], off=[0, 1, 1, 3], row_i1=[0, 0, 2], row_pt1=[p[0], p[0], p[2]],
                                                                        row_pt2=[p[3], p[0], p[2]], max_err1=[57.0, 57.0, 57.0], max_err2=[39.0, 57.0, 57.0])))
    return out


# ------------------------------------------------------------------------------------------------ the gate
def gate_case():
    """One current keyframe of 30 single-entry nodes and four candidates: A matches 20 of them (kept), B 19 (discarded), C 22 of which
    only 12 points are observed in C (kept with 22 matches and 12 rows: iterate will answer TOO_FEW), D is bad.  Exact copies, one bin."""
    rng = np.random.default_rng(7)
    B = Builder()
    k0, ka, kb, kc, kd = B.keyframe(_pose(rng)), B.keyframe(_pose(rng)), B.keyframe(_pose(rng)), B.keyframe(_pose(rng)), B.keyframe(_pose(rng), bad=1)
    pts = [B.point(rng.normal(0, 3, 3)) for _ in range(30)]
    ds = rng.integers(0, 256, (30, 32), dtype=np.uint8)
    for i in range(30):
        B.slot(k0, pts[i], ds[i], 20.0, i % N_LEVELS, node=2 * i + 1)
    for k, n in ((ka, 20), (kb, 19), (kc, 22), (kd, 30)):
        for i in range(n):
            B.slot(k, pts[i], ds[i], 20.0, (i + k) % N_LEVELS, node=2 * i + 1)
    for i in range(10):
        B.observe(pts[2 * i], kc, None)
    return B.tables(), k0, [ka, kb, kc, kd], dict(nmatches=[20, 19, 22, 0], cand_status=[0, 2, 0, 1], off=[0, 20, 20, 32, 32])


# ------------------------------------------------------------------------------------------------ seeded maps
def make(seed):
    """A map of 6-12 keyframes with 300-600 features each over ~25 vocabulary nodes.  Points come in twins that share a base descriptor and
    a node (equal distances), a slot's descriptor is its point's base with 0-5 bits inverted, and a few per cent of everything is
    irregular: bad points and one bad keyframe, slots without points, points whose observation names another slot or is missing,
    rotation outliers, nodes that one keyframe lacks.  Returns dict(tab, cur_kf, cand_kf)."""
    rng = np.random.default_rng(seed)
    nkf, npts, n_nodes = int(rng.integers(6, 13)), 700, 25
    base = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    for p in range(1, npts, 2):
        if rng.random() < 0.5:
            base[p] = base[p - 1]                               # a twin
    node_of = (rng.integers(0, n_nodes, npts // 2 + 1).repeat(2)[:npts]) * 11 + 5
    B = Builder()
    for p in range(npts):
        B.point(rng.normal(0, 4, 3), bad=rng.random() < 0.04)
    bad_kf = int(rng.integers(1, nkf))
    rot = rng.uniform(0, 360, nkf)
    for k in range(nkf):
        B.keyframe(_pose(rng), K4=(400 + k, 405 + k, 320.5, 240.25), bad=k == bad_kf)
        n = int(rng.integers(300, 601))
        held = rng.permutation(npts)[:n]
        skip_nodes = set(rng.choice(np.unique(node_of), 2, replace=False).tolist())
        order = []
        for p in held:
            p = int(p)
            d = flip(base[p], rng.integers(0, 256, int(rng.choice([0, 0, 1, 2, 3, 5]))))
            ang = (rot[k] + rng.normal(0, 4)) % 360 if rng.random() > 0.12 else rng.uniform(0, 360)
            has_pt = rng.random() > 0.2
            nd = int(node_of[p]) if rng.random() > 0.03 else int(rng.choice(node_of))
            order.append((p if has_pt else -1, d, ang, int(rng.integers(0, N_LEVELS)), None if nd in skip_nodes else nd))
        for s in order:
            B.slot(k, *s)
        slots = B.kfs[k]["slots"]
        for i, s in enumerate(slots):
            if s[0] >= 0:
                u = rng.random()
                if u < 0.06:
                    B.observe(s[0], k, None)
                elif u < 0.14:
                    B.observe(s[0], k, int(rng.integers(0, len(slots))))
        if seed % 2:                                            # (list order is not index order)
            for lst in B.kfs[k]["nodes"].values():
                rng.shuffle(lst)
    cand = [k for k in range(1, nkf)] + [0, 1]
    return dict(tab=B.tables(obs_order=rng), cur_kf=0, cand_kf=np.array(cand, np.int32))


# ------------------------------------------------------------------------------------------------ the seam shapes of the kernel
KF2_LISTS = (1, 63, 64, 65, 256, 257, 300)                    # candidate node lists: a lane's four registers, the tail from memory
KF1_LISTS = (64, 65, 130)                                     # current node lists: the 64-entry slice


SEAM_SHAPES = ((64, 1), (65, 63), (130, 64), (64, 65), (65, 256), (130, 257), (64, 300), (65, 257), (130, 300))    # (current, candidate) per node


def seam_case(n_cand=7, seed=5):
    """One current keyframe whose nodes have the SEAM_SHAPES list lengths - every KF1_LISTS and every KF2_LISTS length, the long ones
    paired both ways -, n_cand candidates built alike (the last one has no feature-vector node at all), and a current-side node no
    candidate has.  The current entries copy candidate entries from all over the list - the far end of a 300-entry list included - with a
    few bits inverted.  Every candidate's row is computed on its own, so the first 1 and 2 candidates are cases too."""
    rng = np.random.default_rng(seed)
    B = Builder()
    k0 = B.keyframe(_pose(rng))
    cands = [B.keyframe(_pose(rng), K4=(450.0 + c, 455.0, 310.0, 230.0)) for c in range(n_cand)]
    shapes = SEAM_SHAPES
    assert {a for a, _ in shapes} == set(KF1_LISTS) and {b for _, b in shapes} == set(KF2_LISTS)
    lists2 = {}
    for c, k in enumerate(cands):
        empty = c == n_cand - 1
        for nd, (a, b) in enumerate(shapes):
            lst = []
            for j in range(b):
                d = rng.integers(0, 256, 32, dtype=np.uint8)
                has_pt = rng.random() > 0.1
                B.slot(k, B.point(rng.normal(0, 3, 3), bad=rng.random() < 0.05) if has_pt else -1, d, rng.uniform(0, 360), int(rng.integers(0, N_LEVELS)),
                       node=None if empty else 3 * nd + 2)
                lst.append(d)
            lists2[(c, nd)] = lst
    for nd, (a, b) in enumerate(shapes):
        for j in range(a):
            src = lists2[(int(rng.integers(0, min(n_cand, 2))) if rng.random() < 0.7 else int(rng.integers(0, n_cand)), nd)]    # (mostly the first two)
            pos = b - 1 - (j % b) if j % 3 == 0 else int(rng.integers(0, b))       # (every third copies from the far end backwards)
            d = flip(src[pos], rng.integers(0, 256, int(rng.choice([0, 1, 2, 4]))))
            B.slot(k0, B.point(rng.normal(0, 3, 3)) if rng.random() > 0.1 else -1, d, rng.uniform(0, 360), int(rng.integers(0, N_LEVELS)), node=3 * nd + 2)
    for j in range(5):
        B.slot(k0, B.point(), rng.integers(0, 256, 32, dtype=np.uint8), 0.0, 0, node=1000)
    return dict(tab=B.tables(obs_order=rng), cur_kf=k0, cand_kf=np.array(cands, np.int32))
