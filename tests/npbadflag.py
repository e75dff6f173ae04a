"""Restatement of orbl_set_bad_keyframes: KeyFrame::SetBadFlag (src/KeyFrame.cc:460-553) called on a list of keyframes one after the
other, written as the literal sequential loop over dicts, sets and lists - no closed form.  TEST INFRASTRUCTURE.

A problem is a dict of flat arrays, as the entry point takes them (include/orbslam_hip.h): nkf, npts, tgt_kf, tgt_flags, tgt_mask, kf_bad,
kf_parent, kf_rank, kf_Tcw, child_off / child_kf, conn_off / conn_kf / conn_w, ord_off / ord_kf / ord_w and the point set kf_slot_off /
kf_slot_pt, pt_bad, pt_nobs, pt_ref_kf, obs_off / obs_kf / obs_slot (tgt_flags, tgt_mask, kf_rank may be None).

set_bad_keyframes(pr, points) returns the outputs by the entry's names plus "paths", a Counter of the branches the loop took."""
import copy
from collections import Counter

import numpy as np

PATHS = ("mutual_erase", "one_sided_kept", "resort_grew", "adopt_parent", "adopt_sibling", "tie", "fallback", "bad_child", "weight0", "skip_id0",
         "skip_noerase", "skip_mask", "pt_erase", "pt_ref_moved", "pt_turned_bad", "pt_already_dead", "parent_was_target")


def pose_inverse(T):
    """Twc as KeyFrame::SetPose stores it: Rwc = Rcw^T, Ow = -(Rwc tcw), every sum left to right"""
    o = [0.0] * 12
    for i in range(3):
        for j in range(3):
            o[4 * i + j] = T[4 * j + i]
        o[4 * i + 3] = -((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11])
    return o


def affine_mul(A, B):
    """A o B for row-major 3x4 matrices that stand for 4x4 ones with the last row 0 0 0 1; every sum in index order"""
    C = [0.0] * 12
    for i in range(3):
        for j in range(4):
            b3 = 1.0 if j == 3 else 0.0
            C[4 * i + j] = ((A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]) + A[4 * i + 3] * b3
    return C


class State:
    """the map as the data model holds it"""

    def __init__(self, pr, points):
        nkf = pr["nkf"]
        self.nkf = nkf
        self.rank = [int(v) for v in pr["kf_rank"]] if pr.get("kf_rank") is not None else list(range(nkf))
        self.bad = [int(v) for v in pr["kf_bad"]]
        self.parent = [int(v) for v in pr["kf_parent"]]
        self.in_parent = list(self.parent)
        self.Tcw = [[float(v) for v in row] for row in np.asarray(pr["kf_Tcw"], np.float64).reshape(nkf, 12)]
        co, ck, cw = pr["conn_off"], pr["conn_kf"], pr["conn_w"]
        oo, ok, ow = pr["ord_off"], pr["ord_kf"], pr["ord_w"]
        ho, hk = pr["child_off"], pr["child_kf"]
        self.conn = [{int(ck[e]): int(cw[e]) for e in range(co[k], co[k + 1])} for k in range(nkf)]       # (a dict keeps its insertion order)
        self.ordl = [[(int(ok[e]), int(ow[e])) for e in range(oo[k], oo[k + 1])] for k in range(nkf)]
        self.child = [{int(hk[e]) for e in range(ho[k], ho[k + 1])} for k in range(nkf)]
        self.points = points
        if points:
            so, sp = pr["kf_slot_off"], pr["kf_slot_pt"]
            bo, bk, bs = pr["obs_off"], pr["obs_kf"], pr["obs_slot"]
            self.slots = [[int(sp[s]) for s in range(so[k], so[k + 1])] for k in range(nkf)]
            self.obs = [{int(bk[e]): (int(bs[e]), e) for e in range(bo[p], bo[p + 1])} for p in range(pr["npts"])]    # keyframe -> (slot, entry)
            self.erased = [0] * len(bk)
            self.pt_bad = [int(v) for v in pr["pt_bad"]]
            self.pt_nobs = [int(v) for v in pr["pt_nobs"]]
            self.pt_ref = [int(v) for v in pr["pt_ref_kf"]]


def target_status(pr, t):
    flags = 0 if pr.get("tgt_flags") is None else int(pr["tgt_flags"][t])
    if pr.get("tgt_mask") is not None and not pr["tgt_mask"][t]:
        return 3
    return 1 if flags & 1 else 2 if flags & 2 else 0


def turn(S, B, paths, tally):
    """SetBadFlag() of keyframe B on the state S; returns its Tcp"""
    rank = S.rank
    # 1. (:471-476) for every connected keyframe: EraseConnection(this)
    for k in range(S.nkf):
        if B in S.conn[k] and k not in S.conn[B]:
            paths["one_sided_kept"] += 1
    for k in list(S.conn[B].keys()):
        if B in S.conn[k]:
            paths["mutual_erase"] += 1
            del S.conn[k][B]
            before = len(S.ordl[k])
            S.ordl[k] = sorted(S.conn[k].items(), key=lambda kw: (kw[1], rank[kw[0]]), reverse=True)     # UpdateBestCovisibles
            if len(S.ordl[k]) > before:
                paths["resort_grew"] += 1
    # 2. (:478-480) every map point: EraseObservation(this)
    if S.points:
        for p in S.slots[B]:
            if p < 0:
                continue
            if B not in S.obs[p]:
                paths["pt_already_dead"] += 1
                continue
            paths["pt_erase"] += 1
            S.erased[S.obs[p].pop(B)[1]] = 1
            S.pt_nobs[p] -= 1
            if S.pt_ref[p] == B and S.obs[p]:
                S.pt_ref[p] = next(iter(S.obs[p]))
                paths["pt_ref_moved"] += 1
            if S.pt_nobs[p] <= 2:
                paths["pt_turned_bad"] += 1
                S.pt_bad[p] = 1
                for k, (s, e) in S.obs[p].items():
                    S.slots[k][s] = -1
                    S.erased[e] = 1
                S.obs[p] = {}
    # 3. (:486-487)
    S.conn[B] = {}
    S.ordl[B] = []
    # 4. (:490-544) the spanning tree
    P = S.parent[B]
    if P != S.in_parent[B]:
        paths["parent_was_target"] += 1
    cands = {P}
    while S.child[B]:
        best, found = -1, None
        for c in sorted(S.child[B], key=lambda q: rank[q]):
            if S.bad[c]:
                continue
            for (e, _) in S.ordl[c]:
                if e in cands:
                    w = S.conn[c].get(e, 0)
                    if w > best:
                        best, found = w, (c, e, e not in S.conn[c])
                    elif w == best:
                        paths["tie"] += 1
        if found is None:
            break
        c, e, absent = found
        if absent:
            paths["weight0"] += 1
        paths["adopt_parent" if e == P else "adopt_sibling"] += 1
        S.parent[c] = e
        S.child[e].add(c)
        S.child[B].remove(c)
        cands.add(c)
        tally["adopted"] += 1
    for c in S.child[B]:
        paths["fallback"] += 1
        if S.bad[c]:
            paths["bad_child"] += 1
        S.parent[c] = P
        S.child[P].add(c)
        tally["fallback"] += 1
    # 5. (:544-552)
    S.child[P].discard(B)
    Tcp = affine_mul(S.Tcw[B], pose_inverse(S.Tcw[P]))
    S.bad[B] = 1
    return Tcp


def _i32(x):
    return np.array(x, np.int32).reshape(-1)


def _csr(rows):
    return _i32(np.concatenate([[0], np.cumsum([len(r) for r in rows])])), _i32([v for r in rows for v in r])


def flatten(S, status, Tcp, tally):
    o = dict(tgt_status=_i32(status), tgt_Tcp=np.array(Tcp, np.float64).reshape(-1, 12), kf_bad=np.array(S.bad, np.uint8), kf_parent=_i32(S.parent))
    o["oconn_off"], o["oconn_kf"] = _csr([list(c.keys()) for c in S.conn])
    o["oconn_w"] = _csr([list(c.values()) for c in S.conn])[1]
    o["oord_off"], o["oord_kf"] = _csr([[k for k, _ in r] for r in S.ordl])
    o["oord_w"] = _csr([[w for _, w in r] for r in S.ordl])[1]
    o["ochild_off"], o["ochild_kf"] = _csr([sorted(c, key=lambda q: S.rank[q]) for c in S.child])
    o["counts"] = _i32([sum(1 for s in status if s == 0), len(o["oconn_kf"]), len(o["oord_kf"]), len(o["ochild_kf"]), tally["adopted"], tally["fallback"]])
    if S.points:
        o.update(kf_slot_pt=_i32([p for r in S.slots for p in r]), pt_bad=np.array(S.pt_bad, np.uint8), pt_nobs=_i32(S.pt_nobs), pt_ref_kf=_i32(S.pt_ref),
                 obs_erased=np.array(S.erased, np.uint8))
    return o


def set_bad_keyframes(pr, points=True):
    S = State(pr, points)
    paths, tally = Counter(), Counter()
    status, Tcp = [], []
    for t, B in enumerate(int(v) for v in pr["tgt_kf"]):
        st = target_status(pr, t)
        status.append(st)
        if st:
            paths[{1: "skip_id0", 2: "skip_noerase", 3: "skip_mask"}[st]] += 1
            Tcp.append([0.0] * 12)
            continue
        Tcp.append(turn(S, B, paths, tally))
    o = flatten(S, status, Tcp, tally)
    o["paths"] = paths
    return o


def order_blind(pr, points=True):
    """What an implementation gives that evaluates every target against the INPUT tables: each turn runs on a fresh copy of the input
    state, and what it changed overwrites the merged state (a later target over an earlier one)."""
    S0 = State(pr, points)
    M = copy.deepcopy(S0)
    fields = ["bad", "parent", "conn", "ordl", "child"] + (["slots", "obs", "erased", "pt_bad", "pt_nobs", "pt_ref"] if points else [])
    tally = Counter()
    status, Tcp = [], []
    for t, B in enumerate(int(v) for v in pr["tgt_kf"]):
        st = target_status(pr, t)
        status.append(st)
        if st:
            Tcp.append([0.0] * 12)
            continue
        S = copy.deepcopy(S0)
        Tcp.append(turn(S, B, Counter(), tally))
        for f in fields:
            a, b, m = getattr(S0, f), getattr(S, f), getattr(M, f)
            for i in range(len(a)):
                if a[i] != b[i]:
                    m[i] = b[i]
    return flatten(M, status, Tcp, tally)
