"""Restatement of orbl_apply_map_edits: an ordered list of map-point edits - MapPoint::AddObservation, Replace and SetBadFlag
(src/MapPoint.cc:133-138, :199-233, :174-191, monocular) as LocalMapping, ORBmatcher::Fuse and LoopClosing call them - replayed on the map
tables, written as the literal sequential loop over dicts and lists - no closed form.  TEST INFRASTRUCTURE.

A problem is a dict of flat arrays, as the entry point takes them (include/orbslam_hip.h): nkf, npts, kf_slot_off, kf_rank, obs_off / obs_kf /
obs_slot, obs_dead, kf_slot_level / kf_slot_uv, kf_slot_pt, pt_bad, pt_nobs, pt_found / pt_visible, pt_replaced and the edits op_kind, op_pt,
op_arg, op_kf, op_slot (kf_rank, obs_dead, the kf_slot_level pair, the pt_found pair and pt_replaced may be None).

apply_map_edits(pr) returns the outputs by the entry's names, "status" (the bits the device entry raises) and "paths", a Counter of the
branches the loop took."""
from collections import Counter

import numpy as np

NOP, ADD, REPLACE, SET_BAD, FUSE, FIND_OR_ADD, REPLACE_FOUND = range(7)
ST_OFFSETS, ST_KF, ST_PT, ST_SLOT, ST_CAP = 1, 2, 4, 8, 16

PATHS = ("nop", "add_ok", "add_dup", "add_touch", "add_dup_slot_written", "replace", "replace_same", "replace_move", "replace_erase", "replace_emptied",
         "set_bad", "set_bad_fused_slot", "fuse_skip_bad", "fuse_skip_named", "fuse_q_bad", "fuse_p_replaced", "fuse_q_replaced", "fuse_tie", "fuse_add",
         "find_q_bad", "find_found", "find_add_ok", "find_add_dup", "found_none", "found_replace", "found_again", "late_add", "obs_dead")


class State:
    """the map as the data model holds it: per point an observations_ dict keyframe -> (slot, source entry), in insertion order"""

    def __init__(self, pr):
        self.nkf, self.npts = int(pr["nkf"]), int(pr["npts"])
        self.status = 0
        self.paths = Counter()
        self.slot_off = [int(v) for v in pr["kf_slot_off"]]
        self.slot_pt = [int(v) for v in pr["kf_slot_pt"]]
        bo, bk, bs, dead = pr["obs_off"], pr["obs_kf"], pr["obs_slot"], pr.get("obs_dead")
        self.nobs_in = int(bo[self.npts]) if self.npts else 0
        self.obs = []
        for p in range(self.npts):
            d = {}
            for e in range(int(bo[p]), int(bo[p + 1])):
                k, s = int(bk[e]), int(bs[e])
                if dead is not None and dead[e]:
                    self.paths["obs_dead"] += 1
                elif not 0 <= k < self.nkf:                              # (the device entry: an observation out of range is absent)
                    self.status |= ST_KF
                elif not 0 <= s < self.slot_off[k + 1] - self.slot_off[k]:
                    self.status |= ST_SLOT
                else:
                    d[k] = (s, e)
            self.obs.append(d)
        self.bad = [int(v) for v in pr["pt_bad"]]
        self.nobs = [int(v) for v in pr["pt_nobs"]]
        self.counters = pr.get("pt_found") is not None
        self.found = [int(v) for v in pr["pt_found"]] if self.counters else None
        self.visible = [int(v) for v in pr["pt_visible"]] if self.counters else None
        self.replaced = [int(v) for v in pr["pt_replaced"]] if pr.get("pt_replaced") is not None else None
        self.touched = [0] * self.npts
        self.late = [0] * self.npts
        self.written = set()                                             # the slots an op of this call wrote a point into
        self.n_added = self.n_replace = self.n_set_bad = 0

    def slot(self, K, s):
        return self.slot_off[K] + s

    def touch(self, p):                                                  # ComputeDistinctiveDescriptors, left to the caller
        self.touched[p] = 1
        self.late[p] = 0

    def add_observation(self, p, K, s, src):                             # (:133-138)
        if K in self.obs[p]:
            return False
        self.obs[p][K] = (s, src)
        self.nobs[p] += 1
        return True

    def replace(self, a, b):                                             # (:199-233)
        if a == b:
            self.paths["replace_same"] += 1
            return False
        taken = self.obs[a]
        self.obs[a] = {}
        self.bad[a] = 1
        if self.replaced is not None:
            self.replaced[a] = b
        self.paths["replace" if taken else "replace_emptied"] += 1
        for k, (s, src) in taken.items():
            if k not in self.obs[b]:                                     # !map_point->IsInKeyFrame(keyframe)
                self.slot_pt[self.slot(k, s)] = b
                self.written.add(self.slot(k, s))
                self.add_observation(b, k, s, src)
                self.paths["replace_move"] += 1
            else:
                self.slot_pt[self.slot(k, s)] = -1
                self.paths["replace_erase"] += 1
        if self.counters:                                                # a's counters stay: a second Replace adds them again
            self.found[b] += self.found[a]
            self.visible[b] += self.visible[a]
        self.touch(b)                                                    # (:230)
        self.n_replace += 1
        return True

    def set_bad(self, p):                                                # (:174-191)
        self.bad[p] = 1
        taken = self.obs[p]
        self.obs[p] = {}
        if any(self.slot(k, s) in self.written for k, (s, _) in taken.items()):
            self.paths["set_bad_fused_slot"] += 1
        for k, (s, _) in taken.items():
            self.slot_pt[self.slot(k, s)] = -1
        self.paths["set_bad"] += 1
        self.n_set_bad += 1

    def add(self, i, p, K, s, touch):                                    # AddObservation + KeyFrame::AddMapPoint
        ok = self.add_observation(p, K, s, self.nobs_in + i)
        self.slot_pt[self.slot(K, s)] = p                                # unconditionally
        self.written.add(self.slot(K, s))
        if ok:
            self.n_added += 1
            if self.touched[p]:
                self.late[p] = 1
                self.paths["late_add"] += 1
        if touch:
            self.touch(p)
        return 5 if ok else 6


def _op_absent(S, i, kind, p, arg, K, s, op_kind):
    """the bits of an op the device entry cannot run (the host entry refuses it), 0 when it is in range"""
    if not 0 <= kind <= 6:
        return ST_SLOT
    if kind == NOP:
        return 0
    bits = 0
    if not 0 <= p < S.npts:
        bits |= ST_PT
    if kind == REPLACE and not 0 <= arg < S.npts:
        bits |= ST_PT
    if kind in (ADD, FUSE, FIND_OR_ADD):
        if not 0 <= K < S.nkf:
            bits |= ST_KF
        elif not 0 <= s < S.slot_off[K + 1] - S.slot_off[K]:
            bits |= ST_SLOT
    if kind == REPLACE_FOUND and not (0 <= arg < i and int(op_kind[arg]) == FIND_OR_ADD):
        bits |= ST_SLOT
    return bits


def apply_map_edits(pr, cap_obs=None):
    S = State(pr)
    P = S.paths
    kinds, pts, args, kfs, slots = (pr[k] for k in ("op_kind", "op_pt", "op_arg", "op_kf", "op_slot"))
    nops = len(kinds)
    op_status, op_found = [0] * nops, [-1] * nops
    n_fused = 0
    for i in range(nops):
        kind, p, arg, K, s = int(kinds[i]), int(pts[i]), int(args[i]), int(kfs[i]), int(slots[i])
        bits = _op_absent(S, i, kind, p, arg, K, s, kinds)
        if bits:
            S.status |= bits
            op_status[i] = 10
            continue
        st = 0
        if kind == NOP:
            P["nop"] += 1
        elif kind == ADD:
            held = S.slot_pt[S.slot(K, s)]
            st = S.add(i, p, K, s, arg & 1)
            P["add_ok" if st == 5 else "add_dup"] += 1
            if arg & 1:
                P["add_touch"] += 1
            if st == 6 and held != p:
                P["add_dup_slot_written"] += 1
        elif kind == REPLACE:
            st = 8 if S.replace(p, arg) else 1
        elif kind == SET_BAD:
            S.set_bad(p)
            st = 9
        elif kind == FUSE:                                               # (src/ORBmatcher.cc:746, :824-838)
            if S.bad[p] or K in S.obs[p]:
                st = 1
                P["fuse_skip_bad" if S.bad[p] else "fuse_skip_named"] += 1
            else:
                q = S.slot_pt[S.slot(K, s)]
                if q >= 0:
                    if S.bad[q]:
                        st = 2
                        P["fuse_q_bad"] += 1
                    else:
                        op_found[i] = q
                        if S.nobs[q] > S.nobs[p]:
                            S.replace(p, q)
                            st = 3
                            P["fuse_p_replaced"] += 1
                        else:
                            if S.nobs[q] == S.nobs[p]:
                                P["fuse_tie"] += 1
                            S.replace(q, p)
                            st = 4
                            P["fuse_q_replaced"] += 1
                else:
                    st = S.add(i, p, K, s, 0)
                    P["fuse_add"] += 1
        elif kind == FIND_OR_ADD:                                        # (src/ORBmatcher.cc:941-950)
            q = S.slot_pt[S.slot(K, s)]
            if q >= 0:
                if S.bad[q]:
                    st = 2
                    P["find_q_bad"] += 1
                else:
                    op_found[i] = q
                    st = 7
                    P["find_found"] += 1
            else:
                st = S.add(i, p, K, s, 0)
                P["find_add_ok" if st == 5 else "find_add_dup"] += 1
        elif kind == REPLACE_FOUND:                                      # (src/LoopClosing.cc:615-621)
            a = op_found[arg]
            if a < 0:
                st = 1
                P["found_none"] += 1
            else:
                if S.bad[a]:
                    P["found_again"] += 1
                st = 8 if S.replace(a, p) else 1
                P["found_replace"] += 1
        if kind in (FUSE, FIND_OR_ADD) and st in (2, 3, 4, 5, 7):
            n_fused += 1
        op_status[i] = st
    # the whole new tables, each list in ascending kf_rank
    rank = [int(v) for v in pr["kf_rank"]] if pr.get("kf_rank") is not None else list(range(S.nkf))
    off, okf, oslot, osrc = [0], [], [], []
    for p in range(S.npts):
        for k in sorted(S.obs[p], key=lambda k: rank[k]):
            okf.append(k); oslot.append(S.obs[p][k][0]); osrc.append(S.obs[p][k][1])
        off.append(len(okf))
    n_out = len(okf)
    r = dict(op_status=np.array(op_status, np.int32), op_found=np.array(op_found, np.int32), pt_touched=np.array(S.touched, np.uint8),
             kf_slot_pt=np.array(S.slot_pt, np.int32), pt_bad=np.array(S.bad, np.uint8), pt_nobs=np.array(S.nobs, np.int32),
             pt_found=np.array(S.found, np.int32) if S.counters else None, pt_visible=np.array(S.visible, np.int32) if S.counters else None,
             pt_replaced=np.array(S.replaced, np.int32) if S.replaced is not None else None,
             oobs_off=np.array(off, np.int32), oobs_kf=np.array(okf, np.int32), oobs_slot=np.array(oslot, np.int32), oobs_src=np.array(osrc, np.int32),
             oobs_level=None, oobs_uv=None, paths=P)
    if pr.get("kf_slot_level") is not None:
        lvl, uv = np.asarray(pr["kf_slot_level"], np.int32).reshape(-1), np.asarray(pr["kf_slot_uv"], np.float32).reshape(-1, 2)
        at = [S.slot(k, s) for k, s in zip(okf, oslot)]
        r["oobs_level"] = lvl[at].astype(np.int32) if at else np.zeros(0, np.int32)
        r["oobs_uv"] = uv[at].astype(np.float32) if at else np.zeros((0, 2), np.float32)
    if cap_obs is not None and n_out > cap_obs:
        S.status |= ST_CAP
    r["counts"] = np.array([n_out, S.n_added, S.n_replace, S.n_set_bad, n_fused, sum(S.touched), sum(S.late), 0], np.int32)
    r["status"] = S.status
    return r
