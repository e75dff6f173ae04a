"""Restatement of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:398-488) over the map tables of orbl_fuse_targets, orbl_fuse_rows,
orbl_fuse_candidates, orbl_update_map_points_on_tables and localmapping.search_in_neighbors_on_tables, written as the literal sequential
function over dicts, sets and lists: the target loop, ORBmatcher::Fuse as dropin_checker.fuse_keyframe writes it - with MapPoint::Replace
recomputing the survivor's descriptor IN the loop -, the candidate loop, the final update and UpdateConnections.  No closed form of the
kernels is used: the search goes through the grid of npmatch.Grid, the edits through dicts.  TEST INFRASTRUCTURE.

A map is a dict of flat numpy arrays named as in include/orbslam_hip.h: kf_bad, kf_rank, kf_Tcw [nkf, 12], kf_center [nkf, 3], kf_K4 and
kf_bounds [nkf, 4] float32, kf_slot_off, kf_slot_pt, kf_slot_uv [nslots, 2], kf_slot_level, kf_slot_desc [nslots, 32], X, pt_normal,
pt_min_dist, pt_max_dist, pt_desc, pt_bad, pt_nobs, pt_found, pt_visible, pt_replaced, pt_ref_kf, obs_off / obs_kf / obs_slot (each list
in ascending kf_rank), ord_off / ord_kf, conn_off / conn_kf / conn_w, kf_fuse_target, pt_fuse_cand, scale_factors, inv_level_sigma2.

Every function counts the paths it takes in a Counter."""
import ctypes
import math
from collections import Counter

import numpy as np

from tests import npconnections, npmappoint
from tests.npmatch import Grid

F32 = np.float32
TH_LOW = 50
NOP, FUSE = 0, 4
ST_OFFSETS, ST_KF, ST_PT, ST_LEVEL, ST_CAP, ST_SLOT = 1, 2, 4, 8, 16, 32
DESC, NORMAL_DEPTH = 1, 2
_libm = ctypes.CDLL("libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]
LOG_SCALE = F32(_libm.logf(F32(1.2)))
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)

PATHS = ("tgt_bad", "tgt_stamped", "tgt_second_bad", "tgt_second_stamped", "tgt_second_is_cur", "tgt_listed_twice", "tgt_cut_first", "tgt_cut_second",
         "null", "skip_bad", "skip_in_keyframe", "neg_depth", "out_of_image", "too_near", "too_far", "viewing", "level_clamp_low", "level_clamp_high", "no_cell_range",
         "no_candidate", "level_window", "chi2", "tie_first_wins", "over_th_low", "add", "q_bad", "replace_p", "replace_q", "kp_outside_grid",
         "cand_null", "cand_bad", "cand_stamped", "cand_again", "stale_differs", "inherited_skip", "cur_point_bad_skip", "cur_slot_changed")


def log_ratio(max_dist, dist):
    """logf(max / dist) / log_scale_factor on floats: what PredictScale takes the ceiling of"""
    return F32(F32(_libm.logf(F32(F32(max_dist) / F32(dist)))) / LOG_SCALE)


class Map:
    """the map as the data model holds it: per point an observations_ dict keyframe -> slot, per keyframe its map_points_ list"""

    def __init__(self, tab):
        g = {k: np.array(v) for k, v in tab.items() if v is not None}         # (an entry's map holds the tables that entry reads)
        self.nkf = len(g["kf_slot_off" if "kf_slot_off" in g else "ord_off"]) - 1
        self.npts = len(g["pt_bad"]) if "pt_bad" in g else 0
        self.rank = [int(r) for r in g["kf_rank"]] if "kf_rank" in g else list(range(self.nkf))
        self.kf_bad = [int(v) for v in g["kf_bad"]] if "kf_bad" in g else [0] * self.nkf
        ints = lambda k: [int(v) for v in g[k]] if k in g else None                 # noqa: E731
        if "kf_Tcw" in g:
            self.Tcw = g["kf_Tcw"].astype(np.float64).reshape(-1, 12); self.center = g["kf_center"].astype(np.float64).reshape(-1, 3)
            self.K4 = g["kf_K4"].astype(F32).reshape(-1, 4); self.bounds = g["kf_bounds"].astype(F32).reshape(-1, 4)
        elif "kf_center" in g:
            self.center = g["kf_center"].astype(np.float64).reshape(-1, 3)
        self.mp, self.uv, self.level, self.kdesc = [], [], [], []
        if "kf_slot_off" in g:
            self.slot_off = ints("kf_slot_off")
            ns_ = self.slot_off[-1]
            uv = g["kf_slot_uv"].astype(F32).reshape(-1, 2) if "kf_slot_uv" in g else np.zeros((ns_, 2), F32)
            lvl = g["kf_slot_level"].astype(np.int64).reshape(-1) if "kf_slot_level" in g else np.zeros(ns_, np.int64)
            sd = g["kf_slot_desc"].astype(np.uint8).reshape(-1, 32) if "kf_slot_desc" in g else np.zeros((ns_, 32), np.uint8)
            pt = g["kf_slot_pt"] if "kf_slot_pt" in g else np.full(ns_, -1, np.int32)
            for k in range(self.nkf):
                lo, hi = self.slot_off[k], self.slot_off[k + 1]
                self.mp.append([int(v) for v in pt[lo:hi]]); self.uv.append(uv[lo:hi]); self.level.append(lvl[lo:hi]); self.kdesc.append(sd[lo:hi])
        self._grid = {}
        n = self.npts
        self.X = g["X"].astype(np.float64).reshape(-1, 3) if "X" in g else None
        self.normal = g["pt_normal"].astype(np.float64).reshape(-1, 3).copy() if "pt_normal" in g else np.zeros((n, 3))
        self.min_dist = g["pt_min_dist"].astype(F32).copy() if "pt_min_dist" in g else np.zeros(n, F32)
        self.max_dist = g["pt_max_dist"].astype(F32).copy() if "pt_max_dist" in g else np.zeros(n, F32)
        self.desc = g["pt_desc"].astype(np.uint8).reshape(-1, 32).copy() if "pt_desc" in g else np.zeros((n, 32), np.uint8)
        self.bad = ints("pt_bad") or []
        self.nobs = ints("pt_nobs") or [0] * n
        self.found, self.visible, self.replaced, self.ref_kf = ints("pt_found"), ints("pt_visible"), ints("pt_replaced"), ints("pt_ref_kf")
        self.obs = [{} for _ in range(n)]
        if "obs_off" in g:
            self.obs = [{int(g["obs_kf"][e]): int(g["obs_slot"][e]) for e in range(int(g["obs_off"][p]), int(g["obs_off"][p + 1]))} for p in range(n)]
        self.ord = None
        if "ord_off" in g:
            self.ord = [[int(v) for v in g["ord_kf"][int(g["ord_off"][k]):int(g["ord_off"][k + 1])]] for k in range(self.nkf)]
        self.fuse_target, self.fuse_cand = ints("kf_fuse_target"), ints("pt_fuse_cand")
        if "scale_factors" in g:
            self.sf = g["scale_factors"].astype(F32); self.n_levels = len(self.sf)
        if "inv_level_sigma2" in g:
            self.inv_sigma2 = g["inv_level_sigma2"].astype(F32)
        self.paths = Counter()
        self.desc0 = self.desc.copy()                                        # the descriptors at entry: what a stale search would use
        self.inherited = set()                                               # (p, keyframe): observations p took over through Replace(q, p)
        self.touched = set()

    # ---- KeyFrame
    def grid(self, k):
        if k not in self._grid:
            kps = np.zeros((len(self.uv[k]), 4), F32)
            kps[:, :2] = self.uv[k]; kps[:, 2] = self.level[k]
            self._grid[k] = Grid(kps, self.bounds[k])
            inside = sum(len(c) for col in self._grid[k].cells for c in col)
            self.paths["kp_outside_grid"] += len(kps) - inside
        return self._grid[k]

    def in_image(self, k, u, v):                                             # KeyFrame::IsInImage (src/KeyFrame.cc:624)
        b = self.bounds[k]
        return u >= b[0] and u < b[1] and v >= b[2] and v < b[3]

    # ---- MapPoint
    def sorted_obs(self, p):                                                 # std::map<KeyFrame*, size_t>: pointer order = kf_rank
        return sorted(self.obs[p].items(), key=lambda ks: self.rank[ks[0]])

    def predict_scale(self, p, dist):                                        # (src/MapPoint.cc:390-420), the project's one form
        ns = int(math.ceil(float(log_ratio(self.max_dist[p], dist))))
        if ns < 0:
            self.paths["level_clamp_low"] += 1
            return 0
        if ns >= self.n_levels:
            self.paths["level_clamp_high"] += 1
            return self.n_levels - 1
        return ns

    def add_observation(self, p, k, s):                                      # (:133-138)
        if k in self.obs[p]:
            return
        self.obs[p][k] = s
        self.nobs[p] += 1

    def compute_distinctive_descriptors(self, p):                            # (:256-315)
        if self.bad[p] or not self.obs[p]:
            return
        lst = self.sorted_obs(p)
        e = npmappoint.distinctive_descriptor(np.array([self.kdesc[k][s] for k, s in lst]), [not self.kf_bad[k] for k, _ in lst])
        if e >= 0:
            self.desc[p] = self.kdesc[lst[e][0]][lst[e][1]]

    def update_normal_and_depth(self, p):                                    # (:335-378)
        if self.bad[p] or not self.obs[p]:
            return
        lst = self.sorted_obs(p)
        ref = self.ref_kf[p]
        lvl = npmappoint.reference_level([k for k, _ in lst], [s for _, s in lst], ref, lambda k, i: int(self.level[k][i]))
        n, mn, mx = npmappoint.normal_and_depth(self.X[p], np.array([self.center[k] for k, _ in lst]), self.center[ref], lvl, self.sf)
        self.normal[p] = n; self.min_dist[p] = mn; self.max_dist[p] = mx

    def replace(self, a, b):                                                 # (:199-233)
        if a == b:
            return
        taken = self.sorted_obs(a)
        self.obs[a] = {}
        self.bad[a] = 1
        if self.replaced is not None:
            self.replaced[a] = b
        for k, s in taken:
            if k not in self.obs[b]:
                self.mp[k][s] = b
                self.add_observation(b, k, s)
                self.inherited.add((b, k))
            else:
                self.mp[k][s] = -1
        if self.found is not None:
            self.found[b] += self.found[a]; self.visible[b] += self.visible[a]
        self.compute_distinctive_descriptors(b)                              # (:230) IN the loop
        self.touched.add(b)

    # ---- the projection and its gates (src/ORBmatcher.cc:746-777), as dropin_checker._project_gates
    def project(self, K, p):
        P = self.paths
        T = [float(v) for v in self.Tcw[K]]
        X = [float(v) for v in self.X[p]]
        c = [((T[4 * i] * X[0] + T[4 * i + 1] * X[1]) + T[4 * i + 2] * X[2]) + T[4 * i + 3] for i in range(3)]
        if c[2] < 0.0:
            P["neg_depth"] += 1
            return None
        with np.errstate(all="ignore"):
            invz = F32(1.0 / c[2]) if c[2] != 0.0 else F32(np.inf)
            x, y = F32(c[0] * float(invz)), F32(c[1] * float(invz))
            fx, fy, cx, cy = [F32(v) for v in self.K4[K]]
            u, v = F32(F32(fx * x) + cx), F32(F32(fy * y) + cy)
        if not self.in_image(K, u, v):
            P["out_of_image"] += 1
            return None
        Ow = [float(v) for v in self.center[K]]
        PO = [X[0] - Ow[0], X[1] - Ow[1], X[2] - Ow[2]]
        dist = F32(math.sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]))
        if dist < F32(F32(0.8) * self.min_dist[p]):
            P["too_near"] += 1
            return None
        if dist > F32(F32(1.2) * self.max_dist[p]):
            P["too_far"] += 1
            return None
        Pn = [float(v) for v in self.normal[p]]
        if (PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2] < 0.5 * float(dist):
            P["viewing"] += 1
            return None
        return u, v, self.predict_scale(p, dist)

    def best_keypoint(self, K, u, v, lvl, d, th, count=True):
        """the search loop of Fuse (:779-806) for descriptor d: (best index or -1, best distance or 256)"""
        P = self.paths if count else Counter()
        g = self.grid(K)
        r = F32(F32(th) * self.sf[lvl])
        cand = g.features_in_area(u, v, r)
        if not cand:
            if count:
                x0, x1 = F32(F32(F32(u - g.min_x) - r) * g.winv), F32(F32(F32(u - g.min_x) + r) * g.winv)
                P["no_cell_range" if (math.floor(float(x0)) >= 64 or math.ceil(float(x1)) < 0) else "no_candidate"] += 1
            return -1, 256
        best, bi, ties = 256, -1, 0
        for idx in cand:
            o = int(self.level[K][idx])
            if o < lvl - 1 or o > lvl:
                P["level_window"] += 1
                continue
            ex, ey = F32(u - self.uv[K][idx, 0]), F32(v - self.uv[K][idx, 1])
            e2 = F32(F32(ex * ex) + F32(ey * ey))
            if float(F32(e2 * self.inv_sigma2[o])) > 5.99:
                P["chi2"] += 1
                continue
            dd = int(_POP[np.bitwise_xor(self.kdesc[K][idx], d)].sum())
            if dd < best:
                best, bi, ties = dd, idx, 0
            elif dd == best and idx < bi:
                ties += 1                                                    # an index-order tie-break would have chosen otherwise
        if ties:
            P["tie_first_wins"] += 1
        return bi, best

    def search(self, K, p, th):
        """-> (best_idx, best_dist, u, v, level); level -1 and no best when a gate failed"""
        pr = self.project(K, p)
        if pr is None:
            return -1, 256, F32(0), F32(0), -1
        u, v, lvl = pr
        bi, bd = self.best_keypoint(K, u, v, lvl, self.desc[p], th)
        return bi, bd, u, v, lvl

    # ---- ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:724-842), sequential, with the map mutations
    def fuse(self, K, points, th=3.0, cur_row=None):
        P = self.paths
        fused = 0
        for p in points:
            if p < 0:
                P["null"] += 1
                continue
            if self.bad[p]:
                P["skip_bad"] += 1
                if cur_row is not None and p in cur_row:
                    P["cur_point_bad_skip"] += 1
                continue
            if K in self.obs[p]:
                P["skip_in_keyframe"] += 1
                if (p, K) in self.inherited:
                    P["inherited_skip"] += 1
                continue
            bi, bd, u, v, lvl = self.search(K, p, th)
            if lvl >= 0 and not np.array_equal(self.desc[p], self.desc0[p]):
                si, sd = self.best_keypoint(K, u, v, lvl, self.desc0[p], th, count=False)
                if (si if sd <= TH_LOW else -1) != (bi if bd <= TH_LOW else -1):
                    P["stale_differs"] += 1
            if bi < 0:
                continue
            if bd > TH_LOW:
                P["over_th_low"] += 1
                continue
            q = self.mp[K][bi]
            if q >= 0:
                if not self.bad[q]:
                    if self.nobs[q] > self.nobs[p]:
                        self.replace(p, q); P["replace_p"] += 1
                    else:
                        self.replace(q, p); P["replace_q"] += 1
                else:
                    P["q_bad"] += 1
            else:
                self.add_observation(p, K, bi); self.mp[K][bi] = p
                P["add"] += 1
            fused += 1
        return fused

    # ---- the tables again
    def tables(self):
        off, okf, oslot = [0], [], []
        for p in range(self.npts):
            for k, s in self.sorted_obs(p):
                okf.append(k); oslot.append(s)
            off.append(len(okf))
        r = dict(kf_slot_pt=np.array([v for m in self.mp for v in m], np.int32), pt_bad=np.array(self.bad, np.uint8), pt_nobs=np.array(self.nobs, np.int32),
                 pt_desc=self.desc.copy(), pt_normal=self.normal.copy(), pt_min_dist=self.min_dist.copy(), pt_max_dist=self.max_dist.copy(),
                 obs_off=np.array(off, np.int32), obs_kf=np.array(okf, np.int32), obs_slot=np.array(oslot, np.int32))
        for k, v in (("pt_found", self.found), ("pt_visible", self.visible), ("pt_replaced", self.replaced), ("kf_fuse_target", self.fuse_target),
                     ("pt_fuse_cand", self.fuse_cand)):
            r[k] = None if v is None else np.array(v, np.int32)
        return r


# ------------------------------------------------------------------------------------------------------------------ the four entries
def fuse_targets(tab, cur_kf, cur_id, nn=20, nn2=5, cap=None, M=None):
    """(:400-431) -> dict(tgt_kf, counts = {n_tgt, n_first}, kf_fuse_target, status, paths)"""
    M = Map(tab) if M is None else M
    P = M.paths
    out, n_first = [], 0
    if len(M.ord[cur_kf]) > nn:
        P["tgt_cut_first"] += 1
    for n in M.ord[cur_kf][:nn]:                                             # GetBestCovisibilityKeyFrames(nn)
        if M.kf_bad[n] or M.fuse_target[n] == cur_id:
            P["tgt_bad" if M.kf_bad[n] else "tgt_stamped"] += 1
            continue
        out.append(n)
        M.fuse_target[n] = cur_id
        n_first += 1
        if len(M.ord[n]) > nn2:
            P["tgt_cut_second"] += 1
        for k2 in M.ord[n][:nn2]:
            if M.kf_bad[k2] or M.fuse_target[k2] == cur_id or k2 == cur_kf:
                P["tgt_second_bad" if M.kf_bad[k2] else "tgt_second_stamped" if M.fuse_target[k2] == cur_id else "tgt_second_is_cur"] += 1
                continue
            out.append(k2)
    P["tgt_listed_twice"] += len(out) - len(set(out))
    status = ST_CAP if cap is not None and len(out) > cap else 0
    return dict(tgt_kf=np.array(out, np.int32), counts=np.array([len(out), n_first], np.int32), kf_fuse_target=np.array(M.fuse_target, np.int32), status=status,
                paths=P)


def fuse_rows(tab, K, pts, th=3.0, M=None):
    """the search of Fuse for keyframe K over pts, nothing mutated -> the rows and the nullable outputs of orbl_fuse_rows"""
    M = Map(tab) if M is None else M
    n = len(pts)
    o = dict(op_kind=np.zeros(n, np.int32), op_pt=np.full(n, -1, np.int32), op_arg=np.zeros(n, np.int32), op_kf=np.full(n, K, np.int32),
             op_slot=np.full(n, -1, np.int32), best_idx=np.full(n, -1, np.int32), best_dist=np.full(n, 256, np.int32), q_uv=np.zeros((n, 2), F32),
             q_level=np.full(n, -1, np.int32), status=0, paths=M.paths)
    for i, p in enumerate(int(v) for v in pts):
        if not 0 <= p < M.npts:
            if p != -1:
                o["status"] |= ST_PT
            M.paths["null"] += 1
            continue
        o["op_pt"][i] = p
        bi, bd, u, v, lvl = M.search(K, p, th)
        o["best_idx"][i], o["best_dist"][i], o["q_level"][i] = bi, bd, lvl
        if lvl >= 0:
            o["q_uv"][i] = (u, v)
        if bi >= 0 and bd > TH_LOW:
            M.paths["over_th_low"] += 1
        if bd <= TH_LOW:
            o["op_kind"][i], o["op_slot"][i] = FUSE, bi
    return o


def fuse_candidates(tab, tgt_kf, cur_id, cap=None, M=None):
    """(:445-470) -> dict(cand_pt, counts = {n_cand, n_tgt}, pt_fuse_cand, status, paths); with a capacity the points beyond it stay unstamped"""
    M = Map(tab) if M is None else M
    P = M.paths
    out = []
    seen_here = set()
    for k in (int(v) for v in tgt_kf):
        for p in M.mp[k]:
            if p < 0:
                P["cand_null"] += 1
                continue
            if M.bad[p] or M.fuse_cand[p] == cur_id:
                P["cand_bad" if M.bad[p] else "cand_again" if p in seen_here else "cand_stamped"] += 1
                continue
            M.fuse_cand[p] = cur_id
            seen_here.add(p)
            out.append(p)
    status = 0
    if cap is not None and len(out) > cap:
        status = ST_CAP
        for p in out[cap:]:
            M.fuse_cand[p] = int(np.asarray(tab["pt_fuse_cand"])[p])
    return dict(cand_pt=np.array(out, np.int32), counts=np.array([len(out), len(tgt_kf)], np.int32), pt_fuse_cand=np.array(M.fuse_cand, np.int32), status=status, paths=P)


def update_map_points_on_tables(tab, what, pt_mask=None, mask_kf=-1, M=None):
    """(:474-485 and the in-loop ComputeDistinctiveDescriptors) for the selected points -> dict(pt_desc, pt_normal, pt_min_dist, pt_max_dist)"""
    M = Map(tab) if M is None else M
    sel = set() if pt_mask is None else set(int(p) for p in np.nonzero(np.asarray(pt_mask))[0])
    if mask_kf >= 0:
        sel |= set(p for p in M.mp[mask_kf] if p >= 0)
    for p in sorted(sel):
        if M.bad[p]:
            continue
        if what & DESC:
            M.compute_distinctive_descriptors(p)
        if what & NORMAL_DEPTH:
            M.update_normal_and_depth(p)
    return dict(pt_desc=M.desc.copy(), pt_normal=M.normal.copy(), pt_min_dist=M.min_dist.copy(), pt_max_dist=M.max_dist.copy())


# ------------------------------------------------------------------------------------------------------------------ the whole function
def search_in_neighbors(tab, cur_kf, cur_id, nn=20, nn2=5, th=3.0, conn_th=15):
    """-> dict(tab = every table the function changes, tgt_kf, cand_pt, n_fused = one per Fuse call, connections = what
    npconnections.connections returns for the one keyframe, paths)"""
    M = Map(tab)
    P = M.paths
    tg = fuse_targets(tab, cur_kf, cur_id, nn, nn2, M=M)
    targets = [int(k) for k in tg["tgt_kf"]]
    matches = list(M.mp[cur_kf])                                             # (:435) a snapshot
    row = set(p for p in matches if p >= 0)
    n_fused = [M.fuse(k, matches, th, cur_row=row) for k in targets]         # (:436-442)
    cd = fuse_candidates(tab, targets, cur_id, M=M)
    n_fused.append(M.fuse(cur_kf, [int(p) for p in cd["cand_pt"]], th))       # (:472)
    P["cur_slot_changed"] += sum(1 for a, b in zip(matches, M.mp[cur_kf]) if a != b)
    for p in M.mp[cur_kf]:                                                   # (:475-484)
        if p >= 0 and not M.bad[p]:
            M.compute_distinctive_descriptors(p)
            M.update_normal_and_depth(p)
    out = M.tables()
    lo, hi = M.slot_off[cur_kf], M.slot_off[cur_kf + 1]
    conn = npconnections.connections(dict(nkf=M.nkf, npts=M.npts, th=conn_th, tgt_kf=[cur_kf], tgt_flags=None, slot_off=[0, hi - lo], slot_pt=out["kf_slot_pt"][lo:hi],
                                          obs_off=out["obs_off"], obs_kf=out["obs_kf"], pt_bad=out["pt_bad"], kf_rank=tab.get("kf_rank"), conn_off=tab["conn_off"],
                                          conn_kf=tab["conn_kf"], conn_w=tab["conn_w"], prev_off=None, prev_kf=None))
    return dict(tab=out, tgt_kf=targets, cand_pt=cd["cand_pt"], n_fused=n_fused, connections=conn, paths=P)
