"""Literal-loop numpy restatement of the front of LoopClosing::ComputeSim3 (src/LoopClosing.cc:250-277) on the flat map tables that
orbl_loop_sim3_candidates takes: per candidate SearchByBoW(current keyframe, candidate) - tests/npmatch.search_by_bow, the restatement
of src/ORBmatcher.cc:470-580 -, the `nmatches < 20` gate and the loop of Sim3Solver's constructor (src/Sim3Solver.cc:73-109) written
out as the reference has it.  Test infrastructure only; plain loops, the float arithmetic made explicit."""
import numpy as np

from tests import npmatch as NP

F32 = np.float32
SKIP_NO_MATCH, SKIP_NO_POINT1, SKIP_BAD_POINT, SKIP_NO_INDEX = "no match", "no point in slot i1", "a bad point", "GetIndexInKeyFrame < 0"


def slots(tab, k):
    return int(tab["kf_slot_off"][k]), int(tab["kf_slot_off"][k + 1])


def feature_vector(tab, k):
    """keyframe k's feature_vector_ as npmatch takes it: (node ids, offsets from 0, keypoint indices)"""
    a, b = int(tab["kf_fv_off"][k]), int(tab["kf_fv_off"][k + 1])
    off = np.asarray(tab["fv_ent_off"][a:b + 1], np.int64)
    base = int(off[0]) if b > a else 0
    return (np.asarray(tab["fv_node"][a:b], np.uint32), (off - base).astype(np.uint32) if b > a else np.zeros(1, np.uint32),
            np.asarray(tab["fv_ent"][base:int(off[-1])] if b > a else [], np.uint32))


def search_inputs(tab, k):
    """descriptors, the "holds a point that is not bad" mask and the angles of keyframe k's slots"""
    lo, hi = slots(tab, k)
    pt = np.asarray(tab["kf_slot_pt"][lo:hi])
    valid = np.array([p >= 0 and not tab["pt_bad"][p] for p in pt], np.uint8)
    return np.asarray(tab["kf_slot_desc"], np.uint8).reshape(-1, 32)[lo:hi], valid, np.asarray(tab["kf_slot_angle"][lo:hi], np.float32)


def search_by_bow(tab, k1, k2, nnratio, check_ori):
    d1, v1, a1 = search_inputs(tab, k1)
    d2, v2, a2 = search_inputs(tab, k2)
    return NP.search_by_bow(d1, v1, a1, d2, v2, a2, feature_vector(tab, k1), feature_vector(tab, k2), nnratio, True, check_ori)


def index_in_keyframe(tab, p, k):
    """MapPoint::GetIndexInKeyFrame on the observation tables: the first entry of the point's list that names the keyframe"""
    for e in range(int(tab["obs_off"][p]), int(tab["obs_off"][p + 1])):
        if tab["obs_kf"][e] == k:
            return int(tab["obs_slot"][e])
    return -1


def max_error(sigma2):
    """max_errors_ (src/Sim3Solver.cc:93-94): 9.210 * (float) as a double, stored in a vector<size_t>, compared as a float"""
    return F32(int(9.210 * float(F32(sigma2))))


def to_camera(T12, X):
    """Rcw X + tcw as Sim3SolverT::push_camera sums it: ((R(i,0) x + R(i,1) y) + R(i,2) z) + t(i), doubles"""
    T = np.asarray(T12, np.float64).reshape(3, 4)
    return [((T[i, 0] * X[0] + T[i, 1] * X[1]) + T[i, 2] * X[2]) + T[i, 3] for i in range(3)]


def constructor_rows(tab, k1, k2, match12, skipped=None):
    """The loop of src/Sim3Solver.cc:73-109 over match12 (slot of keyframe k2 per slot of k1, -1 = nullptr).  Returns the rows as a list
    of dicts; skipped: an optional dict that counts the rows left out, by reason."""
    lo1, _ = slots(tab, k1)
    lo2, _ = slots(tab, k2)
    X = np.asarray(tab["X"], np.float64).reshape(-1, 3)
    T = np.asarray(tab["kf_Tcw"], np.float64).reshape(-1, 12)

    def skip(why):
        if skipped is not None:
            skipped[why] = skipped.get(why, 0) + 1
    rows = []
    for i1 in range(len(match12)):
        if match12[i1] < 0:                                     # if (matched_points_1_in_2[i1])
            skip(SKIP_NO_MATCH)
            continue
        p1 = int(tab["kf_slot_pt"][lo1 + i1])
        p2 = int(tab["kf_slot_pt"][lo2 + int(match12[i1])])      # (the pointer SearchByBoW stored: the point in the candidate's slot)
        if p1 < 0:                                              # if (!map_point_1) continue
            skip(SKIP_NO_POINT1)
            continue
        if tab["pt_bad"][p1] or tab["pt_bad"][p2]:
            skip(SKIP_BAD_POINT)
            continue
        x1, x2 = index_in_keyframe(tab, p1, k1), index_in_keyframe(tab, p2, k2)
        if x1 < 0 or x2 < 0:
            skip(SKIP_NO_INDEX)
            continue
        o1, o2 = int(tab["kf_slot_level"][lo1 + x1]), int(tab["kf_slot_level"][lo2 + x2])       # kp.octave at THAT index
        rows.append(dict(i1=i1, pt1=p1, pt2=p2, x1=x1, x2=x2, max_err1=max_error(tab["level_sigma2"][o1]), max_err2=max_error(tab["level_sigma2"][o2]),
                         X1c=to_camera(T[k1], X[p1]), X2c=to_camera(T[k2], X[p2])))
    return rows


def sim3_candidates(tab, cur_kf, cand_kf, nnratio=0.75, check_ori=True, min_matches=20, cap1=None, skipped=None):
    """src/LoopClosing.cc:250-277 for every candidate; the outputs of loopclosing.sim3_candidates, as it lays them out."""
    lo1, hi1 = slots(tab, cur_kf)
    n1, nc = hi1 - lo1, len(cand_kf)
    cap1 = n1 if cap1 is None else cap1
    K4 = np.asarray(tab["kf_K4"], np.float32).reshape(-1, 4)
    o = dict(match12=np.full((nc, cap1), -1, np.int32), nmatches=np.zeros(nc, np.int32), cand_status=np.zeros(nc, np.int32), K1=np.zeros((nc, 4), np.float32),
             K2=np.zeros((nc, 4), np.float32), off=np.zeros(nc + 1, np.int32))
    rows = []
    for c, k2 in enumerate(int(k) for k in cand_kf):
        o["K1"][c] = K4[cur_kf]
        o["off"][c] = len(rows)
        if tab.get("kf_bad") is not None and tab["kf_bad"][k2]:   # (:257-260)
            o["cand_status"][c] = 1
            continue
        o["K2"][c] = K4[k2]
        nm, m12 = search_by_bow(tab, cur_kf, k2, nnratio, check_ori)
        o["match12"][c, :n1] = m12
        o["nmatches"][c] = nm
        if nm < min_matches:                                    # (:265)
            o["cand_status"][c] = 2
            continue
        rows += constructor_rows(tab, cur_kf, k2, m12, skipped)
    o["off"][nc] = len(rows)
    o["counts"] = np.array([len(rows), int((o["cand_status"] == 0).sum())], np.int32)
    o["X1c"] = np.array([r["X1c"] for r in rows], np.float64).reshape(-1, 3)
    o["X2c"] = np.array([r["X2c"] for r in rows], np.float64).reshape(-1, 3)
    for k, dt in (("max_err1", np.float32), ("max_err2", np.float32)):
        o[k] = np.array([r[k] for r in rows], dt)
    for k, key in (("row_i1", "i1"), ("row_pt1", "pt1"), ("row_pt2", "pt2")):
        o[k] = np.array([r[key] for r in rows], np.int32)
    o["_rows"] = rows
    return o


# ------------------------------------------------------------------------------------------------ which paths a search takes
def search_paths(tab, k1, k2, nnratio, check_ori):
    """The walk of src/ORBmatcher.cc:498-576 once more, counting what a case is there to exercise.  Returns (match12, counts); the caller
    holds match12 against search_by_bow, so the counts describe the search that was checked.  counts: one_sided_nodes (a node one
    keyframe has and the other lacks), tied_best (an entry whose smallest distance two free candidates share: list order decides),
    tied_runner_up (the best equals the runner-up and is below TH_LOW: the ratio test fails on the tie), rotation_rejected, blocked
    (an entry that decided differently because a candidate was taken by a match the rotation check cleared later)."""
    d1, v1, a1 = search_inputs(tab, k1)
    d2, v2, a2 = search_inputs(tab, k2)
    n1, i1, e1 = feature_vector(tab, k1)
    n2, i2, e2 = feature_vector(tab, k2)
    L1 = {int(n1[m]): [int(x) for x in e1[i1[m]:i1[m + 1]]] for m in range(len(n1))}
    L2 = {int(n2[m]): [int(x) for x in e2[i2[m]:i2[m + 1]]] for m in range(len(n2))}
    cnt = dict(one_sided_nodes=len(set(L1) ^ set(L2)), tied_best=0, tied_runner_up=0, rotation_rejected=0, blocked=0)

    def decide(idx1, lst, taken):
        best1, bidx, best2, nbest = 256, -1, 256, 0
        for idx2 in lst:
            if taken[idx2] or not v2[idx2]:
                continue
            dist = NP.descriptor_distance(d1[idx1], d2[idx2])
            if dist < best1:
                best2, best1, bidx, nbest = best1, dist, idx2, 1
            elif dist < best2:
                best2 = dist
                nbest += dist == best1
            elif dist == best1:
                nbest += 1
        ok = best1 < NP.TH_LOW and F32(best1) < F32(nnratio) * F32(best2)
        return ok, bidx, best1, best2, nbest

    def walk(free, count):
        """free: candidates that are treated as never taken (the cleared matches of a first walk)"""
        m12, taken, hist = [-1] * len(d1), [False] * len(d2), [[] for _ in range(NP.HISTO_LENGTH)]
        choice = {}
        for node in sorted(set(L1) & set(L2)):
            for idx1 in L1[node]:
                if not v1[idx1]:
                    continue
                seen = [t and j not in free for j, t in enumerate(taken)]
                ok, bidx, best1, best2, nbest = decide(idx1, L2[node], seen)
                choice[idx1] = (ok, bidx)
                if count:
                    cnt["tied_best"] += best1 < 256 and best1 == best2 and nbest > 1
                    cnt["tied_runner_up"] += best1 < NP.TH_LOW and best1 == best2
                if ok:
                    m12[idx1] = bidx
                    taken[bidx] = True
                    if check_ori:
                        hist[NP.rot_bin(a1[idx1], a2[bidx])].append(idx1)
        cleared = set()
        if check_ori:
            for b in NP._keep_bins(hist):
                for idx1 in hist[b]:
                    cleared.add(m12[idx1])
                    m12[idx1] = -1
        return m12, cleared, choice
    m12, cleared, actual = walk(set(), True)
    cnt["rotation_rejected"] = len(cleared)
    if cleared:
        _, _, other = walk(cleared, False)
        cnt["blocked"] = sum(actual[i] != other[i] for i in actual)
    return np.array(m12, np.int32), cnt
