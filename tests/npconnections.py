"""Restatement of KeyFrame::UpdateConnections (src/KeyFrame.cc:314-398) with AddConnection / UpdateBestCovisibles (:158-193), called
on a list of keyframes one after the other, and of the loop links LoopClosing::CorrectLoop derives on the way (src/LoopClosing.cc:551-573),
over the flattened arrays of orbl_update_connections.  The LITERAL loop with the reference's containers (a dict per keyframe for
std::map<KeyFrame*, int>, iterated and tie-broken by kf_rank as the pointer order): TEST INFRASTRUCTURE, independent of the closed form
the kernels use.

A problem is a dict: nkf, npts, th, tgt_kf[ntgt], tgt_flags[ntgt] (None: all 0; bit 0: is_first_connection_ && id_ != 0), slot_off[ntgt + 1],
slot_pt[nslots] (-1: null slot), obs_off[npts + 1], obs_kf[nobs], pt_bad (None: all good), kf_rank (None: index order), conn_off[nkf + 1],
conn_kf / conn_w[nconn], prev_off[ntgt + 1] / prev_kf (None: no links)."""
import numpy as np

PATHS = ("fallback", "max_tie", "empty", "sort_tie", "resort_below_th", "noop_add", "resorted_after_turn", "resorted_before_turn", "parent")


def connections(pr, order_blind=False):
    """-> dict(tgt_status, tgt_parent int32[ntgt], counts int32[4] = {n_aff, n_conn, n_ord, n_link}, aff_kf, conn_off / conn_kf / conn_w,
    ord_off / ord_kf / ord_w, link_off / link_kf (None without prev), paths = {name: how often}).  order_blind=True: every list is its
    keyframe's own entries >= th (no re-sort quirk) - used ONLY to show that the test problems tell the two apart."""
    nkf, th = int(pr["nkf"]), int(pr["th"])
    tgt = [int(k) for k in pr["tgt_kf"]]
    ntgt = len(tgt)
    flags = [0] * ntgt if pr.get("tgt_flags") is None else [int(f) for f in pr["tgt_flags"]]
    rank = list(range(nkf)) if pr.get("kf_rank") is None else [int(r) for r in pr["kf_rank"]]
    bad = None if pr.get("pt_bad") is None else pr["pt_bad"]
    weights = [dict((int(pr["conn_kf"][e]), int(pr["conn_w"][e])) for e in range(int(pr["conn_off"][k]), int(pr["conn_off"][k + 1]))) for k in range(nkf)]
    have_prev = pr.get("prev_off") is not None
    ordered = [None] * nkf                                           # None: the list the keyframe came with (known for the targets only)
    if have_prev:
        for t, k in enumerate(tgt):
            ordered[k] = [(int(pr["prev_kf"][e]), None) for e in range(int(pr["prev_off"][t]), int(pr["prev_off"][t + 1]))]
    written = set()
    resorted = set()
    turn_done = set()
    paths = dict.fromkeys(PATHS, 0)
    target_set = set(tgt)

    def sorted_list(pairs):                                          # sort(pairs) ascending by (weight, pointer), then push_front each
        s = sorted(pairs, key=lambda kw: (kw[1], rank[kw[0]]), reverse=True)
        if any(s[i][1] == s[i + 1][1] for i in range(len(s) - 1)):
            paths["sort_tie"] += 1
        return s

    def add_connection(b, a, w):                                     # (:158-170)
        if weights[b].get(a) == w:
            paths["noop_add"] += 1
            return
        weights[b][a] = w
        written.add(b)
        if order_blind:
            ordered[b] = sorted_list([(k, v) for k, v in weights[b].items() if v >= th])
            return
        ordered[b] = sorted_list(list(weights[b].items()))           # UpdateBestCovisibles (:172-193): ALL of the map
        if b not in target_set and any(v < th for v in weights[b].values()):
            paths["resort_below_th"] += 1
        if b in target_set:
            if b in turn_done:
                paths["resorted_after_turn"] += 1
            elif b not in resorted:
                paths["resorted_before_turn"] += 1
            resorted.add(b)

    status = np.zeros(ntgt, np.int32); parent = np.full(ntgt, -1, np.int32)
    links = []
    for t, a in enumerate(tgt):
        previous = None if not have_prev else [k for k, _ in ordered[a]]                    # (LoopClosing.cc:556-557)
        counter = {}
        for s in range(int(pr["slot_off"][t]), int(pr["slot_off"][t + 1])):                 # (:326-343)
            p = int(pr["slot_pt"][s])
            if p < 0 or (bad is not None and bad[p]):
                continue
            for e in range(int(pr["obs_off"][p]), int(pr["obs_off"][p + 1])):
                k = int(pr["obs_kf"][e])
                if k != a:
                    counter[k] = counter.get(k, 0) + 1
        if not counter:                                              # (:346)
            status[t] = 1
            paths["empty"] += 1
        else:
            nmax, kmax, pairs = 0, None, []
            for k in sorted(counter, key=lambda k: rank[k]):         # (:357-368) the map's iteration order
                if counter[k] > nmax:
                    nmax, kmax = counter[k], k
                if counter[k] >= th:
                    pairs.append((k, counter[k]))
                    add_connection(k, a, counter[k])
            if sum(1 for v in counter.values() if v == nmax) > 1:
                paths["max_tie"] += 1
            if not pairs:                                            # (:370-373)
                pairs.append((kmax, nmax))
                add_connection(kmax, a, nmax)
                paths["fallback"] += 1
            weights[a] = dict(counter)                               # (:387) the whole counter
            ordered[a] = sorted_list(pairs)
            written.add(a)
            if flags[t] & 1:                                         # (:392-396)
                parent[t] = ordered[a][0][0]
                paths["parent"] += 1
        turn_done.add(a)
        if have_prev:                                                # (LoopClosing.cc:561-572)
            keep = set(weights[a]) - set(previous) - target_set
            links.append(sorted(keep, key=lambda k: rank[k]))

    aff = sorted(written)
    conn_off, conn_kf, conn_w, ord_off, ord_kf, ord_w = [0], [], [], [0], [], []
    for b in aff:
        for k in sorted(weights[b], key=lambda k: rank[k]):
            conn_kf.append(k); conn_w.append(weights[b][k])
        conn_off.append(len(conn_kf))
        for k, w in ordered[b]:
            ord_kf.append(k); ord_w.append(weights[b][k] if w is None else w)
        ord_off.append(len(ord_kf))

    def i32(x):
        return np.array(x, np.int32).reshape(-1)
    out = dict(tgt_status=status, tgt_parent=parent, aff_kf=i32(aff), conn_off=i32(conn_off), conn_kf=i32(conn_kf), conn_w=i32(conn_w),
               ord_off=i32(ord_off), ord_kf=i32(ord_kf), ord_w=i32(ord_w), link_off=None, link_kf=None, paths=paths)
    n_link = 0
    if have_prev:
        out["link_off"] = i32(np.concatenate([[0], np.cumsum([len(x) for x in links])])) if ntgt else i32([0])
        out["link_kf"] = i32([k for x in links for k in x])
        n_link = len(out["link_kf"])
    out["counts"] = i32([len(aff), len(conn_kf), len(ord_kf), n_link])
    return out
