"""CeresOptimizer::OptimizeEssentialGraph around its solve, restated on the flat map tables of tests/essgraphcases.py in plain Python loops
that follow src/CeresOptimizer.cc:769-956 line by line, in the reading csrc/compat/orbslam_dropin.h fixed: the parameter blocks are the
keyframes that are not bad, numbered densely in map order; an edge to a keyframe without a block is not added; a point whose reference
keyframe has no block stays.  The Sim(3) values come from the CPU oracle (oracle.pyoracle sim3_log / exp / mul / inverse / act).
Independent of the device code and of tests/dropin_checker.py."""
import numpy as np

from oracle import pyoracle as po


def _row(off, arr, i):
    return [int(v) for v in arr[off[i]:off[i + 1]]]


def _ranks(m):
    return [int(v) for v in (m["kf_rank"] if m.get("kf_rank") is not None else np.arange(m["nkf"]))]


def _is_bad(m, k):
    return m.get("kf_bad") is not None and bool(m["kf_bad"][k])


def _sim3_of_pose(T12):
    """Sophus::Sim3d(Sophus::RxSO3d(1.0, Rcw), tcw): Eigen's matrix -> quaternion through the pose codec"""
    T = np.eye(4); T[:3, :] = np.asarray(T12, np.float64).reshape(3, 4)
    p7 = po.matrix4d_to_pose7(T)
    return np.array([p7[3], p7[4], p7[5], p7[6], p7[0], p7[1], p7[2]])


def assemble(m):
    """-> dict(vtx_kf, kf_vtx, lie7, vtx_fixed, edge_j, edge_i, edge_Sji, edge_kind, counts) and edges = [(kf j, kf i, kind)]"""
    nkf, rank, ids = m["nkf"], _ranks(m), [int(v) for v in m["kf_id"]]
    min_weight, loop_kf, cur_kf = int(m.get("min_weight", 100)), int(m["loop"]), int(m["cur"])
    all_keyframes = sorted(range(nkf), key=lambda k: rank[k])        # Map::GetAllKeyFrames(): std::set<KeyFrame*>
    group = {int(k): c for c, k in enumerate(m["conn_group_kf"])}    # the keys of both KeyFrameAndSim3 maps
    vtx, vtx_kf, lie, fixed = {}, [], [], []
    for keyframe in all_keyframes:                                   # :769
        if _is_bad(m, keyframe):                                     # :771
            continue
        if keyframe in group:                                        # :775-777
            x = po.sim3_log(m["corrected"][group[keyframe]])
        else:                                                        # :779-782
            x = po.sim3_log(_sim3_of_pose(m["kf_Tcw"][keyframe]))
        vtx[keyframe] = len(vtx_kf); vtx_kf.append(keyframe); lie.append(x)
        fixed.append(1 if keyframe == loop_kf else 0)                # :788-791
    edges, S_list = [], []
    dropped = 0

    def block(k):
        return po.sim3_exp(lie[vtx[k]])

    def world(k):                                                    # :830-835, :842-847
        return np.array(m["non_corrected"][group[k]], np.float64) if k in group else block(k)

    def get_weight(i, j):                                            # KeyFrame::GetWeight
        for e in range(m["conn_off"][i], m["conn_off"][i + 1]):
            if int(m["conn_kf"][e]) == j:
                return int(m["conn_w"][e])
        return 0

    inserted_edges = set()                                           # :794
    loop_connections = {int(t): _row(m["link_off"], m["link_kf"], c) for c, t in enumerate(m["tgt_kf"])}
    for keyframe in sorted(loop_connections, key=lambda k: rank[k]):             # :797, std::map<KeyFrame*, ...>
        id_i = ids[keyframe]
        Swi = po.sim3_inverse(block(keyframe)) if keyframe in vtx else None      # :801-802
        for kj in sorted(set(loop_connections[keyframe]), key=lambda k: rank[k]):      # :804, std::set<KeyFrame*>
            id_j = ids[kj]
            if (id_i != ids[cur_kf] or id_j != ids[loop_kf]) and get_weight(keyframe, kj) < min_weight:      # :807-809
                continue
            if keyframe not in vtx or kj not in vtx:
                dropped += 1
                continue
            S_list.append(po.sim3_mul(block(kj), Swi)); edges.append((kj, keyframe, 0))      # :811-817
            inserted_edges.add((min(id_i, id_j), max(id_i, id_j)))   # :819
    n_loop_connection = len(edges)
    for keyframe in all_keyframes:                                   # :824
        if keyframe not in vtx:
            continue
        Swi = po.sim3_inverse(world(keyframe))                       # :830-835
        parent_keyframe = int(m["kf_parent"][keyframe])              # :836
        if parent_keyframe >= 0:
            if parent_keyframe in vtx:
                S_list.append(po.sim3_mul(world(parent_keyframe), Swi)); edges.append((parent_keyframe, keyframe, 1))      # :848-853
            else:
                dropped += 1
        loop_edges = sorted(set(_row(m["loop_off"], m["loop_kf"], keyframe)), key=lambda k: rank[k])       # :857
        for l in loop_edges:                                         # :858
            if ids[l] < ids[keyframe]:                               # :860
                if l not in vtx:
                    dropped += 1
                    continue
                S_list.append(po.sim3_mul(world(l), Swi)); edges.append((l, keyframe, 2))                  # :868-874
        ord_kf = _row(m["ord_off"], m["ord_kf"], keyframe); ord_w = _row(m["ord_off"], m["ord_w"], keyframe)
        n = 0                                                        # KeyFrame::GetCovisiblesByWeight (src/KeyFrame.cc:218-235)
        while n < len(ord_w) and ord_w[n] >= min_weight:
            n += 1
        connected_keyframes = [] if n == len(ord_w) else ord_kf[:n]  # upper_bound == end(): an empty vector
        childs = _row(m["child_off"], m["child_kf"], keyframe)
        for keyframe_n in connected_keyframes:                       # :881
            if keyframe_n != parent_keyframe and keyframe_n not in childs and keyframe_n not in loop_edges:      # :884-885
                if not _is_bad(m, keyframe_n) and ids[keyframe_n] < ids[keyframe]:                              # :886
                    if (min(ids[keyframe], ids[keyframe_n]), max(ids[keyframe], ids[keyframe_n])) in inserted_edges:       # :887-890
                        continue
                    if keyframe_n not in vtx:
                        dropped += 1
                        continue
                    S_list.append(po.sim3_mul(world(keyframe_n), Swi)); edges.append((keyframe_n, keyframe, 3))            # :899-905
    kf_vtx = np.full(nkf, -1, np.int32)
    for k, v in vtx.items():
        kf_vtx[k] = v
    return dict(vtx_kf=np.array(vtx_kf, np.int32), kf_vtx=kf_vtx, lie7=np.array(lie, np.float64).reshape(-1, 7), vtx_fixed=np.array(fixed, np.uint8),
                edge_j=np.array([vtx[j] for j, _, _ in edges], np.int32), edge_i=np.array([vtx[i] for _, i, _ in edges], np.int32),
                edge_Sji=np.array(S_list, np.float64).reshape(-1, 7), edge_kind=np.array([k for _, _, k in edges], np.uint8),
                counts=np.array([len(vtx_kf), len(edges), n_loop_connection, dropped], np.int32), edges=edges)


def _rotation(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def apply(m, vtx_kf, lie_orig, lie_opt, normals=True, normal=None, min_max=None):
    """-> dict(kf_Tcw, kf_center, X, pt_moved, normal, min_max, nd_written, counts); normal / min_max: preset arrays (copied), of which only
    the rows of points with a new normal are rewritten"""
    nkf, npts = m["nkf"], m["npts"]
    T = np.array(m["kf_Tcw"], np.float64).reshape(-1, 12); Cn = np.array(m["kf_center"], np.float64).reshape(-1, 3); X = np.array(m["X"], np.float64).reshape(-1, 3)
    lie_orig = np.asarray(lie_orig, np.float64).reshape(-1, 7); lie_opt = np.asarray(lie_opt, np.float64).reshape(-1, 7)
    vtx = {int(k): v for v, k in enumerate(vtx_kf)}
    corrected_Swcs = {}
    for keyframe, v in vtx.items():                                  # :917
        S = po.sim3_exp(lie_opt[v])                                  # :921
        corrected_Swcs[keyframe] = po.sim3_inverse(S)                # :922
        s = float(S[:4] @ S[:4])
        R = _rotation(S[:4] / np.sqrt(s))                            # :923-925
        t = (1.0 / s) * S[4:]                                        # :928
        T[keyframe] = np.concatenate([R, t.reshape(3, 1)], axis=1).reshape(12)          # :929-932 SetPose
        Cn[keyframe] = -(R.T @ t)
    moved = np.zeros(npts, np.uint8)
    for p in range(npts):                                            # :936
        if m.get("pt_bad") is not None and m["pt_bad"][p]:           # :939
            continue
        if m.get("pt_done") is not None and m["pt_done"][p]:         # :942-943
            r = int(m["pt_corr_ref"][p])
        else:                                                        # :945-946
            r = int(m["pt_ref_kf"][p])
        if r not in vtx:
            continue
        Srw = po.sim3_exp(lie_orig[vtx[r]])                          # :948
        X[p] = po.sim3_act(corrected_Swcs[r], po.sim3_act(Srw, X[p]))            # :951-954
        moved[p] = 1
    out = dict(kf_Tcw=T, kf_center=Cn, X=X, pt_moved=moved, normal=None, min_max=None, nd_written=None, counts=np.array([len(vtx), int(moved.sum())], np.int32))
    if not normals:
        return out
    nrm = np.zeros((npts, 3)) if normal is None else np.array(normal, np.float64)
    mm = np.zeros((npts, 2), np.float32) if min_max is None else np.array(min_max, np.float32)
    wrote = np.zeros(npts, np.uint8)
    sf = np.asarray(m["scale_factors"], np.float32)
    for p in range(npts):                                            # :955 MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:342-378), every centre the new one
        obs = _row(m["obs_off"], m["obs_kf"], p)
        r = int(m["pt_ref_kf"][p])
        if not moved[p] or not obs or r < 0:
            continue
        acc = np.zeros(3)
        for k in obs:
            v = X[p] - Cn[k]
            acc = acc + v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        nrm[p] = acc / float(len(obs))
        d = X[p] - Cn[r]
        dist = np.float32(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        mx = np.float32(dist * sf[int(m["ref_level"][p])])
        mm[p] = (np.float32(mx / sf[len(sf) - 1]), mx)
        wrote[p] = 1
    out.update(normal=nrm, min_max=mm, nd_written=wrote)
    return out
