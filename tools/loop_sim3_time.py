"""Times the front of LoopClosing::ComputeSim3 (src/LoopClosing.cc:250-277) for 1, 4 and 16 loop candidates of 2000 features each on one GPU:
  device_call_ms    loopclosing.sim3_candidates_device on resident tables plus the one read a caller needs (off[]), wall time around work
                    that ends in a device synchronise;
  per_candidate_ms  the same work as a caller had to do it before that entry existed, with the tables resident too: per candidate the
                    download of both keyframes' descriptors, angles, slot rows and feature vectors, one orbm_search_by_bow (host pointers:
                    its own upload, launch and download), the constructor's compaction on the host and the upload of X1c / X2c / max_err.
                    The compaction is vectorised numpy over a host mirror of the observation tables that is built OUTSIDE the timed
                    window, which favours this path.
Before anything is timed both paths must give the same bytes.  The two paths alternate inside one loop; the figures are the median, the
minimum and the 90th percentile of --reps calls after --warmup calls.  There is no bar on these times: they are a record.
    python tools/loop_sim3_time.py [--reps 50] [--warmup 5] [--features 2000] [--out profiles/loop_sim3_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_LEVELS = 8
SIGMA2 = np.array([np.float32(1.2) ** (2 * i) for i in range(N_LEVELS)], np.float32)


def make_map(seed, nkf, nfeat, npts=6000, n_nodes=100):
    """nkf keyframes of nfeat keypoints over n_nodes vocabulary nodes (about nfeat / n_nodes per list, as levelsup = 4 gives): a keypoint
    shows one of npts points - its descriptor the point's with ~2 % of the bits inverted -, a fifth of the slots hold no point, a few per
    cent of the observations name another keypoint or are missing, a few points are bad"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    node_of = rng.integers(0, n_nodes, npts).astype(np.uint32) * 7 + 3
    t = dict(kf_bad=np.zeros(nkf, np.uint8), kf_K4=np.tile(np.array([718.856, 718.856, 607.19, 185.21], np.float32), (nkf, 1)), level_sigma2=SIGMA2,
             pt_bad=(rng.random(npts) < 0.03).astype(np.uint8), X=rng.normal(0, 5, (npts, 3)))
    T = np.zeros((nkf, 12)); T[:, 0] = T[:, 5] = T[:, 10] = 1.0; T[:, 3::4] = rng.normal(0, 1, (nkf, 3))
    t["kf_Tcw"] = T
    shown = np.stack([rng.permutation(npts)[:nfeat] for _ in range(nkf)])                    # [nkf, nfeat]
    t["kf_slot_off"] = (nfeat * np.arange(nkf + 1)).astype(np.int32)
    t["kf_slot_pt"] = np.where(rng.random((nkf, nfeat)) < 0.2, -1, shown).astype(np.int32).reshape(-1)
    t["kf_slot_level"] = rng.integers(0, N_LEVELS, nkf * nfeat).astype(np.int32)
    rot = rng.uniform(0, 360, nkf)
    ang = (rot[:, None] + rng.normal(0, 4, (nkf, nfeat))) % 360
    t["kf_slot_angle"] = np.where(rng.random((nkf, nfeat)) < 0.1, rng.uniform(0, 360, (nkf, nfeat)), ang).astype(np.float32).reshape(-1)
    t["kf_slot_desc"] = (base[shown] ^ np.packbits(rng.random((nkf, nfeat, 256)) < 0.02, axis=2)).reshape(-1, 32)
    fo, node, eo, ent = [0], [], [0], []
    for k in range(nkf):
        nd = node_of[shown[k]]
        order = np.argsort(nd, kind="stable")
        ids, cnt = np.unique(nd, return_counts=True)
        node += ids.tolist(); ent += order.tolist(); eo += (eo[-1] + np.cumsum(cnt)).tolist(); fo.append(len(node))
    t.update(kf_fv_off=np.array(fo, np.int32), fv_node=np.array(node, np.uint32), fv_ent_off=np.array(eo, np.int32), fv_ent=np.array(ent, np.int32))
    kf_of, slot = np.repeat(np.arange(nkf), nfeat), np.tile(np.arange(nfeat), nkf)
    has = (t["kf_slot_pt"] >= 0) & (rng.random(nkf * nfeat) > 0.05)                           # (5 %: the observation is missing)
    o_pt, o_kf, o_slot = t["kf_slot_pt"][has], kf_of[has], slot[has]
    moved = rng.random(len(o_pt)) < 0.05
    o_slot = np.where(moved, rng.integers(0, nfeat, len(o_pt)), o_slot)
    order = np.argsort(o_pt, kind="stable")
    t.update(obs_off=np.concatenate([[0], np.cumsum(np.bincount(o_pt, minlength=npts))]).astype(np.int32), obs_kf=o_kf[order].astype(np.int32),
             obs_slot=o_slot[order].astype(np.int32))
    return t


def per_candidate_path(dt, host, cur, cand, nfeat, matcher):
    """what the caller of the parent commit does, per candidate; dt: the device tables, host: the mirror built outside the timed window"""
    import torch
    out = []

    def down(k):
        a, b = k * nfeat, (k + 1) * nfeat
        f0, f1 = host["kf_fv_off"][k], host["kf_fv_off"][k + 1]
        e0, e1 = host["fv_ent_off"][f0], host["fv_ent_off"][f1]
        return dict(desc=dt["kf_slot_desc"][a:b].cpu().numpy(), ang=dt["kf_slot_angle"][a:b].cpu().numpy(), pt=dt["kf_slot_pt"][a:b].cpu().numpy(),
                    fv=(dt["fv_node"][f0:f1].cpu().numpy().view(np.uint32), (dt["fv_ent_off"][f0:f1 + 1].cpu().numpy() - e0).astype(np.uint32),
                        dt["fv_ent"][e0:e1].cpu().numpy().astype(np.uint32)))
    for k2 in cand:
        A, B = down(cur), down(int(k2))
        v1 = ((A["pt"] >= 0) & (host["pt_bad"][np.maximum(A["pt"], 0)] == 0)).astype(np.uint8)
        v2 = ((B["pt"] >= 0) & (host["pt_bad"][np.maximum(B["pt"], 0)] == 0)).astype(np.uint8)
        nm, m12 = matcher.SearchByBoW(A["desc"], v1, A["ang"], B["desc"], v2, B["ang"], A["fv"], B["fv"], strict=True)
        if nm < 20:
            out.append(None)
            continue
        i1 = np.nonzero(m12 >= 0)[0]
        p1, p2 = A["pt"][i1], B["pt"][m12[i1]]
        x1, x2 = host["index_in_kf"][cur][p1], host["index_in_kf"][int(k2)][p2]
        ok = (x1 >= 0) & (x2 >= 0)
        i1, p1, p2, x1, x2 = i1[ok], p1[ok], p2[ok], x1[ok], x2[ok]
        T1, T2 = host["kf_Tcw"][cur].reshape(3, 4), host["kf_Tcw"][int(k2)].reshape(3, 4)
        X1, X2 = host["X"][p1], host["X"][p2]
        cam = lambda T, X: ((T[:, 0] * X[:, :1] + T[:, 1] * X[:, 1:2]) + T[:, 2] * X[:, 2:3]) + T[:, 3]      # noqa: E731
        e1 = np.floor(9.210 * host["level_sigma2"][host["kf_slot_level"][cur * nfeat + x1]].astype(np.float64)).astype(np.float32)
        e2 = np.floor(9.210 * host["level_sigma2"][host["kf_slot_level"][int(k2) * nfeat + x2]].astype(np.float64)).astype(np.float32)
        h = dict(X1c=cam(T1, X1), X2c=cam(T2, X2), max_err1=e1, max_err2=e2, row_i1=i1.astype(np.int32), match12=m12, nmatches=nm)
        h["_dev"] = [torch.from_numpy(np.ascontiguousarray(h[k])).cuda() for k in ("X1c", "X2c", "max_err1", "max_err2")]
        out.append(h)
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_sim3_time.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool measures on a GPU; there is nothing to fall back to"
    from ceres_mono_orb_slam2_amd import ORBmatcher, loopclosing
    matcher = ORBmatcher(0.75, True)
    nfeat = a.features
    res = dict(device=torch.cuda.get_device_name(0), features=nfeat, reps=a.reps, warmup=a.warmup, cases=[])
    for n_cand in (1, 4, 16):
        tab = make_map(1000 + n_cand, n_cand + 1, nfeat)
        cur, cand = 0, np.arange(1, n_cand + 1, dtype=np.int32)
        dt = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32) if v.dtype == np.uint32 else np.ascontiguousarray(v)).cuda() for k, v in tab.items()}
        dc = torch.from_numpy(cand).cuda()
        host = dict(tab)
        host["index_in_kf"] = []
        for k in range(n_cand + 1):                             # GetIndexInKeyFrame per keyframe as an array over the points (first entry wins)
            ix = np.full(len(tab["pt_bad"]), -1, np.int64)
            e = np.nonzero(tab["obs_kf"] == k)[0][::-1]
            ix[np.repeat(np.arange(len(tab["pt_bad"])), np.diff(tab["obs_off"]))[e]] = tab["obs_slot"][e]
            host["index_in_kf"].append(ix)
        cap_rows = n_cand * nfeat
        ws = out = None

        def device_path():
            nonlocal ws, out
            r = loopclosing.sim3_candidates_device(dt, cur, dc, cap1=nfeat, cap_rows=cap_rows, out=out, workspace=ws)
            ws, out = r["_workspace"], {k: r[k].view(-1) for k, _, _, _ in loopclosing._LS_OUT}
            out["status"] = r["status"]
            return r, r["off"].cpu().numpy()                    # (the read synchronises the stream)
        r, off = device_path()
        assert int(r["status"].cpu()[0]) == 0
        h = per_candidate_path(dt, host, cur, cand, nfeat, matcher)
        for c in range(n_cand):                                 # the same bytes, or nothing is timed
            lo, hi = int(off[c]), int(off[c + 1])
            if h[c] is None:
                assert lo == hi
                continue
            assert np.array_equal(r["match12"][c].cpu().numpy(), h[c]["match12"]) and int(r["nmatches"][c]) == h[c]["nmatches"]
            for k in ("X1c", "X2c", "max_err1", "max_err2", "row_i1"):
                assert r[k][lo:hi].cpu().numpy().tobytes() == np.ascontiguousarray(h[c][k]).tobytes(), (n_cand, c, k)
        td, th = [], []
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter(); device_path(); t1 = time.perf_counter()
            per_candidate_path(dt, host, cur, cand, nfeat, matcher); t2 = time.perf_counter()
            if it >= a.warmup:
                td.append(1e3 * (t1 - t0)); th.append(1e3 * (t2 - t1))
        stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), p90=float(np.percentile(v, 90)))      # noqa: E731
        case = dict(n_cand=n_cand, rows=int(off[-1]), matches=int(r["nmatches"].sum()), device_call_ms=stat(td), per_candidate_ms=stat(th))
        print(json.dumps(case))
        res["cases"].append(case)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
