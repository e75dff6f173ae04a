"""Times LocalMapping::SearchInNeighbors on the resident map tables (localmapping.search_in_neighbors_on_tables and the four entries under
it) on one GPU, on a corridor map of its own vectorised generator: 500 keyframes, 100 000 points, about 30 target keyframes.  Reports
medians of --reps calls:
  chain_resident_wall_ms   the whole function on resident tables, wall time: it holds the count read-backs (one per target plus three),
                           which are host synchronisations, so device events around the launches would flatter it;
  entries                  each device entry alone on the map as it stands at entry (HIP events around its launches): the targets, the rows
                           of the first target, the replay of those rows, the descriptor update of the points it touched, the candidates,
                           the final update of the current keyframe's points, UpdateConnections of the one keyframe;
  chain_host_entries_wall_ms  the same sequence through the HOST entries (numpy tables, every call with its packed upload and its
                           download), --host-reps calls.
Before anything is timed the resident chain and the host-entry chain must leave the same bytes in every table.  There is no -O2
reference-shaped loop here: tests/cpp/mapedit_host_loop.cpp replays edits only, it has no projection search, and a mock of ORBmatcher::Fuse
is not something that harness gives cheaply.  There is no bar on these times: they are a record.
    python tools/search_in_neighbors_time.py [--reps 50] [--host-reps 5] [--nkf 500] [--npts 100000] [--out profiles/search_in_neighbors_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32 = np.float32
SF = (F32(1.2) ** np.arange(8)).astype(F32)
TABLES = ("kf_slot_pt", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced", "obs_off", "obs_kf", "obs_slot", "pt_desc", "pt_normal", "pt_min_dist", "pt_max_dist",
          "kf_fuse_target", "pt_fuse_cand")
MUTATED = ("kf_slot_pt", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced", "pt_desc", "pt_normal", "pt_min_dist", "pt_max_dist", "kf_fuse_target", "pt_fuse_cand")


def _noise(rng, n, p):
    """n x 32 bytes with each bit set with probability p"""
    return np.packbits(rng.random((n, 256)) < p, axis=1)


def make_large(seed, nkf, npts):
    """A corridor: keyframe k at x = 0.05 k looking along z; places in front of it, 40 % of them holding two points a few millimetres
    apart with similar descriptors; a point is seen by 2 to 6 of the 50 keyframes around its place; a tenth of the keypoints hold no point."""
    rng = np.random.default_rng(seed)
    step = 0.05
    ctr = np.stack([step * np.arange(nkf) + rng.normal(0, 0.005, nkf), rng.normal(0, 0.01, nkf), rng.normal(0, 0.01, nkf)], 1)
    T = np.zeros((nkf, 12)); T[:, 0] = T[:, 5] = T[:, 10] = 1.0; T[:, 3::4] = -ctr
    ctr = -T[:, 3::4]                                                        # (the centre as SetPose computes it under R = I)
    nplace = int(npts / 1.4)
    members = 1 + (rng.random(nplace) < 0.4)
    place = np.stack([rng.uniform(-1, step * nkf + 1, nplace), rng.uniform(-1.5, 1.5, nplace), rng.uniform(4, 10, nplace)], 1)
    pt_place = np.repeat(np.arange(nplace), members)
    n = len(pt_place)
    X = place[pt_place] + rng.normal(0, 0.002, (n, 3))
    base = rng.integers(0, 256, (nplace, 32), dtype=np.uint8)
    mbase = base[pt_place] ^ _noise(rng, n, 0.02)
    # observations: up to 6 keyframes of the window around the place, duplicates and out-of-image ones dropped; then keypoints without a point
    nob = rng.integers(2, 7, n)
    kf = np.rint(X[:, None, 0] / step).astype(np.int64) + rng.integers(-25, 26, (n, 6))
    keep = (np.arange(6)[None] < nob[:, None]) & (kf >= 0) & (kf < nkf)
    o_pt, o_kf = np.repeat(np.arange(n), 6)[keep.reshape(-1)], kf.reshape(-1)[keep.reshape(-1)]
    _, first = np.unique(o_pt * nkf + o_kf, return_index=True)
    o_pt, o_kf = o_pt[first], o_kf[first]
    nfree = len(o_pt) // 10
    f_place = rng.integers(0, nplace, nfree)
    f_kf = np.clip(np.rint(place[f_place, 0] / step).astype(np.int64) + rng.integers(-25, 26, nfree), 0, nkf - 1)
    a_pt = np.concatenate([o_pt, np.full(nfree, -1)]); a_kf = np.concatenate([o_kf, f_kf])
    a_X = np.concatenate([X[o_pt], place[f_place]]); a_base = np.concatenate([mbase[o_pt], base[f_place]])
    c = a_X - ctr[a_kf]
    u, v = (500 * c[:, 0] / c[:, 2] + 320 + rng.normal(0, 0.4, len(c))).astype(F32), (500 * c[:, 1] / c[:, 2] + 240 + rng.normal(0, 0.4, len(c))).astype(F32)
    ok = (u > 20) & (u < 620) & (v > 20) & (v < 460)
    a_pt, a_kf, a_X, a_base, u, v = a_pt[ok], a_kf[ok], a_X[ok], a_base[ok], u[ok], v[ok]
    order = np.lexsort((np.arange(len(a_kf)), a_kf))                         # the slots of a keyframe, in this order
    a_pt, a_kf, a_X, a_base, u, v = a_pt[order], a_kf[order], a_X[order], a_base[order], u[order], v[order]
    slot_off = np.zeros(nkf + 1, np.int32); slot_off[1:] = np.cumsum(np.bincount(a_kf, minlength=nkf))
    a_slot = np.arange(len(a_kf)) - slot_off[a_kf]
    held = a_pt >= 0
    # the reference keyframe of a point: its first observer by index; the depth range from there
    ref = np.full(n, nkf, np.int64)
    np.minimum.at(ref, a_pt[held], a_kf[held])
    seen = ref < nkf
    ref[~seen] = 0
    dref = np.linalg.norm(X - ctr[ref], axis=1).astype(F32)
    max_d = (dref * SF[rng.integers(1, 5, n)] * rng.uniform(0.90, 0.99, n).astype(F32)).astype(F32)
    px = np.where(held, a_pt, 0)
    amax = np.where(held, max_d[px], (np.linalg.norm(a_X - ctr[a_kf], axis=1) * 2.0).astype(F32))
    q = np.log(amax / np.linalg.norm(a_X - ctr[a_kf], axis=1).astype(F32)) / np.log(F32(1.2))
    level = np.clip(np.ceil(q).astype(np.int64) - (rng.random(len(q)) < 0.3), 0, 7).astype(np.int32)
    desc = a_base ^ _noise(rng, len(a_base), 0.03)
    rank = rng.permutation(nkf).astype(np.int32)
    e = np.nonzero(held)[0]
    e = e[np.lexsort((rank[a_kf[e]], a_pt[e]))]                              # every list in ascending kf_rank
    obs_off = np.zeros(n + 1, np.int32); obs_off[1:] = np.cumsum(np.bincount(a_pt[e], minlength=n))
    pt_desc = np.zeros((n, 32), np.uint8); pt_desc[a_pt[e][::-1]] = desc[e][::-1]          # (the first observation's descriptor)
    nrm = X - ctr[ref]
    nbr = np.array([1, -1, 2, -2, 3, -3, 4, -4])
    ords = [[k + d for d in nbr if 0 <= k + d < nkf] for k in range(nkf)]
    ord_off = np.zeros(nkf + 1, np.int32); ord_off[1:] = np.cumsum([len(o) for o in ords])
    ord_kf = np.array([k for o in ords for k in o], np.int32)
    tab = dict(kf_bad=np.zeros(nkf, np.uint8), kf_rank=rank, kf_Tcw=T, kf_center=ctr, kf_K4=np.tile(np.array([500, 500, 320, 240], F32), (nkf, 1)),
               kf_bounds=np.tile(np.array([0, 640, 0, 480], F32), (nkf, 1)), kf_slot_off=slot_off, kf_slot_pt=a_pt.astype(np.int32), kf_slot_uv=np.stack([u, v], 1),
               kf_slot_level=level, kf_slot_desc=desc, X=X, pt_normal=nrm / np.linalg.norm(nrm, axis=1)[:, None], pt_min_dist=(max_d / SF[7]).astype(F32), pt_max_dist=max_d,
               pt_desc=pt_desc, pt_bad=(~seen).astype(np.uint8), pt_nobs=np.diff(obs_off).astype(np.int32), pt_found=rng.integers(1, 30, n).astype(np.int32),
               pt_visible=rng.integers(30, 60, n).astype(np.int32), pt_replaced=np.full(n, -1, np.int32), pt_ref_kf=ref.astype(np.int32), obs_off=obs_off,
               obs_kf=a_kf[e].astype(np.int32), obs_slot=a_slot[e].astype(np.int32), ord_off=ord_off, ord_kf=ord_kf, conn_off=ord_off.copy(), conn_kf=ord_kf.copy(),
               conn_w=np.array([100 - 10 * i for o in ords for i in range(len(o))], np.int32), kf_fuse_target=np.zeros(nkf, np.int32), pt_fuse_cand=np.zeros(n, np.int32),
               scale_factors=SF.copy(), inv_level_sigma2=(F32(1) / (SF * SF)).astype(F32))
    return tab, nkf // 2, 1000


def host_chain(lm, cur_kf, cur_id, tab):
    """the sequence of search_in_neighbors_on_tables through the host entries, on numpy tables"""
    t = {k: (None if v is None else np.array(v)) for k, v in tab.items()}
    tg = lm.fuse_targets(cur_kf, cur_id, t)
    t["kf_fuse_target"] = tg["kf_fuse_target"]
    lo, hi = t["kf_slot_off"][cur_kf], t["kf_slot_off"][cur_kf + 1]
    snapshot = t["kf_slot_pt"][lo:hi].copy()
    n_fused = []

    def fuse(K, pts):
        rows = lm.fuse_rows(K, pts, t, extras=False)
        ed = lm.apply_map_edits(rows, dict(t, kf_slot_level=None, kf_slot_uv=None))
        for k in ("kf_slot_pt", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced"):
            t[k] = getattr(ed, k)
        t["obs_off"], t["obs_kf"], t["obs_slot"] = ed.oobs_off, ed.oobs_kf, ed.oobs_slot
        up = lm.update_map_points_on_tables(lm.MP_DESC, t, pt_mask=ed.pt_touched)
        t["pt_desc"] = up["pt_desc"]
        n_fused.append(int(ed.counts[4]))

    for K in tg["tgt_kf"]:
        fuse(int(K), snapshot)
    cd = lm.fuse_candidates(tg["tgt_kf"], cur_id, t)
    t["pt_fuse_cand"] = cd["pt_fuse_cand"]
    fuse(cur_kf, cd["cand_pt"])
    up = lm.update_map_points_on_tables(lm.MP_DESC | lm.MP_NORMAL_DEPTH, t, mask_kf=cur_kf)
    for k in ("pt_desc", "pt_normal", "pt_min_dist", "pt_max_dist"):
        t[k] = up[k]
    conn = lm.update_connections([cur_kf], [0, hi - lo], t["kf_slot_pt"][lo:hi], len(t["kf_bad"]), t["obs_off"], t["obs_kf"], t["conn_off"], t["conn_kf"], t["conn_w"],
                                 pt_bad=t["pt_bad"], kf_rank=t["kf_rank"])
    return t, tg["tgt_kf"].tolist(), n_fused, conn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--nkf", type=int, default=500)
    ap.add_argument("--npts", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ceres_mono_orb_slam2_amd import localmapping as lm
    assert torch.cuda.is_available(), "search_in_neighbors_time.py needs a GPU (there is no CPU fallback to time)"
    tab, cur_kf, cur_id = make_large(0, a.nkf, a.npts)
    dt = dict(lm._SN_TAB)
    pristine = {k: torch.as_tensor(np.ascontiguousarray(v, dt[k])).cuda() for k, v in tab.items()}

    def fresh():
        return {k: (v.clone() if k in MUTATED else v) for k, v in pristine.items()}

    # the two chains must agree before anything is timed
    r = lm.search_in_neighbors_on_tables(cur_kf, cur_id, fresh())
    torch.cuda.synchronize()
    ht, h_tgt, h_fused, h_conn = host_chain(lm, cur_kf, cur_id, tab)
    assert r["status"] == 0 and r["tgt_kf"] == h_tgt and r["n_fused"] == h_fused, (r["status"], r["n_fused"], h_fused)
    for k in TABLES:
        assert np.array_equal(r["tab"][k].cpu().numpy().reshape(-1), np.asarray(ht[k]).reshape(-1)), k
    assert np.array_equal(r["connections"]["counts"].cpu().numpy(), h_conn["counts"])
    wall = []
    for _ in range(a.reps):
        t = fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lm.search_in_neighbors_on_tables(cur_kf, cur_id, t)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    hwall = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        host_chain(lm, cur_kf, cur_id, tab)
        hwall.append((time.perf_counter() - t0) * 1e3)

    # each entry alone, on the map as it stands at entry
    lo, hi = int(tab["kf_slot_off"][cur_kf]), int(tab["kf_slot_off"][cur_kf + 1])
    n_tgt = len(r["tgt_kf"])
    d_tgt = torch.as_tensor(np.array(r["tgt_kf"], np.int32)).cuda()
    cur_word = torch.tensor([cur_kf], dtype=torch.int32, device="cuda")
    row_off = torch.tensor([0, hi - lo], dtype=torch.int32, device="cuda")
    state = {}

    def stage(name):
        t = state["t"]
        if name == "targets":
            return lm.fuse_targets(cur_kf, cur_id, t, device=True)
        if name == "rows_one_target":
            state["rows"] = lm.fuse_rows(d_tgt[:1], t["kf_slot_pt"][lo:hi].clone(), t, device=True, extras=False)
            return state["rows"]
        if name == "edits_one_target":
            state["ed"] = lm.apply_map_edits_device(state["rows"], dict(t, kf_slot_level=None, kf_slot_uv=None))
            return state["ed"]
        if name == "descriptors_of_touched":
            return lm.update_map_points_on_tables(lm.MP_DESC, state["t2"], pt_mask=state["ed"].pt_touched, device=True)
        if name == "candidates":
            return lm.fuse_candidates(d_tgt, cur_id, t, device=True)
        if name == "final_update":
            return lm.update_map_points_on_tables(lm.MP_DESC | lm.MP_NORMAL_DEPTH, state["t2"], mask_kf=cur_kf, device=True)
        t2 = state["t2"]
        return lm.update_connections_device(cur_word, row_off, t2["kf_slot_pt"][lo:hi], a.nkf, t2["obs_off"], t2["obs_kf"], t2["conn_off"], t2["conn_kf"], t2["conn_w"],
                                            pt_bad=t2["pt_bad"], kf_rank=t2["kf_rank"])

    names = ("targets", "rows_one_target", "edits_one_target", "descriptors_of_touched", "candidates", "final_update", "update_connections")
    ev = {k: [] for k in names}
    for rep in range(a.reps + 3):
        state["t"] = fresh()
        for name in names:
            if name == "descriptors_of_touched":                             # (the count read-back and the swap of the tables stay outside the timed span)
                ed = state["ed"]
                nn = int(ed.counts.cpu()[0])
                state["t2"] = dict(state["t"], obs_off=ed.oobs_off, obs_kf=ed.oobs_kf[:nn], obs_slot=ed.oobs_slot[:nn])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            keep = stage(name)
            e1.record()
            torch.cuda.synchronize()
            del keep
            if rep >= 3:
                ev[name].append(e0.elapsed_time(e1))
    touched = int(state["ed"].pt_touched.sum().item())
    res = dict(nkf=a.nkf, npts=len(tab["pt_bad"]), nslots=len(tab["kf_slot_pt"]), nobs=len(tab["obs_kf"]), reps=a.reps, host_reps=a.host_reps, n_targets=n_tgt,
               rows_per_target=hi - lo, n_candidates=len(r["cand_pt"]), n_fused=r["n_fused"], touched_by_first_target=touched,
               chain_resident_wall_ms=float(np.median(wall)), chain_resident_wall_ms_min=float(np.min(wall)), chain_resident_wall_ms_p90=float(np.percentile(wall, 90)),
               chain_host_entries_wall_ms=float(np.median(hwall)), chain_host_entries_wall_ms_min=float(np.min(hwall)),
               entries_device_ms={k: float(np.median(v)) for k, v in ev.items()}, host_reads_per_chain=n_tgt + 4,
               reference_shaped_host_loop_ms=None)
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")][0]
    except (OSError, IndexError):
        pass
    res["host_cpu"] = cpu
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
