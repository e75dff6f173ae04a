"""Times the two map-moving calls of a loop closure on one GPU: orbl_correct_loop (40 connected keyframes of about 2 000 slots each over
100 000 points, tests/mapcorrectcases.py's generator) and orbl_propagate_global_ba (500 keyframes, 100 000 points, 20 keyframes outside
the BA).  Per call it reports: device time of the device entry point on resident tables (HIP events around the call's launches, median of
--reps timed calls after warm-up; the in/out tables are restored before every call, outside the timed window), wall time of the host
entry point with its packed upload and its download (median, through the ctypes wrapper), and - from tests/cpp/test_mapcorrect_dropin.cpp
compiled -O2 in its `time` mode, on a map of the same size built by the mock's own generator - the reference-shaped host loop of
src/LoopClosing.cc:437-523 / :681-739 and the whole drop-in call (flattening + host entry + write-back), best of five.  The results must
equal the restatement before anything is timed.
    python tools/map_correct_time.py [--reps 50] [--out profiles/map_correct_time.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cpp(tmp, *modes):
    from ceres_mono_orb_slam2_amd import _lib
    exe = os.path.join(tmp, "test_mapcorrect_dropin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_mapcorrect_dropin.cpp"), "-o", exe, _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    out = []
    for m in modes:
        w = subprocess.check_output([exe, "time"] + [str(v) for v in m], timeout=900).decode().split()
        assert w[0] == "TIME", w
        out.append(dict(host_loop_ms=float(w[2]), dropin_ms=float(w[4])))
    return out


def _time_device(torch, reps, call, restore):
    for _ in range(5):
        restore(); call()
    torch.cuda.synchronize()
    ev = []
    for _ in range(reps):
        restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    return ev


def _time_host(reps, call):
    call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    return wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--nconn", type=int, default=40)
    ap.add_argument("--slots", type=int, default=2000)
    ap.add_argument("--npts", type=int, default=100000)
    ap.add_argument("--nkf", type=int, default=500)
    ap.add_argument("--outside", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    from tests import mapcorrectcases as mc
    from tests import npmapcorrect as npm
    assert torch.cuda.is_available(), "map_correct_time.py needs a GPU (there is no CPU fallback to time)"
    dev = torch.device("cuda:0")

    def t(x):
        return torch.as_tensor(np.array(x)).to(dev) if isinstance(x, np.ndarray) else x
    # ---- correct_loop
    pr = mc.make_loop(0, a.nconn, a.npts, nkf=a.nkf, max_slots=a.slots * 3 // 2)
    exp = npm.correct_loop(pr)
    lkw = {k: pr[k] for k in ("kf_center", "conn_rank", "pt_bad", "pt_done", "obs_off", "obs_kf", "ref_kf", "ref_level", "scale_factors")}
    largs = [pr[k] for k in ("kf_Tcw", "conn_kf", "Scw", "slot_off", "slot_pt", "X")]
    got = lc.correct_loop(*largs, **lkw)
    moved = exp["pt_owner"] >= 0
    for k in ("kf_Tcw", "kf_center", "X", "corrected", "non_corrected", "pt_owner", "counts"):
        assert np.array_equal(got[k], exp[k]), k
    assert np.array_equal(got["normal"][moved], exp["normal"][moved]) and np.array_equal(got["min_max"][moved], exp["min_max"][moved])
    loop_wall = _time_host(a.reps, lambda: lc.correct_loop(*largs, **lkw))
    d_in = {k: t(pr[k]) for k in ("kf_Tcw", "kf_center", "X")}
    d = {k: t(v) for k, v in list(lkw.items()) + [(k, pr[k]) for k in ("conn_kf", "Scw", "slot_off", "slot_pt")]}
    for k in ("kf_Tcw", "kf_center", "X"):
        d[k] = d_in[k].clone()
    d_out = {}
    r = lc.correct_loop_device(d["kf_Tcw"], d["conn_kf"], d["Scw"], d["slot_off"], d["slot_pt"], d["X"], out=d_out,
                               **{k: d[k] for k in ("kf_center", "conn_rank", "pt_bad", "pt_done", "obs_off", "obs_kf", "ref_kf", "ref_level", "scale_factors")})
    torch.cuda.synchronize()
    assert int(r["status"].item()) == 0 and np.array_equal(r["X"].cpu().numpy().reshape(-1, 3), exp["X"]) and np.array_equal(r["counts"].cpu().numpy(), exp["counts"])
    d_out = {k: r[k] for k in ("corrected", "non_corrected", "pt_owner", "counts", "status", "normal", "min_max", "nd_written")}
    lws = r["_workspace"]

    def loop_call():
        lc.correct_loop_device(d["kf_Tcw"], d["conn_kf"], d["Scw"], d["slot_off"], d["slot_pt"], d["X"], out=d_out, workspace=lws,
                               **{k: d[k] for k in ("kf_center", "conn_rank", "pt_bad", "pt_done", "obs_off", "obs_kf", "ref_kf", "ref_level", "scale_factors")})

    def loop_restore():
        for k in ("kf_Tcw", "kf_center", "X"):
            d[k].copy_(d_in[k])
    loop_ev = _time_device(torch, a.reps, loop_call, loop_restore)
    # ---- propagate_global_ba
    pg = dict(mc.make_gba(1, a.nkf, npts=a.npts))
    rng = np.random.RandomState(2)
    flags = np.ones(a.nkf, np.uint8)
    inner = np.nonzero(pg["kf_parent"] >= 0)[0]
    flags[rng.permutation(inner)[:a.outside]] = 0
    pg["kf_in_gba"] = flags
    eg = npm.propagate_global_ba(pg)
    gargs = [pg[k] for k in ("kf_Tcw", "kf_gba_Tcw", "kf_in_gba", "kf_parent", "origin_kf", "X", "pt_ref_kf")]
    gkw = {k: pg[k] for k in ("kf_center", "pt_bad", "pt_in_gba", "pt_gba_X")}
    got = lc.propagate_global_ba(*gargs, **gkw)
    for k in ("kf_Tcw", "kf_gba_Tcw", "kf_in_gba", "kf_center", "X", "kf_reached", "pt_moved", "counts"):
        assert np.array_equal(got[k], eg[k]), k
    gba_wall = _time_host(a.reps, lambda: lc.propagate_global_ba(*gargs, **gkw))
    g_in = {k: t(pg[k]) for k in ("kf_Tcw", "kf_gba_Tcw", "kf_in_gba", "kf_center", "X")}
    g = {k: t(v) for k, v in list(gkw.items()) + [(k, pg[k]) for k in ("kf_parent", "origin_kf", "pt_ref_kf")]}
    for k in g_in:
        g[k] = g_in[k].clone()
    r = lc.propagate_global_ba_device(g["kf_Tcw"], g["kf_gba_Tcw"], g["kf_in_gba"], g["kf_parent"], g["origin_kf"], g["X"], g["pt_ref_kf"],
                                      **{k: g[k] for k in ("kf_center", "pt_bad", "pt_in_gba", "pt_gba_X")})
    torch.cuda.synchronize()
    assert np.array_equal(r["X"].cpu().numpy().reshape(-1, 3), eg["X"]) and np.array_equal(r["counts"].cpu().numpy(), eg["counts"])
    g_out = {k: r[k] for k in ("kf_bef_Tcw", "kf_reached", "pt_moved", "counts", "status")}
    gws = r["_workspace"]

    def gba_call():
        lc.propagate_global_ba_device(g["kf_Tcw"], g["kf_gba_Tcw"], g["kf_in_gba"], g["kf_parent"], g["origin_kf"], g["X"], g["pt_ref_kf"], out=g_out, workspace=gws,
                                      **{k: g[k] for k in ("kf_center", "pt_bad", "pt_in_gba", "pt_gba_X")})

    def gba_restore():
        for k in g_in:
            g[k].copy_(g_in[k])
    gba_ev = _time_device(torch, a.reps, gba_call, gba_restore)
    with tempfile.TemporaryDirectory() as tmp:
        cpp_loop, cpp_gba = _cpp(tmp, ("loop", a.nconn, a.slots, a.npts), ("gba", a.nkf, a.npts, a.outside))
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")][0]
    except (OSError, IndexError):
        pass

    def stats(ev, wall, cpp):
        return dict(device_ms=float(np.median(ev)), device_ms_min=float(np.min(ev)), device_ms_p90=float(np.percentile(ev, 90)),
                    host_entry_wall_ms=float(np.median(wall)), host_entry_wall_ms_min=float(np.min(wall)), cpp_host_loop_ms=cpp["host_loop_ms"], cpp_dropin_ms=cpp["dropin_ms"])
    res = dict(correct_loop=dict(nconn=a.nconn, nkf=a.nkf, npts=a.npts, nslots=len(pr["slot_pt"]), nobs=len(pr["obs_kf"]), moved=int(exp["counts"][0]),
                                 contested=int(exp["counts"][1]), workspace_bytes=int(lws.numel()), **stats(loop_ev, loop_wall, cpp_loop)),
               propagate_global_ba=dict(nkf=a.nkf, npts=a.npts, outside=int((flags == 0).sum()), reached=int(eg["counts"][0]), propagated=int(eg["counts"][1]),
                                        points_moved=int(eg["counts"][2]), tree_depth_outside=int(eg["depth"]), **stats(gba_ev, gba_wall, cpp_gba)),
               host_cpu=cpu, reps=a.reps)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
