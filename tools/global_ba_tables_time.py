"""Times the two halves of GlobalBundleAdjustment on the map tables on one GPU: orbl_global_ba_assemble and orbl_global_ba_apply on a
500-keyframe, 100 000-point map (tests/globalbacases.py's generator).  Per call it reports: device time of the device entry point on
resident tables (HIP events around the call's launches, median of --reps timed calls after warm-up; the in/out tables are restored before
every stage-0 apply, outside the timed window), wall time of the host entry point with its packed upload and its download (median, through
the ctypes wrapper), and - from tests/cpp/test_globalba_dropin.cpp compiled -O2 in its `time` mode, on a map of the same size built by the
mock's own generator - the flattening and write-back loops of CeresOptimizerT::BundleAdjustment and the drop-in FrameOpsT::AssembleGlobalBA
+ ApplyGlobalBA, the solve excluded in both, best of five.  The results must agree with the restatement, bit for bit, before anything is
timed.
    python tools/global_ba_tables_time.py [--reps 50] [--out profiles/global_ba_tables_time.json]"""
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

TABLES = ("kf_id", "kf_bad", "kf_Tcw", "kf_K4", "X", "pt_bad", "obs_off", "obs_kf", "obs_uv", "obs_level", "inv_level_sigma2", "kf_center", "pt_ref_kf", "ref_level", "scale_factors")
INOUT = ("kf_Tcw", "kf_center", "X")
LISTS = ("cam_kf", "K4", "poses7", "cam_fixed", "gpt_pt", "pts3", "gobs_cam", "gobs_pt", "gobs_uv", "gobs_weight", "gobs_robust", "gobs_src")


def _cpp(tmp, mode):
    from ceres_mono_orb_slam2_amd import _lib
    exe = os.path.join(tmp, "test_globalba_dropin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_globalba_dropin.cpp"), "-o", exe, _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    w = subprocess.check_output([exe, "time"] + [str(v) for v in mode], timeout=900).decode().split()
    assert w[0] == "TIME", w
    return dict(host_loop_ms=float(w[2]), dropin_ms=float(w[4]), cameras=int(w[6]), points=int(w[8]), rows=int(w[10]))


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
    ap.add_argument("--nkf", type=int, default=500)
    ap.add_argument("--npts", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    from tests import globalbacases as gc
    from tests import npglobalba as npg
    assert torch.cuda.is_available(), "global_ba_tables_time.py needs a GPU (there is no CPU fallback to time)"
    dev = torch.device("cuda:0")

    def t(x):
        return torch.as_tensor(np.array(x)).to(dev) if isinstance(x, np.ndarray) else x

    def bits(g, e):
        g, e = np.ascontiguousarray(g).reshape(-1), np.ascontiguousarray(e).reshape(-1)
        return g.dtype == e.dtype and g.size == e.size and np.array_equal(g.view(np.uint8), e.view(np.uint8))
    m = gc.make_map(0, a.nkf, a.npts)
    asm = npg.assemble(m)
    sol = gc.solver_result(1, asm)
    exp = [npg.apply(m, asm["cam_kf"], asm["gpt_pt"], *sol, stage=s) for s in (0, 1)]
    tab = {k: m.get(k) for k in TABLES}
    got = lc.global_ba_assemble(tab, ba_kf=m["ba_kf"], ba_pt=m["ba_pt"])
    for k in LISTS + ("kf_cam", "pt_idx", "counts"):
        assert bits(got[k], asm[k]), k
    for s, keys in ((0, ("kf_Tcw", "kf_center", "X", "normal", "min_max", "nd_written", "counts")), (1, ("kf_gba_Tcw", "kf_in_gba", "pt_gba_X", "pt_in_gba", "counts"))):
        g = lc.global_ba_apply(asm["cam_kf"], asm["gpt_pt"], *sol, tab, stage=s)
        for k in keys:
            assert bits(g[k], exp[s][k]), (s, k)
    asm_wall = _time_host(a.reps, lambda: lc.global_ba_assemble(tab, ba_kf=m["ba_kf"], ba_pt=m["ba_pt"]))
    app_wall = [_time_host(a.reps, lambda s=s: lc.global_ba_apply(asm["cam_kf"], asm["gpt_pt"], *sol, tab, stage=s)) for s in (0, 1)]
    # ---- the device entries on resident tables
    d = {k: t(v) for k, v in tab.items()}
    d_in = {k: d[k].clone() for k in INOUT}
    bk, bp = t(m["ba_kf"]), t(m["ba_pt"])
    r = lc.global_ba_assemble_device(d, ba_kf=bk, ba_pt=bp)
    torch.cuda.synchronize()
    assert int(r["status"].item()) == 0 and np.array_equal(r["counts"].cpu().numpy(), asm["counts"])
    n = [int(v) for v in asm["counts"]]
    assert bits(r["gobs_src"].cpu().numpy()[:n[2]], asm["gobs_src"]) and bits(r["poses7"].cpu().numpy()[:7 * n[0]], asm["poses7"])
    a_out = {k: v for k, v in r.items() if k != "_workspace"}
    a_ws = r["_workspace"]
    asm_ev = _time_device(torch, a.reps, lambda: lc.global_ba_assemble_device(d, ba_kf=bk, ba_pt=bp, out=a_out, workspace=a_ws), lambda: None)
    p7, p3 = t(np.ascontiguousarray(sol[0]).reshape(-1)), t(np.ascontiguousarray(sol[1]).reshape(-1))

    def restore():
        for k in INOUT:
            d[k].copy_(d_in[k])
    app_ev, ws_bytes = [], 0
    for s in (0, 1):
        restore()
        r2 = lc.global_ba_apply_device(r["cam_kf"], r["gpt_pt"], p7, p3, d, stage=s, n=(n[0], n[1]))
        torch.cuda.synchronize()
        assert int(r2["status"].item()) == 0 and np.array_equal(r2["counts"].cpu().numpy(), exp[s]["counts"])
        assert bits(r2["X"].cpu().numpy(), exp[0]["X"]) if s == 0 else bits(r2["pt_gba_X"].cpu().numpy(), exp[1]["pt_gba_X"])
        keys = ("counts", "status", "normal", "min_max", "nd_written") if s == 0 else ("counts", "status", "kf_gba_Tcw", "kf_in_gba", "pt_gba_X", "pt_in_gba")
        p_out = {k: r2[k] for k in keys}
        p_ws = r2["_workspace"]
        ws_bytes = int(p_ws.numel())
        app_ev.append(_time_device(torch, a.reps, lambda s=s, p_out=p_out, p_ws=p_ws: lc.global_ba_apply_device(r["cam_kf"], r["gpt_pt"], p7, p3, d, stage=s, out=p_out, workspace=p_ws,
                                                                                                                n=(n[0], n[1])), restore if s == 0 else (lambda: None)))
    with tempfile.TemporaryDirectory() as tmp:
        cpp = _cpp(tmp, (a.nkf, a.npts))
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")][0]
    except (OSError, IndexError):
        pass

    def stats(ev, wall):
        return dict(device_ms=float(np.median(ev)), device_ms_min=float(np.min(ev)), device_ms_p90=float(np.percentile(ev, 90)),
                    host_entry_wall_ms=float(np.median(wall)), host_entry_wall_ms_min=float(np.min(wall)))
    res_json = dict(map=dict(nkf=a.nkf, npts=a.npts, listed_keyframes=len(m["ba_kf"]), listed_points=len(m["ba_pt"]), cameras=n[0], points=n[1], rows=n[2], nobs=len(m["obs_kf"]),
                             normals_written=int(exp[0]["counts"][2])),
                    assemble=dict(workspace_bytes=int(a_ws.numel()), **stats(asm_ev, asm_wall)), apply_stage0=dict(workspace_bytes=ws_bytes, **stats(app_ev[0], app_wall[0])),
                    apply_stage1=dict(workspace_bytes=ws_bytes, **stats(app_ev[1], app_wall[1])),
                    cpp=dict(note="assemble + apply (n_loop_keyframe == 0) together, the solve excluded, on the mock's own map; best of five runs, not medians", **cpp),
                    host_cpu=cpu, reps=a.reps)
    print(json.dumps(res_json))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res_json, f, indent=1)


if __name__ == "__main__":
    main()
