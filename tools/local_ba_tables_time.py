"""Times the two halves of LocalBundleAdjustment on the map tables on one GPU: orbl_local_ba_assemble and orbl_local_ba_apply on an
81-keyframe, about 8 000-point local map inside a 500-keyframe, 100 000-point map (tests/localbacases.py's generator).  Per call it
reports: device time of the device entry point on resident tables (HIP events around the call's launches, median of --reps timed calls
after warm-up; the in/out tables are restored before every apply, outside the timed window), wall time of the host entry point with its
packed upload of the WHOLE map and its download (median, through the ctypes wrapper), and - from tests/cpp/test_localba_dropin.cpp compiled
-O2 in its `time` mode, on a map of the same size built by the mock's own generator (it spreads the points evenly: its local map is the
size it prints) - the reference-shaped host loops of src/CeresOptimizer.cc:346-406, :423-506, :573-598 and the two drop-in calls (flattening
+ host entries + write-back), best of five.  The results must equal the restatement before anything is timed.
    python tools/local_ba_tables_time.py [--reps 50] [--out profiles/local_ba_tables_time.json]"""
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

TABLES = ("kf_id", "kf_bad", "kf_rank", "kf_Tcw", "kf_K4", "kf_slot_off", "kf_slot_pt", "X", "pt_bad", "pt_rank", "obs_off", "obs_kf", "obs_uv", "obs_level", "inv_level_sigma2",
          "kf_center", "pt_nobs", "pt_ref_kf", "obs_slot", "kf_level0", "scale_factors")
INOUT = ("kf_Tcw", "kf_center", "kf_slot_pt", "X", "pt_bad", "pt_nobs", "pt_ref_kf")


def _cpp(tmp, mode):
    from ceres_mono_orb_slam2_amd import _lib
    exe = os.path.join(tmp, "test_localba_dropin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_localba_dropin.cpp"), "-o", exe, _lib.LIB_PATH, "-lpthread",
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
    ap.add_argument("--half", type=int, default=40)
    ap.add_argument("--local-share", type=float, default=0.07)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ceres_mono_orb_slam2_amd import localmapping as lm
    from tests import localbacases as lc
    from tests import nplocalba as npl
    assert torch.cuda.is_available(), "local_ba_tables_time.py needs a GPU (there is no CPU fallback to time)"
    dev = torch.device("cuda:0")

    def t(x):
        return torch.as_tensor(np.array(x)).to(dev) if isinstance(x, np.ndarray) else x
    m = lc.make_map(0, a.nkf, a.npts, half=a.half, local_share=a.local_share, rest_outside=True)
    asm = npl.assemble(m)
    res = lc.solver_result(1, m, asm)
    exp = npl.apply(m, asm, *res)
    tab = {k: m.get(k) for k in TABLES}
    got = lm.local_ba_assemble(m["cur_kf"], m["nbr_kf"], tab)
    for k in ("counts", "cam_kf", "poses7", "lpt_pt", "pts3", "lobs_cam", "lobs_pt", "lobs_uv", "lobs_inv_sigma2", "lobs_src", "kf_role", "pt_local"):
        assert np.array_equal(got[k], asm[k]), k
    ap_got = lm.local_ba_apply(asm, *res, tab)
    wrote = exp["nd_written"] != 0
    for k in ("kf_Tcw", "kf_center", "kf_slot_pt", "X", "pt_bad", "pt_nobs", "pt_ref_kf", "obs_erased", "nd_written", "counts"):
        assert np.array_equal(np.asarray(ap_got[k]).reshape(-1), np.asarray(exp[k]).reshape(-1)), k
    assert np.array_equal(ap_got["normal"][wrote], exp["normal"][wrote]) and np.array_equal(ap_got["min_max"][wrote], exp["min_max"][wrote])
    asm_wall = _time_host(a.reps, lambda: lm.local_ba_assemble(m["cur_kf"], m["nbr_kf"], tab))
    app_wall = _time_host(a.reps, lambda: lm.local_ba_apply(asm, *res, tab))
    # ---- the device entries on resident tables
    d = {k: t(v) for k, v in tab.items()}
    d_in = {k: d[k].clone() for k in INOUT}
    nbr = t(m["nbr_kf"])
    r = lm.local_ba_assemble_device(m["cur_kf"], nbr, d)
    torch.cuda.synchronize()
    assert int(r["status"].item()) == 0 and np.array_equal(r["counts"].cpu().numpy(), asm["counts"])
    n = (int(asm["counts"][0]), int(asm["counts"][2]), int(asm["counts"][3]))
    assert np.array_equal(r["lobs_src"].cpu().numpy()[:n[2]], asm["lobs_src"])
    a_out = {k: v for k, v in r.items() if k != "_workspace"}
    a_ws = r["_workspace"]
    asm_ev = _time_device(torch, a.reps, lambda: lm.local_ba_assemble_device(m["cur_kf"], nbr, d, out=a_out, workspace=a_ws), lambda: None)
    sol = [t(np.ascontiguousarray(v)) for v in res]
    r2 = lm.local_ba_apply_device(r, sol[0], sol[1], sol[2], d, n=n)
    torch.cuda.synchronize()
    assert int(r2["status"].item()) == 0 and np.array_equal(r2["counts"].cpu().numpy(), exp["counts"]) and np.array_equal(r2["X"].cpu().numpy().reshape(-1, 3), exp["X"])
    p_out = {k: r2[k] for k in ("obs_erased", "counts", "status", "normal", "min_max", "nd_written")}
    p_ws = r2["_workspace"]

    def restore():
        for k in INOUT:
            d[k].copy_(d_in[k])
    app_ev = _time_device(torch, a.reps, lambda: lm.local_ba_apply_device(r, sol[0], sol[1], sol[2], d, out=p_out, n=n, workspace=p_ws), restore)
    with tempfile.TemporaryDirectory() as tmp:
        cpp = _cpp(tmp, (a.nkf, a.npts, a.half))
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")][0]
    except (OSError, IndexError):
        pass

    def stats(ev, wall):
        return dict(device_ms=float(np.median(ev)), device_ms_min=float(np.min(ev)), device_ms_p90=float(np.percentile(ev, 90)),
                    host_entry_wall_ms=float(np.median(wall)), host_entry_wall_ms_min=float(np.min(wall)))
    res_json = dict(map=dict(nkf=a.nkf, npts=a.npts, nslots=len(m["kf_slot_pt"]), nobs=len(m["obs_kf"]), cameras=n[0], local_cameras=int(asm["counts"][1]), local_points=n[1],
                             rows=n[2], rows_erased=int(exp["counts"][0]), points_turned_bad=int(exp["counts"][1]), normals_written=int(exp["counts"][3])),
                    assemble=dict(workspace_bytes=int(a_ws.numel()), **stats(asm_ev, asm_wall)), apply=dict(workspace_bytes=int(p_ws.numel()), **stats(app_ev, app_wall)),
                    cpp=dict(note="assemble + apply together, on the mock's own map; best of five runs, not medians", **cpp), host_cpu=cpu, reps=a.reps)
    print(json.dumps(res_json))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res_json, f, indent=1)


if __name__ == "__main__":
    main()
