"""Times the two halves of OptimizeEssentialGraph on the map tables on one GPU: orbl_essential_graph_assemble and orbl_essential_graph_apply
on a 500-keyframe, 100 000-point map with a group of 40 keyframes (tests/essgraphcases.py's generator).  Per call it reports: device time
of the device entry point on resident tables (HIP events around the call's launches, median of --reps timed calls after warm-up; the
in/out tables are restored before every apply, outside the timed window), wall time of the host entry point with its packed upload and its
download (median, through the ctypes wrapper), and - from tests/cpp/test_essgraph_dropin.cpp compiled -O2 in its `time` mode, on a map of
the same size built by the mock's own generator - the host graph walk CeresOptimizerT::OptimizeEssentialGraph and the drop-in
FrameOpsT::OptimizeEssentialGraph, both halves together with the solve answered at once, best of five.  The results must agree with the
restatement before anything is timed.
    python tools/essential_graph_tables_time.py [--reps 50] [--out profiles/essential_graph_tables_time.json]"""
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

TABLES = ("kf_id", "kf_bad", "kf_rank", "kf_Tcw", "kf_parent", "child_off", "child_kf", "loop_off", "loop_kf", "conn_off", "conn_kf", "conn_w", "ord_off", "ord_kf", "ord_w",
          "conn_group_kf", "corrected", "non_corrected", "tgt_kf", "link_off", "link_kf", "kf_center", "X", "pt_bad", "pt_done", "pt_corr_ref", "pt_ref_kf", "obs_off", "obs_kf",
          "ref_level", "scale_factors")
INOUT = ("kf_Tcw", "kf_center", "X")


def _cpp(tmp, mode):
    from ceres_mono_orb_slam2_amd import _lib
    exe = os.path.join(tmp, "test_essgraph_dropin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_essgraph_dropin.cpp"), "-o", exe, _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    w = subprocess.check_output([exe, "time"] + [str(v) for v in mode], timeout=900).decode().split()
    assert w[0] == "TIME", w
    return dict(host_walk_ms=float(w[2]), dropin_ms=float(w[4]), vertices=int(w[6]), edges=int(w[8]))


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
    ap.add_argument("--group", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ceres_mono_orb_slam2_amd import loopclosing as lc
    from tests import essgraphcases as ec
    from tests import npessgraph as npe
    assert torch.cuda.is_available(), "essential_graph_tables_time.py needs a GPU (there is no CPU fallback to time)"
    dev = torch.device("cuda:0")

    def t(x):
        return torch.as_tensor(np.array(x)).to(dev) if isinstance(x, np.ndarray) else x

    def close(g, e):
        g, e = np.asarray(g, np.float64).reshape(-1), np.asarray(e, np.float64).reshape(-1)
        return g.shape == e.shape and np.abs(g - e).max() <= 1e-12 * max(1.0, np.abs(e).max())
    m = ec.seeded_map(0, a.nkf, a.npts, n_group=a.group)
    asm = npe.assemble(m)
    opt = ec.solver_result(1, asm["lie7"])
    exp = npe.apply(m, asm["vtx_kf"], asm["lie7"], opt)
    tab = {k: m.get(k) for k in TABLES}
    got = lc.essential_graph_assemble(m["loop"], m["cur"], tab)
    for k in ("counts", "vtx_kf", "kf_vtx", "vtx_fixed", "edge_j", "edge_i", "edge_kind"):
        assert np.array_equal(got[k], asm[k]), k
    assert close(got["lie7"], asm["lie7"]) and close(got["edge_Sji"], asm["edge_Sji"])
    ap_got = lc.essential_graph_apply(asm["vtx_kf"], asm["lie7"], opt, tab)
    for k in ("pt_moved", "nd_written", "counts"):
        assert np.array_equal(ap_got[k], exp[k]), k
    assert close(ap_got["kf_Tcw"], exp["kf_Tcw"]) and close(ap_got["X"], exp["X"])
    asm_wall = _time_host(a.reps, lambda: lc.essential_graph_assemble(m["loop"], m["cur"], tab))
    app_wall = _time_host(a.reps, lambda: lc.essential_graph_apply(asm["vtx_kf"], asm["lie7"], opt, tab))
    # ---- the device entries on resident tables
    d = {k: t(v) for k, v in tab.items()}
    d_in = {k: d[k].clone() for k in INOUT}
    r = lc.essential_graph_assemble_device(m["loop"], m["cur"], d)
    torch.cuda.synchronize()
    assert int(r["status"].item()) == 0 and np.array_equal(r["counts"].cpu().numpy(), asm["counts"])
    nv, ne = int(asm["counts"][0]), int(asm["counts"][1])
    assert np.array_equal(r["edge_j"].cpu().numpy()[:ne], asm["edge_j"])
    a_out = {k: v for k, v in r.items() if k != "_workspace"}
    a_ws = r["_workspace"]
    asm_ev = _time_device(torch, a.reps, lambda: lc.essential_graph_assemble_device(m["loop"], m["cur"], d, out=a_out, workspace=a_ws), lambda: None)
    sol = t(np.ascontiguousarray(opt))
    r2 = lc.essential_graph_apply_device(r["vtx_kf"], r["lie7"], sol, d, n_vtx=nv)
    torch.cuda.synchronize()
    assert int(r2["status"].item()) == 0 and np.array_equal(r2["counts"].cpu().numpy(), exp["counts"]) and close(r2["X"].cpu().numpy(), exp["X"])
    p_out = {k: r2[k] for k in ("pt_moved", "counts", "status", "normal", "min_max", "nd_written")}
    p_ws = r2["_workspace"]

    def restore():
        for k in INOUT:
            d[k].copy_(d_in[k])
    app_ev = _time_device(torch, a.reps, lambda: lc.essential_graph_apply_device(r["vtx_kf"], r["lie7"], sol, d, out=p_out, workspace=p_ws, n_vtx=nv), restore)
    with tempfile.TemporaryDirectory() as tmp:
        cpp = _cpp(tmp, (a.nkf, a.npts, a.group))
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")][0]
    except (OSError, IndexError):
        pass

    def stats(ev, wall):
        return dict(device_ms=float(np.median(ev)), device_ms_min=float(np.min(ev)), device_ms_p90=float(np.percentile(ev, 90)),
                    host_entry_wall_ms=float(np.median(wall)), host_entry_wall_ms_min=float(np.min(wall)))
    res_json = dict(map=dict(nkf=a.nkf, npts=a.npts, group=a.group, vertices=nv, edges=ne, loop_connection_edges=int(asm["counts"][2]), nobs=len(m["obs_kf"]),
                             points_moved=int(exp["counts"][1]), normals_written=int(exp["nd_written"].sum())),
                    assemble=dict(workspace_bytes=int(a_ws.numel()), **stats(asm_ev, asm_wall)), apply=dict(workspace_bytes=int(p_ws.numel()), **stats(app_ev, app_wall)),
                    cpp=dict(note="assemble + apply together with the solve answered at once, on the mock's own map; best of five runs, not medians", **cpp), host_cpu=cpu,
                    reps=a.reps)
    print(json.dumps(res_json))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res_json, f, indent=1)


if __name__ == "__main__":
    main()
