"""Times orbl_update_connections_device (KeyFrame::UpdateConnections for a whole keyframe list) on one GPU on a CorrectLoop-sized batch of
tests/connectioncases.py's generator: 500 keyframes, 60 of them targets with about 2 000 slots each, about 5 observers per point, stale
tables.  Reports: device time per call of the device entry point on resident data (HIP events around the call's launches, median of
--reps timed calls after warm-up), wall time of the host entry point with its packed upload and its download (median, through the
ctypes wrapper with preallocated outputs), and - from tests/cpp/test_connections_dropin.cpp compiled -O2 in its `time` mode, on a map of
the same size built by the mock's own generator - the reference-shaped host loop of LoopClosing.cc:551-573 and the whole drop-in call
(flattening + host entry + write-back), best of five.  The device results must equal the restatement before anything is timed.
    python tools/update_connections_time.py [--reps 50] [--nkf 500] [--ntgt 60] [--slots 2000] [--out profiles/update_connections_time.json]"""
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


def _cpp(nkf, ntgt, slots, tmp):
    from ceres_mono_orb_slam2_amd import _lib
    exe = os.path.join(tmp, "test_connections_dropin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_connections_dropin.cpp"), "-o", exe, _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    w = subprocess.check_output([exe, "time", str(nkf), str(ntgt), str(slots)], timeout=600).decode().split()
    assert w[0] == "TIME", w
    return dict(host_loop_ms=float(w[2]), dropin_ms=float(w[4]), slots=int(w[6]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--nkf", type=int, default=500)
    ap.add_argument("--ntgt", type=int, default=60)
    ap.add_argument("--slots", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    from tests import connectioncases as cc
    from tests import npconnections as npc
    assert torch.cuda.is_available(), "update_connections_time.py needs a GPU (there is no CPU fallback to time)"
    pr = cc.make(0, nkf=a.nkf, ntgt=a.ntgt, per_kf=a.slots * 3 // 5, window=4, n_obs=(4, 7))
    exp = npc.connections(pr)
    args = [pr[k] for k in ("tgt_kf", "slot_off", "slot_pt")] + [pr["nkf"]] + [pr[k] for k in ("obs_off", "obs_kf", "conn_off", "conn_kf", "conn_w")]
    kw = {k: pr[k] for k in ("tgt_flags", "pt_bad", "kf_rank", "prev_off", "prev_kf")}
    keys = ("tgt_status", "tgt_parent", "aff_kf", "conn_off", "conn_kf", "conn_w", "ord_off", "ord_kf", "ord_w", "link_off", "link_kf")
    out = {}
    got = localmapping.update_connections(*args, out=out, **kw)               # (warm-up: library load, workspace growth)
    for k in keys:
        assert np.array_equal(got[k], exp[k]), k
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        localmapping.update_connections(*args, out=out, **kw)
        wall.append((time.perf_counter() - t0) * 1e3)
    dev = torch.device("cuda:0")

    def t(x):
        return torch.as_tensor(np.array(x)).to(dev) if isinstance(x, np.ndarray) else x
    d_args = [t(x) for x in args]; d_kw = {k: t(v) for k, v in kw.items()}
    d_out = {}
    d = localmapping.update_connections_device(*d_args, out=d_out, **d_kw)
    ws = d["_workspace"]
    torch.cuda.synchronize()
    c = d["counts"].cpu().numpy()
    assert np.array_equal(c, exp["counts"]) and int(d["status"].item()) == 0
    assert np.array_equal(d["ord_kf"].cpu().numpy()[:c[2]], exp["ord_kf"]) and np.array_equal(d["link_kf"].cpu().numpy()[:c[3]], exp["link_kf"])
    for _ in range(5):
        localmapping.update_connections_device(*d_args, out=d_out, workspace=ws, **d_kw)
    torch.cuda.synchronize()
    ev = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        localmapping.update_connections_device(*d_args, out=d_out, workspace=ws, **d_kw)
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    with tempfile.TemporaryDirectory() as tmp:
        cpp = _cpp(a.nkf, a.ntgt, a.slots, tmp)
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")][0]
    except (OSError, IndexError):
        pass
    res = dict(nkf=a.nkf, ntgt=a.ntgt, nslots=len(pr["slot_pt"]), npts=pr["npts"], nobs=len(pr["obs_kf"]), nconn=len(pr["conn_kf"]),
               affected=int(c[0]), map_entries=int(c[1]), list_entries=int(c[2]), links=int(c[3]), workspace_bytes=int(ws.numel()),
               device_ms=float(np.median(ev)), device_ms_min=float(np.min(ev)), device_ms_p90=float(np.percentile(ev, 90)),
               host_entry_wall_ms=float(np.median(wall)), host_entry_wall_ms_min=float(np.min(wall)), cpp_host_loop_ms=cpp["host_loop_ms"],
               cpp_dropin_ms=cpp["dropin_ms"], cpp_slots=cpp["slots"], host_cpu=cpu, reps=a.reps)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
