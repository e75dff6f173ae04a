"""Times orbl_set_bad_keyframes (KeyFrame::SetBadFlag for a whole keyframe list) on one GPU on a map of tests/badflagcases.py's generator:
500 keyframes, 100 000 points, 5 targets.  Reports medians of --reps calls: device time of the device entry point on resident tables
(HIP events around the call's launches; the in/out tables are restored from a device copy before every call, outside the timed span),
wall time of the host entry point with its packed upload and its download (through the ctypes wrapper), and - from
tests/cpp/test_badflag_dropin.cpp compiled -O2 in its `time` mode, on a map of the same size built by the mock's own generator - the
reference-shaped host loop and the whole drop-in call (flattening + host entry + write-back).  The results must equal the restatement
before anything is timed.  There is no bar on these times: they are a record.
    python tools/set_bad_keyframes_time.py [--reps 50] [--nkf 500] [--ntgt 5] [--slots 800] [--out profiles/set_bad_keyframes_time.json]"""
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

TABLES = ("kf_bad", "kf_parent", "kf_rank", "kf_Tcw", "child_off", "child_kf", "conn_off", "conn_kf", "conn_w", "ord_off", "ord_kf", "ord_w", "kf_slot_off",
          "kf_slot_pt", "pt_bad", "pt_nobs", "pt_ref_kf", "obs_off", "obs_kf", "obs_slot")
INOUT = ("kf_bad", "kf_parent", "kf_slot_pt", "pt_bad", "pt_nobs", "pt_ref_kf")
KEYS = ("tgt_status", "tgt_Tcp", "kf_bad", "kf_parent", "counts", "oconn_off", "oconn_kf", "oconn_w", "oord_off", "oord_kf", "oord_w", "ochild_off", "ochild_kf",
        "kf_slot_pt", "pt_bad", "pt_nobs", "pt_ref_kf", "obs_erased")


def _cpp(nkf, ntgt, slots, reps, tmp):
    from ceres_mono_orb_slam2_amd import _lib
    exe = os.path.join(tmp, "test_badflag_dropin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_badflag_dropin.cpp"), "-o", exe, _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    w = subprocess.check_output([exe, "time", str(nkf), str(ntgt), str(slots), str(reps)], timeout=900).decode().split()
    assert w[0] == "TIME", w
    return dict(host_loop_ms=float(w[2]), dropin_ms=float(w[4]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--nkf", type=int, default=500)
    ap.add_argument("--ntgt", type=int, default=5)
    ap.add_argument("--slots", type=int, default=800)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    from tests import badflagcases as bc
    from tests import npbadflag as npb
    assert torch.cuda.is_available(), "set_bad_keyframes_time.py needs a GPU (there is no CPU fallback to time)"
    pr = bc.make(0, a.nkf, a.ntgt, slots_per_kf=a.slots)
    pr["tgt_flags"][:] = 0; pr["tgt_mask"][:] = 1                    # (every target goes)
    exp = npb.set_bad_keyframes(pr)
    tables = {k: pr[k] for k in TABLES}
    got = localmapping.set_bad_keyframes(pr["tgt_kf"], tables)       # (warm-up: library load, workspace growth)
    for k in KEYS:
        assert np.array_equal(getattr(got, k), exp[k]), k
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        localmapping.set_bad_keyframes(pr["tgt_kf"], tables)
        wall.append((time.perf_counter() - t0) * 1e3)
    dev = torch.device("cuda:0")
    d_tab = {k: torch.as_tensor(np.array(v)).to(dev) for k, v in tables.items()}
    pristine = {k: d_tab[k].clone() for k in INOUT}
    d_tgt = torch.as_tensor(np.array(pr["tgt_kf"])).to(dev)
    d_out, ws, ev = {}, None, []
    for rep in range(a.reps + 5):
        for k in INOUT:
            d_tab[k].copy_(pristine[k])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d = localmapping.set_bad_keyframes_device(d_tgt, d_tab, out=d_out, workspace=ws)
        e1.record()
        torch.cuda.synchronize()
        ws = d._workspace
        d_out = {k: getattr(d, k) for k in ("tgt_status", "tgt_Tcp", "oconn_off", "oconn_kf", "oconn_w", "oord_off", "oord_kf", "oord_w", "ochild_off", "ochild_kf",
                                            "counts", "status", "obs_erased")}
        if rep == 0:
            c = d.counts.cpu().numpy()
            assert np.array_equal(c, exp["counts"]) and int(d.status.item()) == 0
            assert np.array_equal(d.oord_kf.cpu().numpy()[:c[2]], exp["oord_kf"]) and np.array_equal(d.kf_parent.cpu().numpy(), exp["kf_parent"])
            assert np.array_equal(d.pt_nobs.cpu().numpy(), exp["pt_nobs"]) and np.array_equal(d.tgt_Tcp.cpu().numpy(), exp["tgt_Tcp"])
        if rep >= 5:
            ev.append(e0.elapsed_time(e1))
    with tempfile.TemporaryDirectory() as tmp:
        cpp = _cpp(a.nkf, a.ntgt, a.slots, a.reps, tmp)
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")][0]
    except (OSError, IndexError):
        pass
    c = exp["counts"]
    res = dict(nkf=a.nkf, ntgt=a.ntgt, npts=pr["npts"], nslots=len(pr["kf_slot_pt"]), nobs=len(pr["obs_kf"]), nconn=len(pr["conn_kf"]), n_bad=int(c[0]),
               conn_out=int(c[1]), ord_out=int(c[2]), child_out=int(c[3]), adopted=int(c[4]), fallback=int(c[5]), points_turned_bad=int(exp["pt_bad"].sum()),
               workspace_bytes=int(ws.numel()), device_ms=float(np.median(ev)), device_ms_min=float(np.min(ev)), device_ms_p90=float(np.percentile(ev, 90)),
               host_entry_wall_ms=float(np.median(wall)), host_entry_wall_ms_min=float(np.min(wall)), cpp_host_loop_ms=cpp["host_loop_ms"],
               cpp_dropin_ms=cpp["dropin_ms"], host_cpu=cpu, reps=a.reps)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
