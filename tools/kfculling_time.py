"""Times orbl_keyframe_culling (LocalMapping::KeyFrameCulling for the whole candidate list, sequential semantics) on one GPU against
the host loop it replaces, on two problems of tests/cullingcases.py's generator:
  wide   140 keyframes, 3 000 points, two of them seen by every keyframe (the `wide` configuration of the tests, seed 0);
  c4     a C4-sized neighbourhood: 100 keyframes, 10 000 points, about 50 000 observations.
Reports per problem: device time per call of the device entry point on resident data (HIP events around the four launches, median),
wall time of the host entry point with its copies (median, through the ctypes wrapper with preallocated outputs), and the host
baseline tools/cpp/kfculling_host.cpp (-O3: the mock data model's reference-shaped loop, map rebuilt per repeat, loop alone timed).
The three must agree on the decisions before anything is timed.
    python tools/kfculling_time.py [--reps 50] [--out profiles/kfculling_time.json]"""
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


def _host_baseline(pr, reps, tmp, name):
    path = os.path.join(tmp, name + ".bin")
    with open(path, "wb") as f:
        f.write(np.array([len(pr["cand_kf"]), len(pr["slot_pt"]), pr["nkf"], pr["npts"], len(pr["obs_kf"])], np.int32).tobytes())
        for k in ("cand_kf", "cand_flags", "slot_off", "slot_pt", "slot_level", "obs_off", "obs_kf", "obs_level"):
            f.write(np.ascontiguousarray(pr[k], np.int32).tobytes())
    exe = os.path.join(tmp, "kfculling_host")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tools", "cpp", "kfculling_host.cpp"), "-o", exe])
    return json.loads(subprocess.check_output([exe, path, str(reps)], timeout=600).decode().strip().splitlines()[-1])


def _time_problem(name, pr, reps, tmp):
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    from tests import npculling as npc
    assert torch.cuda.is_available(), "kfculling_time.py needs a GPU (there is no CPU fallback to time)"
    exp = npc.culling(pr)
    args = (pr["cand_kf"], pr["cand_flags"], pr["slot_off"], pr["slot_pt"], pr["slot_level"], pr["nkf"], pr["obs_off"], pr["obs_kf"], pr["obs_level"])
    out = {}
    got = localmapping.keyframe_culling(*args, out=out)                       # (warm-up: library load, workspace growth)
    assert np.array_equal(got.culled, exp["culled"]) and np.array_equal(got.pt_bad, exp["pt_bad"]) and np.array_equal(got.obs_erased, exp["obs_erased"])
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        localmapping.keyframe_culling(*args, out=out)
        wall.append((time.perf_counter() - t0) * 1e3)
    dev = torch.device("cuda:0")
    d_in = [torch.as_tensor(np.array(a)).to(dev) if isinstance(a, np.ndarray) else a for a in args]
    d_out = {}
    d = localmapping.keyframe_culling_device(*d_in, out=d_out)
    torch.cuda.synchronize()
    assert np.array_equal(d.culled.cpu().numpy(), exp["culled"]) and int(d.status.item()) == 0
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        localmapping.keyframe_culling_device(*d_in, out=d_out)
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    host = _host_baseline(pr, max(5, reps // 5), tmp, name)
    assert host["flagged"] == int(exp["culled"].sum()), (host, int(exp["culled"].sum()))
    visits = int(sum(int(pr["obs_off"][p + 1] - pr["obs_off"][p]) for p in pr["slot_pt"]))
    return dict(problem=name, ncand=len(pr["cand_kf"]), nslots=len(pr["slot_pt"]), npts=pr["npts"], nobs=len(pr["obs_kf"]), observation_visits=visits,
                culled=int(exp["culled"].sum()), points_turned_bad=int(exp["pt_bad"].sum()), device_ms=float(np.median(ev)), device_ms_min=float(np.min(ev)),
                device_ms_p90=float(np.percentile(ev, 90)), host_entry_wall_ms=float(np.median(wall)), host_baseline_ms=host["host_ms"], reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from tests import cullingcases as cc
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        res.append(_time_problem("wide", cc.make(0, **cc.CONFIGS["wide"][0]), a.reps, tmp))
        res.append(_time_problem("c4", cc.make(0, nkf=101, npts=10000, span=3, q=0.9, lvl_jit=1), a.reps, tmp))
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
