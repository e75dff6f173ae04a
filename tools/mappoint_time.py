"""Times orbl_update_map_points (MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth, batched) on one GPU against the host
loop it replaces, for the two batch shapes of tests/test_gpu_mappoint.py:
  search_in_neighbors  2 000 points, skewed observation counts (tests/npmappoint.py skewed_ns), both parts;
  local_ba_writeback   10 000 points of synth's C4 graph, ORBL_MP_NORMAL_DEPTH only.
Reports per shape: device time per call of the device entry point on resident data (HIP events, median), wall time of the host
entry point with its copies (median, through the ctypes wrapper with preallocated outputs), and the host baseline
tools/cpp/mappoint_host.cpp (-O3: the mock data model's ComputeDistinctiveDescriptors loop and the normal / depth loop).
    python tools/mappoint_time.py [--reps 50] [--out FILE.json]"""
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


def _host_baseline(b, reps, tmp):
    npts = len(b["obs_off"]) - 1
    nobs = int(b["obs_off"][-1])
    desc = b["obs_desc"] if b["obs_desc"] is not None else np.zeros((nobs, 32), np.uint8)
    good = b["obs_kf_good"] if b["obs_kf_good"] is not None else np.ones(nobs, np.uint8)
    path = os.path.join(tmp, "batch.bin")
    with open(path, "wb") as f:
        f.write(np.array([npts, nobs, len(b["kf_center"])], np.int32).tobytes())
        for a, dt in ((b["obs_off"], np.int32), (desc, np.uint8), (good, np.uint8), (b["obs_kf"], np.int32), (b["X"], np.float64),
                      (b["kf_center"], np.float64), (b["ref_kf"], np.int32), (b["ref_level"], np.int32), (b["scale_factors"][:8], np.float32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    exe = os.path.join(tmp, "mappoint_host")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tools", "cpp", "mappoint_host.cpp"), "-o", exe])
    return json.loads(subprocess.check_output([exe, path, str(reps)], timeout=600).decode().strip().splitlines()[-1])


def _time_shape(name, b, what, reps, tmp):
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    from tests import npmappoint as npm
    npts = len(b["obs_off"]) - 1
    out = npm.fresh_outputs(npts)
    args = (b["obs_off"], b["obs_desc"], b["obs_kf_good"], b["X"], b["ref_kf"], b["ref_level"], b["obs_kf"], b["kf_center"], b["scale_factors"], b["pt_good"], what, out)
    localmapping.update_map_points(*args)                                   # (warm-up: library load, workspace growth)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        localmapping.update_map_points(*args)
        wall.append((time.perf_counter() - t0) * 1e3)
    dev = torch.device("cuda:0")
    T = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)          # noqa: E731
    d_in = (T(b["obs_off"], np.int32), T(b["obs_desc"], np.uint8), T(b["obs_kf_good"], np.uint8), T(b["X"], np.float64), T(b["ref_kf"], np.int32),
            T(b["ref_level"], np.int32), T(b["obs_kf"], np.int32), T(b["kf_center"], np.float64), T(b["scale_factors"], np.float32), T(b["pt_good"], np.uint8))
    d_out = {k: torch.from_numpy(v.copy()).to(dev) for k, v in out.items()}
    localmapping.update_map_points_device(*d_in, what, d_out)
    torch.cuda.synchronize()
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        localmapping.update_map_points_device(*d_in, what, d_out)
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    host = _host_baseline(b, max(3, reps // 5), tmp)
    nobs = int(b["obs_off"][-1])
    ng = np.diff(b["obs_off"])
    return dict(shape=name, npts=npts, nobs=nobs, what=what, sum_n2=int((ng.astype(np.int64) ** 2).sum()), device_ms=float(np.median(ev)),
                host_entry_wall_ms=float(np.median(wall)), host_baseline_desc_ms=host["desc_ms"], host_baseline_nd_ms=host["nd_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from tests import npmappoint as npm
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        b = npm.make_batch(3, npm.skewed_ns(3, 2000), nkf=80, bad_kf_frac=0.1, bad_pt_frac=0.02)
        res.append(_time_shape("search_in_neighbors", b, npm.DESC | npm.NORMAL_DEPTH, a.reps, tmp))
        res.append(_time_shape("local_ba_writeback", npm.c4_normal_depth_batch(0), npm.NORMAL_DEPTH, a.reps, tmp))
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
