"""Times orbt_initialize* (Initializer::Initialize, H / F RANSAC + reconstruction) on one GPU:
  one pair at N ~ 100 / 500 / 2 000 / 4 000 matches with 200 iterations: device time of orbt_initialize_batch_device on resident
    data (HIP events, median) and wall time of the host entry orbt_initialize with its copies (median, ctypes wrapper);
  a 64-pair batch at N ~ 2 000: device time per call.
No host baseline: the reference needs Eigen and OpenCV.  The per-kernel split is for ONE shape (one pair, N ~ 2 000): run
    rocprofv3 --kernel-trace --stats -d DIR -o init -- python tools/init_time.py --only single2000 --reps 5
first, then pass DIR's database with --kernel-split-db; the mean duration of each k_init_* dispatch is written with the rows.
    python tools/init_time.py [--reps 20] [--only single2000] [--kernel-split-db DB] [--out profiles/initializer_time.json]"""
import argparse
import glob
import json
import os
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _scene(seed, n_matches):
    from ceres_mono_orb_slam2_amd import synth
    from ceres_mono_orb_slam2_amd.initializer import draw_ransac_sets
    s = synth.make_two_view(seed, "general", int(n_matches / 0.9) + 1, 0.2, 0.3)
    nm = int((s["matches12"] >= 0).sum())
    return s["kps1"], s["kps2"], s["matches12"], s["K4"], draw_ransac_sets(nm, 200, None), nm


def _device_ms(init, pairs, reps):
    import torch
    dev = torch.device("cuda")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731
    off1 = np.cumsum([0] + [len(p[0]) for p in pairs]).astype(np.int32); off2 = np.cumsum([0] + [len(p[1]) for p in pairs]).astype(np.int32)
    args = (t(np.concatenate([p[0] for p in pairs]), np.float32), t(off1, np.int32), t(np.concatenate([p[1] for p in pairs]), np.float32),
            t(off2, np.int32), t(np.concatenate([p[2] for p in pairs]), np.int32), t(np.stack([p[3] for p in pairs]), np.float32), 1.0, 200,
            t(np.stack([p[4] for p in pairs]), np.int32))
    n = len(pairs)
    out = {"R21": torch.zeros((n, 3, 3), dtype=torch.float64, device=dev), "t21": torch.zeros((n, 3), dtype=torch.float64, device=dev),
           "P3D": torch.zeros((int(off1[-1]), 3), dtype=torch.float64, device=dev), "triangulated": torch.zeros(int(off1[-1]), dtype=torch.uint8, device=dev),
           "report": torch.zeros(init.report_bytes(n), dtype=torch.uint8, device=dev)}
    init.initialize_batch_device(*args, out)                    # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); init.initialize_batch_device(*args, out); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def _kernel_split(db_path):
    """mean microseconds per dispatch of every k_init_* kernel in a rocprofv3 database (its `kernels` view)."""
    paths = glob.glob(os.path.join(db_path, "**", "*.db"), recursive=True) if os.path.isdir(db_path) else [db_path]
    db = sqlite3.connect(paths[0])
    rows = db.execute("select name, count(*), avg(\"end\" - start) / 1000.0 from kernels where name like '%k_init%' group by name").fetchall()
    return {name.split("(")[0].replace("orbhip::", "").replace("void ", ""): dict(dispatches=int(n), mean_us=round(float(us), 2)) for name, n, us in rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="single2000: time only one pair at N ~ 2 000 (the shape of the kernel split)")
    ap.add_argument("--kernel-split-db", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ceres_mono_orb_slam2_amd import initializer as init
    rows = []
    for n in ((2000,) if a.only == "single2000" else (100, 500, 2000, 4000)):
        p = _scene(n, n)
        k1, k2, m, K, sets, nm = p
        init.initialize(k1, k2, m, K, 1.0, 200, sets)
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); r = init.initialize(k1, k2, m, K, 1.0, 200, sets); wall.append((time.perf_counter() - t0) * 1e3)
        rows.append(dict(shape="single", n_matches=nm, iterations=200, device_ms=_device_ms(init, [p], a.reps), host_entry_wall_ms=float(np.median(wall)),
                         reason=int(r["reason"])))
        print(json.dumps(rows[-1]), flush=True)
    if a.only is None:
        batch = [_scene(1000 + i, 2000) for i in range(64)]
        rows.append(dict(shape="batch64", npairs=64, n_matches_mean=float(np.mean([b[5] for b in batch])), iterations=200,
                         device_ms=_device_ms(init, batch, max(3, a.reps // 4))))
        print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tools/init_time.py --reps %d" % a.reps, "rows": rows}
    if a.kernel_split_db:
        out["kernel_split_single2000_us"] = _kernel_split(a.kernel_split_db)
        print(json.dumps(out["kernel_split_single2000_us"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
