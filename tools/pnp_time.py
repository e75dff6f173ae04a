"""Times orbt_pnp_* (PnPsolver::iterate: EPnP inside RANSAC) on one GPU:
  one candidate at N = 50 / 200 / 2 000 points (30 % outliers, 0.5 px noise) with the iteration count SetRansacParameters gives:
    device time of orbt_pnp_iterate_batch_device on resident data (HIP events, median), wall time of the host entry
    orbt_pnp_iterate with its copies (median, ctypes wrapper), and for scale the wall time of the numpy restatement with LAPACK
    (tests/nppnp.py, lapack=True) on the same input on the host - a numpy figure, not a claim about the reference's C++;
  a 16-candidate batch at N = 200: device time per call.
A call stops at its first successful refit, so the work depends on the scene; `consumed` is written with every row, and the
`all sets` rows (max_err = 0: no hypothesis qualifies) time the full iteration count without a refit.
The per-kernel split is for ONE shape (16 candidates, N = 200): run
    rocprofv3 --kernel-trace --stats -d DIR -o pnp -- python tools/pnp_time.py --only batch16 --reps 5
first, then pass DIR's database with --kernel-split-db; the mean duration of each k_pnp_* dispatch is written with the rows.
    python tools/pnp_time.py [--reps 20] [--only batch16] [--kernel-split-db DB] [--out profiles/pnp_time.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _cand(seed, n, all_sets=False):
    from ceres_mono_orb_slam2_amd import pnp, synth
    s = synth.make_reloc(seed, n, 0.3, 0.5, "general")
    pr = pnp.ransac_params(n, 0.99, 10, 300, 4, 0.5)
    e = pnp.max_errors(s["sigma2"])
    return dict(p3d=s["p3d"], p2d=s["p2d"], max_err=np.zeros_like(e) if all_sets else e, K4=s["K4"], min_inliers=pr["min_inliers"],
                sets=pnp.draw_sets(n, pr["max_iterations"]))


def _device_ms(pnp, cands, reps):
    import torch
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    nc = len(cands)
    off = np.concatenate([[0], np.cumsum([len(c["p3d"]) for c in cands])]).astype(np.int32)
    nt = int(off[-1])
    args = (up(np.concatenate([c["p3d"] for c in cands])), up(np.concatenate([c["p2d"] for c in cands])), up(np.concatenate([c["max_err"] for c in cands])),
            up(off), up(np.stack([c["K4"] for c in cands])), up(np.array([c["min_inliers"] for c in cands], np.int32)),
            up(np.array([len(c["sets"]) for c in cands], np.int32)), up(np.stack([c["sets"] for c in cands])))
    bc0, bm0 = torch.zeros(nc, dtype=torch.int32, device=dev), torch.zeros(nt, dtype=torch.uint8, device=dev)
    bc, bm, bt = bc0.clone(), bm0.clone(), torch.zeros((nc, 4, 4), dtype=torch.float64, device=dev)
    res, inl = torch.zeros(pnp.result_bytes(nc), dtype=torch.uint8, device=dev), torch.zeros(nt, dtype=torch.uint8, device=dev)
    ws = pnp.iterate_batch_device(*args, bc, bm, bt, res, inl)  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        bc.copy_(bc0); bm.copy_(bm0)                             # a fresh state: every repetition does the same work
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); ws = pnp.iterate_batch_device(*args, bc, bm, bt, res, inl); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    del ws
    r = pnp.decode_results(res.cpu().numpy())
    return float(np.median(ms)), [x["consumed"] for x in r], [x["status"] for x in r]


def _kernel_split(db_path):
    """mean microseconds per dispatch of every k_pnp_* kernel in a rocprofv3 database (its `kernels` view)."""
    paths = glob.glob(os.path.join(db_path, "**", "*.db"), recursive=True) if os.path.isdir(db_path) else [db_path]
    db = sqlite3.connect(paths[0])
    rows = db.execute("select name, count(*), avg(\"end\" - start) / 1000.0 from kernels where name like '%k_pnp%' group by name").fetchall()
    return {name.split("(")[0].replace("orbhip::", "").replace("void ", ""): dict(dispatches=int(n), mean_us=round(float(us), 2)) for name, n, us in rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="batch16: time only the 16-candidate batch (the shape of the kernel split)")
    ap.add_argument("--kernel-split-db", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ceres_mono_orb_slam2_amd import pnp
    rows = []
    if a.only is None:
        import nppnp
        for n in (50, 200, 2000):
            for all_sets in (False, True):
                c = _cand(n, n, all_sets)
                call = lambda: pnp.iterate(c["p3d"], c["p2d"], c["max_err"], c["K4"], c["min_inliers"], c["sets"])   # noqa: E731
                call()
                wall = []
                for _ in range(a.reps):
                    t0 = time.perf_counter(); r = call(); wall.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                nppnp.iterate(c["p3d"], c["p2d"], c["max_err"], c["K4"], c["min_inliers"], c["sets"], lapack=True)
                np_ms = (time.perf_counter() - t0) * 1e3
                dev_ms, consumed, status = _device_ms(pnp, [c], a.reps)
                rows.append(dict(shape="single, all sets" if all_sets else "single", n=n, iterations=len(c["sets"]), consumed=consumed[0], status=status[0],
                                 device_ms=dev_ms, host_entry_wall_ms=float(np.median(wall)), numpy_lapack_host_wall_ms=np_ms))
                assert r["consumed"] == consumed[0]
                print(json.dumps(rows[-1]), flush=True)
    for all_sets in (False, True):
        batch = [_cand(100 + i, 200, all_sets) for i in range(16)]
        dev_ms, consumed, status = _device_ms(pnp, batch, a.reps)
        rows.append(dict(shape="batch16, all sets" if all_sets else "batch16", n_candidates=16, n=200, iterations=len(batch[0]["sets"]), consumed=consumed,
                         device_ms=dev_ms))
        print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tools/pnp_time.py --reps %d" % a.reps, "rows": rows}
    if a.kernel_split_db:
        out["kernel_split_batch16_us"] = _kernel_split(a.kernel_split_db)
        print(json.dumps(out["kernel_split_batch16_us"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
