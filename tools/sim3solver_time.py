"""Times orbt_sim3_* (Sim3Solver::iterate: Horn's closed form inside RANSAC) on one GPU, on resident data:
  one candidate and a 16-candidate batch at n = 50 / 200 / 1 000 correspondences (50 % outliers, noise 0.2 % of the depth) with 300
  sets, thresholds 0 so that every set is consumed (every hypothesis is computed and counted in any case; only the walk is shorter
  when a call succeeds early).
Per shape, in ONE run and alternating: `single_ms` = one single-candidate call, `sixteen_singles_ms` = 16 single-candidate calls
enqueued back to back, `batch16_ms` = one 16-candidate call.  Each figure is the device time of a window of --inner calls between
two HIP events divided by --inner, after a warm-up; --reps windows, median / min / max reported.  The one condition the tool
enforces: the batch call takes less time than the 16 single calls it replaces.  Also the wall time of the host entry
orbt_sim3_iterate with its copies (median).
    python tools/sim3solver_time.py [--reps 20] [--inner 20] [--out profiles/sim3solver_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cand(seed, n):
    from ceres_mono_orb_slam2_amd import sim3solver, synth
    s = synth.make_loop_candidate(seed, n, 0.5, 0.002, 1.1, "general")
    z = np.zeros(n, np.float32)
    return dict(X1c=s["X1c"], X2c=s["X2c"], max_err1=z, max_err2=z, K1=s["K1"], K2=s["K2"], fix_scale=0, min_inliers=20, sets=sim3solver.draw_sets(n, 300))


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "sim3solver_time.py needs a GPU"
    from ceres_mono_orb_slam2_amd import sim3solver
    rows = []
    for n in (50, 200, 1000):
        cands = [_cand(100 + i, n) for i in range(16)]
        batch, _ = sim3solver.upload_batch([dict(c) for c in cands])
        singles = [sim3solver.upload_batch([dict(c)])[0] for c in cands]

        def run_batch():
            return sim3solver.iterate_batch_device(**batch)

        def run_single():
            return sim3solver.iterate_batch_device(**singles[0])

        def run_singles():
            return [sim3solver.iterate_batch_device(**s) for s in singles]
        forms = (("single_ms", run_single), ("sixteen_singles_ms", run_singles), ("batch16_ms", run_batch))
        for _, f in forms:                                         # warm-up of every shape
            for _ in range(3):
                keep = f()
        torch.cuda.synchronize()
        ms = {k: [] for k, _ in forms}
        for _ in range(a.reps):
            for k, f in forms:                                     # alternating: the forms share whatever else the machine does
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                keep = [f() for _ in range(a.inner)]
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.inner)
        del keep
        res = sim3solver.decode_results(batch["result"].cpu().numpy())
        assert all(r["status"] == sim3solver.NOT_FOUND and r["consumed"] == 300 for r in res)
        c = cands[0]
        call = lambda: sim3solver.iterate(c["X1c"], c["X2c"], c["max_err1"], c["max_err2"], c["K1"], c["K2"], 0, 20, c["sets"])   # noqa: E731
        call()
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); call(); wall.append((time.perf_counter() - t0) * 1e3)
        row = dict(n=n, sets=300, n_candidates=16, reps=a.reps, inner=a.inner, host_entry_wall_ms=_stats(wall), **{k: _stats(v) for k, v in ms.items()})
        row["batch_over_sixteen_singles"] = row["batch16_ms"]["median"] / row["sixteen_singles_ms"]["median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/sim3solver_time.py --reps %d --inner %d" % (a.reps, a.inner), "rows": rows}, f, indent=1)
    for row in rows:                                               # the batching has to work: a defect otherwise, not a number to record
        assert row["batch16_ms"]["median"] < row["sixteen_singles_ms"]["median"], row
        assert row["batch16_ms"]["max"] < row["sixteen_singles_ms"]["min"], row


if __name__ == "__main__":
    main()
