"""Times the device KeyFrameDatabase (orbv_db_*: DetectLoopCandidates / DetectRelocalizationCandidates as a scan) on one GPU, on resident data:
databases of 1 000 / 10 000 / 50 000 keyframes of about 1 000 words (synth.make_place_sequence over a vocabulary of a million words, the size of
ORBvoc.txt; the neighbour table filled), queries = views of places of the map.
Per database, in ONE run and alternating: `loop_ms` = one loop query, `reloc_ms` = one relocalisation query, `sixteen_singles_ms` = 16 single
relocalisation queries enqueued back to back, `batch16_ms` = one 16-query call.  Each figure is the device time of a window of --inner calls
between two HIP events divided by --inner, after a warm-up; --reps windows, median / min / max reported.  `scan_bytes` is what k_kfdb_scan reads
per query (every stored word id and the slot records); `scan_bytes_over_query_time_vs_8TBs` divides it by the WHOLE single relocalisation query
(scan, scores, ordering, selection - the scan alone is shorter) and by 8 TB/s.  Also the wall time of the host entry with its copies (median).
The one condition the tool enforces: the batch call takes less device time than the 16 single calls it replaces.
    python tools/kfdb_time.py [--reps 10] [--inner 10] [--sizes 1000,10000,50000] [--out profiles/kfdb_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", default="1000,10000,50000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "kfdb_time.py needs a GPU"
    from ceres_mono_orb_slam2_amd import KeyFrameDatabase, synth
    rows = []
    for n_kf in [int(x) for x in a.sizes.split(",")]:
        seq = synth.make_place_sequence(1, n_kf=n_kf + 16, n_words=1000000, n_feat=1000, step=25, flip=0.25, revisit=min(n_kf // 5, 2000))
        db = KeyFrameDatabase(seq["n_words"])
        for i in range(n_kf):
            db.add(i, seq["bows"][i]); db.set_best_covisibles(i, synth.place_best_covisibles(seq, i, upto=n_kf - 1))
        queries = seq["bows"][n_kf:n_kf + 16]                      # the 16 keyframes after the map: they revisit its start
        n_stored = int(sum(len(seq["bows"][i][0]) for i in range(n_kf)))
        dev = torch.device("cuda")

        def up(qs):
            off = np.zeros(len(qs) + 1, np.int32); off[1:] = np.cumsum([len(w) for w, _ in qs])
            w = np.concatenate([q[0] for q in qs]).astype(np.uint32).view(np.int32); v = np.concatenate([q[1] for q in qs])
            return torch.from_numpy(off).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(v).to(dev)
        singles = [up([q]) for q in queries]; batch = up(queries)
        con = synth.place_connected(seq, n_kf, upto=n_kf - 1)
        d_coff = torch.tensor([0, len(con)], dtype=torch.int32, device=dev); d_con = torch.tensor(con, dtype=torch.int32, device=dev)
        d_ms = torch.tensor([float(db.min_score(queries[0], con))], dtype=torch.float32, device=dev)
        ws = torch.empty((db.workspace_bytes(16),), dtype=torch.uint8, device=dev)
        qid = [0, 0]

        def run_loop():
            qid[0] += 1
            return db.detect_loop_candidates_batch_device(*singles[0], d_coff, d_con, d_ms, qid[0], cap=64, workspace=ws)

        def run_reloc():
            qid[1] += 1
            return db.detect_relocalization_candidates_batch_device(*singles[0], qid[1], cap=64, workspace=ws)

        def run_singles():
            out = []
            for s in singles:
                qid[1] += 1
                out.append(db.detect_relocalization_candidates_batch_device(*s, qid[1], cap=64, workspace=ws))
            return out

        def run_batch():
            qid[1] += 16
            return db.detect_relocalization_candidates_batch_device(*batch, qid[1] - 15, cap=64, workspace=ws)
        forms = (("loop_ms", run_loop), ("reloc_ms", run_reloc), ("sixteen_singles_ms", run_singles), ("batch16_ms", run_batch))
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
        info, cand = run_batch()
        torch.cuda.synchronize()
        res = db.batch_results(info, cand)
        assert all(r[1]["status"] == 0 and r[1]["n_sharing"] > 0 for r in res), res
        del keep
        qid[1] += 1
        db.detect_relocalization_candidates(queries[0], qid[1])
        wall = []
        for _ in range(a.reps):
            qid[1] += 1
            t0 = time.perf_counter(); db.detect_relocalization_candidates(queries[0], qid[1]); wall.append((time.perf_counter() - t0) * 1e3)
        scan_bytes = n_stored * 4 + n_kf * 16
        row = dict(n_keyframes=n_kf, stored_words=n_stored, query_words=int(len(queries[0][0])), reps=a.reps, inner=a.inner, scan_bytes=scan_bytes,
                   n_scored=[r[1]["n_scored"] for r in res], n_cand=[r[1]["n_cand"] for r in res], host_entry_wall_ms=_stats(wall),
                   **{k: _stats(v) for k, v in ms.items()})
        row["scan_bytes_over_query_time_vs_8TBs"] = scan_bytes / (row["reloc_ms"]["median"] * 1e-3) / 8e12
        row["batch_over_sixteen_singles"] = row["batch16_ms"]["median"] / row["sixteen_singles_ms"]["median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del db
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/kfdb_time.py --reps %d --inner %d --sizes %s" % (a.reps, a.inner, a.sizes), "rows": rows}, f, indent=1)
    for row in rows:                                               # the batching has to work: a defect otherwise, not a number to record
        assert row["batch16_ms"]["median"] < row["sixteen_singles_ms"]["median"], row


if __name__ == "__main__":
    main()
