#!/usr/bin/env python
"""Relocalization's refinement behind PnP: the fused call (orbt_relocalization_refine, every candidate of a round at once) against the
chain of per-call host entries it replaces (ba_pose_optimization + orbm_search_by_projection per candidate, tests/nprelocrefine.py's
ChainBackend with the loop stopped at its first empty pass), at 1241 x 376 with 2000 features and 5 candidates that all reach the narrow
search.  Medians of --reps calls, wall clock around the Python wrappers of both (the chain's numpy glue - the projection on the host, as
the drop-in classes do it in C++ - is part of the chain); the fused call's time inside the library (orbt_last_call_ms) is reported too.
Writes profiles/reloc_refine_time.json.
    python tools/reloc_refine_time.py [--reps 50] [--out profiles/reloc_refine_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAUNCHES_PER_CALL = 14      # k_rr_step x 4, (k_rr_gather + k_pose_lm) x 3, (k_rr_project + k_trk_windows) x 2: csrc/orb_relocrefine.inc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc_refine_time.json"))
    a = ap.parse_args()
    from ceres_mono_orb_slam2_amd import ORBextractor, tracking
    from oracle import pyoracle as oracle
    from tests import nprelocrefine as R
    from tests import relocrefinecases as RC
    frames = RC.two_frames(oracle, 41, (1241, 376), 2000, RC.K4_WIDE)
    F = frames[1]
    cands = [RC.candidate(oracle, seed=s, n_correct=30, n_wrong=20, n_extra=30, n_extra_off=18, frames=frames) for s in (9, 12, 14, 15, 16, 17, 18, 19)]
    want = [R.refine(oracle, F, c, True, True, early_exit=True) for c in cands]
    keep = [i for i, w in enumerate(want) if w["n_additional"][1] >= 0][:5]
    assert len(keep) == 5, "fewer than 5 of the candidates reach the narrow search: %s" % [R.STAGE_NAMES[w["stage"]] for w in want]
    cands = [cands[i] for i in keep]; want = [want[i] for i in keep]
    ex = ORBextractor(2000, 1.2, 8, 20, 7)
    z = np.zeros
    tracking.track_with_motion_model(ex, F["img"], F["K4"], F["bounds"], np.eye(4), z((0, 3)), z((0, 32), np.uint8), z(0, np.int32), z(0, np.float32), z(0, np.uint8))
    n_kp = len(F["kps4"])

    def fused():
        return tracking.relocalization_refine(ex, F["K4"], F["bounds"], cands, F["log_scale"], n_kp=n_kp)
    chain = R.ChainBackend()

    def chained():
        return R.refine_round(chain, F, cands, True, True, early_exit=True)
    got = fused()
    for g, w in zip(got["results"], want):
        assert g["stage"] == w["stage"] and g["n_good"] == w["n_good"] and np.array_equal(g["slot_kf"], w["slot_kf"])
    for _ in range(3):
        fused(); chained()
    tf, tl, tc = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); fused(); tf.append((time.perf_counter() - t0) * 1e3); tl.append(tracking.last_call_ms())
    calls0 = chain.calls
    for _ in range(a.reps):
        t0 = time.perf_counter(); chained(); tc.append((time.perf_counter() - t0) * 1e3)
    out = dict(image=[1241, 376], n_keypoints=n_kp, n_keyframe_features=[int(len(c["pt"])) for c in cands], candidates=len(cands), reps=a.reps,
               stages=[R.STAGE_NAMES[g["stage"]] for g in got["results"]], narrow_passes=[g["narrow_passes"] for g in got["results"]],
               fused_ms_median=float(np.median(tf)), fused_ms_min=float(np.min(tf)), fused_inside_library_ms_median=float(np.median(tl)),
               chain_ms_median=float(np.median(tc)), chain_ms_min=float(np.min(tc)), chain_host_round_trips_per_round=(chain.calls - calls0) // a.reps,
               fused_launches_per_call=LAUNCHES_PER_CALL, fused_host_round_trips_per_round=1)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
