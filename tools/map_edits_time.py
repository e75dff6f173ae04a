"""Times orbl_apply_map_edits (an ordered list of map-point edits replayed on the map tables, and the rebuild of the observation tables) on
one GPU on a map of tests/mapeditcases.py's generator: 500 keyframes, 100 000 points.  Two edit lists: one shaped like a
LocalMapping::SearchInNeighbors (30 target keyframes x 150 accepted rows of ORBmatcher::Fuse, a mix of every outcome), and the empty list
(the pure rebuild, with a tenth of the observations dead).  Reports medians of --reps calls: device time of the device entry point on
resident tables (HIP events around the call's launches; the in/out tables are restored from a device copy before every call, outside the
timed span), wall time of the host entry point with its packed upload and its download (through the ctypes wrapper), and - from
tests/cpp/mapedit_host_loop.cpp compiled -O2 - the literal loop over the std::map / std::vector mocks of tests/cpp/mock_orbslam.h on the same
map and the same edits (its Replace computes descriptors inside the loop, as the reference does; the table call defers that), plus
the flattening of those maps into CSR tables (what a host map pays instead of the rebuild).  The results must equal the restatement before
anything is timed.  There is no bar on these times: they are a record.
    python tools/map_edits_time.py [--reps 50] [--nkf 500] [--npts 100000] [--targets 30] [--rows 150] [--out profiles/map_edits_time.json]"""
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

INOUT = ("kf_slot_pt", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced")
KEYS = ("op_status", "op_found", "pt_touched", "kf_slot_pt", "pt_bad", "pt_nobs", "pt_found", "pt_visible", "pt_replaced", "oobs_off", "oobs_kf", "oobs_slot", "oobs_src",
        "oobs_level", "oobs_uv", "counts")


def _cpp(pr, reps, tmp):
    exe, blob = os.path.join(tmp, "mapedit_host_loop"), os.path.join(tmp, "problem.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "mapedit_host_loop.cpp"), "-o", exe])
    if pr.get("obs_dead") is not None:                               # (a host map simply does not hold the dead observations)
        keep = pr["obs_dead"] == 0
        off = np.concatenate([[0], np.cumsum(keep)])[pr["obs_off"]]
        pr = dict(pr, obs_off=off, obs_kf=pr["obs_kf"][keep], obs_slot=pr["obs_slot"][keep])
    words = [np.array([pr["nkf"], pr["npts"], len(pr["kf_slot_pt"]), len(pr["obs_kf"]), len(pr["op_kind"])], np.int32)]
    words += [np.asarray(pr[k]).astype(np.int32) for k in ("kf_slot_off", "kf_slot_pt", "obs_off", "obs_kf", "obs_slot", "pt_bad", "pt_nobs", "op_kind", "op_pt", "op_arg",
                                                           "op_kf", "op_slot")]
    with open(blob, "wb") as f:
        f.write(np.concatenate(words).tobytes())
    w = subprocess.check_output([exe, blob, str(reps)], timeout=900).decode().split()
    assert w[0] == "TIME", w
    return dict(loop_ms=float(w[2]), flatten_ms=float(w[4]), n_obs=int(w[6]), n_bad=int(w[8]))


def _time(pr, exp, reps):
    import torch
    from ceres_mono_orb_slam2_amd import localmapping
    from tests import mapeditcases as mc
    ops, tables = {k: pr[k] for k in mc.OP_KEYS}, {k: pr.get(k) for k in mc.TABLES}
    got = localmapping.apply_map_edits(ops, tables)                  # (warm-up: library load, workspace growth)
    for k in KEYS:
        assert np.array_equal(getattr(got, k), exp[k]), k
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        localmapping.apply_map_edits(ops, tables)
        wall.append((time.perf_counter() - t0) * 1e3)
    dev = torch.device("cuda:0")
    d_tab = {k: None if v is None else torch.as_tensor(np.array(v)).to(dev) for k, v in tables.items()}
    d_ops = {k: torch.as_tensor(np.array(v)).to(dev) for k, v in ops.items()}
    pristine = {k: d_tab[k].clone() for k in INOUT}
    d_out, ws, ev = None, None, []
    for rep in range(reps + 5):
        for k in INOUT:
            d_tab[k].copy_(pristine[k])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d = localmapping.apply_map_edits_device(d_ops, d_tab, out=d_out, workspace=ws)
        e1.record()
        torch.cuda.synchronize()
        ws = d._workspace
        d_out = {k: getattr(d, k) for k in ("op_status", "op_found", "pt_touched", "oobs_off", "oobs_kf", "oobs_slot", "oobs_src", "oobs_level", "oobs_uv", "counts", "status")}
        if rep == 0:
            n = int(exp["counts"][0])
            assert np.array_equal(d.counts.cpu().numpy(), exp["counts"]) and int(d.status.item()) == 0
            assert np.array_equal(d.oobs_kf.cpu().numpy()[:n], exp["oobs_kf"]) and np.array_equal(d.oobs_src.cpu().numpy()[:n], exp["oobs_src"])
            assert np.array_equal(d.kf_slot_pt.cpu().numpy(), exp["kf_slot_pt"]) and np.array_equal(d.op_status.cpu().numpy(), exp["op_status"])
        if rep >= 5:
            ev.append(e0.elapsed_time(e1))
    with tempfile.TemporaryDirectory() as tmp:
        cpp = _cpp(pr, reps, tmp)
    assert cpp["n_obs"] == int(exp["counts"][0]) and cpp["n_bad"] == int(exp["pt_bad"].sum()), (cpp, exp["counts"])
    c = exp["counts"]
    st = np.bincount(exp["op_status"], minlength=11) if len(exp["op_status"]) else np.zeros(11, int)
    return dict(nops=len(pr["op_kind"]), obs_out=int(c[0]), obs_added=int(c[1]), replace_calls=int(c[2]), fused=int(c[4]), touched=int(c[5]), late_adds=int(c[6]),
                status_histogram=[int(v) for v in st], workspace_bytes=int(ws.numel()), device_ms=float(np.median(ev)), device_ms_min=float(np.min(ev)),
                device_ms_p90=float(np.percentile(ev, 90)), host_entry_wall_ms=float(np.median(wall)), host_entry_wall_ms_min=float(np.min(wall)),
                cpp_host_loop_ms=cpp["loop_ms"], cpp_flatten_ms=cpp["flatten_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--nkf", type=int, default=500)
    ap.add_argument("--npts", type=int, default=100000)
    ap.add_argument("--targets", type=int, default=30)
    ap.add_argument("--rows", type=int, default=150)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tests import mapeditcases as mc
    from tests import npmapedit as npm
    assert torch.cuda.is_available(), "map_edits_time.py needs a GPU (there is no CPU fallback to time)"
    slots = max(12, 3 * a.npts * 5 // a.nkf // 2)
    base = mc.make_map(0, a.nkf, a.npts, slots)
    base.pop("_used")
    rng = np.random.default_rng(0)
    fuse = mc.with_ops(base, mc.search_in_neighbors(base, rng, rng.choice(a.nkf, a.targets, replace=False), a.rows, p_masked=0.0))
    rebuild = mc.with_dead(base)
    res = dict(nkf=a.nkf, npts=a.npts, nslots=len(base["kf_slot_pt"]), nobs=len(base["obs_kf"]), reps=a.reps,
               search_in_neighbors=_time(fuse, npm.apply_map_edits(fuse), a.reps), rebuild=_time(rebuild, npm.apply_map_edits(rebuild), a.reps))
    res["rebuild"]["obs_dead"] = int(rebuild["obs_dead"].sum())
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")][0]
    except (OSError, IndexError):
        pass
    res["host_cpu"] = cpu
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
