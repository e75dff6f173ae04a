"""Times Tracking::UpdateLocalMap + TrackLocalMap of one frame on one GPU, two ways, on a map whose local part is about 80 keyframes x
2 000 slots and 8 000 distinct points (100 keyframes, 8 200 points, each seen from 24 keyframes; a 1241 x 376 frame of 2 000 features
that holds 1 500 of them):
  (a) the path without the device entry points: the host loops of the reference's shape (tools/cpp/localmap_host.cpp, -O3: votes into a
      std::map, the walk, the first-occurrence union over copies of the slot tables), the packing of the block, then
      orbt_track_local_map with its upload (orbt_last_call_ms: entry to return inside the library);
  (b) orbt_update_local_map_device + orbt_track_local_map_device over resident tables: wall time of the two calls together (the second
      one synchronises), and HIP events around the first one's seven launches.
The two must produce the same lists and the same tracking result.  The GPU calls of (a) and (b) alternate inside one loop; medians and
the 10th / 90th percentiles over --reps after --warmup.
    python tools/local_map_time.py [--reps 200] [--warmup 10] [--out profiles/local_map_time.json]"""
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

W_IMG, H_IMG = 1241, 376
K4 = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)
BOUNDS = np.array([0, W_IMG, 0, H_IMG], np.float32)


def make_map(seed=0, nkf=100, npts=8200, per_point=24, reach=14, n_kp=2000, held=1500):
    from tests import localmapcases as lc
    rng = np.random.default_rng(seed)
    obs = []
    for p in range(npts):
        c = int(rng.integers(nkf))
        near = np.arange(max(0, c - reach), min(nkf, c + reach + 1))
        obs.append(sorted(int(k) for k in rng.choice(near, size=min(per_point, len(near)), replace=False)))
    slots = [[] for _ in range(nkf)]
    for p in rng.permutation(npts):
        for k in obs[p]:
            slots[k].append(int(p))
    parent = {k: k - 1 for k in range(1, nkf)}
    children = {k: [k + 1] for k in range(nkf - 1)}
    cov = {k: [j for j in (k - 1, k + 1, k - 2, k + 2, k - 3, k + 3, k - 4, k + 4, k - 5, k + 5) if 0 <= j < nkf] for k in range(nkf)}
    centre = nkf // 2
    near = [p for p in range(npts) if any(abs(k - centre) <= 8 for k in obs[p])]
    frame = np.full(n_kp, -1, np.int32)
    frame[rng.permutation(n_kp)[:held]] = rng.choice(near, size=held, replace=False)
    pr = lc.build(nkf, slots, frame, obs=obs, npts=npts, cov=cov, children=children, parent=parent, pt_bad=rng.permutation(npts)[:npts // 50], seen=[], prev=[])
    return pr


def _host_baseline(pr, reps, tmp):
    path = os.path.join(tmp, "localmap.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(pr["frame_pt"]), len(pr["pt_bad"]), len(pr["kf_bad"]), len(pr["obs_kf"]), len(pr["cov_kf"]), len(pr["child_kf"]), len(pr["kf_slot_pt"])], np.int32).tobytes())
        for k in ("frame_pt", "pt_bad", "pt_nobs", "obs_off", "obs_kf", "kf_bad", "kf_parent", "cov_off", "cov_kf", "child_off", "child_kf", "kf_slot_off", "kf_slot_pt"):
            f.write(np.ascontiguousarray(pr[k], np.int32).tobytes())
    exe = os.path.join(tmp, "localmap_host")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tools", "cpp", "localmap_host.cpp"), "-o", exe])
    return json.loads(subprocess.check_output([exe, path, str(reps)], timeout=600).decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ceres_mono_orb_slam2_amd import ORBextractor, synth, tracking
    from tests import nplocalmap as nlm
    assert torch.cuda.is_available(), "local_map_time.py needs a GPU (there is no CPU fallback to time)"
    rng = np.random.default_rng(1)
    img = synth.make_frame(20, W_IMG, H_IMG, "checker")
    ex = ORBextractor(2000, 1.2, 8, 20, 7)
    Tcw = np.eye(4)
    z = np.zeros
    got1 = tracking.track_with_motion_model(ex, img, K4, BOUNDS, Tcw, z((0, 3)), z((0, 32), np.uint8), z(0, np.int32), z(0, np.float32), z(0, np.uint8))
    n_kp = len(got1["kps"])
    pr = make_map(n_kp=n_kp, held=min(1500, n_kp * 3 // 4))
    npts = len(pr["pt_bad"])
    # records: points in front of the camera (identity pose).  Half of them lie on the ray of a keypoint of the frame, one pixel off, with
    # that keypoint's descriptor and a distance range that predicts its octave (they can be matched); the frame's held points lie on
    # their own keypoints' rays; the rest are anywhere in the image with random descriptors.
    depth = rng.uniform(4, 60, npts)
    px = np.stack([rng.uniform(0, W_IMG, npts), rng.uniform(0, H_IMG, npts)], 1)
    D = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    octave = rng.integers(0, 8, npts)
    kxy = np.stack([got1["kps"]["x"], got1["kps"]["y"]], 1).astype(np.float64)
    pick = rng.integers(0, n_kp, npts)
    px[::2] = kxy[pick[::2]] + rng.standard_normal((len(pick[::2]), 2)); D[::2] = got1["desc"][pick[::2]]; octave[::2] = got1["kps"]["octave"][pick[::2]]
    fp = pr["frame_pt"]; has = fp >= 0
    px[fp[has]] = kxy[has]
    X = np.stack([(px[:, 0] - K4[2]) / K4[0] * depth, (px[:, 1] - K4[3]) / K4[1] * depth, depth], 1)
    dist = np.linalg.norm(X, axis=1)
    maxd = dist * 1.2 ** octave                                                  # MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:338-377)
    pr.update(pt_Xw=X, pt_normal=X / dist[:, None], pt_min_dist=(maxd / 1.2 ** 7).astype(np.float32), pt_max_dist=maxd.astype(np.float32), pt_desc=D)
    exp = nlm.update_local_map(pr)
    n, nk = exp["n_local_pt"], exp["n_local_kf"]
    cap_kf, cap_pt = 128, 16384
    log_scale = np.float32(np.log(np.float32(1.2)))
    biggest = int(np.diff(pr["kf_slot_off"]).max())
    host = _host_baseline(pr, a.reps, tempfile.mkdtemp())
    assert (host["n_local_kf"], host["n_local_pt"]) == (nk, n), (host, nk, n)
    # (a) the upload path
    args = (exp["mp_Xw"], exp["mp_normal"], exp["mp_min_dist"], exp["mp_max_dist"], exp["mp_desc"], exp["mp_state"], exp["slot_Xw"], exp["slot_state"])
    want = tracking.track_local_map(ex, K4, BOUNDS, Tcw, log_scale, *args)
    # (b) resident tables; the two paths alternate inside one loop so that whatever else the host does hits both alike
    T = {k: (None if v is None else torch.as_tensor(np.array(v)).cuda()) for k, v in pr.items()}
    out = {}
    up, wall, ev, tlm = [], [], [], []
    for i in range(a.warmup + a.reps):
        tracking.track_local_map(ex, K4, BOUNDS, Tcw, log_scale, *args)
        up.append(tracking.last_call_ms())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        d = tracking.update_local_map_device(T, cap_kf, cap_pt, max_local_slots=(cap_kf + 1) * biggest, votes=False, out=out)
        e1.record()
        got = tracking.track_local_map_device(ex, K4, BOUNDS, Tcw, log_scale, d, cap_pt)
        wall.append((time.perf_counter() - t0) * 1e3)
        tlm.append(tracking.last_call_ms())
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    c = d["counts"].cpu().numpy()
    assert list(c) == [nk, exp["ref_kf"], n, 0] and int(d["status"].item()) == 0 and np.array_equal(d["local_pt"].cpu().numpy()[:n], exp["local_pt"])
    assert np.array_equal(got["match"][:n], want["match"]) and got["pose7"].tobytes() == want["pose7"].tobytes()
    med = lambda v: float(np.median(v[a.warmup:]))                               # noqa: E731
    p10_90 = lambda v: [float(np.percentile(v[a.warmup:], 10)), float(np.percentile(v[a.warmup:], 90))]      # noqa: E731
    res = dict(n_local_kf=nk, n_local_pt=n, local_slots=int(sum(pr["kf_slot_off"][k + 1] - pr["kf_slot_off"][k] for k in exp["local_kf"])), n_kp=n_kp,
               in_view=int(want["n_in_view"]), nmatches=int(want["nmatches"]),
               a_host_loops_ms=host["loops_ms"], a_host_loops_and_packing_ms=host["host_ms"], a_track_local_map_upload_ms=med(up),
               a_total_ms=host["host_ms"] + med(up), a_track_local_map_upload_p10_p90=p10_90(up),
               b_update_device_events_ms=med(ev), b_track_local_map_device_ms=med(tlm), b_total_wall_ms=med(wall), b_total_wall_p10_p90=p10_90(wall), reps=a.reps, warmup=a.warmup)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
